"""The headline kernel's bounce loop, whole frames against the oracle bit for bit: the lane state (ray, attenuation, generator, bounce
count) is written in place by the branch that continues a path, one (closest, hit) pair runs through the slab pool and the run scans,
and the loop pulls pixels in a loop of its own — so every way a lane can pass through an iteration is rendered here, in one wave, at a
frame size whose edge tiles have padding pixels (61 x 35: lanes that scan along without being live) and at one that has none."""
import numpy as np
import pytest

import kernel_variant_cases as K
import pool_octant_scenes as P
import scenes_small as S
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R

pytestmark = pytest.mark.gpu

SIZES = [(64, 36), (61, 35)]
SPP = 8


# the headline family's kernel of a small scene (csrc/pt_render.hip: headline_kernel): blob and materials in LDS, cold lane state in LDS, no grid walk
HEADLINE = dict(lds=1, mlds=1, cl=1, coop=0, grid=0, tripool=0)


def _check(orc, ps, cam, w, h, spp=SPP, depth=50, flags=0, what="", mats=K.MATS_RECTBOX):
    """mats: the material / hittable set of the headline kernel the frame must have run (pt_debug_last_kernels)"""
    c = scenes.make_camera(cam, w, h)
    orc.set_math(True)
    ref = orc.render(ps, c.c, w, h, spp, depth)
    fb, (probe, frame) = K.render_host_tagged(w, h, spp, ps, c, depth, flags=flags)
    assert K.ran(frame, mats=mats, **HEADLINE) and probe is None, (probe, frame)
    assert_bit_identical(fb, ref, f"{what} {w}x{h}x{spp} depth {depth}")


@pytest.mark.parametrize("size", SIZES)
def test_cornell_depth_50(orc, size):
    """(a) every box side, the rect, the light, the sky, lanes of every state in one wave"""
    ps, cam = S.cornell_scene()
    _check(orc, ps, cam, *size, what="cornell")


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_cornell_exhausted_bounces(orc, size, depth):
    """(b) the exhausted-bounce branch next to sky and light"""
    ps, cam = S.cornell_scene()
    _check(orc, ps, cam, *size, depth=depth, what="cornell")


@pytest.mark.parametrize("size", SIZES)
def test_ties(orc, size):
    """(c) equal t, the holder_later rule (this scene has spheres and triangles too, all lambertian over solid colours: the headline kernel for
    every hittable kind, MATS_LAMB_LIGHT_SOLID; test_rect_box_only_ties: the rect / box-only kernel's)"""
    ps, cam = S.ties_scene()
    _check(orc, ps, cam, *size, what="ties", mats=K.MATS_SIMPLE)


def _rectbox_ties_scene(n_boxes):
    """Rects and boxes only (the kernels compiled for such scenes: hit_records_rectbox, the guarded pool in hit_world_range), built of equal-t
    ties: overlapping rects in one plane, boxes that share faces, a box repeated later in the list, a rect in a box's face.  Four boxes get
    a slab pool (the exact trips out of list order, the holder_later rule, more than three candidates: the re-pass); two do not, and the
    same ties go through the guarded loops in list order."""
    from path_tracer_amd.scene import box, lambertian_material, lightsource_material, pack, xy_rect, xz_rect, yz_rect
    white, red, blue = lambertian_material((0.8, 0.8, 0.8)), lambertian_material((0.9, 0.1, 0.1)), lambertian_material((0.1, 0.1, 0.9))
    boxes = [box((-2, -1.5, -3), (2, -1, -1), white), box((-2, -1.5, -3), (0, -1, -1), red),   # shares five faces' planes with the first
             box((0, -1, -3), (2, 0, -2), blue),                                              # stands on the first: its bottom is the first's top
             box((0, -1, -3), (2, 0, -2), red)][:n_boxes]                                      # the same box later in the list: wins every tie
    hs = [xy_rect(-1, 1, -1, 1, -2, red), xy_rect(-0.5, 1.5, -0.5, 1.5, -2, blue),            # same plane, later in the list: wins the overlap
          *boxes,
          xz_rect(-2, 2, -3, -1, -1, blue),                                                   # in the plane of the first box's top
          yz_rect(-1.5, 1, -3, -1, -2, white), xy_rect(-3, 3, 2, 2.5, -2.5, lightsource_material((4, 4, 4)))]
    cam = dict(look_from=(0.3, 0.4, 1), look_at=(0, -0.3, -2), vup=(0, 1, 0), vfov=75.0, aperture=0.0, focus_dist=3.0, time0=0.0, time1=0.0)
    return pack(hs), cam


@pytest.mark.parametrize("n_boxes", [4, 2])
@pytest.mark.parametrize("size", SIZES)
def test_rect_box_only_ties(orc, lib, size, n_boxes):
    """(c') the same ties in the kernels this scene family runs: one (closest, hit) through the pool, its re-pass and the guarded loops"""
    ps, cam = _rectbox_ties_scene(n_boxes)
    assert len(P.pools(*P.flatten(lib, ps))) == (1 if n_boxes == 4 else 0), "four boxes get a slab pool, two do not"
    _check(orc, ps, cam, *size, what=f"rect / box ties, {n_boxes} boxes")
    _check(orc, ps, cam, *size, flags=abi.PT_FLAG_NO_FASTDIV, what=f"rect / box ties, {n_boxes} boxes, plain division")


@pytest.mark.parametrize("size", SIZES)
def test_cornell_with_a_lens(orc, size):
    """(d) the lens path of camera_ray, which lane_regenerate shares"""
    ps, cam = S.cornell_scene()
    _check(orc, ps, dict(cam, aperture=20.0), *size, what="cornell, aperture 20")


@pytest.mark.parametrize("size", SIZES)
def test_cornell_plain_division(orc, size):
    """(e) the irregular-ray path: reg == false, plain-division sides (the guarded loops of hit_records_rectbox), general sky"""
    ps, cam = S.cornell_scene()
    _check(orc, ps, cam, *size, flags=abi.PT_FLAG_NO_FASTDIV, what="cornell, PT_FLAG_NO_FASTDIV")


def test_cornell_probe_and_resume(orc):
    """(f) pt_render with enough samples (>= 16 spp) and tiles (>= 64) for the cost probe: the probe + resume branch of lane_acquire /
    lane_store.  64 x 36 is 40 tiles — the launcher does not probe it, as pt_debug_last_kernels shows; 64 x 72 is 72, and the same
    kernel runs as the probe and as the frame pass that resumes its samples."""
    import torch

    ps, cam = S.cornell_scene()
    ds = R.DeviceScene(ps)
    orc.set_math(True)
    for (w, h, spp), probed in (((64, 36, 40), False), ((64, 72, 40), True)):
        c = scenes.make_camera(cam, w, h)
        fb = R.render(w, h, spp, ds, c)
        torch.cuda.synchronize()
        probe, frame = K.last_kernels(ds)
        assert K.ran(frame, mats=K.MATS_RECTBOX, **HEADLINE) and probe == (frame if probed else None), (probe, frame)
        assert_bit_identical(fb.cpu().numpy(), orc.render(ps, c.c, w, h, spp), f"cornell {w}x{h}x{spp} through pt_render")
