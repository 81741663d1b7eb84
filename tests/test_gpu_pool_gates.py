"""The slab pool's candidate loop (pt_device.hpp: slab_chunk_pass), whole frames against the oracle bit for bit.  Its two gates are one
comparison each on the candidate key — `none` is a NaN pattern that fails both by itself — liveness is folded into the keys once per
pass, and the keys and (closest, hit) are written in place; so the frames here are chosen for what the gates see: scans in which every
key is the sentinel while closest is still +inf, pools of two chunks and of an odd count (the padded entry, the re-pass past three
candidates), rays that start on faces, edges and corners of boxes (the `inside` gate, both outcomes of the proof), a wave with an
irregular ray beside regular ones, a closed room, the generic kernels' pool, and windows whose masked or padding pixels are lanes
that reach the scan without being live (61 x 35 has padding pixels in its edge tiles, 64 x 36 none)."""
import numpy as np
import pytest

import kernel_variant_cases as K
import scenes_small as S
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from path_tracer_amd.scene import box, lambertian_material, lightsource_material, pack, xy_rect

pytestmark = pytest.mark.gpu

SIZES = [(64, 36), (61, 35)]
SPP = 8


def _check(orc, ps, cam, w, h, spp=SPP, depth=50, flags=0, what="", scene=None, mats=K.MATS_RECTBOX):
    """mats: the material / hittable set of the LDS-resident headline kernel the frame must have run (pt_debug_last_kernels)"""
    c = scenes.make_camera(cam, w, h)
    orc.set_math(True)
    ref = orc.render(ps, c.c, w, h, spp, depth)
    if scene is not None:
        fb = R.render_host(w, h, spp, scene, c, depth, flags=flags)
        frame = K.last_kernels(scene)[1]
    else:
        fb, (_, frame) = K.render_host_tagged(w, h, spp, ps, c, depth, flags=flags)
    assert K.ran(frame, lds=1, grid=0, mats=mats), frame
    assert_bit_identical(fb, ref, f"{what} {w}x{h}x{spp} depth {depth}")


def _box_field(n_small, seed=5):
    """Rects and boxes only, every coordinate an integer: n_small boxes of edge 1 or 2 on the lattice (they overlap, share faces, edges and
    corners, so bounce rays start on faces, edges and corners of their neighbours), every fourth a light; one rect in a lattice plane; two
    nested boxes around everything with the camera inside both — a ray there has L == min for at least two entries, and three more
    candidates in front of it are common: the re-pass.  n_small + 3 pool entries."""
    g = np.random.default_rng(seed)
    cols = [lambertian_material(c) for c in ((0.8, 0.8, 0.8), (0.9, 0.2, 0.2), (0.2, 0.9, 0.2), (0.2, 0.2, 0.9))]
    light = lightsource_material((4, 4, 4))
    hs = []
    for i in range(n_small):
        lo = np.array([g.integers(-4, 3), g.integers(-4, 3), g.integers(-9, -2)])
        hi = lo + g.integers(1, 3, 3)
        hs.append(box(tuple(int(v) for v in lo), tuple(int(v) for v in hi), light if i % 4 == 0 else cols[i % 4]))
    hs.insert(n_small // 2, xy_rect(-3, 3, -3, 3, -9, cols[1]))
    hs += [box((-6, -6, -11), (6, 6, 3), cols[0]), box((-7, -7, -12), (7, 7, 4), cols[3])]
    cam = dict(look_from=(0.3, 0.4, 2), look_at=(0, 0, -5), vup=(0, 1, 0), vfov=70.0, aperture=0.0, focus_dist=5.0, time0=0.0, time1=0.0)
    return pack(hs), cam


@pytest.mark.parametrize("size", SIZES)
def test_no_ray_has_a_candidate(orc, size):
    """the camera turned away from the Cornell-style scene: every key of every scan is the sentinel while closest is +inf"""
    ps, cam = S.cornell_scene()
    _check(orc, ps, dict(cam, look_at=(278, 278, -1600)), *size, what="cornell, camera turned away")


@pytest.mark.parametrize("n_small", [18, 4])
@pytest.mark.parametrize("size", SIZES)
def test_box_field_on_a_lattice(orc, size, n_small):
    """21 entries: two chunks, the second of an odd count (the padded all-NaN entry); 7 entries: one odd chunk.  Origins on faces, edges
    and corners; more than three candidates per chunk (had3 / more / kdone)"""
    ps, cam = _box_field(n_small)
    _check(orc, ps, cam, *size, what=f"box field, {n_small + 3} entries")


@pytest.mark.parametrize("size", SIZES)
def test_cornell_depth_50(orc, size):
    """rays that leave the faces of the walls and blocks: the proof drops most of those keys and must keep the rest"""
    ps, cam = S.cornell_scene()
    _check(orc, ps, cam, *size, what="cornell")


def _far_scene():
    """A pooled rect / box scene 2^27 away along x, where floats are 8 or 16 apart: a camera looking down -z there has camera rays whose
    x component is exactly 0 next to rays with +-8, +-16 in the same 8 x 8 tile."""
    X = float(2 ** 27)
    cols = [lambertian_material(c) for c in ((0.8, 0.8, 0.8), (0.9, 0.2, 0.2), (0.2, 0.2, 0.9))]
    hs = [box((X - 32, -10, -90), (X - 8, -2, -50), cols[0]), box((X - 8, -4, -80), (X + 16, 6, -60), cols[1]),
          box((X + 16, -10, -100), (X + 48, 10, -70), cols[2]), box((X - 64, -12, -120), (X + 64, -10, -30), cols[0]),
          xy_rect(X - 64, X + 64, -12, 12, -120, lightsource_material((3, 3, 3)))]
    cam = dict(look_from=(X, 0.5, 0.0), look_at=(X, 0.5, -64.0), vup=(0, 1, 0), vfov=24.0, aperture=0.0, focus_dist=64.0, time0=0.0, time1=0.0)
    return pack(hs), cam


@pytest.mark.parametrize("size", SIZES)
def test_a_wave_with_an_irregular_ray(orc, size):
    ps, cam = _far_scene()
    c = scenes.make_camera(cam, *size).c
    f = np.float32
    dx = {float(f(f(f(c.lower_left_corner[0]) + f(f(s) * f(c.horizontal[0]))) - f(c.origin[0]))) for s in np.linspace(0.4, 0.6, 401, dtype=np.float32)}
    assert 0.0 in dx and len(dx) > 1, dx  # neighbouring pixels: a zero x component beside regular ones
    _check(orc, ps, cam, *size, what="far scene, zero direction components")


@pytest.mark.parametrize("size", SIZES)
def test_closed_room(orc, size):
    """the Cornell-style scene inside one large box: no ray reaches the sky, every path runs to its light or to depth 50"""
    hs, cam = scenes.cornell_box()
    ps = pack(hs + [box((-1000, -1000, -2000), (1500, 1500, 1500), lambertian_material((0.73, 0.73, 0.73)))])
    _check(orc, ps, cam, *size, what="closed room")


@pytest.mark.parametrize("size", SIZES)
def test_generic_family_pool(orc, size):
    """ties_scene (spheres and triangles beside the rects and boxes: the copy of the loop in the kernels for every hittable kind — lambertian
    over solid colours only, so MATS_LAMB_LIGHT_SOLID), its four rects / boxes in a pool"""
    ps, cam = S.ties_scene()
    ds = R.DeviceScene(ps, tuning=abi.tuning(slab_pools=1))
    _check(orc, ps, cam, *size, what="ties, pool forced", scene=ds, mats=K.MATS_SIMPLE)
    ds.close()


def test_progressive_and_adaptive_windows(orc):
    """a plain window split, and a masked adaptive window: masked pixels (and 61 x 35's padding pixels) are lanes that are not live"""
    import torch

    w, h = 61, 35
    ps, cam = _box_field(4)
    c = scenes.make_camera(cam, w, h)
    orc.set_math(True)
    ref = {n: orc.render(ps, c.c, w, h, n, 50) for n in (4, 8)}
    ds = R.DeviceScene(ps)
    acc = R.Accumulator(w, h, ds, c)
    acc.add(3).add(5)
    assert_bit_identical(acc.resolve().cpu().numpy(), ref[8], "box field, windows 3 + 5")
    acc.close()
    mask = torch.from_numpy((np.random.default_rng(3).random((h, w)) < 0.5).astype(np.uint8)).cuda()
    acc = R.Accumulator(w, h, ds, c, adaptive=True)
    acc.add(4).add(4, mask)
    fb, m = acc.resolve().cpu().numpy(), mask.cpu().numpy().astype(bool)
    acc.close()
    assert 0 < m.sum() < m.size
    assert_bit_identical(fb[m], ref[8][m], "box field, masked pixels at 8 spp")
    assert_bit_identical(fb[~m], ref[4][~m], "box field, unmasked pixels at 4 spp")
    ds.close()
