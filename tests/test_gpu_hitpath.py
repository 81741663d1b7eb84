"""From the hit to the next sample in the headline kernel, whole frames against the oracle bit for bit at depth 50: a hit is shaded
from its ONE shade record (pt_flatten.hpp: Flat::shade; pt_device.hpp: shade_record) and the cold lane state lives in two 16-byte
LDS records per thread (pt_render.hip: Cold<true>).  Every case reads back that the headline kernel ran (pt_debug_last_kernels) and
which way it took to the pool (pt_debug_last_pool_word).  The shade record is found from the hit word, whichever way the hit was found:
the planned one-chunk pool (word 2), the walk of a larger pool (word 1) and the run scans of irregular rays all go through it, and
the case under PT_FLAG_NO_LDS renders the same frames with the reads of the hittable's and the material's records (another kernel).
Every reference is computed once and shared, read-only."""
import ctypes as C
import functools

import numpy as np
import pytest

import kernel_variant_cases as K
import pool_octant_scenes as P
import pool_plan_scenes as PP
import scenes_small as S
from conftest import assert_bit_identical
from dist_util import unshard_reference
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from path_tracer_amd.scene import box, lambertian_material, lightsource_material, pack, xy_rect, xz_rect, yz_rect

pytestmark = pytest.mark.gpu

HEADLINE = dict(lds=1, mlds=1, cl=1, coop=0, grid=0, tripool=0, mats=K.MATS_RECTBOX)
PLANNED, WALKED, NO_PLAN = 2, 1, 0  # pt_debug_last_pool_word


def _rect_light():
    """the camera looks straight at a rect light (xy) between a red yz rect and a green xz rect, three boxes in front of it (enough for a
    pool): camera rays hit the light, all three rect axes and box sides directly — axis and kind come from the shade record"""
    white, red, green = (lambertian_material(c) for c in ((0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15)))
    hs = [xy_rect(-2, 2, -1, 2, -6, lightsource_material((5, 4, 3))), yz_rect(-2, 3, -7, 1, -3, red), xz_rect(-4, 4, -7, 1, -2, green),
          box((-2.5, -2, -4), (-1.5, -0.5, -3), white), box((1.5, -2, -4.5), (2.5, 0, -3.5), red), box((-0.5, -2, -3.5), (0.5, -1.2, -2.5), white),
          xz_rect(-4, 4, -7, 1, 3, white)]
    cam = dict(look_from=(0, 0.3, 1), look_at=(0, 0.3, -6), vup=(0, 1, 0), vfov=60.0, aperture=0.0, focus_dist=6.0, time0=0.0, time1=0.0)
    return pack(hs), cam


SCENES = {"cornell": S.cornell_scene, "field16": lambda: P.box_field(13), "field17": PP.field17, "rect_light": _rect_light}


def _word(ds):
    out = C.c_int32(-1)
    abi.check(ds.lib.pt_debug_last_pool_word(ds.handle, C.byref(out)), "pt_debug_last_pool_word")
    return out.value


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def _reference(name, w, h, spp, depth=50):
    from oracle import binding as orc
    orc.load()
    orc.set_math(True)
    ps, cam = _scene(name)
    ref = orc.render(ps, scenes.make_camera(cam, w, h).c, w, h, spp, depth)
    ref.setflags(write=False)
    return ref


def _render(name, w, h, spp, flags=0, shard=(0, 1)):
    ps, cam = _scene(name)
    ds = R.DeviceScene(ps)
    try:
        fb = R.render_host(w, h, spp, ds, scenes.make_camera(cam, w, h), 50, flags=flags, shard_index=shard[0], shard_count=shard[1])
        return fb, K.last_kernels(ds)[1], _word(ds)
    finally:
        ds.close()


def test_cornell_40x24x8(orc):
    """40 x 24: whole tiles only; 37 x 21: edge tiles on both axes, whose padding pixels pass lane_acquire without a `begin`"""
    for w, h in ((40, 24), (37, 21)):
        fb, tag, word = _render("cornell", w, h, 8)
        assert K.ran(tag, **HEADLINE) and word == PLANNED, (tag, word)
        assert_bit_identical(fb, _reference("cornell", w, h, 8), f"cornell {w}x{h}x8")


@pytest.mark.parametrize("name,word", [("field16", PLANNED), ("field17", WALKED)])
def test_one_chunk_pool_and_walked_pool(orc, name, word):
    fb, tag, got = _render(name, 24, 16, 4)
    assert K.ran(tag, **HEADLINE) and got == word, (tag, got)
    assert_bit_identical(fb, _reference(name, 24, 16, 4), f"{name} 24x16x4")


def test_rect_light_hit_by_camera_rays(orc):
    ps, _ = _scene("rect_light")
    blob, n_runs = P.flatten(abi.load_library(), ps)
    assert [p[1] for p in P.pools(blob, n_runs)] == [7] and n_runs > 2, "one pool over several rect and box runs"
    fb, tag, word = _render("rect_light", 24, 16, 4)
    assert K.ran(tag, **HEADLINE) and word == PLANNED, (tag, word)
    ref = _reference("rect_light", 24, 16, 4)
    assert (ref[6:10, 10:14] == np.float32([5, 4, 3])).all(), "the frame's centre sees the light itself"
    assert_bit_identical(fb, ref, "rect_light 24x16x4")


def test_the_records_of_hittable_and_material_give_the_same_frames(orc):
    """PT_FLAG_NO_LDS: the scalar-cache kernel, which reads R0, R1 of the hittable and M0, M1 of its material"""
    for name in ("cornell", "rect_light"):
        fb, tag, word = _render(name, 24, 16, 4, flags=abi.PT_FLAG_NO_LDS)
        assert K.ran(tag, lds=0, mats=K.MATS_RECTBOX) and word == NO_PLAN, (tag, word)
        assert_bit_identical(fb, _reference(name, 24, 16, 4), f"{name} 24x16x4 without LDS")


def test_windows_17_15_equal_one_32_sample_render(orc):
    """resume, keep_state and the probe's branch of lane_store on the two-record cold state"""
    import torch

    w, h = 24, 16
    ps, cam = _scene("cornell")
    ds = R.DeviceScene(ps)
    acc = R.Accumulator(w, h, ds, scenes.make_camera(cam, w, h))
    try:
        for window in (17, 15):
            acc.add(window)
            torch.cuda.synchronize()
            assert K.ran(K.last_kernels(ds)[1], **HEADLINE) and _word(ds) == PLANNED, (K.last_kernels(ds), _word(ds))
        fb = acc.resolve()
        torch.cuda.synchronize()
        assert_bit_identical(fb.cpu().numpy(), _reference("cornell", w, h, 32), "windows of 17 + 15 samples")
    finally:
        acc.close()
        ds.close()


def test_the_same_frame_in_three_shards(orc):
    """get_pix indexes a shard's local tiles"""
    w, h, n = 24, 16, 3
    ref = _reference("cornell", w, h, 32)
    parts = []
    for i in range(n):
        part, tag, word = _render("cornell", w, h, 32, shard=(i, n))
        assert K.ran(tag, **HEADLINE) and word == PLANNED, (i, tag, word)
        parts.append(part)
    assert_bit_identical(unshard_reference(np.stack(parts), w, h, n), ref, "three shards of 24x16x32")


def test_infinite_direction_component_through_the_bounce_probe(lib, orc):
    """a ray with an infinite direction component, and its finite twin, through the bounce probe against the oracle.  (No shortcut for
    regular rays was taken in the face test: the products with the normal's zeros stay in resolve_hit and in shade_record alike, so there
    is no second branch to hold to the reference — and a rect or a box is never hit with an infinite component: the hit point is not finite.)"""
    ps, _ = _scene("rect_light")
    ds = R.DeviceScene(ps)
    try:
        recs = (abi.PtBounceIn * 2)()
        for k, d in enumerate(((float("inf"), 0.0, -1.0), (0.1, 0.0, -1.0))):
            recs[k].origin[:] = [0.0, 0.3, 1.0]
            recs[k].dir[:] = list(d)
            recs[k].time = 0.0
            recs[k].rng_state = 4711 + k
            recs[k].attenuation[:] = [1.0, 1.0, 1.0]
        out = (abi.PtBounceOut * 2)()
        abi.check(lib.pt_debug_bounce(ds.handle, recs, out, 2), "pt_debug_bounce")
        orc.set_math(True)
        ref = orc.bounce(ps, recs)
        assert ref[1].status != abi.PT_BOUNCE_MISS, "the finite twin hits the light"
        for k in range(2):
            assert out[k].status == ref[k].status, (k, out[k].status, ref[k].status)
            if ref[k].status != abi.PT_BOUNCE_MISS:
                assert (out[k].hittable, out[k].front_face) == (ref[k].hittable, ref[k].front_face), k
                assert np.float32(out[k].t).view(np.uint32) == np.float32(ref[k].t).view(np.uint32), k
    finally:
        ds.close()
