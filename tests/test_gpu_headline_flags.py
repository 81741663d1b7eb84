"""The lane flags and votes of the headline kernel's loop, whole frames against the oracle bit for bit.  The loop's vote on "every live ray
regular" is scalar arithmetic on two wave masks (the irregular lanes' from make_ctx's comparisons, the live lanes'), a pool of one chunk
is passed without the chunk loop, a larger one is left to the walk, the frame's size reaches camera_ray as floats, and the exact trip
closes inside its last side's statement: every way a lane's flags can change is rendered here at the smallest frame that holds it, and
every case reads back that the kernel it means ran (pt_debug_last_kernels) and which path that kernel took to the pool
(pt_debug_last_pool_word: 2 the planned one-chunk path, 1 a claimed pool it walked, 0 no plan).  Every reference is computed once and
shared, read-only."""
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
from path_tracer_amd.scene import box, lambertian_material, lightsource_material, pack, xy_rect

pytestmark = pytest.mark.gpu

# the headline kernel (csrc/pt_render.hip: headline_kernel): blob, materials and cold lane state in LDS, rects and boxes only, no grid walk
HEADLINE = dict(lds=1, mlds=1, cl=1, coop=0, grid=0, tripool=0, mats=K.MATS_RECTBOX)
PLANNED, WALKED, NO_PLAN = 2, 1, 0  # pt_debug_last_pool_word


def _far_scene():
    """a pooled rect / box scene 2^27 away along x, where floats are 8 or 16 apart: camera rays whose x component is exactly 0 (axis-parallel:
    irregular) next to rays with +-8, +-16 in the same 8 x 8 tile"""
    X = float(2 ** 27)
    cols = [lambertian_material(c) for c in ((0.8, 0.8, 0.8), (0.9, 0.2, 0.2), (0.2, 0.2, 0.9))]
    hs = [box((X - 32, -10, -90), (X - 8, -2, -50), cols[0]), box((X - 8, -4, -80), (X + 16, 6, -60), cols[1]),
          box((X + 16, -10, -100), (X + 48, 10, -70), cols[2]), box((X - 64, -12, -120), (X + 64, -10, -30), cols[0]),
          xy_rect(X - 64, X + 64, -12, 12, -120, lightsource_material((3, 3, 3)))]
    cam = dict(look_from=(X, 0.5, 0.0), look_at=(X, 0.5, -64.0), vup=(0, 1, 0), vfov=24.0, aperture=0.0, focus_dist=64.0, time0=0.0, time1=0.0)
    return pack(hs), cam


def _word(ds):
    out = C.c_int32(-1)
    abi.check(ds.lib.pt_debug_last_pool_word(ds.handle, C.byref(out)), "pt_debug_last_pool_word")
    return out.value


def _lens():
    ps, cam = S.cornell_scene()
    return ps, dict(cam, aperture=20.0)


SCENES = {"cornell": S.cornell_scene, "lens": _lens, "far": _far_scene, "field16": lambda: P.box_field(13), "field17": PP.field17}


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


def _render(name, w, h, spp, depth=50, flags=0, shard=(0, 1)):
    """one render of a fresh device scene: (frame, frame-pass tag, plan read-back + the word the kernel read)"""
    ps, cam = _scene(name)
    ds = R.DeviceScene(ps)
    try:
        fb = R.render_host(w, h, spp, ds, scenes.make_camera(cam, w, h), depth, flags=flags, shard_index=shard[0], shard_count=shard[1])
        return fb, K.last_kernels(ds)[1], (*PP.last_plan(ds), _word(ds))
    finally:
        ds.close()


def _check(name, w, h, spp, depth=50, flags=0, kernel=HEADLINE, entries=8, word=PLANNED):
    fb, tag, plan = _render(name, w, h, spp, depth, flags)
    assert K.ran(tag, **kernel), tag
    assert (plan[0], plan[1], plan[4]) == (int(word != NO_PLAN), entries, word), plan
    assert_bit_identical(fb, _reference(name, w, h, spp, depth), f"{name} {w}x{h}x{spp} depth {depth} flags {flags}")


@pytest.mark.parametrize("size", [(3, 2), (20, 12), (64, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_sizes(orc, size):
    """3 x 2: less than one tile, 58 padding lanes that must never become live; 20 x 12: edge tiles on both axes; 64 x 8: whole tiles only"""
    _check("cornell", *size, 8)


@pytest.mark.parametrize("spp", [1, 2])
def test_one_and_two_samples(orc, spp):
    """a lane's first sample is its last (live -> idle in the iteration that started it), and the one after"""
    _check("cornell", 20, 12, spp)


def test_seventeen_samples_through_the_probe(orc):
    """pt_render at 17 spp on 72 tiles: the cost probe runs the same kernel and the frame pass resumes every pixel where the probe stopped"""
    import torch

    ps, cam = _scene("cornell")
    ds = R.DeviceScene(ps)
    try:
        w, h, spp = 64, 72, 17
        fb = R.render(w, h, spp, ds, scenes.make_camera(cam, w, h))
        torch.cuda.synchronize()
        probe, frame = K.last_kernels(ds)
        assert K.ran(frame, **HEADLINE) and probe == frame and _word(ds) == PLANNED, (probe, frame, _word(ds))
        assert_bit_identical(fb.cpu().numpy(), _reference("cornell", w, h, spp), "cornell 64x72x17 through the probe")
    finally:
        ds.close()


@pytest.mark.parametrize("depth", [1, 2, 50])
def test_depths(orc, depth):
    """depth 1: every path ends in the iteration that began it; 2: the first scattered ray; 50: the reference's"""
    _check("cornell", 20, 12, 8, depth=depth)


def test_shard_one_of_three(orc):
    w, h, n = 40, 24, 3
    part, tag, plan = _render("cornell", w, h, 8, shard=(1, n))
    assert K.ran(tag, **HEADLINE) and plan[4] == PLANNED, (tag, plan)
    mine = np.zeros((n, *part.shape), np.float32)
    mine[1] = 1.0
    own = unshard_reference(mine, w, h, n)[..., 0] != 0  # the pixels of shard 1
    got = np.zeros((n, *part.shape), np.float32)
    got[1] = part
    assert own.sum() == (w // 8) * (h // 8) // n * 64
    assert_bit_identical(unshard_reference(got, w, h, n)[own], _reference("cornell", w, h, 8)[own], "shard 1 of 3")


def test_lens_camera(orc):
    """the non-pinhole branch of camera_ray takes the float width / height too"""
    _check("lens", 20, 12, 8)


def test_axis_parallel_camera_rays(orc):
    """2^27 away along x a camera ray's x component is 0, +-8 or +-16: pixel rays are axis-parallel, their waves irregular — the vote fails
    and the run scans, with plain divisions, render them"""
    _check("far", 33, 33, 4, entries=P.pools(*P.flatten(abi.load_library(), _scene("far")[0]))[0][1])


def test_plain_division(orc):
    """PT_FLAG_NO_FASTDIV: no ray is regular, the irregular lanes' mask is every lane"""
    _check("cornell", 20, 12, 8, flags=abi.PT_FLAG_NO_FASTDIV, word=NO_PLAN)


@pytest.mark.parametrize("name,entries,word", [("field16", 16, PLANNED), ("field17", 17, WALKED)])
def test_one_pool_of_sixteen_and_of_seventeen(orc, name, entries, word):
    """16 entries: one full chunk, passed from the plan without the chunk loop (word 2); 17: two chunks — the plan reports the pool, the
    kernel leaves it to the walk, which scans the runs record by record (word 1).  Both blobs (5.7 and 6.4 KB with their octant tables) stay
    below the 10 KB up to which the cold lane state rides along in LDS: the headline kernel itself renders them."""
    blob, n_runs = P.flatten(abi.load_library(), _scene(name)[0])
    assert [p[1] for p in P.pools(blob, n_runs)] == [entries]
    _check(name, 48, 32, 4, entries=entries, word=word)


def test_sample_windows_5_12_23(orc):
    """[0, 5) [5, 17) [17, 40) through pt_render_accumulate against one 40-sample render"""
    import torch

    w, h = 20, 12
    ps, cam = _scene("cornell")
    ds = R.DeviceScene(ps)
    acc = R.Accumulator(w, h, ds, scenes.make_camera(cam, w, h))
    try:
        for window in (5, 12, 23):
            acc.add(window)
            torch.cuda.synchronize()
            assert K.ran(K.last_kernels(ds)[1], **HEADLINE) and _word(ds) == PLANNED, (K.last_kernels(ds), _word(ds))
        fb = acc.resolve()
        torch.cuda.synchronize()
        assert_bit_identical(fb.cpu().numpy(), _reference("cornell", w, h, 40), "windows of 5 + 12 + 23 samples")
    finally:
        acc.close()
        ds.close()


def test_masked_window_half_of_every_tile(orc):
    """an adaptive window whose mask drops every other pixel of each tile: half the lanes of an active tile ask again and never go live"""
    import torch

    w, h, spp = 24, 16, 4
    ps, cam = _scene("cornell")
    ds = R.DeviceScene(ps)
    acc = R.Accumulator(w, h, ds, scenes.make_camera(cam, w, h), adaptive=True)
    try:
        ys, xs = np.mgrid[0:h, 0:w]
        mask = ((xs + ys) % 2 == 0).astype(np.uint8)
        acc.add(spp, torch.from_numpy(mask).cuda())
        torch.cuda.synchronize()
        assert K.ran(K.last_kernels(ds)[1], **HEADLINE) and _word(ds) == PLANNED, (K.last_kernels(ds), _word(ds))
        fb = acc.resolve().cpu().numpy()
        on = mask != 0
        assert_bit_identical(fb[on], _reference("cornell", w, h, spp)[on], "the window's pixels")
        assert not fb[~on].view(np.uint32).any(), "pixels outside the mask stay at no samples"
    finally:
        acc.close()
        ds.close()
