"""The pool plan on the GPU (pt_device.hpp: PoolPlan; hit_world_range, PLANNED): a rect / box-only scene whose whole list is one slab pool
reaches the pool from its kernel arguments, every other scene walks its run list.  Every frame here is the oracle's bit for bit, and every
case also reads back which kernel ran (pt_debug_last_kernels) and whether it was given the plan (pt_debug_last_pool_plan).  Sizes are the
smallest at which each path can go wrong; every frame and window is a single render, every reference is computed once."""
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
from test_gpu_pool_octants import _far_scene

pytestmark = pytest.mark.gpu

SCENES = {"cornell": S.cornell_scene, "field17": PP.field17, "row": PP.row_of_boxes, "two_pools": PP.two_pools,
          "pool_then_lone_rect": PP.pool_then_lone_rect, "far": _far_scene}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def _reference(name, w, h, spp, depth=50):
    """the oracle's frame (portable math), computed once per case and shared; read-only"""
    from oracle import binding as orc
    orc.load()
    orc.set_math(True)
    ps, cam = _scene(name)
    ref = orc.render(ps, scenes.make_camera(cam, w, h).c, w, h, spp, depth)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _tables(name):
    """(entries, exact entries' offset, octant table's offset) of the scene's first pool, from the blob"""
    blob, n_runs = P.flatten(abi.load_library(), _scene(name)[0])
    off, n, _ = P.pools(blob, n_runs)[0]
    return n, off + 2 * (n + (n & 1)), off + 2 * (n + (n & 1)) + 2 * n


def _render(name, w, h, spp, depth=50, flags=0, shard=(0, 1)):
    """one render of a fresh device scene: (frame, frame-pass tag, plan read-back)"""
    ps, cam = _scene(name)
    ds = R.DeviceScene(ps)
    try:
        fb = R.render_host(w, h, spp, ds, scenes.make_camera(cam, w, h), depth, flags=flags, shard_index=shard[0], shard_count=shard[1])
        return fb, K.last_kernels(ds)[1], PP.last_plan(ds)
    finally:
        ds.close()


def _planned(name, tag, plan, **kernel):
    """the LDS-resident rect / box-only kernel ran, with the plan of the scene's one pool"""
    assert K.ran(tag, lds=1, grid=0, coop=0, mats=K.MATS_RECTBOX, **kernel), tag
    assert plan == (1, *_tables(name)), (plan, _tables(name))


@pytest.mark.parametrize("size,spp", [((64, 48), 8), ((9, 7), 3)], ids=["64x48x8", "9x7x3"])
def test_cornell(orc, size, spp):
    """every box side, the rect, the light, the sky; 9 x 7: two edge tiles, most lanes padding"""
    fb, tag, plan = _render("cornell", *size, spp)
    _planned("cornell", tag, plan, cl=1)
    assert plan[1] == 8
    assert_bit_identical(fb, _reference("cornell", *size, spp), f"cornell {size} x {spp}")


@pytest.mark.parametrize("depth", [1, 2])
def test_cornell_first_bounces(orc, depth):
    """depth 1: the camera's ray alone; depth 2: the first ray that leaves a face"""
    fb, tag, plan = _render("cornell", 64, 48, 8, depth=depth)
    _planned("cornell", tag, plan, cl=1)
    assert_bit_identical(fb, _reference("cornell", 64, 48, 8, depth), f"cornell depth {depth}")


def test_seventeen_entries_two_chunks(orc):
    fb, tag, plan = _render("field17", 48, 32, 4)
    _planned("field17", tag, plan)
    assert plan[1] == 17
    assert_bit_identical(fb, _reference("field17", 48, 32, 4), "17 pooled entries")


def test_more_than_three_candidates_in_a_row(orc):
    """the pool's pass repeated for lanes that used up their three candidates"""
    fb, tag, plan = _render("row", 32, 32, 4)
    _planned("row", tag, plan)
    assert plan[1] == 10
    assert_bit_identical(fb, _reference("row", 32, 32, 4), "a row of boxes inside nested boxes")


@pytest.mark.parametrize("name", ["two_pools", "pool_then_lone_rect"])
def test_lists_one_pool_does_not_cover_walk(orc, name):
    fb, tag, plan = _render(name, 48, 32, 4)
    assert K.ran(tag, lds=1, grid=0, mats=K.MATS_SIMPLE), tag  # (a sphere separates the stretches: not the rect / box-only kernel)
    assert plan[0] == 0, plan
    assert_bit_identical(fb, _reference(name, 48, 32, 4), name)


def test_irregular_lanes_in_regular_waves(orc):
    """2^27 away along x a camera ray's x component is 0, +-8 or +-16: tiles mix irregular rays with regular ones, and a wave with an
    irregular live ray must walk the list although the launch has the plan"""
    fb, tag, plan = _render("far", 33, 33, 4)
    _planned("far", tag, plan)
    ref = _reference("far", 33, 33, 4)
    assert_bit_identical(fb, ref, "far scene, 33 x 33")


def test_shard_one_of_three(orc):
    w, h, n = 64, 48, 3
    part, tag, plan = _render("cornell", w, h, 8, shard=(1, n))
    _planned("cornell", tag, plan, cl=1)
    mine = np.zeros((n, *part.shape), np.float32)
    mine[1] = 1.0
    own = unshard_reference(mine, w, h, n)[..., 0] != 0  # the pixels of shard 1
    got = np.zeros((n, *part.shape), np.float32)
    got[1] = part
    assert own.sum() == (w // 8) * (h // 8) // n * 64
    assert_bit_identical(unshard_reference(got, w, h, n)[own], _reference("cornell", w, h, 8)[own], "shard 1 of 3")


def test_no_lds_walks(orc):
    fb, tag, plan = _render("cornell", 64, 48, 8, flags=abi.PT_FLAG_NO_LDS)
    assert K.ran(tag, lds=0, grid=0, mats=K.MATS_RECTBOX), tag
    assert plan == (0, *_tables("cornell")), plan
    assert_bit_identical(fb, _reference("cornell", 64, 48, 8), "cornell, PT_FLAG_NO_LDS")


def test_sample_windows_of_five_and_three(orc):
    import torch

    ps, cam = _scene("cornell")
    ds = R.DeviceScene(ps)
    acc = R.Accumulator(64, 48, ds, scenes.make_camera(cam, 64, 48))
    try:
        for window in (5, 3):
            acc.add(window)
            torch.cuda.synchronize()
            _planned("cornell", K.last_kernels(ds)[1], PP.last_plan(ds), cl=1)
        fb = acc.resolve()
        torch.cuda.synchronize()
        assert_bit_identical(fb.cpu().numpy(), _reference("cornell", 64, 48, 8), "windows of 5 + 3 samples")
    finally:
        acc.close()
        ds.close()


def test_masked_adaptive_window_over_half_the_tiles(orc):
    import torch

    w, h, spp = 64, 48, 4
    ps, cam = _scene("cornell")
    ds = R.DeviceScene(ps)
    acc = R.Accumulator(w, h, ds, scenes.make_camera(cam, w, h), adaptive=True)
    try:
        mask = np.zeros((h, w), np.uint8)
        ys, xs = np.mgrid[0:h, 0:w]
        mask[((ys // 8) * (w // 8) + xs // 8) % 2 == 0] = 1  # every other tile
        acc.add(spp, torch.from_numpy(mask).cuda())
        torch.cuda.synchronize()
        _planned("cornell", K.last_kernels(ds)[1], PP.last_plan(ds), cl=1)
        fb = acc.resolve().cpu().numpy()
        on = mask != 0
        assert_bit_identical(fb[on], _reference("cornell", w, h, spp)[on], "the window's pixels")
        assert not fb[~on].view(np.uint32).any(), "pixels outside the mask stay at no samples"
    finally:
        acc.close()
        ds.close()
