"""The pool plan's derivation without a device (pt_debug_pool_plan: flatten, the scene's facts, choose_variant, pass_pool_plan — the calls
a render makes): a rect / box-only scene whose first run heads a pool with an octant table that spans every run, rendered by an LDS-resident
kernel compiled for such scenes, gets `one` and the table offsets slab_pool would compute from the aux record's (pool offset, n); every
other scene, kernel or flag leaves `one` clear and walks the list."""
import ctypes as C

import numpy as np
import pytest

import kernel_variant_cases as K
import pool_octant_scenes as P
import pool_plan_scenes as PP
import scenes_small as S
from path_tracer_amd import abi, scenes

W, H, SPP = 64, 48, 8


def _tables(blob, n_runs):
    """(pool offset, n, exact entries, octant table) of the blob's first pool, as pt_device.hpp pool_tables lays them out"""
    off, n, first = P.pools(blob, n_runs)[0]
    x_off = off + 2 * (n + (n & 1))
    return off, n, x_off, x_off + 2 * n, first


def test_entry_points_are_declared(lib):
    assert abi.POOL_PLAN_SYMBOLS == {"pt_debug_last_pool_plan", "pt_debug_pool_plan"} and abi.POOL_PLAN_SYMBOLS <= set(abi.SIGNATURES)
    out = (C.c_int32 * 12)(*([7] * 12))
    assert lib.pt_debug_pool_plan(None, None, None, out) == abi.PT_ERR_INVALID_ARG and list(out) == [7] * 12
    assert lib.pt_debug_last_pool_plan(None, out) == abi.PT_ERR_INVALID_ARG and list(out) == [7] * 12
    assert b"pt_debug_last_pool_plan" in lib.pt_last_error()


@pytest.mark.parametrize("name", ["cornell_small", "cornell_headline"])
def test_cornell_style_scene_is_one_pool_of_eight(lib, name):
    ps, _ = S.cornell_scene() if name == "cornell_small" else scenes.build("cornell")
    blob, n_runs = P.flatten(lib, ps)
    off, n, x_off, oct_off, first = _tables(blob, n_runs)
    assert n == 8 and len(P.pools(blob, n_runs)) == 1
    aux = blob[first - 1].view(np.int32)
    assert aux[1] == n_runs, "the pool spans every run"
    assert first - 1 == oct_off + 16 * (n + (n & 1)), "the octant table ends at the head run's aux record"
    for w, h in ((W, H), (9, 7), (1920, 1080)):
        pl = PP.derived_plan(lib, ps, w, h, SPP)
        assert (pl["one"], pl["n"], pl["x_off"], pl["oct_off"], pl["pool_off"]) == (1, 8, x_off, oct_off, off), pl
        assert pl["scene_allows"] == 1 and pl["lds"] == 1 and pl["mats"] == K.MATS_RECTBOX, pl
        run0 = blob[0].view(np.int32)
        assert (pl["kind"], pl["off"], pl["count"]) == (int(run0[0]), int(run0[1]), int(run0[2])) and pl["off"] == first, pl
        assert pl["bmax_bits"] == int(blob[first - 1].view(np.int32)[0]), pl


def test_seventeen_entries_and_150_boxes(lib):
    ps, _ = PP.field17()
    blob, n_runs = P.flatten(lib, ps)
    off, n, x_off, oct_off, _ = _tables(blob, n_runs)
    pl = PP.derived_plan(lib, ps, 48, 32, 4)
    assert n == 17 and (pl["one"], pl["n"], pl["x_off"], pl["oct_off"]) == (1, 17, off + 36, off + 36 + 34), pl
    ps, _ = K.boxes()  # over 16 KB: the LDS kernel without the material table; 150 boxes would go cooperative
    pl = PP.derived_plan(lib, ps, 48, 32, 4, flags=abi.PT_FLAG_NO_COOP)
    assert (pl["one"], pl["n"], pl["lds"], pl["mats"]) == (1, 150, 1, K.MATS_RECTBOX), pl
    pl = PP.derived_plan(lib, ps, 48, 32, 4)
    assert (pl["one"], pl["scene_allows"], pl["mats"]) == (0, 1, K.MATS_ALL), ("the cooperative kernel walks the list", pl)


@pytest.mark.parametrize("name", ["two_pools", "pool_then_lone_rect"])
def test_lists_one_pool_does_not_cover_are_not_claimed(lib, name):
    ps, _ = getattr(PP, name)()
    blob, n_runs = P.flatten(lib, ps)
    assert len(P.pools(blob, n_runs)) == (2 if name == "two_pools" else 1)
    aux = blob[blob[0].view(np.int32)[1] - 1].view(np.int32)
    assert 0 < aux[1] < n_runs, "run 0 heads a pool that ends before the list does"
    pl = PP.derived_plan(lib, ps, 48, 32, 4)
    assert pl["one"] == 0 and pl["scene_allows"] == 0, pl


def test_pool_without_octant_table_is_not_claimed(lib):
    ps, _ = P.many_boxes(300)
    blob, n_runs = P.flatten(lib, ps)
    (off, n, first), = P.pools(blob, n_runs)
    assert n == 300 and first - 1 == off + 4 * n, "a pool of 300, no octant table"
    pl = PP.derived_plan(lib, ps, 48, 32, 4)
    assert (pl["one"], pl["scene_allows"], pl["n"], pl["lds"], pl["mats"]) == (0, 0, 300, 0, K.MATS_RECTBOX), pl


@pytest.mark.parametrize("flags,lds", [(abi.PT_FLAG_NO_LDS, 0), (abi.PT_FLAG_NO_FASTDIV, 1), (abi.PT_FLAG_FORCE_STREAM, 0)],
                         ids=["no_lds", "no_fastdiv", "force_stream"])
def test_flags_that_take_the_walk(lib, flags, lds):
    ps, _ = S.cornell_scene()
    pl = PP.derived_plan(lib, ps, W, H, SPP, flags=flags)
    assert (pl["one"], pl["scene_allows"], pl["n"], pl["lds"]) == (0, 1, 8, lds), pl


def test_scenes_without_a_pool_or_of_other_kinds(lib):
    pl = PP.derived_plan(lib, S.cornell_scene()[0], W, H, SPP, tuning=abi.tuning(slab_pools=-1))
    assert (pl["one"], pl["scene_allows"], pl["n"], pl["lds"], pl["mats"]) == (0, 0, 0, 1, K.MATS_RECTBOX), pl
    for extra, mats in (("sphere", K.MATS_SIMPLE), ("metal", K.MATS_ALL)):
        pl = PP.derived_plan(lib, K.cornell(extra)[0], W, H, SPP)
        assert pl["one"] == 0 and pl["mats"] == 0, (extra, pl)  # (another kernel family's business: not asked)
    pl = PP.derived_plan(lib, S.ALL["mixed"]()[0], W, H, SPP)
    assert pl["one"] == 0, pl
