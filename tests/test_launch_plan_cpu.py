"""The launcher's geometry rules (csrc/pt_render.hip: plan_pass) without a GPU, through pt_debug_plan_pass: plain integers in, plain integers out.

(a) Worked rows: numbers that follow from the rules as their comments in plan_pass state them, computed by hand below — and the rows of
    tests/golden/launch_decisions.json (recorded on an MI355X) whose kernel facts are known, which the planner must reproduce here.
(b) Properties over a sweep of pixel counts on a "chip" of 2 CUs with 1 .. 8 resident workgroups per CU, where every regime boundary is a
    few hundred pixels away.
(c) pixel_footprint — KArgs.foot of the camera rays' candidate cache — against the arithmetic it was factored out of, in a stand-alone
    host program under AddressSanitizer + UBSan (tests/cpp/footprint_main.cpp).
"""
import ctypes as C
import itertools
import json
import os
import subprocess
from pathlib import Path

import pytest

from path_tracer_amd import abi

ROOT = Path(__file__).resolve().parent.parent
TG, PG, FAST = abi.PT_FLAG_TILE_GRANULAR, abi.PT_FLAG_PIXEL_GRANULAR, abi.PT_FLAG_FAST_RNG
WAVES = 4  # waves per workgroup of 256 threads


def plan(lib, pixels, **facts):
    """pt_debug_plan_pass of a pass over `pixels` local pixels; defaults: 256 CUs, 4 workgroups per CU, 256 threads, one work unit per
    tile, 16 spp, whole tiles per wave, a frame pass without order."""
    f = dict(num_cus=256, per_cu=4, block_threads=64 * WAVES, n_local_pixels=pixels, launch_units=pixels // 64, samples=16, tile_granular=1)
    assert not set(facts) - set(abi.PLAN_FACTS), facts
    f.update(facts)
    words = (C.c_int64 * len(abi.PLAN_FACTS))(*[int(f.get(name, 0)) for name in abi.PLAN_FACTS])
    out = (C.c_int32 * len(abi.PLAN_WORDS))()
    abi.check(lib.pt_debug_plan_pass(words, out), "pt_debug_plan_pass")
    pl = dict(zip(abi.PLAN_WORDS, out))
    # what pt_debug_last_launch reports is the plan itself
    assert (pl["last_workgroups"], pl["last_lanes_cap"], pl["last_heavy_pixels"]) == (pl["workgroups"], pl["lanes_cap"], pl["heavy_pixels"])
    assert pl["last_queued_walk"] == (1 if f.get("queued_walk") else 0)
    assert pl["n_waves_resident"] == pl["workgroups"] * (f["block_threads"] // 64)
    return pl


def test_entry_point_is_declared_and_optional():
    assert abi.PLAN_SYMBOLS == {"pt_debug_plan_pass"} and abi.PLAN_SYMBOLS <= set(abi.SIGNATURES)
    assert not abi.PLAN_SYMBOLS & (abi.ACCUM_SYMBOLS | abi.ADAPTIVE_SYMBOLS | abi.AOV_SYMBOLS | abi.DENOISE_SYMBOLS)
    assert abi.SIGNATURES["pt_debug_plan_pass"] == (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int32)])
    assert len(abi.PLAN_FACTS) == 20 and len(abi.PLAN_WORDS) == 14
    text = (ROOT / "include" / "pt_render.h").read_text()
    assert "int pt_debug_plan_pass(const int64_t facts[20], int32_t out[14]);" in text


def test_bad_facts_are_refused(lib):
    out = (C.c_int32 * 14)(*[7] * 14)
    good = dict(zip(abi.PLAN_FACTS, [2, 4, 256, 0, 1, 0, 0, 0, 0, 0, 0, 10, 640, 16, 0, 0, 0, 1, 0, 0]))
    assert lib.pt_debug_plan_pass(None, out) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_debug_plan_pass((C.c_int64 * 20)(*good.values()), None) == abi.PT_ERR_INVALID_ARG
    for name, bad in (("num_cus", 0), ("per_cu", 0), ("per_cu", -1), ("block_threads", 0), ("block_threads", 100), ("block_threads", 2048),
                      ("n_local_pixels", -64), ("n_local_pixels", 1 << 31), ("launch_units", -1), ("samples", 0), ("scatter_p", -1), ("fast_chunks", -1)):
        assert lib.pt_debug_plan_pass((C.c_int64 * 20)(*dict(good, **{name: bad}).values()), out) == abi.PT_ERR_INVALID_ARG, (name, bad)
        assert b"pt_debug_plan_pass" in lib.pt_last_error()
    assert list(out) == [7] * 14
    assert lib.pt_debug_plan_pass((C.c_int64 * 20)(*good.values()), out) == abi.PT_OK


# ---- (a) worked rows ---------------------------------------------------------------------------------------------------------------

def test_grid_kernel_rows_on_256_cus(lib):
    """Grid kernel, 4 workgroups per CU: 1024 resident workgroups, 4 096 waves, 262 144 lanes.
    1080p whole (2 073 600 pixels): 16 rho = 126.6 -> 127 with the rounding term -> (127 + 2) / 4 * 4 = 128 -> 64: whole tiles; rho = 7.9 >= 6:
      no narrow head; 32 400 tiles / 4 waves = 8 100 workgroups wanted -> the 1024 resident ones.
    a third (691 200): 16 rho = 42.2 -> 42 -> 44 > 24 -> 64; rho = 2.64 in [1.5, 6): head = min(4 x 256, 10 800 / 2) = 1024 tiles = 65 536 pixels.
    an eighth (259 200): 16 rho = 15.8 -> 16 -> (16 + 2) / 4 * 4 = 16 lanes, single pixels; ceil(259 200 / (16 x 4)) = 4 050 -> 1024 workgroups."""
    whole = plan(lib, 2_073_600, use_grid=1, has_order=1)
    assert (whole["workgroups"], whole["lanes_cap"], whole["heavy_pixels"], whole["tile_granular"]) == (1024, 64, 0, 1)
    third = plan(lib, 691_200, use_grid=1, has_order=1)
    assert (third["lanes_cap"], third["heavy_pixels"], third["heavy_lanes"], third["tile_granular"]) == (64, 4 * 256 * 64, 16, 1)
    assert plan(lib, 691_200, use_grid=1, has_order=1, probe=1)["heavy_pixels"] == 0   # the probe pass itself: no order yet to cut a head from
    assert plan(lib, 691_200, use_grid=1, has_order=0)["heavy_pixels"] == 0
    eighth = plan(lib, 259_200, use_grid=1)
    assert (eighth["workgroups"], eighth["lanes_cap"], eighth["tile_granular"], eighth["heavy_pixels"]) == (1024, 16, 0, 0)
    assert plan(lib, 259_200, use_grid=1, has_order=1)["heavy_pixels"] == 0            # (no head under a lanes cap)


def test_headline_kernel_rows_on_256_cus(lib):
    """Headline kernel, 7 workgroups per CU, chain-bound: the bound is 1.15 x 7 x 4 x 256 = 8 243.2 work units.
    8 100 tiles (a quarter of 1080p) < the bound: four per CU = 1024 resident, 2 025 wanted -> 1024.  10 800 (a third) >= the bound: seven per
    CU = 1792, 2 700 wanted -> 1792.  4 050 (an eighth): four per CU, ceil(4 050 / 4) = 1013 wanted -> 1013."""
    for units, workgroups in ((8100, 1024), (10800, 1792), (4050, 1013), (8243, 1024), (8244, 1792)):
        pl = plan(lib, units * 64, per_cu=7, chain_bound=1)
        assert (pl["workgroups"], pl["lanes_cap"], pl["heavy_pixels"]) == (workgroups, 64, 0), units
        # 16 spp, frame pass: priorities from the middle of the queue on, thresholds samples / 8, / 4, / 2
        assert (pl["prio_onset"], pl["prio_t1"], pl["prio_t2"], pl["prio_t3"]) == (units * 64 // 2, 2, 4, 8), units
    zero = (0, 0, 0, 0)
    prios = lambda **kw: tuple(plan(lib, 8100 * 64, per_cu=7, chain_bound=1, **kw)[k] for k in ("prio_onset", "prio_t1", "prio_t2", "prio_t3"))  # noqa: E731
    assert prios(samples=8) == zero and prios(samples=15) == zero and prios(probe=1) == zero
    assert prios(no_chain_prio=1) == zero and prios(tile_granular=0) == zero and prios(fast_chunks=2) == zero
    assert plan(lib, 8100 * 64, per_cu=7, chain_bound=0)["prio_t1"] == 0
    assert prios(samples=1024) == (8100 * 32, 128, 256, 512)


def test_recorded_rows_follow_from_the_planner(lib):
    """tests/golden/launch_decisions.json: the 1080p rows of the headline scene (their kernel: chain-bound, 7 workgroups per CU — 1792 / 256,
    the whole frame's row) and of the 496-hittable scene under the queued walk (4 per CU), with and without a probe."""
    golden = json.loads((ROOT / "tests" / "golden" / "launch_decisions.json").read_text())
    cus, rows, tiles = golden["cus"], golden["rows"], 240 * 135
    per_cu = rows["cornell-1080p-0of1-16spp"]["launch"][0] // cus
    for n, spp in itertools.product((1, 2, 3, 4, 6, 8), (16, 8)):
        local = (tiles + n - 1) // n
        pl = plan(lib, local * 64, num_cus=cus, per_cu=per_cu, chain_bound=1, samples=spp, has_order=spp >= 16)
        assert [pl[k] for k in abi.PLAN_WORDS[10:]] == rows[f"cornell-1080p-0of{n}-{spp}spp"]["launch"], (n, spp)
    for name, local in (("smoke-1080p-0of1", tiles), ("smoke-1080p-0of3", tiles // 3), ("smoke-1080p-0of8", tiles // 8), ("smoke-4k-0of8", 480 * 270 // 8)):
        pl = plan(lib, local * 64, num_cus=cus, per_cu=4, use_grid=1, queued_walk=1, has_order=1)
        assert [pl[k] for k in abi.PLAN_WORDS[10:]] == rows[name]["launch"], name


# ---- (b) properties on a chip of 2 CUs --------------------------------------------------------------------------------------------

CUS = 2
PIXELS = sorted(set(range(64, 64 * 130, 64)) | {64 * 150, 64 * 200, 64 * 256, 64 * 400, 64 * 1000})


def ceil_div(a, b):
    return -(-a // b)


def test_lanes_cap_and_narrow_head_properties(lib):
    for per_cu, pixels in itertools.product(range(1, 9), PIXELS):
        lanes = per_cu * CUS * WAVES * 64
        rho = pixels / lanes
        modes = ((0, 0), (0, -1), (0, 8), (TG, 0), (PG, 0), (FAST, 0))  # (flags, PtTuning.lanes_cap)
        for (flags, knob_cap), knob_heavy, order, probe, granular in itertools.product(modes, (0, -1, 3), (0, 1), (0, 1), (0, 1)):
            pl = plan(lib, pixels, num_cus=CUS, per_cu=per_cu, use_grid=1, flags=flags, lanes_cap=knob_cap, heavy_tiles=knob_heavy, has_order=order,
                      probe=probe, tile_granular=granular)
            where = (per_cu, pixels, flags, knob_cap, knob_heavy, order, probe, granular, pl)
            cap = pl["lanes_cap"]
            assert cap == 64 or (cap % 4 == 0 and 4 <= cap <= 24) or cap == knob_cap, where
            if flags or knob_cap < 0:  # the flags and lanes_cap = -1 keep what they ask for
                assert cap == 64 and pl["tile_granular"] == granular and pl["heavy_pixels"] == 0, where
            if cap < 64:
                assert pl["tile_granular"] == 0 and pl["workgroups"] <= per_cu * CUS, where
                assert pl["workgroups"] == min(per_cu * CUS, ceil_div(pixels, cap * WAVES)), where
            else:
                assert pl["tile_granular"] == granular, where
            if knob_cap == 0 and not flags:  # the rule: 16 rho to the nearest integer, that to the nearest multiple of 4, whole tiles beyond 24
                nearest = (16 * pixels + lanes // 2) // lanes
                assert cap == (64 if nearest >= 26 else max(4, (nearest + 2) // 4 * 4)), where
            if pl["heavy_pixels"]:
                assert cap == 64 and order and not probe and (1.5 <= rho < 6.0 or knob_heavy > 0), where
                assert pl["heavy_lanes"] == 16 and pl["heavy_pixels"] % 64 == 0 and pl["heavy_pixels"] // 64 <= pixels // 64 // 2, where
            else:
                assert pl["heavy_lanes"] == 64, where
            if not flags and knob_cap >= 0 and cap == 64 and granular and order and not probe and knob_heavy == 0:
                head = min(4 * CUS, pixels // 64 // 2) if 1.5 <= rho < 6.0 else 0
                assert pl["heavy_pixels"] == head * 64, where
    # no scatter stride goes with a narrow head or the 16 rho cap
    for pixels in PIXELS:
        pl = plan(lib, pixels, num_cus=CUS, per_cu=4, use_grid=1, has_order=1, scatter_p=7, tile_granular=0)
        assert pl["heavy_pixels"] == 0, (pixels, pl)


def test_four_workgroups_per_cu_applies_exactly_when_its_conditions_hold(lib):
    for per_cu, pixels in itertools.product(range(1, 9), PIXELS):
        units = pixels // 64
        for chain, knob, split, scatter in itertools.product((0, 1), (0, 2, 6), (0, 1), (0, 5)):
            pl = plan(lib, pixels, num_cus=CUS, per_cu=per_cu, chain_bound=chain, blocks_per_cu=knob, has_split=split, scatter_p=scatter,
                      tile_granular=0 if scatter else 1)
            capped = chain and not knob and not split and not scatter and units < 1.15 * per_cu * WAVES * CUS
            resident = (min(per_cu, 4) if capped else min(per_cu, knob) if knob else per_cu) * CUS
            if scatter:
                wanted = ceil_div(pixels, 64 * WAVES) * 64
            else:
                wanted = resident if split else ceil_div(units, WAVES)
            assert pl["workgroups"] == max(1, min(wanted, resident)), (per_cu, pixels, chain, knob, split, scatter, pl)


def test_scattered_launches_share_the_pixels_out_evenly(lib):
    """scatter_p > 0 (the triangle-pool kernels): a wave per pixel — in whole groups of 64 workgroups — up to the chip, and lanes_cap =
    ceil(pixels / waves) clamped to [1, 64].
    "Every wave gets at least one pixel" does NOT hold for the rule as it stands, which this refactor keeps: it launches ceil(pixels / 256) x 64
    workgroups of 4 waves, i.e. the pixel count rounded UP to a multiple of 256 waves, so a launch whose pixel count is not such a multiple has up
    to 255 waves more than pixels (one tile, 64 pixels: 256 waves where the chip holds them).  Asserted here: waves <= pixels where 256 divides
    the pixel count, and waves < pixels + 256 otherwise — the rule, not the property."""
    for per_cu, pixels in itertools.product(range(1, 9), PIXELS + [64 * 5000]):
        for flags, knob_cap in ((0, 0), (0, 8), (FAST, 0)):
            pl = plan(lib, pixels, num_cus=CUS, per_cu=per_cu, scatter_p=3, tile_granular=0, flags=flags, lanes_cap=knob_cap)
            waves = pl["n_waves_resident"]
            assert pl["workgroups"] <= per_cu * CUS and waves < pixels + 64 * WAVES, (per_cu, pixels, pl)
            if pixels % (64 * WAVES) == 0:
                assert waves <= pixels, (per_cu, pixels, pl)
            assert pl["lanes_cap"] == min(64, max(1, ceil_div(pixels, waves))), (per_cu, pixels, pl)
            assert pl["tile_granular"] == 0 and pl["heavy_pixels"] == 0


# ---- (c) the footprint function, stand-alone under the sanitizers ------------------------------------------------------------------

def test_pixel_footprint_under_asan_ubsan(tmp_path):
    """tests/cpp/footprint_main.cpp includes the launcher's source as host code, and compares pixel_footprint with the lines it replaced,
    bit for bit, for the Cornell camera at 1920 x 1080 and three more cameras."""
    exe = tmp_path / "footprint_main"
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++20", "-O1", "-g", "--cuda-host-only", "-cuid=footprint", "-ffp-contract=off", "-fno-fast-math", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-Xarch_host", "-fno-sanitize-recover=undefined", "-Wno-unused-function", "-Wno-unused-variable", "-x", "hip",
           str(ROOT / "tests" / "cpp" / "footprint_main.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert out.returncode == 0 and "FOOTPRINT_OK" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
