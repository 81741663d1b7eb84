"""The launch decisions of launch_render that the library reports (csrc/pt_render.hip: choose_variant, plan_pass and the pass sequence),
replayed against a recording.  Not among the reported words: the chain priorities (prio_onset, prio_t1..3) — the chain_priority = -1 row and
the 8 spp rows pin the rest of such a launch, the priorities themselves are held by tests/test_launch_plan_cpu.py alone.

A row renders one small frame and reads back what the launcher decided: pt_debug_last_launch (workgroups, lanes_cap, heavy_pixels,
queued walk), pt_debug_last_kernels (the probe pass's and the frame pass's kernel) and pt_debug_schedule (tiles through the wide phase,
lanes per pixel there).  tests/golden/launch_decisions.json holds the same words as recorded on an MI355X BEFORE the launcher was split
into plan_pass / enqueue_pass: a row must match its recording exactly.  The decisions depend on the chip's CU count, which the recording
carries: on a device with another count the rows skip (on an MI355X none does).  No image is compared here — tests/test_gpu_kernel_variants.py
and tests/test_gpu_parity.py hold the images to the oracle.

The rows are the smallest frames that reach each regime of the rules on 256 CUs, at 16 spp where a probe pass is wanted (samples / 16 >= 1)
and 8 spp where not, depth 4.  A launcher change that moves a decision ON PURPOSE records again:  python tests/test_gpu_launch_decisions.py
"""
import ctypes as C
import functools
import json
import sys
from pathlib import Path

import pytest

if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import kernel_variant_cases as K
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "launch_decisions.json"
DEPTH = 4
HD, UHD, SMALL = (1920, 1080), (3840, 2160), (400, 225)
F = abi


@functools.lru_cache(maxsize=None)
def scene(name):
    if name in ("cornell", "smoke"):
        return scenes.build(name)
    if name == "tris":  # the triangle-pool recipe of tests/kernel_variant_cases.py (tuning tri_min_run = 256: what tri_pools() sets)
        return K.tris()
    if name == "coop":  # its cooperative recipe: 300 spheres under PT_FLAG_FORCE_COOP
        return K.field(300)
    raise KeyError(name)


def frame(scene_name, size, spp, shards=1, flags=0, **tuning):
    return dict(kind="frame", scene=scene_name, size=size, spp=spp, shards=shards, flags=flags, tuning=tuning)


CASES = {}
for n in (1, 2, 3, 4, 6, 8):
    CASES[f"cornell-1080p-0of{n}-16spp"] = frame("cornell", HD, 16, n)
    CASES[f"cornell-1080p-0of{n}-8spp"] = frame("cornell", HD, 8, n)  # no probe, no priorities
CASES["cornell-400x225"] = frame("cornell", SMALL, 16)
CASES["cornell-1080p-blocks_per_cu=2"] = frame("cornell", HD, 16, blocks_per_cu=2)
CASES["cornell-1080p-0of4-blocks_per_cu=2"] = frame("cornell", HD, 16, 4, blocks_per_cu=2)
CASES["cornell-1080p-chain_priority=-1"] = frame("cornell", HD, 16, chain_priority=-1)
CASES["smoke-400x225"] = frame("smoke", SMALL, 16)  # rho ~ 0.3: a small lanes_cap
for n in (1, 3, 8):
    CASES[f"smoke-1080p-0of{n}"] = frame("smoke", HD, 16, n)
CASES["smoke-4k-0of8"] = frame("smoke", UHD, 16, 8)  # rho ~ 4: the narrow head
for v in (-1, 8):
    CASES[f"smoke-1080p-0of8-lanes_cap={v}"] = frame("smoke", HD, 16, 8, lanes_cap=v)
for v in (-1, 7):
    CASES[f"smoke-1080p-0of3-heavy_tiles={v}"] = frame("smoke", HD, 16, 3, heavy_tiles=v)
for v in (1, 2):
    CASES[f"smoke-1080p-grid_walk={v}"] = frame("smoke", HD, 16, grid_walk=v)
    CASES[f"smoke-1080p-0of8-grid_walk={v}"] = frame("smoke", HD, 16, 8, grid_walk=v)
for name, flag in (("tile_granular", F.PT_FLAG_TILE_GRANULAR), ("pixel_granular", F.PT_FLAG_PIXEL_GRANULAR), ("force_stream", F.PT_FLAG_FORCE_STREAM)):
    CASES[f"smoke-1080p-0of8-{name}"] = frame("smoke", HD, 16, 8, flags=flag)
CASES["smoke-1080p-0of3-no_lpt"] = frame("smoke", HD, 16, 3, flags=F.PT_FLAG_NO_LPT)
CASES["smoke-1080p-0of8-no_lpt"] = frame("smoke", HD, 16, 8, flags=F.PT_FLAG_NO_LPT)
CASES["smoke-1080p-0of8-fast_rng-128spp"] = frame("smoke", HD, 128, 8, flags=F.PT_FLAG_FAST_RNG)
for size in ((64, 36), (640, 360)):  # fewer pixels than lanes; more
    for mode in (-1, 0, 1):
        CASES[f"tris-{size[0]}x{size[1]}-scatter_mode={mode}"] = frame("tris", size, 16, tri_min_run=256, scatter_mode=mode)
COOP_SIZE = (128, 64)  # 128 tiles: a probe pass, and with it the wide phase
CASES["coop"] = frame("coop", COOP_SIZE, 16, flags=F.PT_FLAG_FORCE_COOP)
CASES["coop-no_split"] = frame("coop", COOP_SIZE, 16, flags=F.PT_FLAG_FORCE_COOP | F.PT_FLAG_NO_SPLIT)
CASES["coop-split_tiles=3"] = frame("coop", COOP_SIZE, 16, flags=F.PT_FLAG_FORCE_COOP, split_tiles_mode=1, split_tiles=3)
CASES["coop-split_tiles=-1"] = frame("coop", COOP_SIZE, 16, flags=F.PT_FLAG_FORCE_COOP, split_tiles_mode=1, split_tiles=-1)
# Sample windows (pt_render_accumulate) on the shard whose frame launch has a narrow head — which needs a tile order: the second window
# is too short to probe and shows the head only because it reuses the accumulator's order.  Two rows: after 16 spp, after 4 more.
CASES["window-16spp"] = dict(kind="windows", scene="smoke", size=HD, shards=3, windows=(16,))
CASES["window-16spp-then-4spp"] = dict(kind="windows", scene="smoke", size=HD, shards=3, windows=(16, 4))
# One masked window of an adaptive accumulator (pt_adaptive_window) over the bottom quarter of the whole frame's tiles
CASES["masked-window-quarter"] = dict(kind="masked", scene="smoke", size=HD, spp=16)


def decisions(torch, ds):
    torch.cuda.synchronize()
    launch, kernels, schedule = (C.c_int32 * 4)(), (C.c_int32 * 24)(), (C.c_int32 * 2)()
    abi.check(ds.lib.pt_debug_last_launch(ds.handle, launch), "pt_debug_last_launch")
    abi.check(ds.lib.pt_debug_last_kernels(ds.handle, kernels), "pt_debug_last_kernels")
    abi.check(ds.lib.pt_debug_schedule(ds.handle, schedule), "pt_debug_schedule")
    return dict(launch=list(launch), kernels=list(kernels), schedule=list(schedule))


def run_case(torch, case):
    ps, cam_args = scene(case["scene"])
    w, h = case["size"]
    cam = scenes.make_camera(cam_args, w, h)
    tuning = case.get("tuning")
    ds = R.DeviceScene(ps, abi.tuning(**tuning) if tuning else None)
    try:
        if case["kind"] == "frame":
            R.render(w, h, case["spp"], ds, cam, DEPTH, flags=case["flags"], shard_index=0, shard_count=case["shards"])
        elif case["kind"] == "windows":
            acc = R.Accumulator(w, h, ds, cam, DEPTH, shard_index=0, shard_count=case["shards"])
            for n in case["windows"]:
                acc.add(n)
            torch.cuda.synchronize()
            acc.close()
        else:
            acc = R.Accumulator(w, h, ds, cam, DEPTH, adaptive=True)
            mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
            mask[: h // 4] = 1
            acc.add(case["spp"], mask)
            torch.cuda.synchronize()
            acc.close()
        return decisions(torch, ds)
    finally:
        ds.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_recording_covers_the_matrix(golden):
    assert sorted(golden["rows"]) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_decisions_are_the_recorded_ones(torch, golden, name):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != golden["cus"]:
        pytest.skip(f"recorded on {golden['cus']} CUs, this device has {cus}: the decisions depend on the count")
    got = run_case(torch, CASES[name])
    print(name, got)
    assert got == golden["rows"][name]


def record():
    import torch
    assert torch.cuda.is_available(), "the recorder needs the GPU box"
    rows = {name: run_case(torch, case) for name, case in CASES.items()}
    body = ",\n".join(f'  {json.dumps(name)}: {json.dumps(row)}' for name, row in rows.items())
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else GOLDEN
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(f'{{"cus": {torch.cuda.get_device_properties(0).multi_processor_count},\n "rows": {{\n{body}\n }}}}\n')
    print(f"recorded {len(rows)} rows to {out}")


if __name__ == "__main__":
    record()
