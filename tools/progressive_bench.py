"""Progressive rendering (render.Accumulator / pt_render_accumulate): what a frame costs when it is rendered in sample windows, against
pt_render of the same frame in the same process.  One JSON line per case, stamped with pt_build_id().

Each timing brackets the whole sequence of windows (the last window's end included; no resolve in between) with device events and a
synchronise, after a warm-up of the same shape; the window sequence and the one-shot render alternate, `--reps` times each, and the
lines report the median and the spread.  The resolve and fused resolve + tonemap kernels are timed on their own (cfg2's frame).

    python tools/progressive_bench.py [--cases cfg2,cfg3,cfg5,resolve] [--reps 5]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from path_tracer_amd import abi, scenes  # noqa: E402
from path_tracer_amd import render as R  # noqa: E402

CONFIGS = {"cfg2": ("cornell", 1920, 1080, 1024, (1, 2, 4, 8, 16, 64)),
           "cfg3": ("smoke", 1920, 1080, 1024, (1, 8)),
           "cfg5": ("triangles", 1920, 1080, 256, (1, 8))}


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="cfg2,cfg3,cfg5,resolve")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    build = abi.load_library().pt_build_id().decode()
    cases = a.cases.split(",")
    for cfg in [c for c in cases if c in CONFIGS]:
        scene, W, H, spp, splits = CONFIGS[cfg]
        packed, cam_args = scenes.build(scene)
        cam = scenes.make_camera(cam_args, W, H)
        ds = R.DeviceScene(packed)
        ds.reserve(W, H, spp)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        reps = a.reps if scene != "triangles" else max(2, a.reps // 2)
        for k in splits:
            step = spp // k
            acc = R.Accumulator(W, H, ds, cam)

            def seq():
                acc.reset()
                for _ in range(k):
                    acc.add(step)

            def one():
                R.render(W, H, spp, ds, cam, out=out)

            seq()  # warm-up of the same shapes (workspaces sized, occupancy cached)
            one()
            t_seq, t_one = [], []
            for _ in range(reps):  # alternated
                t_seq.append(timed(torch, seq))
                t_one.append(timed(torch, one))
            same = bool(torch.equal(acc.resolve().view(torch.int32), out.view(torch.int32)))
            acc.close()
            ms, m1 = statistics.median(t_seq), statistics.median(t_one)
            print(json.dumps({"tool": "progressive_bench", "build_id": build, "case": cfg, "workload": f"{W}x{H}x{spp}", "scene": scene,
                              "windows": k, "window_spp": step, "windows_ms": stats(t_seq), "pt_render_ms": stats(t_one),
                              "excess_ms": round(ms - m1, 3), "excess_per_extra_window_ms": round((ms - m1) / (k - 1), 3) if k > 1 else None,
                              "resolve_equals_pt_render": same}), flush=True)
    if "resolve" in cases:
        packed, cam_args = scenes.build("cornell")
        W, H = 1920, 1080
        cam = scenes.make_camera(cam_args, W, H)
        acc = R.Accumulator(W, H, R.DeviceScene(packed), cam)
        acc.add(4)
        fb = acc.resolve()
        acc.tonemap_rgb8()
        t_res = [timed(torch, lambda: acc.resolve(out=fb)) for _ in range(20)]
        t_tm = [timed(torch, acc.tonemap_rgb8) for _ in range(20)]
        t_sep = [timed(torch, lambda: R.tonemap_rgb8(acc.resolve(out=fb))) for _ in range(20)]
        acc.close()
        for what, xs in (("resolve", t_res), ("tonemap_rgb8_fused", t_tm), ("resolve_then_tonemap_rgb8", t_sep)):
            print(json.dumps({"tool": "progressive_bench", "build_id": build, "case": what, "workload": f"{W}x{H}", "bytes_read": W * H * 12,
                              "time": stats(xs)}), flush=True)


if __name__ == "__main__":
    main()
