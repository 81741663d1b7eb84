"""Temporal reprojection (render.TemporalAccumulator: pt_temporal_push) at 1920x1080 with every guide, against two yardsticks in the same
process: pt_variance_denoise (its defaults; one call = a packing prepass + 5 a-trous levels) and a device-to-device copy that moves the
same number of bytes as one push — the push's streaming floor.  One JSON line, stamped with pt_build_id().

The Cornell-style scene (cfg2): frames of --spp samples from one adaptive accumulator continued with next_frame, the camera moving by
--move units per frame, guides from render_aov at --aov-spp; the history is built with three pushes, then the timed pushes alternate
between the last two frames (every timed push has a history to fetch, through a camera that differs from its own).

Bytes one push moves per pixel, counted from the kernel: reads 12 colour + 4 depth + 12 normal + 4 id + 12 variance_in = 44 and the
history, 48 (each record is fetched by up to four neighbouring pixels but comes from memory once); writes 12 + 12 + 4 (colour, variance,
history length) + 48 (the three records) = 76.  168 B per pixel; the copy moves 84 B per pixel in and 84 out.

HIP events on the launch stream around --batch back-to-back calls (one call is ~0.1 ms: a single one would time the clock), divided by
the batch; the three alternate --reps times after a warm-up; medians.

    python tools/temporal_bench.py [--reps 21] [--batch 16] [--spp 4] [--aov-spp 4] [--move 10]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from path_tracer_amd import abi, scenes  # noqa: E402
from path_tracer_amd import render as R  # noqa: E402

W, H = 1920, 1080
PUSH_BYTES_PER_PIXEL = 44 + 48 + 28 + 48


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--aov-spp", type=int, default=4)
    ap.add_argument("--move", type=float, default=10.0)
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    lib = abi.load_library()
    packed, cam_args = scenes.build("cornell")
    lf = cam_args["look_from"]
    cams = [scenes.make_camera(dict(cam_args, look_from=(lf[0] + f * a.move, lf[1], lf[2])), W, H) for f in range(3)]
    ds = R.DeviceScene(packed)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    acc, hist, frames = R.Accumulator(W, H, ds, cams[0], adaptive=True), R.TemporalAccumulator(W, H), []
    for f, cam in enumerate(cams):
        if f:
            acc.next_frame(cam)
        acc.add(a.spp - a.spp // 2).add(a.spp // 2)
        g = R.render_aov(W, H, a.aov_spp, ds, cam, planes=("albedo", "normal", "depth", "id"))
        frames.append(dict(cam=cam, fb=acc.resolve(), var=acc.variance(), **g))
        color, variance, history = hist.push(frames[-1]["fb"], cam, variance=frames[-1]["var"], **g)
    torch.cuda.synchronize()
    carried = float((history > 2.5).float().mean())
    out, vout = torch.empty_like(color), torch.empty_like(color)
    hout = torch.empty_like(history)
    p = abi.PtTemporalParams()
    lib.pt_temporal_params_init(C.byref(p))

    def push(k):
        fr = frames[1 + k % 2]
        abi.check(lib.pt_temporal_push(hist.handle, C.byref(p), C.byref(fr["cam"].c), fr["fb"].data_ptr(), fr["depth"].data_ptr(), fr["normal"].data_ptr(),
                                       fr["id"].data_ptr(), fr["var"].data_ptr(), out.data_ptr(), vout.data_ptr(), hout.data_ptr(), stream), "pt_temporal_push")

    vp = abi.PtVarianceDenoiseParams()
    lib.pt_variance_denoise_params_init(C.byref(vp), W, H)
    scratch = torch.empty(lib.pt_variance_denoise_scratch_floats(W, H), dtype=torch.float32, device="cuda")
    filtered, residual = torch.empty_like(color), torch.empty_like(color)
    last = frames[-1]

    def vdn(k):
        abi.check(lib.pt_variance_denoise(C.byref(vp), color.data_ptr(), variance.data_ptr(), last["albedo"].data_ptr(), last["normal"].data_ptr(),
                                          last["depth"].data_ptr(), filtered.data_ptr(), residual.data_ptr(), scratch.data_ptr(), stream), "pt_variance_denoise")

    half = W * H * PUSH_BYTES_PER_PIXEL // 2
    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")

    def copy(k):
        dst.copy_(src)

    def timed(call):
        torch.cuda.synchronize()
        e0.record()
        for k in range(a.batch):
            call(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.batch

    calls = {"push": push, "variance_denoise": vdn, "copy": copy}
    for c in calls.values():
        timed(c)
    times = {k: [] for k in calls}
    for _ in range(a.reps):  # alternated
        for k, c in calls.items():
            times[k].append(timed(c))
    med = {k: statistics.median(v) for k, v in times.items()}
    moved = W * H * PUSH_BYTES_PER_PIXEL
    print(json.dumps({"tool": "temporal_bench", "build_id": lib.pt_build_id().decode(), "scene": "cornell", "workload": f"{W}x{H}", "spp": a.spp,
                      "aov_spp": a.aov_spp, "move": a.move, "batch": a.batch, "share_of_pixels_with_history_over_2": round(carried, 4),
                      "push_ms": stats(times["push"]), "push_spread_pct": round(100 * (max(times["push"]) - min(times["push"])) / med["push"], 2),
                      "variance_denoise_ms": stats(times["variance_denoise"]), "copy_ms": stats(times["copy"]),
                      "bytes_moved_per_push": moved, "push_gb_per_s": round(moved / med["push"] / 1e6, 1),
                      "copy_gb_per_s": round(moved / med["copy"] / 1e6, 1), "push_over_copy": round(med["push"] / med["copy"], 3),
                      "push_over_one_fifth_of_variance_denoise": round(med["push"] / (med["variance_denoise"] / 5), 3)}), flush=True)
    acc.close()
    hist.close()


if __name__ == "__main__":
    main()
