"""The variance-guided denoiser (render.denoise_variance: pt_variance_estimate + pt_variance_denoise) at 1920x1080 against pt_denoise, its
yardstick, in the same process on the same frame.  One JSON line per read path, stamped with pt_build_id().  The Cornell-style scene
(cfg2) on an ADAPTIVE accumulator after two windows of --window samples, the guides of render_aov at --aov-spp, then

  estimate  pt_variance_estimate: HIP events on the launch stream around the library call alone
  filter    pt_variance_denoise with the default parameters (5 iterations, every guide, demodulated, variance_out written): events
            around the library call alone (scratch, out and variance_out allocated once)
  by step   the same call at 1 ... 5 iterations; the cost of the iteration with step 2^(n-1) is the difference of the medians at n and
            n - 1 iterations (the call at 1 iteration carries the packing prepass, reported with step 1)
  plain     pt_denoise with ITS default parameters over the same resolved frame and guides, timed the same way, alternated with the rest

for each read path of --paths: `default` (LDS-staged tiles for the steps 1 and 2, global memory beyond) and `global`
(PT_VDENOISE_NO_LDS) — the A/B.  The two paths must give the same bits: checked here.  After a warm-up the paths and the yardstick
alternate `--reps` times per iteration count.

    python tools/variance_denoise_bench.py [--reps 9] [--window 8] [--aov-spp 16] [--paths default,global]
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
PATH_FLAGS = {"default": 0, "global": abi.PT_VDENOISE_NO_LDS}


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--aov-spp", type=int, default=16)
    ap.add_argument("--paths", default="default,global")
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    lib = abi.load_library()
    build = lib.pt_build_id().decode()
    packed, cam_args = scenes.build("cornell")
    cam = scenes.make_camera(cam_args, W, H)
    ds = R.DeviceScene(packed)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    acc = R.Accumulator(W, H, ds, cam, adaptive=True)
    acc.add(a.window).add(a.window)
    fb = acc.resolve()
    var = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    planes = R.render_aov(W, H, a.aov_spp, ds, cam, planes=("albedo", "normal", "depth"))
    torch.cuda.synchronize()

    def timed(call):
        torch.cuda.synchronize()
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def estimate():
        return timed(lambda: abi.check(lib.pt_variance_estimate(acc.handle, var.data_ptr(), stream), "pt_variance_estimate"))

    estimate()
    t_est = [estimate() for _ in range(a.reps)]
    out, vout, plain_out = (torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(3))
    scratch = torch.empty(lib.pt_variance_denoise_scratch_floats(W, H), dtype=torch.float32, device="cuda")
    plain_scratch = torch.empty(lib.pt_denoise_scratch_floats(W, H), dtype=torch.float32, device="cuda")
    guides = [planes[k].data_ptr() for k in ("albedo", "normal", "depth")]

    def filt(iterations, flags):
        p = abi.PtVarianceDenoiseParams()
        lib.pt_variance_denoise_params_init(C.byref(p), W, H)
        p.iterations = iterations
        p.flags |= flags
        ms = timed(lambda: abi.check(lib.pt_variance_denoise(C.byref(p), fb.data_ptr(), var.data_ptr(), *guides, out.data_ptr(), vout.data_ptr(),
                                                             scratch.data_ptr(), stream), "pt_variance_denoise"))
        which = (C.c_int32 * 8)()
        abi.check(lib.pt_debug_last_variance_denoise(which), "pt_debug_last_variance_denoise")
        return ms, list(which)

    def plain(iterations):
        p = abi.PtDenoiseParams()
        lib.pt_denoise_params_init(C.byref(p), W, H)
        p.iterations = iterations
        return timed(lambda: abi.check(lib.pt_denoise(C.byref(p), fb.data_ptr(), *guides, plain_out.data_ptr(), plain_scratch.data_ptr(), stream),
                                       "pt_denoise"))

    paths = a.paths.split(",")
    n_it = abi.PT_VDENOISE_DEFAULT_ITERATIONS
    times = {k: {n: [] for n in range(1, n_it + 1)} for k in paths}
    t_plain = {n: [] for n in range(1, n_it + 1)}
    ran, results = {}, {}
    for k in paths:  # warm-up, and the bits of each path
        _, ran[k] = filt(n_it, PATH_FLAGS[k])
        results[k] = (out.clone(), vout.clone())
    same = all(bool(torch.equal(results[k][j].view(torch.int32), results[paths[0]][j].view(torch.int32))) for k in paths for j in (0, 1))
    for n in range(1, n_it + 1):
        for k in paths:
            filt(n, PATH_FLAGS[k])
        plain(n)
        for _ in range(a.reps):  # alternated
            for k in paths:
                times[k][n].append(filt(n, PATH_FLAGS[k])[0])
            t_plain[n].append(plain(n))
    med_plain = {n: statistics.median(t_plain[n]) for n in t_plain}
    for k in paths:
        med = {n: statistics.median(times[k][n]) for n in times[k]}
        by_step = {str(1 << (n - 1)): round(med[n] - (med[n - 1] if n > 1 else 0.0), 4) for n in med}
        plain_by_step = {str(1 << (n - 1)): round(med_plain[n] - (med_plain[n - 1] if n > 1 else 0.0), 4) for n in med_plain}
        whole = times[k][n_it]
        print(json.dumps({"tool": "variance_denoise_bench", "build_id": build, "scene": "cornell", "workload": f"{W}x{H}", "path": k,
                          "read_path_per_iteration": ran[k], "iterations": n_it, "windows": [a.window, a.window], "filter_ms": stats(whole),
                          "ms_by_step": by_step, "ms_at_iterations": {str(n): stats(times[k][n]) for n in med},
                          "spread_pct": round(100 * (max(whole) - min(whole)) / med[n_it], 2), "estimate_ms": stats(t_est),
                          "pt_denoise_ms": stats(t_plain[n_it]), "pt_denoise_ms_by_step": plain_by_step,
                          "filter_over_pt_denoise": round(med[n_it] / med_plain[n_it], 3),
                          "estimate_plus_filter_over_pt_denoise": round((med[n_it] + statistics.median(t_est)) / med_plain[n_it], 3),
                          "aov_spp": a.aov_spp, "paths_bit_identical": same}), flush=True)
    acc.close()


if __name__ == "__main__":
    main()
