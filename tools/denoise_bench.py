"""The a-trous denoiser (render.denoise: pt_denoise) at 1920x1080 against the passes around it.  One JSON line per read path, stamped
with pt_build_id().  The Cornell-style scene (cfg2): the frame at --spp, the guides of render_aov at --aov-spp, then

  filter   pt_denoise with the default parameters (5 iterations, every guide, demodulated): HIP events on the launch stream around the
           library call alone (scratch and out allocated once), as pt_render_timed's events bracket its launch
  by step  the same call at 1 ... 5 iterations; the cost of the iteration with step 2^(n-1) is the difference of the medians at n and
           n - 1 iterations (the call at 1 iteration carries the guide-packing prepass, reported with step 1)
  aov      the AOV pass that makes the guides (events around pt_render_aov alone)
  frame    pt_render_timed at --spp

for each read path of --paths: `default` (the library's rule: LDS-staged tiles for the steps 1 and 2, global memory beyond) and `global`
(PT_DENOISE_NO_LDS: every iteration reads its taps from global memory) — the A/B.  The two paths must give the same bits: checked here.
After a warm-up the paths alternate `--reps` times per iteration count.

    python tools/denoise_bench.py [--reps 9] [--spp 16] [--aov-spp 16] [--paths default,global]
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
PATH_FLAGS = {"default": 0, "global": abi.PT_DENOISE_NO_LDS}


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--spp", type=int, default=16)
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
    ds.reserve(W, H, a.spp)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    fb, frame_ms = R.render(W, H, a.spp, ds, cam, timed=True)
    frame = [R.render(W, H, a.spp, ds, cam, timed=True)[1] for _ in range(3)]
    planes = {k: torch.empty((H, W, 3) if abi.AOV_CHANNELS[k] == 3 else (H, W), dtype=torch.float32, device="cuda") for k in ("albedo", "normal", "depth")}
    bufs = abi.PtAovBuffers(struct_size=C.sizeof(abi.PtAovBuffers), **{k: v.data_ptr() for k, v in planes.items()})
    pa = abi.PtRenderParams(W, H, a.aov_spp, 1, 0, 1, 0, 0)

    def aov():
        torch.cuda.synchronize()
        e0.record()
        abi.check(lib.pt_render_aov(ds.handle, C.byref(cam.c), C.byref(pa), C.byref(bufs), stream), "pt_render_aov")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    aov()
    t_aov = [aov() for _ in range(a.reps)]
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    scratch = torch.empty(lib.pt_denoise_scratch_floats(W, H), dtype=torch.float32, device="cuda")

    def filt(iterations, flags):
        p = abi.PtDenoiseParams()
        lib.pt_denoise_params_init(C.byref(p), W, H)
        p.iterations = iterations
        p.flags |= flags
        torch.cuda.synchronize()
        e0.record()
        abi.check(lib.pt_denoise(C.byref(p), fb.data_ptr(), planes["albedo"].data_ptr(), planes["normal"].data_ptr(), planes["depth"].data_ptr(),
                                 out.data_ptr(), scratch.data_ptr(), stream), "pt_denoise")
        e1.record()
        torch.cuda.synchronize()
        which = (C.c_int32 * 8)()
        abi.check(lib.pt_debug_last_denoise(which), "pt_debug_last_denoise")
        return e0.elapsed_time(e1), list(which)

    paths = a.paths.split(",")
    n_it = abi.PT_DENOISE_DEFAULT_ITERATIONS
    times = {k: {n: [] for n in range(1, n_it + 1)} for k in paths}
    ran, results = {}, {}
    for k in paths:  # warm-up, and the bits of each path
        _, ran[k] = filt(n_it, PATH_FLAGS[k])
        results[k] = out.clone()
    same = all(bool(torch.equal(results[k].view(torch.int32), results[paths[0]].view(torch.int32))) for k in paths)
    for n in range(1, n_it + 1):
        for k in paths:
            filt(n, PATH_FLAGS[k])
        for _ in range(a.reps):  # alternated
            for k in paths:
                times[k][n].append(filt(n, PATH_FLAGS[k])[0])
    for k in paths:
        med = {n: statistics.median(times[k][n]) for n in times[k]}
        by_step = {str(1 << (n - 1)): round(med[n] - (med[n - 1] if n > 1 else 0.0), 4) for n in med}
        whole = times[k][n_it]
        print(json.dumps({"tool": "denoise_bench", "build_id": build, "scene": "cornell", "workload": f"{W}x{H}", "path": k, "read_path_per_iteration": ran[k],
                          "iterations": n_it, "filter_ms": stats(whole), "ms_by_step": by_step, "ms_at_iterations": {str(n): stats(times[k][n]) for n in med},
                          "spread_pct": round(100 * (max(whole) - min(whole)) / med[n_it], 2),
                          "aov_spp": a.aov_spp, "aov_ms": stats(t_aov), "frame_spp": a.spp, "frame_ms": stats(frame),
                          "filter_over_aov": round(med[n_it] / statistics.median(t_aov), 3), "filter_over_frame": round(med[n_it] / statistics.median(frame), 4),
                          "paths_bit_identical": same}), flush=True)


if __name__ == "__main__":
    main()
