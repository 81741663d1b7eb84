"""The first-hit feature buffers (render.render_aov: pt_render_aov) against the renders around them.  One JSON line per config, stamped
with pt_build_id().  Per scene (cfg2, cfg3, cfg5 at 1920x1080):

  aov      the AOV pass at 16 samples, all six planes (allocated once): HIP events on the launch stream around pt_render_aov alone,
           as pt_render_timed's events bracket its launch
  depth1   pt_render_timed at depth 1 and the same 16 spp — the same stream per pixel, the same rays, through the render kernels: the
           yardstick (its `direct` plane is this frame, bit for bit; checked here too)
  frame    pt_render_timed at full depth and the config's own spp

After a warm-up of each, `aov` and `depth1` alternate `--reps` times; `frame` runs `--frame-reps` times.  Ratios are of the medians;
`pair_spread_pct` is the larger of the two (max - min) ranges over the depth-1 median — a ratio inside it says nothing.

    python tools/aov_bench.py [--configs cfg2,cfg3,cfg5] [--reps 7] [--frame-reps 2] [--spp 16]
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

CONFIGS = {"cfg2": ("cornell", 1024), "cfg3": ("smoke", 1024), "cfg5": ("triangles", 256)}  # BASELINE.json configs: scene, spp
W, H = 1920, 1080


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg3,cfg5")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frame-reps", type=int, default=2)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    build = abi.load_library().pt_build_id().decode()
    for cfg in a.configs.split(","):
        scene, frame_spp = CONFIGS[cfg]
        packed, cam_args = scenes.build(scene, **({"n_triangles": 100_000} if scene == "triangles" else {}))
        cam = scenes.make_camera(cam_args, W, H)
        ds = R.DeviceScene(packed)
        ds.reserve(W, H, frame_spp)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        # the planes are allocated once and the events bracket the library call alone, as pt_render_timed's bracket its launch
        lib = abi.load_library()
        planes = {k: torch.empty((H, W, 3) if abi.AOV_CHANNELS[k] == 3 else (H, W), dtype=torch.int32 if k == "id" else torch.float32, device="cuda")
                  for k in abi.AOV_PLANES}
        bufs = abi.PtAovBuffers(struct_size=C.sizeof(abi.PtAovBuffers), **{k: v.data_ptr() for k, v in planes.items()})
        p = abi.PtRenderParams(W, H, a.spp, 1, 0, 1, 0, 0)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def aov():
            torch.cuda.synchronize()
            e0.record()
            abi.check(lib.pt_render_aov(ds.handle, C.byref(cam.c), C.byref(p), C.byref(bufs), stream), "pt_render_aov")
            e1.record()
            torch.cuda.synchronize()
            return planes, e0.elapsed_time(e1)

        def depth1():
            return R.render(W, H, a.spp, ds, cam, depth=1, timed=True)

        planes, _ = aov()
        fb, _ = depth1()
        same = bool(torch.equal(planes["direct"].view(torch.int32), fb.view(torch.int32)))
        coverage = float(planes["coverage"].double().mean())
        which = (C.c_int32 * 2)()
        abi.check(lib.pt_debug_last_aov(ds.handle, which), "pt_debug_last_aov")
        del fb
        t_a, t_d = [], []
        for _ in range(a.reps):  # alternated
            t_a.append(aov()[1])
            t_d.append(depth1()[1])
        t_f = []
        if a.frame_reps > 0:  # (0: an A/B of the pass alone)
            R.render(W, H, frame_spp, ds, cam, timed=True)  # warm-up
            t_f = [R.render(W, H, frame_spp, ds, cam, timed=True)[1] for _ in range(a.frame_reps)]
        m_a, m_d, m_f = statistics.median(t_a), statistics.median(t_d), statistics.median(t_f) if t_f else None
        print(json.dumps({"tool": "aov_bench", "build_id": build, "config": cfg, "scene": scene, "workload": f"{W}x{H}", "aov_spp": a.spp,
                          "aov_ms": stats(t_a), "depth1_ms": stats(t_d), "frame_spp": frame_spp, "frame_ms": stats(t_f) if t_f else None,
                          "aov_over_depth1": round(m_a / m_d, 3), "aov_over_frame": round(m_a / m_f, 4) if t_f else None,
                          "aov_mrays_per_s": round(W * H * a.spp / m_a / 1e3, 1),
                          "pair_spread_pct": round(100 * max(max(t_a) - min(t_a), max(t_d) - min(t_d)) / m_d, 2),
                          "direct_is_depth1": same, "aov_kernel": {"uv_tracked": bool(which[1]), "grid_walk": int(which[0])}, "mean_coverage": round(coverage, 4)}), flush=True)


if __name__ == "__main__":
    main()
