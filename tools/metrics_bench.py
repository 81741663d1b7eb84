"""The image error (render.image_error: pt_image_error = imgerr_accumulate_kernel + imgerr_finish_kernel, include/pt_metrics.h) at
1920x1080 on a rendered Cornell frame against another (--spp against --ref-spp), the accumulators in LDS and PT_IMAGE_ERROR_NO_LDS
alternated, without and with the error plane, against two yardsticks in the same process: a device-to-device copy that moves the bytes
the call reads, and pt_variance_estimate on an adaptive accumulator of the same size — the yardsticks of the other stages' records.
Writes a table and one JSON line, stamped with pt_build_id(), to --out (default profiles/metrics_bench.txt): everything in that file
above the line that starts with MARKER — the hand-written record — is kept.

Bytes per pixel, counted from the kernel: read 12 (a) + 12 (ref) = 24, written 0 (4 with the plane); the result is 104 bytes per call.  A
copy of n bytes moves 2 n, so the yardstick copy is 12 bytes per pixel (14 with the plane).  Every pixel makes nine terms of at most
three chunks each: at most 27 atomic adds.  The paths are checked to give the same bits before anything is timed.

HIP events on the launch stream around --batch back-to-back calls (--slow-batch for the global-atomics path, which is much slower),
divided by the batch; the timed calls alternate --reps times after a warm-up; medians, with the spread.  The frames (50 MB) fit the
Infinity Cache and are touched again by the next call of a batch: the copy is a cache-resident copy, as in tools/firefly_bench.py.

    python tools/metrics_bench.py [--reps 21] [--batch 16] [--slow-batch 2] [--spp 4] [--ref-spp 16] [--out profiles/metrics_bench.txt]
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
MARKER = "# ---- tools/metrics_bench.py"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--slow-batch", type=int, default=2)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=16)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "metrics_bench.txt"))
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    lib = abi.load_library()
    packed, cam_args = scenes.build("cornell")
    cam = scenes.make_camera(cam_args, W, H)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ds = R.DeviceScene(packed)
    fb, ref = R.render(W, H, a.spp, ds, cam), R.render(W, H, a.ref_spp, ds, cam)
    acc = R.Accumulator(W, H, ds, cam, adaptive=True)
    acc.add(a.spp - a.spp // 2).add(max(a.spp // 2, 1))
    est_out = torch.empty_like(fb)
    plane = torch.empty((H, W), dtype=torch.float32, device="cuda")
    scratch = torch.empty(lib.pt_image_error_scratch_bytes() // 8, dtype=torch.int64, device="cuda")
    result = torch.empty(C.sizeof(abi.PtImageErrorResult) // 8, dtype=torch.int64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def timed(call, batch):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(batch):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / batch

    def stage(no_lds, with_plane):  # straight through the C ABI: the host's share of a call stays small
        p = abi.PtImageErrorParams()
        lib.pt_image_error_params_init(C.byref(p), W, H)
        p.flags = abi.PT_IMAGE_ERROR_NO_LDS if no_lds else 0
        p.scratch_bytes = lib.pt_image_error_scratch_bytes()
        args = (C.byref(p), ptr(fb), ptr(ref), ptr(result), ptr(plane) if with_plane else None, ptr(scratch), stream)
        return lambda: abi.check(lib.pt_image_error(*args), "pt_image_error")

    def copier(bytes_per_pixel):
        n = W * H * bytes_per_pixel
        src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
        return lambda: dst.copy_(src)

    def estimate():
        abi.check(lib.pt_variance_estimate(acc.handle, ptr(est_out), stream), "pt_variance_estimate")

    calls = {"lds": stage(False, False), "no_lds": stage(True, False), "lds_plane": stage(False, True), "no_lds_plane": stage(True, True),
             "copy_12": copier(12), "copy_14": copier(14), "variance_estimate": estimate}
    batch = {k: a.slow_batch if k.startswith("no_lds") else a.batch for k in calls}
    seen = {}
    for name in ("lds", "no_lds", "lds_plane", "no_lds_plane"):
        calls[name]()
        torch.cuda.synchronize()
        seen[name] = result.clone()
    same = all(torch.equal(seen["lds"], v) for v in seen.values())
    assert same, "the paths differ"
    e = R.ImageError(seen["lds"], None, None)
    last = (C.c_int32 * 4)()
    abi.check(lib.pt_debug_last_image_error(last), "pt_debug_last_image_error")
    for k, c in calls.items():
        timed(c, batch[k])
    times = {k: [] for k in calls}
    for _ in range(a.reps):  # alternated
        for k, c in calls.items():
            times[k].append(timed(c, batch[k]))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"tool": "metrics_bench", "build_id": lib.pt_build_id().decode(), "scene": "cornell", "workload": f"{W}x{H}", "spp": a.spp,
           "ref_spp": a.ref_spp, "batch": a.batch, "slow_batch": a.slow_batch, "reps": a.reps, "mse": e.mse, "rel_mse": e.rel_mse, "pixels": e.pixels,
           "skipped": e.skipped, "last_image_error": list(last), "same_bits": same,
           "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)} for k, v in times.items()},
           "lds_over_copy_12": round(med["lds"] / med["copy_12"], 2), "lds_plane_over_copy_14": round(med["lds_plane"] / med["copy_14"], 2),
           "lds_over_no_lds": round(med["lds"] / med["no_lds"], 4), "lds_over_variance_estimate": round(med["lds"] / med["variance_estimate"], 2),
           "plane_cost_ms": {"lds": round(med["lds_plane"] - med["lds"], 5), "no_lds": round(med["no_lds_plane"] - med["no_lds"], 5)}}
    lines = [f"{MARKER} as it stands: python tools/metrics_bench.py --reps {a.reps} --batch {a.batch} --slow-batch {a.slow_batch} --spp {a.spp} --ref-spp {a.ref_spp}   (build {res['build_id']})",
             f"# pt_image_error at {W}x{H}: the Cornell frame at {a.spp} spp against the one at {a.ref_spp} spp: MSE {e.mse!r}, relMSE {e.rel_mse!r}, {e.pixels} pixels, "
             f"{e.skipped} skipped; {last[1]} workgroups; every path gives the same bits",
             "# median ms of one call (min .. max over the reps); lds = the accumulators in LDS, no_lds = global atomics only, _plane = with the error plane; "
             "copy_N = a device-to-device copy of N bytes per pixel, which moves 2 N"]
    for k, v in res["ms"].items():
        lines.append(f"#   {k:<20} {v['median']:.4f}   ({v['min']:.4f} .. {v['max']:.4f})")
    lines.append(f"#   LDS / copy of its 24 bytes per pixel {res['lds_over_copy_12']:.1f}     with the plane / copy of its 28 {res['lds_plane_over_copy_14']:.1f}"
                 f"     LDS / NO_LDS {res['lds_over_no_lds']:.4f}     LDS / pt_variance_estimate {res['lds_over_variance_estimate']:.1f}"
                 f"     what the plane adds: LDS {res['plane_cost_ms']['lds']:.4f} ms   NO_LDS {res['plane_cost_ms']['no_lds']:.4f} ms")
    lines += ["# ---- the run", json.dumps(res)]
    path = Path(a.out)
    head = path.read_text().split(MARKER)[0] if path.exists() and MARKER in path.read_text() else ""
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(head + "\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    acc.close()
    ds.close()


if __name__ == "__main__":
    main()
