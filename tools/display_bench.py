"""The display stage (render.Display: pt_display_meter = display_meter_kernel + display_solve_kernel, pt_display_apply =
display_apply_kernel) at 1920x1080, against two yardsticks on the same frame in the same process: pt_tonemap_rgb8 (the output stage it
extends) and device-to-device copies that move the bytes each part reads and writes.  Writes a table and one JSON line, stamped with
pt_build_id(), to --out (default profiles/display_bench.txt).

Three frames: the Cornell-style scene (cfg2) rendered at --spp samples; a constant frame (every pixel in ONE bin: same-address LDS
atomics serialise, which would make it the metering kernel's worst case); exp2(uniform(-20, 20)) per channel (the bins spread as wide
as they go).  On each: meter + solve; apply with the ACES curve into rgb8; and both.  (The forms of the two streaming kernels that were
tried — grids, per-wave histograms, a ballot over equal bins, pixels per load — are timed by tools/ubench/display_stage.hip.)

Bytes per pixel, counted from the kernels: meter reads 12 (the solve kernel touches 2 KB); apply reads 12 and writes 3.  A copy of n
bytes moves 2 n, so the yardstick copies are 6, 7.5 and 13.5 bytes per pixel.

HIP events on the launch stream around --batch back-to-back calls (one call is a few hundredths of a ms: a single one would time the
clock), divided by the batch; every timed call alternates --reps times after a warm-up; medians.

    python tools/display_bench.py [--reps 21] [--batch 16] [--spp 16] [--out profiles/display_bench.txt] [--only FRAME]

Kernel times come from a trace in a run of its own, one frame per run so that the names tell the rows apart:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/display_bench.py --only constant --reps 3 --out DIR/bench.txt
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "display_bench.txt"))
    ap.add_argument("--only", default=None, choices=["cornell", "constant", "random"], help="one frame only (for a kernel trace of that frame)")
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    lib = abi.load_library()
    packed, cam_args = scenes.build("cornell")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    frames = {
        "cornell": R.render(W, H, a.spp, packed, scenes.make_camera(cam_args, W, H)),
        "constant": torch.full((H, W, 3), 0.7, dtype=torch.float32, device="cuda"),
        "random": torch.exp2(torch.rand((H, W, 3), generator=gen, device="cuda") * 40.0 - 20.0),
    }
    if a.only:
        frames = {a.only: frames[a.only]}
    rgb8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    disp = R.Display("aces")
    last = (C.c_int32 * 8)()

    def timed(call):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.batch):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def copier(bytes_per_pixel):
        n = int(W * H * bytes_per_pixel)
        src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
        return lambda: dst.copy_(src)

    copies = {"copy_meter": copier(6), "copy_apply": copier(7.5), "copy_both": copier(13.5)}
    result = {"tool": "display_bench", "build_id": lib.pt_build_id().decode(), "workload": f"{W}x{H}", "spp": a.spp, "batch": a.batch, "reps": a.reps, "frames": {}}
    for fname, fb in frames.items():
        hist, ev = disp.meter(fb).histogram(), disp.exposure()
        ptr, out8 = C.c_void_p(fb.data_ptr()), C.c_void_p(rgb8.data_ptr())

        def meter():  # straight through the C ABI: the host's share of a call stays as small as ctypes makes it
            abi.check(lib.pt_display_meter(disp.handle, C.byref(disp.params), ptr, W, H, stream), "pt_display_meter")

        def apply():
            abi.check(lib.pt_display_apply(disp.handle, C.byref(disp.params), ptr, W, H, out8, None, stream), "pt_display_apply")

        meter(), apply()
        abi.check(lib.pt_debug_last_display(last), "pt_debug_last_display")
        calls = {"meter": meter, "apply": apply, "both": lambda: (meter(), apply())}
        calls["tonemap_rgb8"] = lambda: abi.check(lib.pt_tonemap_rgb8(ptr, W, H, out8, stream), "pt_tonemap_rgb8")
        calls.update(copies)
        for c in calls.values():
            timed(c)
        times = {k: [] for k in calls}
        for _ in range(a.reps):  # alternated
            for k, c in calls.items():
                times[k].append(timed(c))
        med = {k: statistics.median(v) for k, v in times.items()}
        result["frames"][fname] = {
            "exposure_ev": round(ev, 4), "bins_in_use": int((hist[:256] > 0).sum()), "rejected": int(hist[256]), "last_display": list(last),
            "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)} for k, v in times.items()},
            "meter_over_copy": round(med["meter"] / med["copy_meter"], 3), "apply_over_copy": round(med["apply"] / med["copy_apply"], 3),
            "both_over_copy": round(med["both"] / med["copy_both"], 3), "apply_over_tonemap_rgb8": round(med["apply"] / med["tonemap_rgb8"], 3),
            "both_over_tonemap_rgb8": round(med["both"] / med["tonemap_rgb8"], 3),
        }
    if not a.only:  # what a constant frame costs the metering, against the frame that spreads the bins widest and against the rendered one
        ms = {f: result["frames"][f]["ms"]["meter"]["median"] for f in frames}
        result["constant_penalty"] = {"over_random": round(ms["constant"] / ms["random"], 3), "over_cornell": round(ms["constant"] / ms["cornell"], 3)}
    lines = [f"# The display stage at {W}x{H}: python tools/display_bench.py --reps {a.reps} --batch {a.batch} --spp {a.spp}   (build {result['build_id']})",
             "# median ms of one call (min .. max over the reps); meter = display_meter_kernel + display_solve_kernel, apply = display_apply_kernel (ACES, rgb8)"]
    for fname, r in result["frames"].items():
        lines.append(f"#\n# frame `{fname}`: {r['bins_in_use']} bins in use, {r['rejected']} pixels rejected, solved exposure {r['exposure_ev']:+.3f} EV; "
                     f"metering grid {r['last_display'][0]} x {r['last_display'][1]}, {r['last_display'][2]} trips of {r['last_display'][3]} pixels; apply grid "
                     f"{r['last_display'][4]} x {r['last_display'][5]}, {r['last_display'][6]} values per thread")
        for k, v in r["ms"].items():
            lines.append(f"#   {k:<16} {v['median']:.4f}   ({v['min']:.4f} .. {v['max']:.4f})")
        lines.append(f"#   meter / copy of its bytes {r['meter_over_copy']:.2f}   apply / copy {r['apply_over_copy']:.2f}   both / copy {r['both_over_copy']:.2f}   "
                     f"apply / pt_tonemap_rgb8 {r['apply_over_tonemap_rgb8']:.2f}   both / pt_tonemap_rgb8 {r['both_over_tonemap_rgb8']:.2f}")
    if not a.only:
        p = result["constant_penalty"]
        lines.append(f"#\n# the constant frame's penalty (meter ms on `constant` over `random` / over `cornell`): {p['over_random']:.2f} / {p['over_cornell']:.2f}")
    lines += ["# ---- the run", json.dumps(result)]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    disp.close()


if __name__ == "__main__":
    main()
