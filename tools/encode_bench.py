"""The encode stage (render.encode: pt_encode, pt_display_encode = encode_kernel, include/pt_encode.h) at 1920x1080 on a rendered
Cornell frame, against its yardstick in the same run: pt_display_apply to rgb8 as it stands (0.010 ms in profiles/display_bench.txt).
Timed, alternated, in one process:
    apply_rgb8        pt_display_apply (ACES) -> rgb8                                  the yardstick: 12 bytes in, 3 out per pixel
    apply_linear      pt_display_apply (ACES) -> linear_out                            12 in, 12 out
    encode            pt_encode of that plane                                          12 in, 3 out
    two_calls         apply_linear + encode                                            24 in, 15 out
    fused             pt_display_encode                                                12 in, 3 out
    copy              a device-to-device copy of 7.5 bytes per pixel (moves 15)        cache-resident: the frame is smaller than the cache
for sRGB without and with the dither, and once more under PT_ENCODE_NO_VEC (one value per lane).  Writes a table and one JSON line,
stamped with pt_build_id(), to --out (default profiles/encode_bench.txt).

HIP events on the launch stream around --batch back-to-back calls (one call is a hundredth of a ms: a single one would time the clock),
divided by the batch; every timed call alternates --reps times after a warm-up; medians.

    python tools/encode_bench.py [--reps 21] [--batch 16] [--spp 16] [--out profiles/encode_bench.txt]
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "encode_bench.txt"))
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    lib = abi.load_library()
    assert abi.has_encode(lib)
    packed, cam_args = scenes.build("cornell")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fb = R.render(W, H, a.spp, packed, scenes.make_camera(cam_args, W, H))
    rgb8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    linear = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    disp = R.Display("aces")
    disp.meter(fb)
    ptr, lin, out8 = C.c_void_p(fb.data_ptr()), C.c_void_p(linear.data_ptr()), C.c_void_p(rgb8.data_ptr())
    n = int(W * H * 7.5)
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    last = (C.c_int32 * 8)()

    def timed(call):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.batch):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def apply_rgb8():  # straight through the C ABI: the host's share of a call stays as small as ctypes makes it
        abi.check(lib.pt_display_apply(disp.handle, C.byref(disp.params), ptr, W, H, out8, None, stream), "pt_display_apply")

    def apply_linear():
        abi.check(lib.pt_display_apply(disp.handle, C.byref(disp.params), ptr, W, H, None, lin, stream), "pt_display_apply")

    result = {"tool": "encode_bench", "build_id": lib.pt_build_id().decode(), "workload": f"{W}x{H}", "spp": a.spp, "batch": a.batch, "reps": a.reps,
              "exposure_ev": round(disp.exposure(), 4), "modes": {}}
    for mode, dither, no_vec in (("srgb", False, False), ("srgb+dither", True, False), ("srgb no_vec", False, True), ("srgb+dither no_vec", True, True)):
        ep = R._encode_params(lib, W, H, "srgb", dither, (0, 0), no_vec)

        def encode():
            abi.check(lib.pt_encode(C.byref(ep), lin, out8, stream), "pt_encode")

        def fused():
            abi.check(lib.pt_display_encode(disp.handle, C.byref(disp.params), C.byref(ep), ptr, out8, stream), "pt_display_encode")

        calls = {"apply_rgb8": apply_rgb8, "apply_linear": apply_linear, "encode": encode, "two_calls": lambda: (apply_linear(), encode()), "fused": fused,
                 "copy": lambda: dst.copy_(src)}
        apply_linear(), encode()
        two = rgb8.clone()
        fused()
        abi.check(lib.pt_debug_last_encode(last), "pt_debug_last_encode")
        torch.cuda.synchronize()
        assert torch.equal(two, rgb8), f"{mode}: the fused call and the two calls differ"
        for c in calls.values():
            timed(c)
        times = {k: [] for k in calls}
        for _ in range(a.reps):  # alternated
            for k, c in calls.items():
                times[k].append(timed(c))
        med = {k: statistics.median(v) for k, v in times.items()}
        result["modes"][mode] = {
            "last_encode": list(last),
            "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)} for k, v in times.items()},
            "fused_over_apply_rgb8": round(med["fused"] / med["apply_rgb8"], 3), "fused_over_two_calls": round(med["fused"] / med["two_calls"], 3),
            "encode_over_apply_rgb8": round(med["encode"] / med["apply_rgb8"], 3), "two_calls_over_apply_rgb8": round(med["two_calls"] / med["apply_rgb8"], 3),
            "fused_over_copy": round(med["fused"] / med["copy"], 3), "encode_over_copy": round(med["encode"] / med["copy"], 3),
        }
    lines = [f"# The encode stage at {W}x{H}: python tools/encode_bench.py --reps {a.reps} --batch {a.batch} --spp {a.spp}   (build {result['build_id']})",
             f"# a rendered Cornell frame at {a.spp} spp, metered exposure {result['exposure_ev']:+.3f} EV, the ACES curve; median ms of one call (min .. max over",
             "# the reps).  apply_rgb8 = pt_display_apply -> rgb8, the yardstick; two_calls = pt_display_apply -> linear_out, then pt_encode; fused =",
             "# pt_display_encode; copy = 7.5 bytes per pixel copied device to device (cache-resident).  The fused call's bytes equal the two calls' (asserted)."]
    for mode, r in result["modes"].items():
        le = r["last_encode"]
        lines.append(f"#\n# {mode}: grid {le[1]} x {le[2]}, {le[3]} values per lane")
        for k, v in r["ms"].items():
            lines.append(f"#   {k:<14} {v['median']:.4f}   ({v['min']:.4f} .. {v['max']:.4f})")
        lines.append(f"#   fused / apply_rgb8 {r['fused_over_apply_rgb8']:.2f}   fused / two_calls {r['fused_over_two_calls']:.2f}   encode / apply_rgb8 "
                     f"{r['encode_over_apply_rgb8']:.2f}   two_calls / apply_rgb8 {r['two_calls_over_apply_rgb8']:.2f}   fused / copy {r['fused_over_copy']:.2f}   "
                     f"encode / copy {r['encode_over_copy']:.2f}")
    lines += ["# ---- the run", json.dumps(result)]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    disp.close()


if __name__ == "__main__":
    main()
