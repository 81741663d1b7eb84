"""The firefly stage (render.firefly: pt_firefly = firefly_kernel, include/pt_post.h) at 1920x1080 on a rendered Cornell frame, the LDS path and
PT_FIREFLY_NO_LDS, against the yardstick tools/temporal_bench.py and tools/display_bench.py use: a device-to-device copy that moves the same
bytes, on the same frame sizes in the same process.  Writes a table and one JSON line, stamped with pt_build_id(), to --out (default
profiles/firefly_bench.txt): everything in that file above the line that starts with MARKER — the hand-written record — is kept.

Bytes per pixel, counted from the kernel: 12 read + 12 written without a variance plane (the halo's re-reads hit the caches), 24 + 24 with
one; with counts, a memset of 8 bytes and one 64-bit atomic per workgroup that clamped or repaired anything (NO_LDS: per wave).  A copy of n bytes moves 2 n, so the yardstick copies are
12 and 24 bytes per pixel.  The counts are timed apart (lds_counts, no_lds_counts: no variance plane).

HIP events on the launch stream around --batch back-to-back calls (one call is a hundredth of a ms: a single one would time the clock),
divided by the batch; the timed calls alternate --reps times after a warm-up; medians, with the spread.  The frame (25 MB) is smaller than
the Infinity Cache and is touched again by the next call of a batch: the copies are cache-resident copies, as in the other two tools.

    python tools/firefly_bench.py [--reps 21] [--batch 16] [--spp 4] [--out profiles/firefly_bench.txt]

Kernel times come from a trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/firefly_bench.py --reps 3 --out DIR/bench.txt
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
MARKER = "# ---- tools/firefly_bench.py"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "firefly_bench.txt"))
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    lib = abi.load_library()
    packed, cam_args = scenes.build("cornell")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fb = R.render(W, H, a.spp, packed, scenes.make_camera(cam_args, W, H))
    var = (fb * fb) * 0.05  # a plane of the variance's size and range: its values are multiplied or copied, never tested
    out, vout = torch.empty_like(fb), torch.empty_like(fb)
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def timed(call):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.batch):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.batch

    def stage(no_lds, variance, with_counts):  # straight through the C ABI: the host's share of a call stays as small as ctypes makes it
        p = abi.PtFireflyParams()
        lib.pt_firefly_params_init(C.byref(p), W, H)
        p.flags |= abi.PT_FIREFLY_NO_LDS if no_lds else 0
        args = (C.byref(p), ptr(fb), ptr(var) if variance else None, ptr(out), ptr(vout) if variance else None, ptr(counts) if with_counts else None, stream)
        return lambda: abi.check(lib.pt_firefly(*args), "pt_firefly")

    def copier(bytes_per_pixel):
        n = W * H * bytes_per_pixel
        src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
        return lambda: dst.copy_(src)

    calls = {"lds": stage(False, False, False), "no_lds": stage(True, False, False), "lds_variance": stage(False, True, False),
             "no_lds_variance": stage(True, True, False), "lds_counts": stage(False, False, True), "no_lds_counts": stage(True, False, True),
             "copy_12": copier(12), "copy_24": copier(24)}
    calls["lds_counts"]()
    torch.cuda.synchronize()
    clamped, repaired = (int(v) for v in counts.cpu().numpy())
    last = (C.c_int32 * 4)()
    abi.check(lib.pt_debug_last_firefly(last), "pt_debug_last_firefly")
    for c in calls.values():
        timed(c)
    times = {k: [] for k in calls}
    for _ in range(a.reps):  # alternated
        for k, c in calls.items():
            times[k].append(timed(c))
    med = {k: statistics.median(v) for k, v in times.items()}
    result = {"tool": "firefly_bench", "build_id": lib.pt_build_id().decode(), "scene": "cornell", "workload": f"{W}x{H}", "spp": a.spp, "batch": a.batch,
              "reps": a.reps, "clamped": clamped, "repaired": repaired, "last_firefly": list(last),
              "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)} for k, v in times.items()},
              "lds_over_copy": round(med["lds"] / med["copy_12"], 3), "no_lds_over_copy": round(med["no_lds"] / med["copy_12"], 3),
              "lds_over_no_lds": round(med["lds"] / med["no_lds"], 3), "lds_variance_over_copy": round(med["lds_variance"] / med["copy_24"], 3),
              "no_lds_variance_over_copy": round(med["no_lds_variance"] / med["copy_24"], 3),
              "counts_cost_ms": {"lds": round(med["lds_counts"] - med["lds"], 5), "no_lds": round(med["no_lds_counts"] - med["no_lds"], 5)}}
    lines = [f"{MARKER} as it stands: python tools/firefly_bench.py --reps {a.reps} --batch {a.batch} --spp {a.spp}   (build {result['build_id']})",
             f"# pt_firefly at {W}x{H} on the Cornell frame at {a.spp} spp, defaults (rank 1, k 1, repair): {clamped} pixels clamped, {repaired} repaired; "
             f"{last[1]} x {last[2]} tiles of {abi.PT_FIREFLY_TILE_W} x {abi.PT_FIREFLY_TILE_H} pixels",
             "# median ms of one call (min .. max over the reps); copy_N = a device-to-device copy of N bytes per pixel, which moves 2 N"]
    for k, v in result["ms"].items():
        lines.append(f"#   {k:<16} {v['median']:.4f}   ({v['min']:.4f} .. {v['max']:.4f})")
    lines.append(f"#   LDS / copy of its 24 bytes per pixel {result['lds_over_copy']:.2f}   NO_LDS / copy {result['no_lds_over_copy']:.2f}   LDS / NO_LDS "
                 f"{result['lds_over_no_lds']:.2f}   with the variance plane (48 bytes per pixel): LDS / copy {result['lds_variance_over_copy']:.2f}   "
                 f"NO_LDS / copy {result['no_lds_variance_over_copy']:.2f}")
    lines.append(f"#   what the counts add (the memset of 8 bytes and one 64-bit atomic per workgroup; NO_LDS: per wave): LDS {result['counts_cost_ms']['lds']:.4f} ms   "
                 f"NO_LDS {result['counts_cost_ms']['no_lds']:.4f} ms")
    lines += ["# ---- the run", json.dumps(result)]
    path = Path(a.out)
    head = path.read_text().split(MARKER)[0] if path.exists() and MARKER in path.read_text() else ""
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(head + "\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
