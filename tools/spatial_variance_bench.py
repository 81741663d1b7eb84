"""The spatial variance estimate (render.spatial_variance: pt_spatial_variance = svar_kernel, include/pt_spatial_variance.h) at 1920x1080 on a
rendered Cornell frame with every guide and demodulation (the defaults), the LDS path and PT_SVAR_NO_LDS alternated, at radius 1, 2 and
3, on a frame of all holes to fill (variance_in = +inf everywhere: every pixel does its window) and on frames where 90 % of the pixels are
kept (they do no window work; their workgroups still stage the tile) — chosen at random per pixel, and per block of 48 x 12 pixels, which
is how disocclusions lie —, against two yardsticks in the same process: a device-to-device
copy that moves the bytes the call moves, and pt_variance_estimate on an adaptive accumulator of the same size — the other source of a
variance plane.  Writes a table and one JSON line, stamped with pt_build_id(), to --out (default profiles/spatial_variance_bench.txt):
everything in that file above the line that starts with MARKER — the hand-written record — is kept.

Bytes per pixel, counted from the kernel: read 12 (color) + 12 (albedo) + 12 (normal) + 4 (depth) + 4 (id) + 12 (variance_in), written 12:
68 (the halo's re-reads hit the caches).  A copy of n bytes moves 2 n, so the yardstick copy is 34 bytes per pixel.  The paths are checked
to give the same bits before anything is timed.

HIP events on the launch stream around --batch back-to-back calls, divided by the batch; the timed calls alternate --reps times after a
warm-up; medians, with the spread.  The planes (141 MB) fit the Infinity Cache and are touched again by the next call of a batch: the copy
is a cache-resident copy, as in tools/firefly_bench.py.

    python tools/spatial_variance_bench.py [--reps 21] [--batch 16] [--spp 4] [--aov-spp 4] [--out profiles/spatial_variance_bench.txt]
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
MARKER = "# ---- tools/spatial_variance_bench.py"
BYTES_PER_PIXEL = 68


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--aov-spp", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spatial_variance_bench.txt"))
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    lib = abi.load_library()
    packed, cam_args = scenes.build("cornell")
    cam = scenes.make_camera(cam_args, W, H)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ds = R.DeviceScene(packed)
    fb = R.render(W, H, a.spp, ds, cam)
    g = R.render_aov(W, H, a.aov_spp, ds, cam, planes=("albedo", "normal", "depth", "id"))
    acc = R.Accumulator(W, H, ds, cam, adaptive=True)
    acc.add(a.spp - a.spp // 2).add(max(a.spp // 2, 1))
    holes_in = torch.full_like(fb, float("inf"))                      # every pixel is one to estimate
    kept_in = torch.where(torch.rand((H, W, 1), device="cuda") < 0.9, torch.full_like(fb, 0.01), holes_in).contiguous()  # 90 % kept
    blocks = (torch.rand(((H + 11) // 12, (W + 47) // 48), device="cuda") < 0.9).repeat_interleave(12, 0).repeat_interleave(48, 1)[:H, :W, None]
    kept_blocks_in = torch.where(blocks, torch.full_like(fb, 0.01), holes_in).contiguous()  # 90 % kept, in blocks of 48 x 12 pixels
    out, est_out = torch.empty_like(fb), torch.empty_like(fb)
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

    def stage(no_lds, radius, variance_in, with_counts=False):  # straight through the C ABI: the host's share of a call stays small
        p = abi.PtSpatialVarianceParams()
        lib.pt_spatial_variance_params_init(C.byref(p), W, H)
        p.radius = radius
        p.flags |= abi.PT_SVAR_NO_LDS if no_lds else 0
        args = (C.byref(p), ptr(fb), ptr(g["albedo"]), ptr(g["normal"]), ptr(g["depth"]), ptr(g["id"]), ptr(variance_in), ptr(out),
                ptr(counts) if with_counts else None, stream)
        return lambda: abi.check(lib.pt_spatial_variance(*args), "pt_spatial_variance")

    def copier(bytes_per_pixel):
        n = W * H * bytes_per_pixel
        src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
        return lambda: dst.copy_(src)

    def estimate():
        abi.check(lib.pt_variance_estimate(acc.handle, ptr(est_out), stream), "pt_variance_estimate")

    dr = abi.PT_SVAR_DEFAULT_RADIUS
    calls = {}
    for radius in (1, 2, 3):
        calls[f"lds_r{radius}"] = stage(False, radius, holes_in)
        calls[f"no_lds_r{radius}"] = stage(True, radius, holes_in)
    calls.update({"lds_kept90": stage(False, dr, kept_in), "no_lds_kept90": stage(True, dr, kept_in),
                  "lds_kept90_blocks": stage(False, dr, kept_blocks_in), "no_lds_kept90_blocks": stage(True, dr, kept_blocks_in),
                  "lds_counts": stage(False, dr, holes_in, True), "no_lds_counts": stage(True, dr, holes_in, True),
                  f"copy_{BYTES_PER_PIXEL // 2}": copier(BYTES_PER_PIXEL // 2), "variance_estimate": estimate})
    # the same bits from both paths, and what the frames hold
    seen = {}
    for name in ("lds", "no_lds"):
        for radius in (1, 2, 3):
            calls[f"{name}_r{radius}"]()
            torch.cuda.synchronize()
            seen[name, radius] = out.clone()
    same = all(torch.equal(seen["lds", r].view(torch.int32), seen["no_lds", r].view(torch.int32)) for r in (1, 2, 3))
    assert same, "the LDS path and PT_SVAR_NO_LDS differ"
    calls["lds_counts"]()
    torch.cuda.synchronize()
    estimated, holes = (int(v) for v in counts.cpu().numpy())
    kept = int((kept_in[..., 0] < float("inf")).sum())
    last = (C.c_int32 * 4)()
    abi.check(lib.pt_debug_last_spatial_variance(last), "pt_debug_last_spatial_variance")
    for c in calls.values():
        timed(c)
    times = {k: [] for k in calls}
    for _ in range(a.reps):  # alternated
        for k, c in calls.items():
            times[k].append(timed(c))
    med = {k: statistics.median(v) for k, v in times.items()}
    copy = med[f"copy_{BYTES_PER_PIXEL // 2}"]
    result = {"tool": "spatial_variance_bench", "build_id": lib.pt_build_id().decode(), "scene": "cornell", "workload": f"{W}x{H}", "spp": a.spp,
              "aov_spp": a.aov_spp, "batch": a.batch, "reps": a.reps, "estimated": estimated, "holes": holes, "kept_of_kept90": kept,
              "last_spatial_variance": list(last), "same_bits": same,
              "ms": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)} for k, v in times.items()},
              "lds_over_no_lds": {f"r{r}": round(med[f"lds_r{r}"] / med[f"no_lds_r{r}"], 3) for r in (1, 2, 3)},
              "lds_over_copy": {f"r{r}": round(med[f"lds_r{r}"] / copy, 2) for r in (1, 2, 3)},
              "lds_over_variance_estimate": {f"r{r}": round(med[f"lds_r{r}"] / med["variance_estimate"], 2) for r in (1, 2, 3)},
              "kept90_over_all_holes": {"lds": round(med["lds_kept90"] / med[f"lds_r{dr}"], 3), "no_lds": round(med["no_lds_kept90"] / med[f"no_lds_r{dr}"], 3)},
              "kept90_blocks_over_all_holes": {"lds": round(med["lds_kept90_blocks"] / med[f"lds_r{dr}"], 3),
                                               "no_lds": round(med["no_lds_kept90_blocks"] / med[f"no_lds_r{dr}"], 3)},
              "counts_cost_ms": {"lds": round(med["lds_counts"] - med[f"lds_r{dr}"], 5), "no_lds": round(med["no_lds_counts"] - med[f"no_lds_r{dr}"], 5)}}
    lines = [f"{MARKER} as it stands: python tools/spatial_variance_bench.py --reps {a.reps} --batch {a.batch} --spp {a.spp} --aov-spp {a.aov_spp}   (build {result['build_id']})",
             f"# pt_spatial_variance at {W}x{H} on the Cornell frame at {a.spp} spp, every guide ({a.aov_spp} rays), demodulated, min_pairs {abi.PT_SVAR_DEFAULT_MIN_PAIRS}; at radius {dr}: "
             f"{estimated} pixels estimated, {holes} holes; {last[1]} x {last[2]} tiles of {abi.PT_SVAR_TILE_W} x {abi.PT_SVAR_TILE_H} pixels; both paths give the same bits",
             f"# median ms of one call (min .. max over the reps); _rN = radius N on a frame of all holes to fill; _kept90 = radius {dr}, {kept} of {W * H} pixels kept, chosen per pixel; _kept90_blocks = the same share "
             f"chosen per block of 48 x 12 pixels; "
             f"_counts = radius {dr}, all holes, with counts; copy_N = a device-to-device copy of N bytes per pixel, which moves 2 N"]
    for k, v in result["ms"].items():
        lines.append(f"#   {k:<20} {v['median']:.4f}   ({v['min']:.4f} .. {v['max']:.4f})")
    lines.append("#   LDS / NO_LDS  " + "  ".join(f"r{r} {result['lds_over_no_lds'][f'r{r}']:.2f}" for r in (1, 2, 3)) +
                 "     LDS / copy of its 68 bytes per pixel  " + "  ".join(f"r{r} {result['lds_over_copy'][f'r{r}']:.1f}" for r in (1, 2, 3)) +
                 "     LDS / pt_variance_estimate  " + "  ".join(f"r{r} {result['lds_over_variance_estimate'][f'r{r}']:.1f}" for r in (1, 2, 3)))
    lines.append(f"#   90 % kept / all holes: LDS {result['kept90_over_all_holes']['lds']:.2f}   NO_LDS {result['kept90_over_all_holes']['no_lds']:.2f}"
                 f"   in blocks: LDS {result['kept90_blocks_over_all_holes']['lds']:.2f}   NO_LDS {result['kept90_blocks_over_all_holes']['no_lds']:.2f}"
                 f"     what the counts add: LDS {result['counts_cost_ms']['lds']:.4f} ms   NO_LDS {result['counts_cost_ms']['no_lds']:.4f} ms")
    lines += ["# ---- the run", json.dumps(result)]
    path = Path(a.out)
    head = path.read_text().split(MARKER)[0] if path.exists() and MARKER in path.read_text() else ""
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(head + "\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    acc.close()
    ds.close()


if __name__ == "__main__":
    main()
