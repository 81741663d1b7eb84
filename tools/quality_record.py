"""What the post-render chain buys at a size given on the command line, measured on the GPU with the image error (render.image_error:
include/pt_metrics.h) — the chains whose ratios README.md and DESIGN.md section 1 quote from numpy models over the oracle's 64 x 40 frames:

  denoise              R.denoise at its defaults (guides: --aov-spp camera rays per pixel)
  variance (halves)    R.denoise_variance over the adaptive accumulator's two-half estimate (Accumulator.denoise_variance)
  variance (spatial)   R.denoise_variance over R.spatial_variance of the plain frame (the header's defaults, demodulated, every guide)
  firefly, denoise     R.firefly at its defaults, then R.denoise
  temporal             render_temporal without the filter: --temporal-frames frames of --temporal-spp spp, the camera moving by 0 / 2 / 10 / 40
                       units per frame along x; the last accumulated frame against the last noisy one

on the built-in scenes (--scenes) at 8 / 32 / 128 spp.  Every figure is r = MSE(filtered, ref) / MSE(noisy, ref) (render.mse_ratio's), the
reference being a render of the tool's own at --ref-spp samples (for the temporal rows: at the last camera); below 1 the chain helped.
Every MSE is pt_image_error's exact sum, so the table does not depend on the order in which the device adds.  The random numbers of a
frame do not depend on its sample count's windows, so `noisy` at n spp shares its first n samples with the reference: at --ref-spp >> n
the bias of that is n / ref_spp of the noisy MSE, stated with the table.

A table to stdout and to --out (default profiles/quality_1080p.txt), stamped with pt_build_id().  Nothing asserts these numbers.  It reads
nothing outside the repository.

    python tools/quality_record.py [--width 1920] [--height 1080] [--ref-spp 4096] [--aov-spp 16] [--scenes cornell,smoke] [--out FILE]
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from path_tracer_amd import abi, scenes  # noqa: E402
from path_tracer_amd import render as R  # noqa: E402

SPPS = (8, 32, 128)
MOVES = (0.0, 2.0, 10.0, 40.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--aov-spp", type=int, default=16)
    ap.add_argument("--scenes", default="cornell,smoke")
    ap.add_argument("--temporal-frames", type=int, default=8)
    ap.add_argument("--temporal-spp", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "quality_1080p.txt"))
    a = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    lib = abi.load_library()
    w, h = a.width, a.height
    t_start = time.perf_counter()
    lines = [f"# tools/quality_record.py --width {w} --height {h} --ref-spp {a.ref_spp} --aov-spp {a.aov_spp} --scenes {a.scenes} --temporal-frames "
             f"{a.temporal_frames} --temporal-spp {a.temporal_spp}   (build {lib.pt_build_id().decode()})",
             f"# r = MSE(filtered, ref) / MSE(noisy, ref) at {w}x{h}, every MSE pt_image_error's (exact sums, rounded once); ref = {a.ref_spp} spp of the same scene and camera.",
             "# Below 1 the chain helped.  `noisy MSE` and `relMSE` are the noisy frame's against the reference; skipped = pixels with a NaN or inf on either side."]

    def row(name, cells):
        lines.append(f"  {name:<20}" + "".join(f"{c:>14}" for c in cells))

    for scene in a.scenes.split(","):
        packed, cam_args = scenes.build(scene)
        cam = scenes.make_camera(cam_args, w, h)
        ds = R.DeviceScene(packed)
        ref = R.render(w, h, a.ref_spp, ds, cam)
        guides = R.render_aov(w, h, a.aov_spp, ds, cam, planes=("albedo", "normal", "depth", "id"))
        agd = dict(albedo=guides["albedo"], normal=guides["normal"], depth=guides["depth"])
        cols = {k: [] for k in ("noisy MSE", "noisy relMSE", "skipped", "denoise", "variance (halves)", "variance (spatial)", "firefly, denoise")}
        for n in SPPS:
            noisy = R.render(w, h, n, ds, cam)
            base = R.image_error(noisy, ref)
            cols["noisy MSE"].append(f"{base.mse:.6g}")
            cols["noisy relMSE"].append(f"{base.rel_mse:.6g}")
            cols["skipped"].append(str(base.skipped))
            ratio = lambda f: f"{R.image_error(f, ref).mse / base.mse:.4f}"  # noqa: E731
            cols["denoise"].append(ratio(R.denoise(noisy, **agd)))
            acc = R.Accumulator(w, h, ds, cam, adaptive=True)
            acc.add(n - n // 2).add(n // 2)
            halves = R.image_error(acc.resolve(), ref)  # (the accumulator's frame IS the noisy frame: the same samples)
            cols["variance (halves)"].append(f"{R.image_error(acc.denoise_variance(a.aov_spp), ref).mse / halves.mse:.4f}")
            acc.close()
            var = R.spatial_variance(noisy, **guides)
            cols["variance (spatial)"].append(ratio(R.denoise_variance(noisy, var, **agd)))
            cols["firefly, denoise"].append(ratio(R.denoise(R.firefly(noisy), **agd)))
            torch.cuda.synchronize()
        lines.append(f"\n{scene}: {packed.n_hittables} hittables")
        row("spp", SPPS)
        for k, v in cols.items():
            row(k, v)
        # the temporal sequence: the last accumulated frame against the last noisy one, both against a reference at the last camera
        cells = []
        for move in MOVES:
            cams = [scenes.make_camera(dict(cam_args, look_from=tuple(float(p) + f * d for p, d in zip(cam_args["look_from"], (move, 0.0, 0.0)))), w, h)
                    for f in range(a.temporal_frames)]
            last = None
            for last in R.render_temporal(w, h, a.temporal_spp, ds, cams, aov_spp=a.aov_spp, denoise=False):
                pass
            ref_last = ref if move == 0.0 else R.render(w, h, a.ref_spp, ds, cams[-1])
            cells.append(f"{R.mse_ratio(last['temporal'], last['noisy'], ref_last):.4f}")
            torch.cuda.synchronize()
        row(f"temporal: move", [f"{m:g}" for m in MOVES])
        row(f"  {a.temporal_frames} x {a.temporal_spp} spp", cells)
        ds.close()
    lines.append(f"\n# {time.perf_counter() - t_start:.1f} s in all")
    text = "\n".join(lines) + "\n"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
