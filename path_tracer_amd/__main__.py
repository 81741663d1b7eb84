"""Command-line caller of the hot path — the role of the reference's src/main.cpp:61-197 (scene → render → PNG).

    python -m path_tracer_amd --scene cornell --width 800 --height 480 --spp 100 --out out.png
    python -m path_tracer_amd --scene cornell --spp 1024 --preview-every 64 --preview-dir previews --out out.png

    python -m path_tracer_amd --scene cornell --spp 1024 --noise-threshold 0.02 --min-spp 16 --counts-out counts.png --out out.png

With --preview-every N the frame is rendered progressively (render.Accumulator): windows of N samples, DIR/preview_<spp>.png after
each; the final --out PNG is byte-identical to the one written without these options.
With --noise-threshold T the frame is rendered adaptively (render.render_adaptive): --min-spp samples of every pixel, then windows of
--adaptive-step samples of the pixels whose noise estimate is above T, up to --spp; --counts-out writes the per-pixel counts as a grey
PNG (row 0 at the top, --spp = white).  A negative T renders every pixel to --spp: the same out.png as without the options.
With --aov-dir DIR the first-hit feature buffers a denoiser takes (render.render_aov: a pass of its own, --aov-spp camera rays per pixel)
are written next to the frame: DIR/albedo.png, DIR/normal.png (as (n + 1) / 2), DIR/coverage.png and DIR/aov.npz with all six planes
(albedo, normal, direct, depth, coverage, id; row 0 = the bottom scan-line, as the frame buffer); out.png is byte-identical to the one
written without the options.
With --denoise-out FILE the frame is also filtered by the edge-avoiding a-trous denoiser (render.denoise; --denoise-iterations and the
--denoise-sigma-* options; the defaults are include/pt_render.h's) over feature buffers of --aov-spp camera rays per pixel — the ones
--aov-dir writes, or a pass of its own — and FILE gets the filtered frame through the same output stage; out.png is byte-identical to
the one written without the option.
With --denoise-variance (needs --denoise-out and --noise-threshold) the filtered frame comes from the variance-guided filter instead
(render.denoise_variance; --denoise-sigma-variance replaces --denoise-sigma-color): its colour tolerance is each pixel's own noise
estimate, taken from the adaptive accumulator's half buffers, so one setting fits every sample count in the frame.
With --frames N --frames-dir DIR a camera path is rendered as well: frame f looks from look_from + f x --move (dx,dy,dz) and goes to
DIR/frame_<f>.png through the same output stage, --spp samples each.  With --temporal the frames come from render.render_temporal — one
adaptive accumulator continued from frame to frame (no frame repeats another's random numbers) and the history reprojected across the
camera moves (render.TemporalAccumulator) — and frame_<f>.png is the accumulated frame; with --temporal --denoise-variance it is that
frame filtered by the variance-guided filter, fed the temporal variance.  out.png is byte-identical to the one written without the
options.
With --display-out FILE the frame also goes through the display stage (render.Display; include/pt_render.h: PtDisplay) into FILE: --tone
picks the curve (reference, reinhard, aces; default aces), --exposure EV is a manual exposure in stops, and with --auto-exposure the
exposure is solved on the device from the frame's luminance histogram (--exposure is then a bias on it).  With --frames-dir and any of
these options the frame PNGs go through the display stage as well, metered in order: with --auto-exposure the exposure adapts from frame to
frame at the rates --adapt-up and --adapt-down (1 = instant, the default).  out.png is byte-identical to the one written without the
options.
With --firefly-clamp [K] the firefly stage (render.firefly; include/pt_post.h) runs on the frame before --denoise-out, --display-out and the
--frames-dir frames consume it: a pixel brighter than K times (default 1) its brightest neighbour — with --firefly-rank 2 its second
brightest — is scaled down to that, and a pixel that is not finite becomes the mean of its finite neighbours.  The clamp is biased (it
removes energy), so it is never on unless asked; the numbers of clamped and repaired pixels are printed.  out.png is byte-identical to the
one written without the options.
With --spatial-variance [RADIUS] the spatial variance estimate (render.spatial_variance; include/pt_spatial_variance.h) gives
--denoise-variance the variance of the pixels that have none, from the squared differences of adjacent pixels in a (2 RADIUS + 1)^2 window
(default: the header's radius) on the pixel's own surface: --denoise-variance then works WITHOUT --noise-threshold — the whole plane is
estimated from the plain frame —, with --noise-threshold the stage fills the pixels the half buffers give no estimate for, and with
--temporal those of a young history.  The numbers of estimated pixels and of holes (no estimate either) are printed.  out.png is
byte-identical to the one written without the option.
With --compare REF.npy the image error (render.image_error; include/pt_metrics.h) measures the frame behind out.png — and the filtered
frame of --denoise-out, if given — against a reference frame, a float32 [height][width][3] array with y = 0 the bottom row as --save-frame
FILE.npy writes it: MSE, relMSE (eps 1e-4), PSNR against a peak of 1, the pixels that took part and the skipped ones (a NaN or inf on
either side).  The sums behind them are exact and rounded once on the device, so the printed MSE does not depend on the order in which
the hardware adds.  out.png is byte-identical to the one written without the options.
With --encode srgb the files of --display-out and --frames-dir hold exact sRGB codes (render.encode; include/pt_encode.h) instead of the
reference's gamma-2 quantiser — fused with the display stage where that runs — and carry an sRGB chunk; --dither adds the 8 x 8 ordered
dither in linear light.  out.png is byte-identical to the one written without the options.
"""
import argparse
import os
import time

from . import render as R
from . import scenes
from .png import write_png


def write_aovs(aov_dir, planes) -> None:
    """DIR/albedo.png, normal.png ((n + 1) / 2) and coverage.png — linear values (guide images, not pictures: no gamma), clamped to
    [0, 0.999] and scaled by 256 like out.png, row 0 = top like out.png — and DIR/aov.npz with the six planes as rendered."""
    import numpy as np
    import torch

    os.makedirs(aov_dir, exist_ok=True)
    grey = planes["coverage"].unsqueeze(-1).expand(-1, -1, 3)
    for name, fb in (("albedo", planes["albedo"]), ("normal", (planes["normal"] + 1.0) * 0.5), ("coverage", grey)):
        rgb8 = (fb.clamp(0.0, 0.999) * 256.0).to(torch.uint8).flip(0).contiguous()
        write_png(os.path.join(aov_dir, f"{name}.png"), rgb8.cpu().numpy())
    np.savez(os.path.join(aov_dir, "aov.npz"), **{k: v.cpu().numpy() for k, v in planes.items()})


def make_shower(a):
    """The output stage of a frame -> uint8 image: the reference's (render.tonemap_rgb8) without display options; with them the display
    stage — a manual exposure, or with --auto-exposure one Display whose exposure adapts over the frames it is shown in order.  With
    --encode the bytes are the encode stage's (fused with the display stage where that runs): sRGB codes, and the files say so."""
    enc = {} if a.encode_kw is None else {"encode": a.encode_kw}  # (absent: exactly the calls there always were)
    if not a.display:
        return R.tonemap_rgb8 if a.encode_kw is None else lambda fb: R.encode(fb, **a.encode_kw)
    ev = 0.0 if a.exposure is None else a.exposure
    if not a.auto_exposure:
        return lambda fb: R.display(fb, a.tone, ev, **enc)
    disp = R.Display(a.tone, ev_bias=ev, adapt_up=1.0 if a.adapt_up is None else a.adapt_up, adapt_down=1.0 if a.adapt_down is None else a.adapt_down)
    return lambda fb: disp.meter(fb).apply(fb, **enc)


def clamp_fireflies(a, fb, what, variance=None):
    """--firefly-clamp: the frame (and its variance) through the firefly stage, the counts printed; without the option, as they came."""
    if a.firefly_kw is None:
        return (fb, variance) if variance is not None else fb
    *res, n = R.firefly(fb, variance, counts=True, **a.firefly_kw)
    print_firefly_counts(a, what, n)
    return tuple(res) if variance is not None else res[0]


def print_firefly_counts(a, what, n) -> None:
    clamped, repaired = (int(v) for v in n.cpu().numpy())
    print(f"{what}: firefly clamp (rank {a.firefly_kw['rank']}, k {a.firefly_kw['k']:g}): {clamped} pixels clamped, {repaired} repaired")


def print_variance_counts(a, what, n) -> None:
    estimated, holes = (int(v) for v in n.cpu().numpy())
    print(f"{what}: spatial variance (radius {a.spatial_kw['radius']}): {estimated} pixels estimated, {holes} holes")


def print_compare(a, what, fb, ref) -> None:
    """--compare: one line of figures for the frame `fb` against the reference (all of them from one ImageError)."""
    e = R.image_error(fb, ref)
    print(f"{what} vs {a.compare}: MSE {e.mse!r} relMSE {e.rel_mse!r} PSNR {e.psnr(1.0):.4f} dB (peak 1), {e.pixels} pixels, {e.skipped} skipped")


def write_frames(a, packed, cam_args, move, denoise_kw) -> None:
    """The camera path of --frames: DIR/frame_<f>.png, frame f looking from look_from + f x move.  Plain: render() per frame.  --temporal:
    render_temporal's accumulated frame, or with --denoise-variance that frame through the variance-guided filter.  Each frame leaves
    through make_shower's output stage, in order.  --firefly-clamp: each frame goes through the firefly stage first (--temporal: before its
    history takes it in)."""
    show = make_shower(a)
    os.makedirs(a.frames_dir, exist_ok=True)
    cams = [scenes.make_camera(dict(cam_args, look_from=tuple(float(p) + f * d for p, d in zip(cam_args["look_from"], move))), a.width, a.height)
            for f in range(a.frames)]
    if not a.temporal:
        for f, c in enumerate(cams):
            fb = clamp_fireflies(a, R.render(a.width, a.height, a.spp, packed, c, a.depth), f"frame {f}")
            write_png(os.path.join(a.frames_dir, f"frame_{f}.png"), show(fb).cpu().numpy(), **a.png_kw)
        return
    extra = {} if a.firefly_kw is None else {"firefly": a.firefly_kw}  # (absent: render_temporal issues exactly the calls it always did)
    if a.spatial_kw is not None:
        extra["spatial_variance"] = a.spatial_kw
    for f, frame in enumerate(R.render_temporal(a.width, a.height, a.spp, packed, cams, a.depth, aov_spp=a.aov_spp, denoise=a.denoise_variance,
                                                denoise_kw=denoise_kw, **extra)):
        if a.firefly_kw is not None:
            print_firefly_counts(a, f"frame {f}", frame["firefly_counts"])
        if a.spatial_kw is not None:
            print_variance_counts(a, f"frame {f}", frame["variance_counts"])
        write_png(os.path.join(a.frames_dir, f"frame_{f}.png"), show(frame["filtered" if a.denoise_variance else "temporal"]).cpu().numpy(), **a.png_kw)


def main() -> None:
    ap = argparse.ArgumentParser(prog="python -m path_tracer_amd")
    ap.add_argument("--scene", default="smoke", choices=["smoke", "cornell", "triangles"],
                    help="smoke = the default scene of the reference's main.cpp")
    ap.add_argument("--width", type=int, default=800)    # CMakeLists.txt:44-54 defaults
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--spp", type=int, default=100)      # main.cpp:186
    ap.add_argument("--depth", type=int, default=50)     # render.hpp:144
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--out", default="out.png")          # main.cpp:57
    ap.add_argument("--textures", default="reference", choices=["reference", "procedural"],
                    help="smoke scene: the decoded reference images (tests/golden/cfg1_textures.npz) or generated stand-ins")
    ap.add_argument("--export-textures", metavar="DIR", help="write Xilinx.ppm / SYCL.ppm for the C++ host and exit (no GPU)")
    ap.add_argument("--preview-every", type=int, default=0, metavar="N",
                    help="render in windows of N samples and write a preview PNG after each (progressive rendering)")
    ap.add_argument("--preview-dir", default="previews", metavar="DIR", help="where --preview-every writes preview_<spp>.png")
    ap.add_argument("--noise-threshold", type=float, default=None, metavar="T",
                    help="adaptive sampling: render each pixel until its noise estimate is <= T (--spp is the maximum)")
    ap.add_argument("--min-spp", type=int, default=None, metavar="N", help="adaptive sampling: samples of every pixel (default 16)")
    ap.add_argument("--adaptive-step", type=int, default=None, metavar="N", help="adaptive sampling: samples per window (default --min-spp)")
    ap.add_argument("--counts-out", default=None, metavar="PATH", help="adaptive sampling: grey PNG of the per-pixel sample counts")
    ap.add_argument("--aov-dir", default=None, metavar="DIR",
                    help="also write first-hit feature buffers for a denoiser: DIR/albedo.png, normal.png, coverage.png, aov.npz")
    ap.add_argument("--aov-spp", type=int, default=None, metavar="N", help="feature buffers: camera rays per pixel (default 16)")
    ap.add_argument("--denoise-out", default=None, metavar="FILE",
                    help="also write the frame filtered by the a-trous denoiser (guided by feature buffers of --aov-spp rays per pixel)")
    ap.add_argument("--denoise-iterations", type=int, default=None, metavar="N", help="denoiser: a-trous levels, 1 .. 8 (default 5)")
    for term in ("color", "normal", "depth", "albedo"):
        ap.add_argument(f"--denoise-sigma-{term}", type=float, default=None, metavar="S",
                        help=f"denoiser: sigma of the {term} term, <= 0 turns it off (default: include/pt_render.h)")
    ap.add_argument("--denoise-variance", action="store_true",
                    help="denoiser: the variance-guided filter over the adaptive accumulator's noise estimate (needs --noise-threshold)")
    ap.add_argument("--denoise-sigma-variance", type=float, default=None, metavar="S",
                    help="variance-guided denoiser: colour tolerance in standard deviations, <= 0 turns it off (default: include/pt_render.h)")
    ap.add_argument("--frames", type=int, default=None, metavar="N", help="also render a camera path of N frames into --frames-dir")
    ap.add_argument("--move", default=None, metavar="DX,DY,DZ", help="camera path: look_from moves by this per frame (default 0,0,0)")
    ap.add_argument("--frames-dir", default=None, metavar="DIR", help="camera path: where frame_<f>.png goes")
    ap.add_argument("--temporal", action="store_true",
                    help="camera path: carry each frame's history across the camera moves (temporal reprojection)")
    ap.add_argument("--tone", default=None, choices=["reference", "reinhard", "aces"], help="display stage: the tone curve (default aces)")
    ap.add_argument("--exposure", type=float, default=None, metavar="EV",
                    help="display stage: exposure in stops (manual; with --auto-exposure a bias on the metered exposure)")
    ap.add_argument("--auto-exposure", action="store_true", help="display stage: solve the exposure from the frame's luminance histogram")
    ap.add_argument("--adapt-up", type=float, default=None, metavar="A", help="auto-exposure over --frames: rate towards a higher exposure, in (0, 1]")
    ap.add_argument("--adapt-down", type=float, default=None, metavar="A", help="auto-exposure over --frames: rate towards a lower exposure, in (0, 1]")
    ap.add_argument("--display-out", default=None, metavar="FILE", help="also write the frame through the display stage (exposure + tone curve)")
    ap.add_argument("--encode", default=None, choices=["srgb"],
                    help="encode stage: write --display-out and the --frames-dir frames as exact sRGB codes (tagged sRGB) instead of the "
                         "reference's gamma-2 quantiser; out.png stays as it is")
    ap.add_argument("--dither", action="store_true", help="encode stage: 8 x 8 ordered dither in linear light (needs --encode srgb)")
    ap.add_argument("--firefly-clamp", type=float, nargs="?", const=1.0, default=None, metavar="K",
                    help="firefly stage: scale a pixel brighter than K x (default 1) its brightest neighbour down to that, repair NaN / inf; "
                         "acts on what --denoise-out, --display-out and --frames-dir consume (biased: off unless given)")
    ap.add_argument("--firefly-rank", type=int, default=None, metavar="R", help="firefly stage: 1 = the brightest neighbour (default), 2 = the second brightest")
    ap.add_argument("--spatial-variance", type=int, nargs="?", const=R.abi.PT_SVAR_DEFAULT_RADIUS, default=None, metavar="RADIUS",
                    help=f"spatial variance estimate: give --denoise-variance a variance where there is none, from a (2 RADIUS + 1)^2 window "
                         f"(1 .. {R.abi.PT_SVAR_MAX_RADIUS}, default {R.abi.PT_SVAR_DEFAULT_RADIUS}); --denoise-variance then needs no --noise-threshold")
    ap.add_argument("--compare", default=None, metavar="REF.npy",
                    help="image error: print MSE, relMSE, PSNR and the skipped pixels of the frame behind --out (and of --denoise-out) against "
                         "this float32 [height][width][3] frame")
    ap.add_argument("--save-frame", default=None, metavar="FILE.npy", help="write the frame behind --out as float32 [height][width][3] (a reference for --compare)")
    a = ap.parse_args()
    if a.save_frame is not None and not a.save_frame.endswith(".npy"):
        ap.error("--save-frame needs a file name that ends in .npy")
    if a.compare is not None:
        if a.save_frame is not None and os.path.abspath(a.compare) == os.path.abspath(a.save_frame):
            ap.error("--compare and --save-frame name the same file")
        import numpy as np
        try:
            ref_frame = np.load(a.compare, mmap_mode="r", allow_pickle=False)
        except (OSError, ValueError) as e:
            ap.error(f"--compare: cannot read {a.compare}: {e}")
        if ref_frame.dtype != np.float32 or ref_frame.shape != (a.height, a.width, 3):
            ap.error(f"--compare: {a.compare} holds {ref_frame.dtype} {list(ref_frame.shape)}, not float32 [{a.height}, {a.width}, 3] (--height, --width)")
    if a.dither and a.encode is None:
        ap.error("--dither needs --encode srgb")
    if a.encode is not None and a.display_out is None and a.frames_dir is None:
        ap.error("--encode and --dither need --display-out or --frames-dir")
    a.encode_kw = None if a.encode is None else dict(transfer=a.encode, dither=a.dither)
    a.png_kw = {} if a.encode is None else {"srgb": True}
    if a.spatial_variance is not None and not a.denoise_variance:
        ap.error("--spatial-variance needs --denoise-variance (the filter that takes the variance)")
    if a.spatial_variance is not None and not 1 <= a.spatial_variance <= R.abi.PT_SVAR_MAX_RADIUS:
        ap.error(f"--spatial-variance must be in 1 .. {R.abi.PT_SVAR_MAX_RADIUS}")
    a.spatial_kw = None if a.spatial_variance is None else dict(radius=a.spatial_variance)
    if a.firefly_rank is not None and a.firefly_clamp is None:
        ap.error("--firefly-rank needs --firefly-clamp")
    if a.firefly_clamp is not None and a.denoise_out is None and a.display_out is None and a.frames_dir is None:
        ap.error("--firefly-clamp needs --denoise-out, --display-out or --frames-dir")
    if a.firefly_clamp is not None and not (0.0 < a.firefly_clamp < float("inf")):
        ap.error("--firefly-clamp must be finite and > 0")
    if a.firefly_rank is not None and a.firefly_rank not in (1, 2):
        ap.error("--firefly-rank must be 1 or 2")
    a.firefly_kw = None if a.firefly_clamp is None else dict(rank=1 if a.firefly_rank is None else a.firefly_rank, k=a.firefly_clamp)
    a.display = a.tone is not None or a.exposure is not None or a.auto_exposure or a.adapt_up is not None or a.adapt_down is not None
    if a.display and a.display_out is None and a.frames_dir is None:
        ap.error("--tone, --exposure, --auto-exposure, --adapt-up and --adapt-down need --display-out or --frames-dir")
    a.display = a.display or a.display_out is not None
    a.tone = "aces" if a.tone is None else a.tone
    if (a.adapt_up is not None or a.adapt_down is not None) and not a.auto_exposure:
        ap.error("--adapt-up and --adapt-down need --auto-exposure")
    if any(v is not None and not 0.0 < v <= 1.0 for v in (a.adapt_up, a.adapt_down)):
        ap.error("--adapt-up and --adapt-down must be in (0, 1]")
    if a.exposure is not None and not -32.0 <= a.exposure <= 32.0:
        ap.error("--exposure must be in -32 .. 32")
    if a.frames is None and (a.move is not None or a.frames_dir is not None or a.temporal):
        ap.error("--move, --frames-dir and --temporal need --frames")
    move = (0.0, 0.0, 0.0)
    if a.frames is not None:
        if a.frames < 1:
            ap.error("--frames must be >= 1")
        if a.frames_dir is None:
            ap.error("--frames needs --frames-dir")
        if a.move is not None:
            try:
                move = tuple(float(v) for v in a.move.split(","))
            except ValueError:
                move = ()
            if len(move) != 3 or any(v != v or v in (float("inf"), float("-inf")) for v in move):
                ap.error("--move must be three finite numbers dx,dy,dz")
        if a.spp < 1:
            ap.error("--frames needs --spp >= 1")
    temporal_filter = a.temporal and a.denoise_variance
    if temporal_filter and a.denoise_out is not None and a.noise_threshold is None and a.spatial_kw is None:
        ap.error("--denoise-out with --denoise-variance needs --noise-threshold (without --denoise-out, --temporal --denoise-variance filters the frames only)")
    if a.denoise_variance and a.noise_threshold is None and not a.temporal and a.spatial_kw is None:
        ap.error("--denoise-variance needs --noise-threshold (the variance comes from the adaptive accumulator's half buffers)")
    if a.denoise_variance and a.denoise_out is None and not a.temporal:
        ap.error("--denoise-variance needs --denoise-out")
    if a.denoise_sigma_variance is not None and not a.denoise_variance:
        ap.error("--denoise-sigma-variance needs --denoise-variance")
    if a.denoise_variance and a.denoise_sigma_color is not None:
        ap.error("--denoise-sigma-color does not apply to --denoise-variance (use --denoise-sigma-variance)")
    denoise_kw = {k: v for k, v in (("iterations", a.denoise_iterations), ("sigma_color", a.denoise_sigma_color),
                                    ("sigma_variance", a.denoise_sigma_variance),
                                    ("sigma_normal", a.denoise_sigma_normal), ("sigma_depth", a.denoise_sigma_depth),
                                    ("sigma_albedo", a.denoise_sigma_albedo)) if v is not None}
    if denoise_kw and a.denoise_out is None and not temporal_filter:
        ap.error("--denoise-iterations and --denoise-sigma-* need --denoise-out")
    if a.denoise_iterations is not None and not 1 <= a.denoise_iterations <= 8:
        ap.error("--denoise-iterations must be in 1 .. 8")
    if any(v != v or v in (float("inf"), float("-inf")) for k, v in denoise_kw.items() if k != "iterations"):
        ap.error("--denoise-sigma-* must be finite")
    if a.aov_spp is not None and a.aov_dir is None and a.denoise_out is None and not a.temporal:
        ap.error("--aov-spp needs --aov-dir")
    a.aov_spp = 16 if a.aov_spp is None else a.aov_spp
    if not 1 <= a.aov_spp <= 1 << 24:
        ap.error(f"--aov-spp must be in 1 .. {1 << 24}")
    if a.preview_every < 0:
        ap.error("--preview-every must be >= 0")
    adaptive = a.noise_threshold is not None
    if not adaptive and (a.min_spp is not None or a.adaptive_step is not None or a.counts_out is not None):
        ap.error("--min-spp, --adaptive-step and --counts-out need --noise-threshold")
    if adaptive:
        if a.preview_every > 0:
            ap.error("--noise-threshold cannot be combined with --preview-every")
        a.min_spp = 16 if a.min_spp is None else a.min_spp
        a.adaptive_step = a.min_spp if a.adaptive_step is None else a.adaptive_step
        if a.min_spp <= 0 or a.adaptive_step <= 0:
            ap.error("--min-spp and --adaptive-step must be > 0")
        if a.spp < a.min_spp or (a.spp - a.min_spp) % a.adaptive_step != 0:
            ap.error(f"--spp ({a.spp}) must be --min-spp ({a.min_spp}) plus a multiple of --adaptive-step ({a.adaptive_step})")
    if a.export_textures:
        print(*scenes.export_reference_textures(a.export_textures), sep="\n")
        return
    import numpy as np
    import torch

    kw = {"n_triangles": a.triangles} if a.scene == "triangles" else {"textures": a.textures} if a.scene == "smoke" else {}
    packed, cam_args = scenes.build(a.scene, **kw)
    cam = scenes.make_camera(cam_args, a.width, a.height)
    t0 = time.perf_counter()
    mean_spp = None
    variance = [None]  # (the adaptive path's estimate; --spatial-variance makes or completes it)
    if adaptive:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fb, counts, *estimate = R.render_adaptive(a.width, a.height, packed, cam, a.depth, threshold=a.noise_threshold, min_spp=a.min_spp,
                                                  max_spp=a.spp, step=a.adaptive_step, variance=a.denoise_variance)
        e1.record()
        variance = estimate or variance
        rgb8 = R.tonemap_rgb8(fb)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        counts = counts.cpu().numpy()
        mean_spp = float(counts.mean())
        if a.counts_out:
            grey = np.round(counts[::-1].astype(np.float64) * (255.0 / a.spp)).astype(np.uint8)  # row 0 = top, like out.png
            write_png(a.counts_out, np.repeat(grey[:, :, None], 3, axis=2))
    elif a.preview_every > 0:
        os.makedirs(a.preview_dir, exist_ok=True)
        acc = R.Accumulator(a.width, a.height, packed, cam, a.depth)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = 0.0
        while acc.samples < a.spp:
            e0.record()
            acc.add(min(a.preview_every, a.spp - acc.samples))
            e1.record()
            rgb8 = acc.tonemap_rgb8()
            torch.cuda.synchronize()
            ms += e0.elapsed_time(e1)
            write_png(os.path.join(a.preview_dir, f"preview_{acc.samples}.png"), rgb8.cpu().numpy())
        fb = acc.resolve() if a.denoise_out or a.display_out or a.compare or a.save_frame else None
        acc.close()
    else:
        fb, ms = R.render(a.width, a.height, a.spp, packed, cam, a.depth, timed=True)
        rgb8 = R.tonemap_rgb8(fb)
    torch.cuda.synchronize()
    write_png(a.out, rgb8.cpu().numpy())
    if a.save_frame:
        np.save(a.save_frame, fb.cpu().numpy())
    ref = torch.from_numpy(np.ascontiguousarray(ref_frame)).cuda() if a.compare else None
    if a.compare:
        print_compare(a, a.out, fb, ref)
    planes = R.render_aov(a.width, a.height, a.aov_spp, packed, cam) if a.aov_dir or a.denoise_out else None
    if a.aov_dir:
        write_aovs(a.aov_dir, planes)
    if a.denoise_out or a.display_out:
        if a.denoise_out and a.denoise_variance and variance[0] is not None:
            fb, variance[0] = clamp_fireflies(a, fb, "frame", variance[0])
        else:
            fb = clamp_fireflies(a, fb, "frame")
    if a.denoise_out and a.spatial_kw is not None:
        variance[0], n_var = R.spatial_variance(fb, variance[0], out=variance[0], counts=True, **planes, **a.spatial_kw)
        print_variance_counts(a, "frame", n_var)
    if a.denoise_out:
        filtered = R.denoise_variance(fb, variance[0], **planes, **denoise_kw) if a.denoise_variance else R.denoise(fb, **planes, **denoise_kw)
        write_png(a.denoise_out, R.tonemap_rgb8(filtered).cpu().numpy())
        if a.compare:
            print_compare(a, a.denoise_out, filtered, ref)
    if a.display_out:
        write_png(a.display_out, make_shower(a)(fb).cpu().numpy(), **a.png_kw)
    if a.frames is not None:
        write_frames(a, packed, cam_args, move, denoise_kw)
    if mean_spp is not None:
        n = int(counts.sum())
        print(f"{a.scene}: {packed.n_hittables} hittables, {a.width}x{a.height}, adaptive {a.min_spp}..{a.spp} spp (threshold "
              f"{a.noise_threshold:g}), mean {mean_spp:.1f} spp -> {a.out}; {ms:.1f} ms = {n / ms / 1e3:.1f} Msamples/s "
              f"(wall {time.perf_counter() - t0:.2f} s)")
        return
    n = a.width * a.height * a.spp
    print(f"{a.scene}: {packed.n_hittables} hittables, {a.width}x{a.height}x{a.spp} spp -> {a.out}; "
          f"kernel {ms:.1f} ms = {n / ms / 1e3:.1f} Msamples/s (wall {time.perf_counter() - t0:.2f} s)")


if __name__ == "__main__":
    main()
