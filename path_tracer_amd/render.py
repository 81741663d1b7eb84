"""render() — the host-side mirror of the reference's hot-path entry point, over the C ABI.

Reference: `render<width,height,samples>(queue, frame_buf, hittables, cam)` include/render.hpp:141-160.
Here:      `render(width, height, samples, scene, cam, depth=50, ...) -> torch.Tensor [H][W][3]` on the GPU.

PyTorch is plumbing only: it owns the device framebuffer, the current HIP stream and (for N GPUs)
the RCCL process group.  All arithmetic happens in the hand-written gfx950 kernels of
`csrc/pt_render.hip`, reached through `include/pt_render.h`.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from . import abi
from .scene import PackedScene, camera, pack


class DeviceScene:
    """The flattened, HBM-resident scene (pt_scene_create).  Replaces the sycl::buffer wrapping of the
    hittable vector and image_texture::freeze() (render.hpp:146-148); may be reused across renders."""

    def __init__(self, scene: PackedScene, tuning: "abi.PtTuning | None" = None):
        """tuning: an abi.PtTuning (performance-only knobs, include/pt_render.h; abi.tuning(sphere_grid=-1, ...)); None = the
        library's defaults with the PT_* environment applied."""
        self.lib = abi.load_library()
        self.handle = C.c_void_p()
        self._packed = scene  # keep the host tables alive
        if tuning is None:
            abi.check(self.lib.pt_scene_create(C.byref(scene.desc), C.byref(self.handle)), "pt_scene_create")
        else:
            abi.check(self.lib.pt_scene_create_tuned(C.byref(scene.desc), C.byref(tuning), C.byref(self.handle)), "pt_scene_create_tuned")

    def reserve(self, width, height, samples, depth=50, shard_index=0, shard_count=1, flags=0) -> None:
        """pt_scene_reserve: allocate the launch workspaces for these parameters now, so that render() never allocates."""
        p = _params(width, height, samples, depth, shard_index, shard_count, flags)
        abi.check(self.lib.pt_scene_reserve(self.handle, C.byref(p)), "pt_scene_reserve")

    def close(self):
        if self.handle:
            self.lib.pt_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def _params(width, height, samples, depth, shard_index=0, shard_count=1, flags=0) -> abi.PtRenderParams:
    return abi.PtRenderParams(int(width), int(height), int(samples), int(depth), int(shard_index), int(shard_count),
                              int(flags), 0)


_DEVICE_SCENE_CACHE = 4  # device scenes kept per PackedScene (one per (device, stream) in use)


def _as_device_scene(scene, cache_key=None) -> DeviceScene:
    """DeviceScene of whatever the caller handed over.  With `cache_key` (the asynchronous torch path) the device scene of a
    PackedScene is kept on it, per (device, stream): no re-flatten / re-upload / hipMalloc per call, and — the point — no temporary
    whose destructor (pt_scene_destroy -> hipFree, an implicit device synchronisation) would run while the kernels it
    launched are still in flight."""
    if isinstance(scene, DeviceScene):
        return scene
    if not isinstance(scene, PackedScene):
        scene = pack(scene)  # a list of hittables, like std::vector<hittable_t>
        cache_key = None
    if cache_key is None:
        return DeviceScene(scene)
    # a small LRU per PackedScene: a device scene holds a full copy of the flattened scene (25 MB for the 100 k-triangle mesh) plus
    # launch workspaces, and the key contains the raw stream handle — programs that create streams on the fly must not pile up a
    # copy per stream that ever existed (a handle reused after its stream died aliases at worst a scene that is still valid: scene
    # data is immutable and its workspaces are only touched in launch order of whichever stream uses them next)
    cache = scene.__dict__.setdefault("_pt_device_scenes", {})
    if cache_key in cache:
        cache[cache_key] = cache.pop(cache_key)  # most recently used last
        return cache[cache_key]
    while len(cache) >= _DEVICE_SCENE_CACHE:
        cache.pop(next(iter(cache)))  # destroyed when the last frame that references it is gone (DeviceScene.__del__)
    cache[cache_key] = DeviceScene(scene)
    return cache[cache_key]


def _stream_ptr(torch) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the image stages' host prelude: what every stage below checks before it calls the library; a new stage is written against it --------

def _stage(me, has, what, entry):
    """A stage's first two checks — a HIP device, and a library that has the stage (`has`: abi.has_*) — and the library."""
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError(f"path_tracer_amd.{me} needs a HIP device: there is no CPU path in the product")
    lib = abi.load_library()
    if not has(lib):
        raise ImportError(f"{abi.library_path()} predates {what} (no {entry})")
    return lib


def _aov_kwargs_ok(me, other_planes) -> None:
    """`**other_planes` takes render_aov()'s planes that the stage does not use, and nothing else."""
    unknown = set(other_planes) - set(abi.AOV_PLANES)
    if unknown:
        raise TypeError(f"{me}() got unexpected keyword arguments {sorted(unknown)}")


def _whole_frame(fb):
    """(H, W) of a frame [H][W][3]."""
    if fb is None or fb.dim() != 3 or fb.shape[2] != 3:
        raise ValueError("fb must be a whole frame [H][W][3] (gather and unshard a multi-GPU frame first)")
    return int(fb.shape[0]), int(fb.shape[1])


def _plane(t, shape, what, dtype=None):
    """None -> None; a contiguous CUDA tensor of `shape` (an int: of that many elements) and `dtype` (float32 unless given; a tuple: any of
    them) -> its pointer."""
    import torch

    if t is None:
        return None
    dtypes = dtype if isinstance(dtype, tuple) else (dtype or torch.float32,)
    fits = t.numel() == shape if isinstance(shape, int) else tuple(t.shape) == shape
    if not fits or t.dtype not in dtypes or not t.is_cuda or not t.is_contiguous():
        names = " (or ".join(str(d).replace("torch.", "") for d in dtypes) + ")" * (len(dtypes) - 1)
        raise ValueError(f"{what} must be a contiguous {names} CUDA tensor of " + (f"{shape} elements" if isinstance(shape, int) else f"shape {shape}"))
    return C.c_void_p(t.data_ptr())


def _frame_ptr(fb, what="fb"):
    """_plane() for a frame whose size is not known yet."""
    import torch

    if fb is None or fb.dim() != 3 or fb.shape[2] != 3 or fb.dtype != torch.float32 or not fb.is_cuda or not fb.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 CUDA tensor of shape [H][W][3]")
    return C.c_void_p(fb.data_ptr())


def _optional_out(arg, shape, dtype, what, device):
    """An optional output: True allocates it (`dtype`, or the first of a tuple), a tensor is checked and written, False / None give None."""
    import torch

    if arg is None or arg is False:
        return None
    if arg is True:
        return torch.empty(shape, dtype=dtype[0] if isinstance(dtype, tuple) else dtype, device=device)
    _plane(arg, shape, what, dtype)
    return arg


def _counts(arg, device):
    """The `counts=` of firefly() and spatial_variance(): two uint32 words (an int32 tensor is taken too)."""
    import torch

    return _optional_out(arg, 2, (torch.uint32, torch.int32), "counts", device)


def _stage_kw(arg, who, name, allowed):
    """The `firefly=` / `spatial=` / `spatial_variance=` keyword of the hosts that take one: None / False -> None (the stage is not run),
    True -> {} (the defaults), a dict -> the stage's keyword arguments, of `allowed`."""
    if arg is None or arg is False:
        return None
    if arg is True:
        return {}
    if isinstance(arg, dict) and not set(arg) - set(allowed):
        return dict(arg)
    raise TypeError(f"{who}: {name} must be True or a dict of {', '.join(allowed)}")


_FIREFLY_KW = ("rank", "k", "repair", "no_lds")
_SPATIAL_KW = ("radius", "min_pairs", "tol_depth", "tol_normal", "demodulate", "no_lds")


def render(width: int, height: int, samples: int, scene, cam: camera, depth: int = 50, *, flags: int = 0,
           out=None, shard_index: int = 0, shard_count: int = 1, timed: bool = False):
    """Launch the render kernel on torch's current device/stream; asynchronous like queue.submit
    (render.hpp:151) unless `timed`.  `scene`: a DeviceScene (reuse it across renders), a PackedScene (its device scene is
    created once per device and kept on it) or a list of hittables (packed + uploaded for this call; kept alive by the
    returned tensor).  Returns the framebuffer tensor — [H][W][3] float32, y=0 bottom
    row — or, for shard_count>1, this shard's tiles [tiles][64][3].  With `timed`, returns
    (tensor, kernel_ms) measured with HIP events on the launch stream."""
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("path_tracer_amd.render needs a HIP device: there is no CPU path in the product")
    lib = abi.load_library()
    # one device scene per (device, stream): a PtScene owns per-scene launch workspaces (tile costs / order / partial sums),
    # so renders on ONE PtScene must be stream-ordered (include/pt_render.h); two streams get two scenes
    ds = _as_device_scene(scene, cache_key=("cuda", torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream))
    p = _params(width, height, samples, depth, shard_index, shard_count, flags)
    n = lib.pt_framebuffer_floats(C.byref(p))
    if n < 0:
        abi.check(abi.PT_ERR_INVALID_ARG, "pt_framebuffer_floats")
    shape = (height, width, 3) if shard_count == 1 else (n // (abi.PT_TILE_PIXELS * 3), abi.PT_TILE_PIXELS, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device="cuda")
    elif out.numel() != n or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 CUDA tensor of pt_framebuffer_floats() elements")
    if timed:
        ms = C.c_float()
        abi.check(lib.pt_render_timed(ds.handle, C.byref(cam.c), C.byref(p), C.c_void_p(out.data_ptr()),
                                      _stream_ptr(torch), C.byref(ms)), "pt_render_timed")
        return out, float(ms.value)
    abi.check(lib.pt_render(ds.handle, C.byref(cam.c), C.byref(p), C.c_void_p(out.data_ptr()), _stream_ptr(torch)),
              "pt_render")
    out._pt_scene = ds  # a scene built from a list of hittables lives as long as the frame it is still rendering into
    return out


def render_aov(width: int, height: int, samples: int, scene, cam: camera, *, planes=abi.AOV_PLANES, shard_index: int = 0,
               shard_count: int = 1) -> dict:
    """First-hit feature buffers (include/pt_render.h: pt_render_aov) — guide images for a denoiser, mattes for compositing: the
    reference's render at depth 1 with the first bounce's record kept, `samples` camera rays per pixel from the pixel's own stream, a
    pass of its own that needs nothing from render().  Asynchronous on torch's current stream.  `scene`: as for render().
    Returns {plane: tensor} for the `planes` asked for: albedo, normal, direct float32 [H][W][3] (y = 0 the bottom row), depth,
    coverage float32 [H][W], id int32 [H][W] — for shard_count > 1 this shard's tiles, [tiles][64][3] and [tiles][64]."""
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("path_tracer_amd.render_aov needs a HIP device: there is no CPU path in the product")
    lib = abi.load_library()
    if not abi.has_aov(lib):
        raise ImportError(f"{abi.library_path()} predates the feature buffers (no pt_render_aov entry point)")
    planes = tuple(planes)
    unknown = [k for k in planes if k not in abi.AOV_CHANNELS]
    if unknown or not planes or len(set(planes)) != len(planes):
        raise ValueError(f"planes must be a non-empty selection of {abi.AOV_PLANES} without repeats, not {planes}")
    ds = _as_device_scene(scene, cache_key=("cuda", torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream))
    p = _params(width, height, samples, 1, shard_index, shard_count, 0)
    n = lib.pt_aov_plane_elems(C.byref(p), 1)
    if n < 0:
        abi.check(abi.PT_ERR_INVALID_ARG, "pt_aov_plane_elems")
    shape = (height, width) if shard_count == 1 else (n // abi.PT_TILE_PIXELS, abi.PT_TILE_PIXELS)
    bufs = abi.PtAovBuffers(struct_size=C.sizeof(abi.PtAovBuffers))
    out = {}
    for k in planes:
        out[k] = torch.empty(shape + ((3,) if abi.AOV_CHANNELS[k] == 3 else ()), dtype=torch.int32 if k == "id" else torch.float32, device="cuda")
        setattr(bufs, k, out[k].data_ptr())
    abi.check(lib.pt_render_aov(ds.handle, C.byref(cam.c), C.byref(p), C.byref(bufs), _stream_ptr(torch)), "pt_render_aov")
    for t in out.values():
        t._pt_scene = ds  # a scene built from a list of hittables lives as long as the planes it is still rendering into
    return out


def _filter_call(me, entry, has, stage, fb, out, other_planes, **needed):
    """What denoise() and denoise_variance() (`me`) do before they call `entry`: the device and entry-point checks, the unknown keywords,
    the frame's shape, the planes in `needed` that must not be None, `out` and the scratch.  Returns the library, H, W, out, the scratch
    tensor (the caller keeps it alive across the call) and the stream."""
    import torch

    lib = _stage(me, has, f"the {stage}", f"{entry} entry point")
    _aov_kwargs_ok(me, other_planes)
    h, w = _whole_frame(fb)
    for what, t in needed.items():
        if t is None:
            raise ValueError(f"{what} must be a contiguous float32 CUDA tensor shaped like fb")
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.float32, device=fb.device)
    n = getattr(lib, entry + "_scratch_floats")(w, h)
    if n < 0:
        abi.check(abi.PT_ERR_INVALID_ARG, entry + "_scratch_floats")
    return lib, h, w, out, torch.empty(n, dtype=torch.float32, device=fb.device), _stream_ptr(torch)


def denoise(fb, *, albedo=None, normal=None, depth=None, iterations: int = abi.PT_DENOISE_DEFAULT_ITERATIONS,
            sigma_color: float = abi.PT_DENOISE_DEFAULT_SIGMA_COLOR, sigma_normal: float = abi.PT_DENOISE_DEFAULT_SIGMA_NORMAL,
            sigma_depth: float = abi.PT_DENOISE_DEFAULT_SIGMA_DEPTH, sigma_albedo: float = abi.PT_DENOISE_DEFAULT_SIGMA_ALBEDO,
            demodulate: bool = True, no_lds: bool = False, out=None, **other_planes):
    """The edge-avoiding a-trous filter over a finished frame (include/pt_render.h: pt_denoise), guided by the feature buffers:
    denoise(fb, **render_aov(...)) — the planes the filter does not take (direct, coverage, id) are ignored.  `fb`: [H][W][3] float32
    on the GPU, as render() returns it for a whole frame; albedo, normal [H][W][3], depth [H][W]: each optional; a sigma <= 0 turns
    its term off; `demodulate` (needs albedo) filters color / (albedo + 1e-3) and multiplies the albedo back, so textures stay sharp.
    `no_lds`: the A/B switch PT_DENOISE_NO_LDS (every tap from global memory; the same bits).
    Asynchronous on torch's current stream; torch allocates the scratch.  Returns the filtered frame — `out` if given, which may be
    `fb` itself."""
    lib, h, w, out, scratch, stream = _filter_call("denoise", "pt_denoise", abi.has_denoise, "denoiser", fb, out, other_planes)
    p = abi.PtDenoiseParams(C.sizeof(abi.PtDenoiseParams), w, h, int(iterations), float(sigma_color), float(sigma_normal), float(sigma_depth),
                            float(sigma_albedo), (abi.PT_DENOISE_DEMODULATE if demodulate else 0) | (abi.PT_DENOISE_NO_LDS if no_lds else 0), 0)
    abi.check(lib.pt_denoise(C.byref(p), _plane(fb, (h, w, 3), "fb"), _plane(albedo, (h, w, 3), "albedo"), _plane(normal, (h, w, 3), "normal"),
                             _plane(depth, (h, w), "depth"), _plane(out, (h, w, 3), "out"), C.c_void_p(scratch.data_ptr()), stream), "pt_denoise")
    return out


def denoise_variance(fb, variance, *, albedo=None, normal=None, depth=None, iterations: int = abi.PT_VDENOISE_DEFAULT_ITERATIONS,
                     sigma_variance: float = abi.PT_VDENOISE_DEFAULT_SIGMA_VARIANCE, sigma_normal: float = abi.PT_VDENOISE_DEFAULT_SIGMA_NORMAL,
                     sigma_depth: float = abi.PT_VDENOISE_DEFAULT_SIGMA_DEPTH, sigma_albedo: float = abi.PT_VDENOISE_DEFAULT_SIGMA_ALBEDO,
                     demodulate: bool = True, no_lds: bool = False, out=None, variance_out=None, **other_planes):
    """The variance-guided a-trous filter (include/pt_render.h: pt_variance_denoise): denoise() with the colour tolerance taken per pixel
    from `variance` — the variance of each pixel's mean, [H][W][3] float32 on the GPU, from Accumulator.variance() or anywhere else —
    so one setting fits every sample count in an adaptive frame: denoise_variance(acc.resolve(), acc.variance(), **render_aov(...)).
    The planes, their checks, `demodulate` and `no_lds` (PT_VDENOISE_NO_LDS) are denoise()'s; `sigma_variance` is the colour tolerance
    in standard deviations (<= 0: guide-only).  `variance_out` (optional, may be `variance`) receives the filtered frame's residual
    variance.  Asynchronous on torch's current stream; torch allocates the scratch.  Returns the filtered frame — `out` if given, which
    may be `fb` itself."""
    lib, h, w, out, scratch, stream = _filter_call("denoise_variance", "pt_variance_denoise", abi.has_variance_denoise,
                                                   "variance-guided denoiser", fb, out, other_planes, variance=variance)
    p = abi.PtVarianceDenoiseParams(C.sizeof(abi.PtVarianceDenoiseParams), w, h, int(iterations), float(sigma_variance), float(sigma_normal),
                                    float(sigma_depth), float(sigma_albedo),
                                    (abi.PT_VDENOISE_DEMODULATE if demodulate else 0) | (abi.PT_VDENOISE_NO_LDS if no_lds else 0), 0)
    abi.check(lib.pt_variance_denoise(C.byref(p), _plane(fb, (h, w, 3), "fb"), _plane(variance, (h, w, 3), "variance"),
                                      _plane(albedo, (h, w, 3), "albedo"), _plane(normal, (h, w, 3), "normal"), _plane(depth, (h, w), "depth"),
                                      _plane(out, (h, w, 3), "out"), _plane(variance_out, (h, w, 3), "variance_out"),
                                      C.c_void_p(scratch.data_ptr()), stream), "pt_variance_denoise")
    return out


def firefly(fb, variance=None, *, rank: int = abi.PT_FIREFLY_DEFAULT_RANK, k: float = abi.PT_FIREFLY_DEFAULT_K, repair: bool = True,
            no_lds: bool = False, out=None, variance_out=None, counts=False):
    """The firefly stage (include/pt_post.h: pt_firefly), before the filters: a pixel whose luminance exceeds `k` times the largest
    (`rank` 1) or second largest (`rank` 2) luminance among its up to eight neighbours is scaled down to that; with `repair` a pixel that
    is not finite becomes the mean of its finite neighbours.  The clamp is BIASED — it only removes energy — so nothing applies it unless
    asked.  `fb`: [H][W][3] float32 on the GPU, a whole frame; `variance` (optional): the variance of each pixel's mean, shaped like fb —
    scaled by s^2 where a pixel was scaled by s, +inf where it was repaired.  `out` must not be `fb`; `variance_out` may be `variance`.
    `no_lds`: the A/B switch PT_FIREFLY_NO_LDS (the same bits).  Asynchronous on torch's current stream.
    Returns the frame; with `variance`, (frame, variance_out); with `counts` (True, or a 2-element uint32 / int32 device tensor to write),
    the uint32 device tensor {clamped, repaired} appended — nothing is read back: .cpu() it when the numbers are wanted."""
    import torch

    lib = _stage("firefly", abi.has_firefly, "the firefly stage", "pt_firefly entry point")
    h, w = _whole_frame(fb)
    if variance is None and variance_out is not None:
        raise ValueError("variance_out needs variance")
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.float32, device=fb.device)
    if variance is not None and variance_out is None:
        variance_out = torch.empty((h, w, 3), dtype=torch.float32, device=fb.device)
    planes = [_plane(t, (h, w, 3), what) for what, t in (("fb", fb), ("variance", variance), ("out", out), ("variance_out", variance_out))]
    n = _counts(counts, fb.device)
    p = abi.PtFireflyParams(C.sizeof(abi.PtFireflyParams), w, h, int(rank), float(k),
                            (abi.PT_FIREFLY_REPAIR if repair else 0) | (abi.PT_FIREFLY_NO_LDS if no_lds else 0))
    abi.check(lib.pt_firefly(C.byref(p), *planes, C.c_void_p(n.data_ptr()) if n is not None else None, _stream_ptr(torch)), "pt_firefly")
    res = (out,) + ((variance_out,) if variance is not None else ()) + ((n.view(torch.uint32),) if n is not None else ())
    return res[0] if len(res) == 1 else res


_firefly = firefly  # (the hosts below take a keyword named `firefly`)


def spatial_variance(fb, variance=None, *, albedo=None, normal=None, depth=None, id=None, radius: int = abi.PT_SVAR_DEFAULT_RADIUS,
                     min_pairs: int = abi.PT_SVAR_DEFAULT_MIN_PAIRS, tol_depth: float = abi.PT_SVAR_DEFAULT_TOL_DEPTH,
                     tol_normal: float = abi.PT_SVAR_DEFAULT_TOL_NORMAL, demodulate=None, no_lds: bool = False, out=None, counts=False,
                     **other_planes):
    """The spatial variance estimate (include/pt_spatial_variance.h: pt_spatial_variance): the variance of each pixel's mean, estimated
    from the squared differences of adjacent pixels in a (2 `radius` + 1)^2 window over the pixels that lie on the centre's surface by the
    guides.  `fb`: [H][W][3] float32 on the GPU, a whole frame; `albedo`, `normal` [H][W][3], `depth` [H][W], `id` [H][W] int32
    (optional): its feature buffers — spatial_variance(fb, **render_aov(...)) works: the planes the stage does not take are ignored.
    `variance` (optional): a plane shaped like fb — FILL MODE: a pixel whose three values are >= 0 and finite keeps them bit for bit, the
    others (+inf "no estimate", NaN, negative) are estimated.  A pixel with fewer than `min_pairs` pairs gets +inf.  `demodulate`: estimate
    on fb / (albedo + 1e-3); None (the default) = where `albedo` is given.  `out` may be `variance`.  `no_lds`: the A/B switch
    PT_SVAR_NO_LDS (the same bits).  Asynchronous on torch's current stream.
    Returns the variance plane; with `counts` (True, or a 2-element uint32 / int32 device tensor to write), (plane, counts): the uint32
    device tensor {estimated, holes} — nothing is read back: .cpu() it when the numbers are wanted."""
    import torch

    lib = _stage("spatial_variance", abi.has_spatial_variance, "the spatial variance estimate", "pt_spatial_variance entry point")
    _aov_kwargs_ok("spatial_variance", other_planes)
    h, w = _whole_frame(fb)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.float32, device=fb.device)
    ptr = {what: _plane(t, (h, w, 3), what) for what, t in (("fb", fb), ("variance", variance), ("albedo", albedo), ("normal", normal), ("out", out))}
    ptr.update(depth=_plane(depth, (h, w), "depth"), id=_plane(id, (h, w), "id", torch.int32))
    n = _counts(counts, fb.device)
    if demodulate is None:
        demodulate = albedo is not None
    p = abi.PtSpatialVarianceParams(C.sizeof(abi.PtSpatialVarianceParams), w, h, int(radius), int(min_pairs), float(tol_depth), float(tol_normal),
                                    (abi.PT_SVAR_DEMODULATE if demodulate else 0) | (abi.PT_SVAR_NO_LDS if no_lds else 0))
    abi.check(lib.pt_spatial_variance(C.byref(p), *(ptr[k] for k in ("fb", "albedo", "normal", "depth", "id", "variance", "out")),
                                      C.c_void_p(n.data_ptr()) if n is not None else None, _stream_ptr(torch)), "pt_spatial_variance")
    return (out, n.view(torch.uint32)) if n is not None else out


_spatial_variance = spatial_variance  # (render_temporal takes a keyword named `spatial_variance`)


class ImageError:
    """What image_error() returns: the DEVICE result of one pt_image_error call (include/pt_metrics.h: PtImageErrorResult), read back on
    demand — the first property that wants a number copies the 104 bytes once (synchronising on them), and every figure comes from that
    copy.  The sums are the stage's exact sums rounded once; the derived figures are ORDINARY binary64 host arithmetic on them, in the
    order the header writes: mse = ((sum_sq.r + sum_sq.g) + sum_sq.b) / (3.0 * pixels), mae and rel_mse likewise from sum_abs and sum_rel,
    psnr(peak) = 10 log10(peak^2 / mse).  pixels = 0 gives NaN.  `plane` is the per-pixel error plane ([H][W] float32 on the device) where
    one was asked for, else None; `result` the device tensor itself (13 int64 words)."""

    def __init__(self, result, plane, scratch):
        self.result, self.plane, self._scratch, self._host = result, plane, scratch, None

    def read(self) -> "abi.PtImageErrorResult":
        """The result struct on the host (copied once)."""
        if self._host is None:
            raw = self.result.cpu().numpy().tobytes()
            self._host = abi.PtImageErrorResult.from_buffer_copy(raw)
        return self._host

    def sums(self) -> dict:
        """The raw doubles: {"sq": (r, g, b), "abs": (r, g, b), "rel": (r, g, b)}."""
        r = self.read()
        return {"sq": tuple(r.sum_sq), "abs": tuple(r.sum_abs), "rel": tuple(r.sum_rel)}

    @staticmethod
    def _mean(v, pixels):
        return ((v[0] + v[1]) + v[2]) / (3.0 * pixels) if pixels else math.nan

    @property
    def pixels(self) -> int:
        return int(self.read().pixels)

    @property
    def skipped(self) -> int:
        return int(self.read().skipped)

    @property
    def max_abs(self) -> tuple:
        return tuple(float(v) for v in self.read().max_abs)

    @property
    def mse(self) -> float:
        return self._mean(self.read().sum_sq, self.pixels)

    @property
    def mae(self) -> float:
        return self._mean(self.read().sum_abs, self.pixels)

    @property
    def rel_mse(self) -> float:
        return self._mean(self.read().sum_rel, self.pixels)

    def psnr(self, peak: float = 1.0) -> float:
        """10 log10(peak^2 / mse); +inf for identical frames, NaN where no pixel took part."""
        m = self.mse
        if math.isnan(m):
            return math.nan
        return math.inf if m == 0.0 else 10.0 * math.log10(float(peak) * float(peak) / m)


def image_error(a, ref, *, rect=None, eps: float = abi.PT_IMAGE_ERROR_DEFAULT_EPS, error_plane=False, no_lds: bool = False) -> ImageError:
    """The image error (include/pt_metrics.h: pt_image_error): frame `a` against frame `ref`, both [H][W][3] float32 on the GPU, whole
    frames; `a` may be `ref`.  `rect` = (x0, y0, x1, y1), None for the whole frame.  A pixel takes part iff its six values and three
    differences are finite; the others are counted in `.skipped`.  Each sum — of d^2, |d| and d^2 / (ref^2 + eps) per channel — is the
    EXACT sum of its terms rounded once to binary64: it does not depend on the order in which the device adds.  `error_plane`: True
    allocates, a [H][W] float32 device tensor is written — the per-pixel mean squared difference, +inf where a pixel is skipped or outside
    `rect`.  `no_lds`: the A/B switch PT_IMAGE_ERROR_NO_LDS (the same bits).  Asynchronous on torch's current stream; nothing is read back
    until a property of the returned ImageError asks for a number."""
    import torch

    lib = _stage("image_error", abi.has_metrics, "the image error", "pt_image_error entry point")
    _frame_ptr(a, "a")
    _frame_ptr(ref, "ref")
    if a.shape != ref.shape:
        raise ValueError("a and ref must have the same shape")
    h, w, _ = (int(n) for n in a.shape)
    plane = _optional_out(error_plane, (h, w), torch.float32, "error_plane", a.device)
    p = abi.PtImageErrorParams()
    lib.pt_image_error_params_init(C.byref(p), w, h)
    if rect is not None:
        x0, y0, x1, y1 = (int(v) for v in rect)
        if (x0, y0, x1, y1) == (0, 0, 0, 0):
            raise ValueError("rect (0, 0, 0, 0) means the whole frame at the C boundary: pass None for that, or another empty rectangle")
        p.rect_x0, p.rect_y0, p.rect_x1, p.rect_y1 = x0, y0, x1, y1
    p.eps = float(eps)
    p.flags = abi.PT_IMAGE_ERROR_NO_LDS if no_lds else 0
    p.scratch_bytes = int(lib.pt_image_error_scratch_bytes())
    scratch = torch.empty((p.scratch_bytes + 7) // 8, dtype=torch.int64, device=a.device)
    result = torch.empty(C.sizeof(abi.PtImageErrorResult) // 8, dtype=torch.int64, device=a.device)
    abi.check(lib.pt_image_error(C.byref(p), C.c_void_p(a.data_ptr()), C.c_void_p(ref.data_ptr()), C.c_void_p(result.data_ptr()),
                                 C.c_void_p(plane.data_ptr()) if plane is not None else None, C.c_void_p(scratch.data_ptr()),
                                 _stream_ptr(torch)), "pt_image_error")
    return ImageError(result, plane, scratch)


def mse_ratio(filtered, noisy, ref) -> float:
    """MSE(filtered, ref) / MSE(noisy, ref): the figure every quality record of DESIGN.md quotes (below 1: the filter helped).  Two
    image_error() calls; the division is the host's."""
    f, n = image_error(filtered, ref), image_error(noisy, ref)
    return f.mse / n.mse


def render_host(width: int, height: int, samples: int, scene, cam: camera, depth: int = 50, *, flags: int = 0,
                shard_index: int = 0, shard_count: int = 1) -> np.ndarray:
    """Torch-free path: pt_render_host renders into a numpy array (allocates, copies back, syncs)."""
    lib = abi.load_library()
    ds = _as_device_scene(scene)
    p = _params(width, height, samples, depth, shard_index, shard_count, flags)
    n = lib.pt_framebuffer_floats(C.byref(p))
    if n < 0:
        abi.check(abi.PT_ERR_INVALID_ARG, "pt_framebuffer_floats")
    fb = np.empty(n, dtype=np.float32)
    abi.check(lib.pt_render_host(ds.handle, C.byref(cam.c), C.byref(p), fb.ctypes.data_as(C.POINTER(C.c_float))),
              "pt_render_host")
    return fb.reshape((height, width, 3) if shard_count == 1 else (-1, abi.PT_TILE_PIXELS, 3))


def unshard(gathered, width: int, height: int, shard_count: int):
    """[shard_count][tiles_per_shard][64][3] (the RCCL-gathered buffer) -> [H][W][3] on the root GPU."""
    import torch

    lib = abi.load_library()
    p = _params(width, height, 1, 1, 0, shard_count)
    fb = torch.empty((height, width, 3), dtype=torch.float32, device=gathered.device)
    abi.check(lib.pt_unshard_tiles(C.c_void_p(gathered.data_ptr()), C.byref(p), C.c_void_p(fb.data_ptr()),
                                   _stream_ptr(torch)), "pt_unshard_tiles")
    return fb


def gather_frame(local, width: int, height: int, group=None, unshard_fn=None):
    """The exchange step of the N-GPU path: ONE gather of every rank's float tiles to rank 0 (RCCL over xGMI
    with the nccl backend; gloo in the CPU tests), then the un-interleave on the root.  `local` is this rank's
    [tiles_per_shard][64][3] tensor.  Returns the [H][W][3] frame on rank 0, None elsewhere."""
    import torch
    import torch.distributed as dist

    world, rank = dist.get_world_size(group), dist.get_rank(group)
    # one contiguous [world][tiles][64][3] receive buffer, the gather list = its slices (no re-pack before the un-interleave)
    gathered = torch.empty((world,) + tuple(local.shape), dtype=local.dtype, device=local.device) if rank == 0 else None
    bufs = list(gathered.unbind(0)) if rank == 0 else None
    dist.gather(local, bufs, dst=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    if rank != 0:
        return None
    if world == 1:
        return gathered[0]  # a one-shard render is already [H][W][3]
    return (unshard_fn or unshard)(gathered, width, height, world)


def render_distributed(width: int, height: int, samples: int, scene, cam: camera, depth: int = 50, *,
                       flags: int = 0, group=None, gather: bool = True):
    """One process per GPU (torch.distributed, backend nccl == RCCL).  Tiles are dealt round-robin to
    ranks (tile g -> rank g % world), each rank renders its tiles with the pixels' GLOBAL seeds
    (render.hpp:130-131), so the assembled frame is bit-identical to a single-GPU render.  No collective
    inside the render; one gather of the framebuffer at the end (gather_frame).
    Returns (frame on rank 0 | None elsewhere, local tiles)."""
    import torch.distributed as dist

    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    if world == 1:
        fb = render(width, height, samples, scene, cam, depth, flags=flags)
        return fb, fb
    local = render(width, height, samples, scene, cam, depth, flags=flags, shard_index=rank, shard_count=world)
    if not gather:
        return None, local
    return gather_frame(local, width, height, group), local


def tonemap_rgb8(fb):
    """Output stage of main.cpp:33-59 on the device: sqrt gamma, clamp [0,0.999], x256 -> u8, rows flipped
    (row 0 = top).  Returns a uint8 tensor [H][W][3]."""
    import torch

    lib = abi.load_library()
    src = _frame_ptr(fb)
    h, w, _ = fb.shape
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=fb.device)
    abi.check(lib.pt_tonemap_rgb8(src, w, h, C.c_void_p(out.data_ptr()), _stream_ptr(torch)),
              "pt_tonemap_rgb8")
    return out


_ENCODE_KW = ("transfer", "dither", "phase", "no_vec")


def _encode_kw(arg, who):
    """The `encode=` keyword of the display hosts: None / False -> None (today's call, the reference's quantiser), "srgb" / True -> the sRGB
    transfer, a dict -> encode()'s transfer, dither, phase, no_vec."""
    if arg is None or arg is False:
        return None
    if arg is True or arg == "srgb":
        return {}
    if isinstance(arg, dict) and not set(arg) - set(_ENCODE_KW):
        return dict(arg)
    raise TypeError(f"{who}: encode must be None, \"srgb\" or a dict of {', '.join(_ENCODE_KW)}")


def _encode_params(lib, w, h, transfer="srgb", dither=False, phase=(0, 0), no_vec=False) -> "abi.PtEncodeParams":
    if isinstance(transfer, str):
        if transfer not in abi.TRANSFERS:
            raise ValueError(f"transfer must be one of {sorted(abi.TRANSFERS)}")
        transfer = abi.TRANSFERS[transfer]
    p = abi.PtEncodeParams()
    lib.pt_encode_params_init(C.byref(p), w, h)
    p.transfer = int(transfer)
    p.flags = (abi.PT_ENCODE_DITHER if dither else 0) | (abi.PT_ENCODE_NO_VEC if no_vec else 0)
    p.phase_x, p.phase_y = int(phase[0]), int(phase[1])
    return p


def encode(linear, transfer="srgb", dither: bool = False, phase=(0, 0), out=None, *, no_vec: bool = False):
    """The encode stage (include/pt_encode.h: pt_encode): a linear-light frame [H][W][3] float32 on the GPU -> the uint8 image [H][W][3],
    row 0 = top (`out` if given), by the exact sRGB transfer ("srgb": the code of the real sRGB function, correctly rounded, for every
    binary32 value) or the reference's quantiser ("reference": tonemap_rgb8's bytes).  `dither`: the 8 x 8 ordered dither in linear
    light, its pattern offset by `phase` = (x, y) pixels (sRGB only).  no_vec: the A/B switch PT_ENCODE_NO_VEC (same bits).
    Asynchronous on torch's current stream; allocates nothing on the device but `out`."""
    import torch

    lib = _stage("encode", abi.has_encode, "the encode stage", "pt_encode")
    h, w = _whole_frame(linear)
    src = _frame_ptr(linear, "linear")
    p = _encode_params(lib, w, h, transfer, dither, phase, no_vec)
    out = _optional_out(True if out is None else out, (h, w, 3), torch.uint8, "out", linear.device)
    abi.check(lib.pt_encode(C.byref(p), src, C.c_void_p(out.data_ptr()), _stream_ptr(torch)), "pt_encode")
    return out


def _display_encode(lib, handle, p, fb, out, ekw):
    """pt_display_encode: pt_display_apply's exposure and curve and the encode stage in one pass -> the uint8 image [H][W][3], row 0 = top."""
    import torch

    if not abi.has_encode(lib):
        raise ImportError(f"{abi.library_path()} predates the encode stage (no pt_display_encode)")
    src = _frame_ptr(fb)
    h, w, _ = fb.shape
    ep = _encode_params(lib, w, h, **ekw)
    out = _optional_out(True if out is None else out, (h, w, 3), torch.uint8, "out", fb.device)
    abi.check(lib.pt_display_encode(handle, C.byref(p), C.byref(ep), src, C.c_void_p(out.data_ptr()), _stream_ptr(torch)), "pt_display_encode")
    return out


def _display_params(tone, ev_bias, ev_min, ev_max, lo_permille, hi_permille, adapt_up, adapt_down, white, rect) -> abi.PtDisplayParams:
    if isinstance(tone, str):
        if tone not in abi.TONES:
            raise ValueError(f"tone must be one of {sorted(abi.TONES)}")
        tone = abi.TONES[tone]
    x0, y0, x1, y1 = (0, 0, 0, 0) if rect is None else rect
    return abi.PtDisplayParams(C.sizeof(abi.PtDisplayParams), int(tone), 0, float(ev_bias), float(ev_min), float(ev_max), int(lo_permille),
                               int(hi_permille), float(adapt_up), float(adapt_down), float(white), int(x0), int(y0), int(x1), int(y1), 0)


def _display_apply(lib, handle, p, fb, out, linear, encode=None, who="display"):
    """pt_display_apply -> the uint8 image [H][W][3] (row 0 = top), or (image, linear plane) with `linear`: True allocates the plane, a tensor
    is written (it may be `fb`).  With `encode` (see _encode_kw) the fused pt_display_encode instead: the image alone, no plane."""
    import torch

    ekw = _encode_kw(encode, who)
    if ekw is not None:
        if linear is not None and linear is not False:
            raise ValueError(f"{who}: encode= takes the fused call, which writes no linear plane (call encode() on the plane instead)")
        return _display_encode(lib, handle, p, fb, out, ekw)

    src = _frame_ptr(fb)
    h, w, _ = fb.shape
    out = _optional_out(True if out is None else out, (h, w, 3), torch.uint8, "out", fb.device)
    lin = _optional_out(linear, (h, w, 3), torch.float32, "linear", fb.device)
    abi.check(lib.pt_display_apply(handle, C.byref(p), src, w, h, C.c_void_p(out.data_ptr()), C.c_void_p(lin.data_ptr()) if lin is not None else None,
                                   _stream_ptr(torch)), "pt_display_apply")
    return out if lin is None else (out, lin)


class Display:
    """The display stage (include/pt_render.h: PtDisplay): meter() builds the frame's luminance histogram on the device, solves an exposure
    from it and adapts towards it (the first metering is instant); apply() scales by 2^exposure, applies the tone curve and the output
    stage's quantiser.  Nothing between the two comes back to the host.  Whole frames [H][W][3] float32 on the GPU; asynchronous on
    torch's current stream; the calls on one Display must be stream-ordered.
    tone: "reference", "reinhard" or "aces"; rect: the metering rectangle (x0, y0, x1, y1), y = 0 the bottom row (None: the whole frame);
    the other parameters and their defaults are the header's (PtDisplayParams)."""

    def __init__(self, tone="aces", *, ev_bias: float = abi.PT_DISPLAY_DEFAULT_EV_BIAS, ev_min: float = abi.PT_DISPLAY_DEFAULT_EV_MIN,
                 ev_max: float = abi.PT_DISPLAY_DEFAULT_EV_MAX, lo_permille: int = abi.PT_DISPLAY_DEFAULT_LO_PERMILLE,
                 hi_permille: int = abi.PT_DISPLAY_DEFAULT_HI_PERMILLE, adapt_up: float = abi.PT_DISPLAY_DEFAULT_ADAPT_UP,
                 adapt_down: float = abi.PT_DISPLAY_DEFAULT_ADAPT_DOWN, white: float = abi.PT_DISPLAY_DEFAULT_WHITE, rect=None):
        self.lib = _stage("render.Display", abi.has_display, "the display stage", "pt_display_* entry points")
        self.params = _display_params(tone, ev_bias, ev_min, ev_max, lo_permille, hi_permille, adapt_up, adapt_down, white, rect)
        self.handle = C.c_void_p()
        abi.check(self.lib.pt_display_create(C.byref(self.handle)), "pt_display_create")

    @property
    def frames(self) -> int:
        """Meterings since the constructor or the last reset()."""
        return int(self.lib.pt_display_frames(self.handle))

    def meter(self, fb) -> "Display":
        """Histogram, solve and adaptation over the frame `fb`."""
        import torch

        src = _frame_ptr(fb)
        h, w, _ = fb.shape
        abi.check(self.lib.pt_display_meter(self.handle, C.byref(self.params), src, w, h, _stream_ptr(torch)), "pt_display_meter")
        return self

    def apply(self, fb, out=None, linear=False, encode=None):
        """The frame at the state's exposure through the tone curve: the uint8 image [H][W][3], row 0 = top (`out` if given); with `linear`
        (True, or a float32 tensor to write, which may be `fb`) also the curve's output before the quantiser: (image, plane).
        encode: None — the reference's quantiser, as ever —, "srgb" or a dict of encode()'s transfer, dither, phase: the curve's output
        through the encode stage instead, in one pass (pt_display_encode); not with `linear`."""
        return _display_apply(self.lib, self.handle, self.params, fb, out, linear, encode, "Display.apply")

    def exposure(self) -> float:
        """The exposure in stops (synchronises the stream: for inspection)."""
        import torch

        ev = C.c_float()
        abi.check(self.lib.pt_display_exposure(self.handle, C.byref(ev), _stream_ptr(torch)), "pt_display_exposure")
        return float(ev.value)

    def histogram(self) -> np.ndarray:
        """The last metering's 256 bins followed by the rejected count, uint32[257] (synchronises the stream: for inspection)."""
        import torch

        host = np.zeros(257, dtype=np.uint32)
        abi.check(self.lib.pt_display_histogram(self.handle, host.ctypes.data_as(C.POINTER(C.c_uint32)), _stream_ptr(torch)), "pt_display_histogram")
        return host

    def set_exposure(self, ev: float) -> "Display":
        """A manual exposure in stops (clamped to +-32); a later meter() adapts from it."""
        import torch

        abi.check(self.lib.pt_display_set_exposure(self.handle, float(ev), _stream_ptr(torch)), "pt_display_set_exposure")
        return self

    def reset(self) -> None:
        """Forget the exposure: the next meter() is instant."""
        import torch

        abi.check(self.lib.pt_display_reset(self.handle, _stream_ptr(torch)), "pt_display_reset")

    def close(self) -> None:
        if self.handle:
            self.lib.pt_display_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def display(fb, tone="aces", ev: float = 0.0, *, white: float = abi.PT_DISPLAY_DEFAULT_WHITE, out=None, linear=False, encode=None):
    """The stateless display stage: `fb` at a manual exposure of `ev` stops through the tone curve -> uint8 [H][W][3], row 0 = top (with
    `linear`: (image, plane), as Display.apply; with `encode`: through the encode stage, as there).  display(fb, "reference", 0.0) is
    tonemap_rgb8(fb)."""
    lib = abi.load_library()
    if not abi.has_display(lib):
        raise ImportError(f"{abi.library_path()} predates the display stage (no pt_display_* entry points)")
    p = _display_params(tone, ev, abi.PT_DISPLAY_DEFAULT_EV_MIN, abi.PT_DISPLAY_DEFAULT_EV_MAX, abi.PT_DISPLAY_DEFAULT_LO_PERMILLE,
                        abi.PT_DISPLAY_DEFAULT_HI_PERMILLE, 1.0, 1.0, white, None)
    return _display_apply(lib, None, p, fb, out, linear, encode, "display")


class Accumulator:
    """Progressive rendering (include/pt_render.h PtAccum): one frame rendered in sample windows.

    After windows totalling N samples, resolve() gives the same bits as render(..., samples=N, ...) with the same scene, camera,
    depth, flags and shard — for every split of N.  `add` is asynchronous on torch's current stream; the accumulator and the scene
    it renders must be used from one stream (as render() requires of a scene).  `scene`: as for render().
    """

    def __init__(self, width: int, height: int, scene, cam: camera, depth: int = 50, *, flags: int = 0, shard_index: int = 0,
                 shard_count: int = 1, adaptive: bool = False):
        """adaptive: per-pixel sample counts (pt_adaptive_create) — add() takes a mask, and counts() / error() / select() drive it;
        each pixel resolves to the bits render() gives at its own count."""
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("path_tracer_amd.render.Accumulator needs a HIP device: there is no CPU path in the product")
        self.lib = abi.load_library()
        if not abi.has_accumulator(self.lib):
            raise ImportError(f"{abi.library_path()} predates progressive rendering (no pt_accum_* entry points)")
        if adaptive and not abi.has_adaptive(self.lib):
            raise ImportError(f"{abi.library_path()} predates adaptive sampling (no pt_adaptive_* entry points)")
        self.width, self.height, self.depth, self.flags = int(width), int(height), int(depth), int(flags)
        self.shard_index, self.shard_count = int(shard_index), int(shard_count)
        self.adaptive = bool(adaptive)
        self.cam = cam
        self.handle = C.c_void_p()
        self._ds = _as_device_scene(scene, cache_key=("cuda", torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream))
        self._p = _params(width, height, 1, depth, shard_index, shard_count, flags)
        create = self.lib.pt_adaptive_create if self.adaptive else self.lib.pt_accum_create
        abi.check(create(self._ds.handle, C.byref(self._p), C.byref(self.handle)), "pt_adaptive_create" if self.adaptive else "pt_accum_create")

    @property
    def samples(self) -> int:
        """Samples of every pixel rendered so far (adaptive: the samples of the windows rendered without a mask)."""
        return int(self.lib.pt_accum_samples(self.handle))

    def add(self, samples: int, mask=None) -> "Accumulator":
        """Render the next `samples` samples of every pixel (asynchronous on torch's current stream) — on an adaptive accumulator, of
        every pixel whose `mask` element is nonzero (a CUDA uint8 / bool tensor shaped like one channel of resolve(); a mask
        synchronises the stream once)."""
        import torch

        if mask is None:
            abi.check(self.lib.pt_render_accumulate(self.handle, C.byref(self.cam.c), int(samples), _stream_ptr(torch)), "pt_render_accumulate")
            return self
        mask = self._pixel_array(mask, (torch.uint8, torch.bool), "mask")
        abi.check(self.lib.pt_adaptive_window(self.handle, C.byref(self.cam.c), int(samples), C.c_void_p(mask.data_ptr()), _stream_ptr(torch)),
                  "pt_adaptive_window")
        return self

    def _shape(self, n: int):
        return (self.height, self.width, 3) if self.shard_count == 1 else (n // (abi.PT_TILE_PIXELS * 3), abi.PT_TILE_PIXELS, 3)

    def _pixel_shape(self):
        return self._shape(self.lib.pt_framebuffer_floats(C.byref(self._p)))[:2]

    def _pixel_array(self, t, dtypes, what):
        if tuple(t.shape) != self._pixel_shape() or t.dtype not in dtypes or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous CUDA tensor of {self._pixel_shape()} ({', '.join(map(str, dtypes))})")
        return t

    def counts(self):
        """Each pixel's sample count (adaptive): int32, shaped like one channel of resolve()."""
        import torch

        out = torch.empty(self._pixel_shape(), dtype=torch.int32, device="cuda")
        abi.check(self.lib.pt_adaptive_counts(self.handle, C.c_void_p(out.data_ptr()), _stream_ptr(torch)), "pt_adaptive_counts")
        return out

    def error(self, ref=None, **kw):
        """Without `ref`: each pixel's two-half-buffer error estimate (adaptive; include/pt_render.h): float32, shaped like counts().
        With `ref` (a [H][W][3] float32 device frame): image_error(resolve(), ref, **kw) — the accumulated frame's error against a
        reference (whole frames only), an ImageError."""
        import torch

        if ref is not None:
            if self.shard_count != 1:
                raise ValueError("Accumulator.error(ref): whole frames only (gather and unshard first)")
            return image_error(self.resolve(), ref, **kw)
        out = torch.empty(self._pixel_shape(), dtype=torch.float32, device="cuda")
        abi.check(self.lib.pt_adaptive_error(self.handle, C.c_void_p(out.data_ptr()), _stream_ptr(torch)), "pt_adaptive_error")
        return out

    def select(self, threshold: float, min_spp: int, max_spp: int, dilate: bool = True):
        """(mask, n_active): the pixels the next window should render (pt_adaptive_select; synchronises the stream)."""
        import torch

        mask = torch.empty(self._pixel_shape(), dtype=torch.uint8, device="cuda")
        n = C.c_int64()
        abi.check(self.lib.pt_adaptive_select(self.handle, float(threshold), int(min_spp), int(max_spp), abi.PT_ADAPTIVE_DILATE if dilate else 0,
                                              C.c_void_p(mask.data_ptr()), C.byref(n), _stream_ptr(torch)), "pt_adaptive_select")
        return mask, int(n.value)

    def resolve(self, out=None):
        """The mean of the samples so far, as render() returns it ([H][W][3], or this shard's tiles [tiles][64][3])."""
        import torch

        n = self.lib.pt_framebuffer_floats(C.byref(self._p))
        if out is None:
            out = torch.empty(self._shape(n), dtype=torch.float32, device="cuda")
        elif out.numel() != n or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 CUDA tensor of pt_framebuffer_floats() elements")
        abi.check(self.lib.pt_accum_resolve(self.handle, C.c_void_p(out.data_ptr()), _stream_ptr(torch)), "pt_accum_resolve")
        return out

    def denoise(self, aov_spp: int = 16, *, firefly=None, **kw):
        """resolve(), the feature buffers of the accumulator's own scene and bound camera (render_aov at `aov_spp` camera rays per
        pixel) and denoise() over them: denoise(resolve(), **render_aov(...), **kw).  Whole frames only.  `firefly` (True, or a dict of
        firefly()'s rank, k, repair): the firefly stage runs on the resolved frame before the filter."""
        if self.shard_count != 1:
            raise ValueError("Accumulator.denoise: whole frames only (the filter reads neighbours: gather and unshard first)")
        fkw = _stage_kw(firefly, "Accumulator.denoise", "firefly", _FIREFLY_KW)
        guides = render_aov(self.width, self.height, aov_spp, self._ds, self.cam, planes=("albedo", "normal", "depth"))
        if fkw is None:
            return denoise(self.resolve(), **guides, **kw)
        return denoise(_firefly(self.resolve(), **fkw), **guides, **kw)

    def variance(self, out=None):
        """The per-channel variance of each resolved pixel, estimated from the two half buffers (adaptive; include/pt_render.h:
        pt_variance_estimate): float32, shaped like resolve(); +inf where a pixel has no estimate yet."""
        import torch

        if not abi.has_variance_denoise(self.lib):
            raise ImportError(f"{abi.library_path()} predates the variance estimate (no pt_variance_estimate entry point)")
        n = self.lib.pt_framebuffer_floats(C.byref(self._p))
        if out is None:
            out = torch.empty(self._shape(n), dtype=torch.float32, device="cuda")
        elif out.numel() != n or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 CUDA tensor of pt_framebuffer_floats() elements")
        abi.check(self.lib.pt_variance_estimate(self.handle, C.c_void_p(out.data_ptr()), _stream_ptr(torch)), "pt_variance_estimate")
        return out

    def denoise_variance(self, aov_spp: int = 16, *, firefly=None, spatial=None, **kw):
        """resolve(), variance(), the feature buffers of the accumulator's own scene and bound camera (render_aov at `aov_spp` camera
        rays per pixel) and denoise_variance() over them.  Adaptive accumulators, whole frames only.  `firefly` (True, or a dict of
        firefly()'s rank, k, repair): the firefly stage runs on the resolved frame and its variance before the filter.
        `spatial` (True, or a dict of spatial_variance()'s radius, min_pairs, tol_depth, tol_normal, demodulate): the spatial variance
        estimate (guides: albedo, normal, depth and id) fills the pixels of variance() that have no estimate — after the firefly stage,
        whose repaired pixels are such — and on a PLAIN accumulator, which has no variance(), it makes the whole plane: the only way
        this method works on one."""
        if self.shard_count != 1:
            raise ValueError("Accumulator.denoise_variance: whole frames only (the filter reads neighbours: gather and unshard first)")
        fkw = _stage_kw(firefly, "Accumulator.denoise_variance", "firefly", _FIREFLY_KW)
        skw = _stage_kw(spatial, "Accumulator.denoise_variance", "spatial", _SPATIAL_KW)
        if skw is not None:
            guides = render_aov(self.width, self.height, aov_spp, self._ds, self.cam, planes=("albedo", "normal", "depth", "id"))
            color, var = self.resolve(), self.variance() if self.adaptive else None
            if fkw is not None:
                if var is None:
                    color = _firefly(color, **fkw)
                else:
                    color, var = _firefly(color, var, variance_out=var, **fkw)
            var = _spatial_variance(color, var, out=var, **guides, **skw)
            return denoise_variance(color, var, albedo=guides["albedo"], normal=guides["normal"], depth=guides["depth"], **kw)
        guides = render_aov(self.width, self.height, aov_spp, self._ds, self.cam, planes=("albedo", "normal", "depth"))
        if fkw is None:
            return denoise_variance(self.resolve(), self.variance(), **guides, **kw)
        var = self.variance()
        color, var = _firefly(self.resolve(), var, variance_out=var, **fkw)
        return denoise_variance(color, var, **guides, **kw)

    def tonemap_rgb8(self):
        """resolve() + tonemap_rgb8() in one pass (whole frames): uint8 [H][W][3], row 0 = top."""
        import torch

        out = torch.empty((self.height, self.width, 3), dtype=torch.uint8, device="cuda")
        abi.check(self.lib.pt_accum_tonemap_rgb8(self.handle, C.c_void_p(out.data_ptr()), _stream_ptr(torch)), "pt_accum_tonemap_rgb8")
        return out

    def display(self, disp: "Display", out=None, encode=None):
        """resolve(), then disp.meter() and disp.apply() over it: the uint8 image [H][W][3], row 0 = top, at the exposure the Display
        adapted to (whole frames).  encode: Display.apply's."""
        if self.shard_count != 1:
            raise ValueError("Accumulator.display: whole frames only (gather and unshard first)")
        fb = self.resolve()
        return disp.meter(fb).apply(fb, out=out, encode=encode)

    def reset(self) -> None:
        """Back to 0 samples (the next window binds its camera: set .cam first to render another view)."""
        import torch

        abi.check(self.lib.pt_accum_reset(self.handle, _stream_ptr(torch)), "pt_accum_reset")

    def next_frame(self, cam: "camera | None" = None) -> "Accumulator":
        """A new image that CONTINUES every pixel's random stream (adaptive; include/pt_render.h: pt_adaptive_next_frame): sums and
        counts back to 0, the camera binding released, the generator states kept — so the frames of a sequence carry independent noise
        (reset() re-seeds: its frames repeat theirs).  The next window binds `cam` if given, else the camera used so far."""
        import torch

        if not abi.has_temporal(self.lib):
            raise ImportError(f"{abi.library_path()} predates temporal reprojection (no pt_adaptive_next_frame entry point)")
        abi.check(self.lib.pt_adaptive_next_frame(self.handle, _stream_ptr(torch)), "pt_adaptive_next_frame")
        if cam is not None:
            self.cam = cam
        return self

    def state(self) -> np.ndarray:
        """The exported state (pt_accum_export: header, sums, generator states; adaptive: pt_adaptive_export's format 2, which adds
        H and the counts n and a) as bytes in a uint8 array."""
        import torch

        if self.adaptive:
            buf = np.empty(self.lib.pt_adaptive_state_bytes(C.byref(self._p)), dtype=np.uint8)
            abi.check(self.lib.pt_adaptive_export(self.handle, buf.ctypes.data_as(C.c_void_p), buf.size, _stream_ptr(torch)), "pt_adaptive_export")
            return buf
        buf = np.empty(self.lib.pt_accum_state_bytes(C.byref(self._p)), dtype=np.uint8)
        abi.check(self.lib.pt_accum_export(self.handle, buf.ctypes.data_as(C.c_void_p), buf.size, _stream_ptr(torch)), "pt_accum_export")
        return buf

    def save(self, path) -> None:
        """Checkpoint to a raw file (the pt_accum_export / pt_adaptive_export format, include/pt_render.h)."""
        with open(path, "wb") as f:
            f.write(self.state().tobytes())

    @classmethod
    def load(cls, path, scene, cam: "camera | None" = None, adaptive: bool = False) -> "Accumulator":
        """A new accumulator over `scene` (the same tables as the saved one's) resumed from a checkpoint; the frame parameters and
        the camera come from the file (`cam` is needed only for a state saved at 0 samples).  A format-2 state makes an adaptive
        accumulator; `adaptive=True` also continues a plain (format-1) state adaptively."""
        buf = np.fromfile(path, dtype=np.uint8)
        if buf.size < abi.PT_ACCUM_HEADER_BYTES:
            raise ValueError(f"{path}: not an accumulator state")
        magic, fmt, w, h, depth, si, sc, flags, _done, bound = np.frombuffer(buf[:40].tobytes(), dtype="<u4").astype(np.int64)
        if magic != abi.PT_ACCUM_MAGIC or fmt not in (abi.PT_ACCUM_FORMAT, abi.PT_ADAPTIVE_FORMAT):
            raise ValueError(f"{path}: not an accumulator state")
        if bound:
            cam = _BoundCamera(abi.PtCamera.from_buffer_copy(buf[64:abi.PT_ACCUM_HEADER_BYTES].tobytes()))
        elif cam is None:
            raise ValueError(f"{path}: the state has no samples (no bound camera): pass cam")
        acc = cls(int(w), int(h), scene, cam, int(depth), flags=int(flags), shard_index=int(si), shard_count=int(sc),
                  adaptive=adaptive or fmt == abi.PT_ADAPTIVE_FORMAT)
        acc.restore(buf)
        return acc

    def restore(self, state: np.ndarray) -> None:
        """pt_accum_import of an exported state (the header must match this accumulator's frame parameters); adaptive:
        pt_adaptive_import, which also takes a plain (format-1) state."""
        import torch

        state = np.ascontiguousarray(state, dtype=np.uint8)
        if self.adaptive:
            abi.check(self.lib.pt_adaptive_import(self.handle, state.ctypes.data_as(C.c_void_p), state.size, _stream_ptr(torch)),
                      "pt_adaptive_import")
        else:
            abi.check(self.lib.pt_accum_import(self.handle, state.ctypes.data_as(C.c_void_p), state.size, _stream_ptr(torch)), "pt_accum_import")
        if int(np.frombuffer(state[36:40].tobytes(), dtype="<i4")[0]):  # the state's camera is bound: windows continue with it
            self.cam = _BoundCamera(abi.PtCamera.from_buffer_copy(state[64:abi.PT_ACCUM_HEADER_BYTES].tobytes()))

    def close(self) -> None:
        if self.handle:
            self.lib.pt_accum_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class _BoundCamera:
    """A camera given as its PtCamera (the one an exported state is bound to)."""

    def __init__(self, c: "abi.PtCamera"):
        self.c = c


class TemporalAccumulator:
    """Temporal reprojection (include/pt_render.h: PtTemporal): the history of one image sequence, carried across camera moves.

    push() blends a frame into the history of the frames before it, fetched through the previous push's camera and rejected where the
    guides (render_aov's depth, normal, id for the frame's camera) say the surface is another one.  Whole frames only; asynchronous on
    torch's current stream; pushes of one TemporalAccumulator must be stream-ordered."""

    def __init__(self, width: int, height: int):
        self.lib = _stage("render.TemporalAccumulator", abi.has_temporal, "temporal reprojection", "pt_temporal_* entry points")
        self.width, self.height = int(width), int(height)
        self.handle = C.c_void_p()
        abi.check(self.lib.pt_temporal_create(self.width, self.height, C.byref(self.handle)), "pt_temporal_create")

    @property
    def frames(self) -> int:
        """Pushes since the constructor or the last reset()."""
        return int(self.lib.pt_temporal_frames(self.handle))

    def push(self, fb, cam: camera, *, depth, normal=None, id=None, variance=None, out=None, alpha: float = abi.PT_TEMPORAL_DEFAULT_ALPHA,
             tol_depth: float = abi.PT_TEMPORAL_DEFAULT_TOL_DEPTH, tol_normal: float = abi.PT_TEMPORAL_DEFAULT_TOL_NORMAL, **other_planes):
        """One frame: `fb` [H][W][3] float32 on the GPU (render()'s or Accumulator.resolve()'s), `cam` its camera, depth [H][W] (required),
        normal [H][W][3], id [H][W] int32 (optional) its feature buffers — push(fb, cam, **render_aov(...)) works: the planes the pass
        does not take are ignored — and `variance` [H][W][3] (optional) the frame's own variance estimate, passed through where the
        history is younger than 4 frames.  Returns (color, variance, history): the accumulated frame (`out` if given, which may be
        `fb`), the variance of the accumulated mean (+inf where there is no estimate) and the history length [H][W]."""
        import torch

        _aov_kwargs_ok("push", other_planes)
        h, w = self.height, self.width
        if fb is None or depth is None:
            raise ValueError("push() needs the frame and its depth plane")
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.float32, device=fb.device)
        var_out = torch.empty((h, w, 3), dtype=torch.float32, device=fb.device)
        hist = torch.empty((h, w), dtype=torch.float32, device=fb.device)
        p = abi.PtTemporalParams(C.sizeof(abi.PtTemporalParams), float(alpha), float(tol_depth), float(tol_normal), 0)
        abi.check(self.lib.pt_temporal_push(self.handle, C.byref(p), C.byref(cam.c), _plane(fb, (h, w, 3), "fb"), _plane(depth, (h, w), "depth"),
                                            _plane(normal, (h, w, 3), "normal"), _plane(id, (h, w), "id", torch.int32),
                                            _plane(variance, (h, w, 3), "variance"), _plane(out, (h, w, 3), "out"),
                                            C.c_void_p(var_out.data_ptr()), C.c_void_p(hist.data_ptr()), _stream_ptr(torch)), "pt_temporal_push")
        return out, var_out, hist

    def reset(self) -> None:
        """Forget the history: the next push starts one."""
        import torch

        abi.check(self.lib.pt_temporal_reset(self.handle, _stream_ptr(torch)), "pt_temporal_reset")

    def close(self) -> None:
        if self.handle:
            self.lib.pt_temporal_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def render_temporal(width: int, height: int, spp: int, scene, cams, depth: int = 50, *, aov_spp: int = 4, denoise: bool = True,
                    denoise_kw: "dict | None" = None, display: "Display | None" = None, firefly=None, spatial_variance=None, encode=None, **params):
    """A camera path rendered at `spp` samples per frame with its history carried along: for each camera of `cams` yields a dict with
    `noisy` (the frame alone), `temporal`, `variance`, `history` (TemporalAccumulator.push's results) and, with `denoise`, `filtered` —
    denoise_variance() over the temporal colour and variance with that frame's guides (render_aov at `aov_spp` camera rays per pixel).
    One adaptive accumulator renders every frame, with next_frame() between them: no frame repeats another's random numbers.  A frame
    of 2 samples or more is rendered in two windows, so that its own variance estimate (Accumulator.variance(), from the two halves)
    exists and is what `variance` holds where the history is younger than 4 frames.
    With `display` (a Display) each frame also has `rgb8`: the end of the chain — `filtered` (or `temporal` without `denoise`) metered and
    shown by it, its exposure adapting from frame to frame.  With `encode` ("srgb", or a dict of encode()'s transfer, dither, phase) `rgb8`
    is the encode stage's, fused with the display's curve (Display.apply's `encode`); it needs `display`.
    With `firefly` (True, or a dict of firefly()'s rank, k, repair) the firefly stage runs on `noisy` and its variance before the push, and
    each frame also has `clamped`: the frame the history took in (`noisy` stays the frame alone), and `firefly_counts`: the stage's
    {clamped, repaired} as a uint32 device tensor.
    With `spatial_variance` (True, or a dict of spatial_variance()'s radius, min_pairs, tol_depth, tol_normal, demodulate) the spatial
    variance estimate runs after the push, on the accumulated colour with the frame's guides, and fills `variance` in place where the push
    left no estimate (a young history without one of the frame's own, a repaired pixel); each frame also has `variance_counts`: the
    stage's {estimated, holes} as a uint32 device tensor.
    `params`: push()'s alpha, tol_depth, tol_normal; `denoise_kw`: denoise_variance()'s parameters."""
    import torch

    if spp <= 0:
        raise ValueError("spp must be > 0")
    if _encode_kw(encode, "render_temporal") is not None and display is None:
        raise ValueError("render_temporal: encode needs display")
    fkw = _stage_kw(firefly, "render_temporal", "firefly", _FIREFLY_KW)
    skw = _stage_kw(spatial_variance, "render_temporal", "spatial_variance", _SPATIAL_KW)
    ds = _as_device_scene(scene, cache_key=("cuda", torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream))
    acc, hist = None, TemporalAccumulator(width, height)
    try:
        for cam in cams:
            if acc is None:
                acc = Accumulator(width, height, ds, cam, depth, adaptive=True)
            else:
                acc.next_frame(cam)
            acc.add(spp - spp // 2)
            if spp >= 2:
                acc.add(spp // 2)
            noisy, var = acc.resolve(), acc.variance()
            guides = render_aov(width, height, aov_spp, ds, cam, planes=("albedo", "normal", "depth", "id"))
            clamped = None
            if fkw is not None:
                clamped, var, firefly_counts = _firefly(noisy, var, variance_out=var, counts=True, **fkw)
            color, variance, history = hist.push(noisy if clamped is None else clamped, cam, variance=var, **guides, **params)
            frame = dict(noisy=noisy, temporal=color, variance=variance, history=history)
            if clamped is not None:
                frame["clamped"], frame["firefly_counts"] = clamped, firefly_counts
            if skw is not None:
                _, frame["variance_counts"] = _spatial_variance(color, variance, out=variance, counts=True, **guides, **skw)
            if denoise:
                frame["filtered"] = denoise_variance(color, variance, albedo=guides["albedo"], normal=guides["normal"], depth=guides["depth"],
                                                     **(denoise_kw or {}))
            if display is not None:
                shown = frame["filtered" if denoise else "temporal"]
                frame["rgb8"] = display.meter(shown).apply(shown, encode=encode)
            yield frame
    finally:
        if acc is not None:
            acc.close()
        hist.close()


def render_progressive(width: int, height: int, samples: int, scene, cam: camera, depth: int = 50, *, step: int, flags: int = 0,
                       shard_index: int = 0, shard_count: int = 1):
    """Render `samples` spp in windows of `step` (the last one shorter): yields (samples_done, framebuffer) after each window; the
    last framebuffer has the bits render() gives at `samples`."""
    if step <= 0 or samples <= 0:
        raise ValueError("samples and step must be > 0")
    acc = Accumulator(width, height, scene, cam, depth, flags=flags, shard_index=shard_index, shard_count=shard_count)
    try:
        done = 0
        while done < samples:
            n = min(step, samples - done)
            acc.add(n)
            done += n
            yield done, acc.resolve()
    finally:
        acc.close()


def render_adaptive(width: int, height: int, scene, cam: camera, depth: int = 50, *, threshold: float, min_spp: int = 16,
                    max_spp: int = 1024, step: int = 16, dilate: bool = True, flags: int = 0, variance: bool = False):
    """Adaptive sampling (include/pt_render.h: pt_adaptive_*): a window of min_spp samples of every pixel, then windows of `step`
    samples of the pixels pt_adaptive_select keeps active (noise estimate above `threshold`, or below min_spp; with `dilate`, next to
    such a pixel) until none is.  Returns (framebuffer, counts): each pixel holds the bits render() gives at its own count, which lies
    in [min_spp, max_spp] and is min_spp + a multiple of `step`.  A window whose mask is every pixel runs unmasked (cost probe, tile
    order).  A negative threshold renders every pixel to max_spp: render(..., samples=max_spp, ...).

    Each select synchronises the stream (its count decides the next window).  With a negative threshold every pixel below max_spp is
    noisy, so the selection follows from the counts alone: while every window has been unmasked, every pixel is active until the
    counts reach max_spp, and the loop skips the select (and its synchronisation) — the same windows, asynchronous like
    render_progressive.

    `variance=True` also returns the per-pixel variance estimate of the finished frame (Accumulator.variance(), what
    denoise_variance() takes): (framebuffer, counts, variance)."""
    if min_spp <= 0 or step <= 0 or max_spp < min_spp or (max_spp - min_spp) % step != 0:
        raise ValueError("need 0 < min_spp <= max_spp, step > 0 and (max_spp - min_spp) % step == 0")
    acc = Accumulator(width, height, scene, cam, depth, flags=flags, adaptive=True)
    try:
        acc.add(min_spp)
        pixels = width * height
        uniform = True  # only unmasked windows so far: every pixel has acc.samples samples
        while True:
            if threshold < 0 and uniform:
                n_active, mask = (pixels if acc.samples < max_spp else 0), None
            else:
                mask, n_active = acc.select(threshold, min_spp, max_spp, dilate)
            if n_active == 0:
                break
            uniform = uniform and n_active == pixels
            acc.add(step, None if n_active == pixels else mask)
        if variance:
            return acc.resolve(), acc.counts(), acc.variance()
        return acc.resolve(), acc.counts()
    finally:
        acc.close()
