"""CPU test of the ORDER in which the eight image-stage entry points report their refusals (pt_denoise, pt_variance_denoise,
pt_temporal_push, pt_display_meter, pt_display_apply, pt_firefly, pt_spatial_variance, pt_image_error).  Every call below is wrong in TWO
ways at once; the return code and pt_last_error() say which defect the entry point reports, and that is the one its own sequence of checks
reaches first.  The per-stage *_cpu.py tests pin each refusal alone; this one pins their order, which a shared host prelude must not
rearrange.  The expected strings are those of the library before the stages' host code was folded onto one prelude.  No device is touched:
every pointer is a made-up aligned address that is never dereferenced, and every call is refused on the host.  (pt_temporal_push judges its
overlaps by the frame size its state holds, so those need a live state and are tests/test_gpu_temporal.py's.)"""
import ctypes as C
import math

import pytest

from path_tracer_amd import abi
from path_tracer_amd.scene import camera

W, H = 64, 40
FRAME, PLANE = W * H * 12, W * H * 4
BIG = dict(width=1 << 16, height=(1 << 14) + 1)  # one row more than 2^30 pixels
BAD, LARGE = abi.PT_ERR_INVALID_ARG, abi.PT_ERR_TOO_LARGE

# the planes of every stage, 16 MiB apart: further than any frame or scratch at W x H
NAMES = ("state", "color", "variance", "albedo", "normal", "depth", "id", "out", "variance_out", "out_history", "scratch", "counts", "rgb8",
         "linear", "ref", "result", "plane")
ADDR = {name: 0x10000000 + i * 0x1000000 for i, name in enumerate(NAMES)}


def good_camera():
    return camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0, 1.6, 0.0, 1.0, 0.0, 0.0).c


def _init(lib, entry):
    """The stage's parameter struct at its defaults for a W x H frame, and the trailing (width, height) arguments of the display calls."""
    if entry == "pt_denoise":
        p = abi.PtDenoiseParams()
        lib.pt_denoise_params_init(C.byref(p), W, H)
    elif entry == "pt_variance_denoise":
        p = abi.PtVarianceDenoiseParams()
        lib.pt_variance_denoise_params_init(C.byref(p), W, H)
    elif entry == "pt_temporal_push":
        p = abi.PtTemporalParams()
        lib.pt_temporal_params_init(C.byref(p))
    elif entry in ("pt_display_meter", "pt_display_apply"):
        p = abi.PtDisplayParams()
        lib.pt_display_params_init(C.byref(p))
    elif entry == "pt_firefly":
        p = abi.PtFireflyParams()
        lib.pt_firefly_params_init(C.byref(p), W, H)
    elif entry == "pt_spatial_variance":
        p = abi.PtSpatialVarianceParams()
        lib.pt_spatial_variance_params_init(C.byref(p), W, H)
    else:
        p = abi.PtImageErrorParams()
        lib.pt_image_error_params_init(C.byref(p), W, H)
        p.scratch_bytes = lib.pt_image_error_scratch_bytes()
    return p


# the pointer arguments of each entry point, in its order, by the names of ADDR ("cam" and the display calls' frame size are handled below)
PLANES = {
    "pt_denoise": ("color", "albedo", "normal", "depth", "out", "scratch"),
    "pt_variance_denoise": ("color", "variance", "albedo", "normal", "depth", "out", "variance_out", "scratch"),
    "pt_temporal_push": ("color", "depth", "normal", "id", "variance", "out", "variance_out", "out_history"),
    "pt_display_meter": ("color",),
    "pt_display_apply": ("color",),
    "pt_firefly": ("color", "variance", "out", "variance_out", "counts"),
    "pt_spatial_variance": ("color", "albedo", "normal", "depth", "id", "variance", "variance_out", "counts"),
    "pt_image_error": ("color", "ref", "result", "plane", "scratch"),
}


def call(lib, entry, fields, ptrs):
    p = _init(lib, entry)
    w, h = fields.pop("w", W), fields.pop("h", H)
    for k, v in fields.items():
        setattr(p, k, v)
    at = dict(ADDR, **ptrs)
    planes = [at[name] for name in PLANES[entry]]
    fn = getattr(lib, entry)
    if entry == "pt_temporal_push":
        cam = at.get("cam", good_camera())
        return fn(at["state"], C.byref(p), C.byref(cam) if cam is not None else None, *planes, None)
    if entry == "pt_display_meter":
        return fn(at["state"], C.byref(p), planes[0], w, h, None)
    if entry == "pt_display_apply":
        return fn(at["state"], C.byref(p), planes[0], w, h, at["rgb8"], at["linear"], None)
    return fn(C.byref(p), *planes, None)


RECT_OUT = dict(rect_x0=0, rect_y0=0, rect_x1=W + 1, rect_y1=H)      # leaves the frame
RECT_EMPTY = dict(rect_x0=5, rect_y0=0, rect_x1=5, rect_y1=3)        # empty: the display refuses it, the image error takes it

# (entry point, parameter fields, pointers, the return code, what pt_last_error() names): the first defect is the one reported
CASES = [
    ("pt_denoise", dict(struct_size=0, width=0), dict(color=None), BAD, "NULL params, color, out or scratch"),
    ("pt_denoise", dict(struct_size=0, width=0), {}, BAD, "struct_size is not this library's"),
    ("pt_denoise", dict(width=0, iterations=0), {}, BAD, "width and height must be > 0"),
    ("pt_denoise", dict(iterations=9, sigma_depth=math.nan), {}, BAD, "need 1 <= iterations <= 8"),
    ("pt_denoise", dict(sigma_depth=math.nan, flags=4), {}, BAD, "a sigma is not finite"),
    ("pt_denoise", dict(flags=4, **BIG), {}, BAD, "unknown flags"),
    ("pt_denoise", dict(sigma_color=1e-30, flags=abi.PT_DENOISE_DEMODULATE), dict(albedo=None), BAD, "PT_DENOISE_DEMODULATE needs the albedo plane"),
    ("pt_denoise", dict(sigma_color=1e-30, sigma_normal=1e-30), {}, BAD, "1 / sigma_color^2 leaves binary32"),
    ("pt_denoise", dict(sigma_normal=1e-30, **BIG), {}, BAD, "1 / sigma_normal^2 leaves binary32"),
    ("pt_denoise", dict(sigma_depth=1e30, sigma_albedo=1e-30), {}, BAD, "sigma_depth^2 leaves binary32"),
    ("pt_denoise", dict(sigma_albedo=1e-30, **BIG), {}, BAD, "1 / sigma_albedo^2 leaves binary32"),
    ("pt_denoise", dict(BIG), dict(scratch=ADDR["scratch"] + 4), LARGE, "more than 2^30 pixels"),
    ("pt_denoise", {}, dict(scratch=ADDR["scratch"] + 4, out=ADDR["albedo"]), BAD, "scratch must be 16-byte aligned"),
    ("pt_denoise", {}, dict(out=ADDR["normal"] + 12, scratch=ADDR["color"]), BAD, "out and scratch must not overlap a guide plane"),
    ("pt_denoise", {}, dict(scratch=ADDR["depth"] - 16), BAD, "out and scratch must not overlap a guide plane"),
    ("pt_denoise", {}, dict(scratch=ADDR["color"] + FRAME - 16), BAD, "scratch must not overlap color or out"),

    ("pt_variance_denoise", dict(struct_size=44, iterations=0), dict(variance=None), BAD, "NULL params, color, variance, out or scratch"),
    ("pt_variance_denoise", dict(struct_size=44, iterations=0), {}, BAD, "struct_size is not this library's"),
    ("pt_variance_denoise", dict(height=-1, flags=8), {}, BAD, "width and height must be > 0"),
    ("pt_variance_denoise", dict(flags=8, **BIG), {}, BAD, "unknown flags"),
    ("pt_variance_denoise", dict(sigma_variance=1e-30, sigma_depth=1e30), {}, BAD, "sigma_variance^2 or its reciprocal leaves binary32"),
    ("pt_variance_denoise", dict(BIG), dict(scratch=ADDR["scratch"] + 8), LARGE, "more than 2^30 pixels"),
    ("pt_variance_denoise", {}, dict(scratch=ADDR["scratch"] + 8, variance_out=ADDR["color"]), BAD, "scratch must be 16-byte aligned"),
    ("pt_variance_denoise", {}, dict(variance_out=ADDR["normal"] + 12, scratch=ADDR["variance"]), BAD,
     "out, variance_out and scratch must not overlap a guide plane"),
    ("pt_variance_denoise", {}, dict(scratch=ADDR["variance"], variance_out=ADDR["color"] + 12), BAD,
     "scratch must not overlap color, variance, out or variance_out"),
    ("pt_variance_denoise", {}, dict(variance_out=ADDR["out"] + 12), BAD, "variance_out must not overlap color or out"),

    ("pt_temporal_push", dict(struct_size=0, alpha=0.0), dict(state=None), BAD, "NULL state, params, cam, color, depth or out_color"),
    ("pt_temporal_push", dict(struct_size=0, alpha=0.0), {}, BAD, "struct_size is not this library's"),
    ("pt_temporal_push", dict(alpha=0.0, tol_depth=0.0), {}, BAD, "need 0 < alpha <= 1"),
    ("pt_temporal_push", dict(tol_normal=math.nan, flags=1), {}, BAD, "a tolerance is not a finite number > 0"),
    ("pt_temporal_push", dict(flags=1), dict(cam=abi.PtCamera()), BAD, "unknown flags"),
    ("pt_temporal_push", {}, dict(cam=abi.PtCamera()), BAD, "a degenerate camera"),

    ("pt_display_meter", dict(struct_size=0, w=0), dict(color=None), BAD, "NULL params or color"),
    ("pt_display_meter", dict(struct_size=0, w=0), {}, BAD, "struct_size is not this library's"),
    ("pt_display_meter", dict(w=0, tone=3), {}, BAD, "width and height must be > 0"),
    ("pt_display_meter", dict(w=1 << 16, h=(1 << 15) + 1, flags=1), {}, BAD, "more than 2^31 pixels"),
    ("pt_display_meter", dict(tone=3, flags=1), dict(state=None), BAD, "unknown tone"),
    ("pt_display_meter", dict(flags=1, lo_permille=-1), {}, BAD, "unknown flags"),
    ("pt_display_meter", dict(lo_permille=-1, adapt_up=0.0), {}, BAD, "need 0 <= lo_permille < hi_permille <= 1000"),
    ("pt_display_meter", dict(adapt_down=2.0, ev_min=-33.0), {}, BAD, "an adaptation rate is outside (0, 1]"),
    ("pt_display_meter", dict(ev_max=33.0, ev_bias=math.nan), {}, BAD, "need -32 <= ev_min <= ev_max <= 32"),
    ("pt_display_meter", dict(ev_bias=math.nan, white=0.0), {}, BAD, "ev_bias is not finite"),
    ("pt_display_meter", dict(white=0.0, **RECT_OUT), {}, BAD, "white: 1 / (white * white)"),
    ("pt_display_meter", dict(RECT_OUT), dict(state=None), BAD, "the metering rectangle is empty or leaves the frame"),
    ("pt_display_meter", dict(RECT_EMPTY), dict(state=None), BAD, "the metering rectangle is empty or leaves the frame"),
    ("pt_display_meter", {}, dict(state=None), BAD, "pt_display_meter: NULL state"),

    ("pt_display_apply", dict(tone=-1), dict(rgb8=None, linear=None), BAD, "unknown tone"),
    ("pt_display_apply", dict(RECT_EMPTY), dict(rgb8=None, linear=None, state=None), BAD, "the metering rectangle is empty or leaves the frame"),
    ("pt_display_apply", {}, dict(rgb8=None, linear=None, state=None), BAD, "rgb8_out and linear_out are both NULL"),
    ("pt_display_apply", {}, dict(rgb8=ADDR["color"], linear=ADDR["color"] + 4), BAD, "rgb8_out overlaps color or linear_out"),
    ("pt_display_apply", {}, dict(rgb8=ADDR["linear"] + 8), BAD, "rgb8_out overlaps color or linear_out"),
    ("pt_display_apply", {}, dict(linear=ADDR["color"] + 4, state=None), BAD, "linear_out overlaps color without being color"),

    ("pt_firefly", dict(struct_size=0, width=0), dict(out=None), BAD, "NULL params, color or out"),
    ("pt_firefly", dict(struct_size=0, width=0), {}, BAD, "struct_size is not this library's"),
    ("pt_firefly", dict(width=0, rank=3), {}, BAD, "width and height must be > 0"),
    ("pt_firefly", dict(rank=3, **BIG), {}, BAD, "rank must be 1 or 2"),
    ("pt_firefly", dict(k=math.nan, flags=4), {}, BAD, "k must be finite and > 0"),
    ("pt_firefly", dict(flags=4, **BIG), {}, BAD, "unknown flags"),
    ("pt_firefly", dict(BIG), dict(variance=None), BAD, "variance_out needs variance"),
    ("pt_firefly", dict(BIG), dict(counts=ADDR["counts"] + 4), LARGE, "more than 2^30 pixels"),
    ("pt_firefly", {}, dict(counts=ADDR["counts"] + 4, out=ADDR["color"]), BAD, "counts must be 8-byte aligned"),
    ("pt_firefly", {}, dict(out=ADDR["color"] + 12, counts=ADDR["variance_out"]), BAD, "must not overlap color or variance (variance_out may be variance itself)"),
    ("pt_firefly", {}, dict(variance_out=ADDR["variance"], counts=ADDR["variance"] + 8), BAD, "must not overlap color or variance (variance_out may be variance itself)"),
    ("pt_firefly", {}, dict(variance_out=ADDR["variance"], counts=ADDR["out"] + 8), BAD, "out, variance_out and counts must not overlap one another"),
    ("pt_firefly", {}, dict(variance_out=ADDR["variance"], out=ADDR["variance"] + 12), BAD, "must not overlap color or variance (variance_out may be variance itself)"),

    ("pt_spatial_variance", dict(struct_size=0, radius=0), dict(variance_out=None), BAD, "NULL params, color or variance_out"),
    ("pt_spatial_variance", dict(struct_size=0, radius=0), {}, BAD, "struct_size is not this library's"),
    ("pt_spatial_variance", dict(height=0, radius=0), {}, BAD, "width and height must be > 0"),
    ("pt_spatial_variance", dict(radius=0, min_pairs=0), {}, BAD, "radius must be 1 ... PT_SVAR_MAX_RADIUS"),
    ("pt_spatial_variance", dict(min_pairs=0, tol_depth=math.nan), {}, BAD, "min_pairs must be >= 1"),
    ("pt_spatial_variance", dict(tol_depth=math.nan, tol_normal=0.0), {}, BAD, "tol_depth must be finite and > 0"),
    ("pt_spatial_variance", dict(tol_normal=0.0, flags=4), {}, BAD, "tol_normal must be finite and > 0"),
    ("pt_spatial_variance", dict(flags=4 | abi.PT_SVAR_DEMODULATE), dict(albedo=None), BAD, "unknown flags"),
    ("pt_spatial_variance", dict(flags=abi.PT_SVAR_DEMODULATE, **BIG), dict(albedo=None), BAD, "PT_SVAR_DEMODULATE needs albedo"),
    ("pt_spatial_variance", dict(BIG), dict(counts=ADDR["counts"] + 4), LARGE, "more than 2^30 pixels"),
    ("pt_spatial_variance", {}, dict(counts=ADDR["counts"] + 4, variance_out=ADDR["color"]), BAD, "counts must be 8-byte aligned"),
    ("pt_spatial_variance", {}, dict(variance_out=ADDR["id"] + PLANE - 4, counts=ADDR["id"] + PLANE), BAD,
     "must not overlap color, a guide or variance_in (variance_out may be variance_in itself)"),
    ("pt_spatial_variance", {}, dict(variance_out=ADDR["variance"], counts=ADDR["variance"] + 8), BAD,
     "must not overlap color, a guide or variance_in (variance_out may be variance_in itself)"),
    ("pt_spatial_variance", {}, dict(variance_out=ADDR["variance"] + 12), BAD,
     "must not overlap color, a guide or variance_in (variance_out may be variance_in itself)"),
    ("pt_spatial_variance", {}, dict(counts=ADDR["variance_out"] + FRAME - 8), BAD, "variance_out and counts must not overlap one another"),

    ("pt_image_error", dict(struct_size=0, width=0), dict(result=None), BAD, "NULL params, a, ref, result or scratch"),
    ("pt_image_error", dict(struct_size=0, width=0), {}, BAD, "struct_size is not this library's"),
    ("pt_image_error", dict(width=0, **RECT_OUT), {}, BAD, "width and height must be > 0"),
    ("pt_image_error", dict(eps=0.0, **RECT_OUT), {}, BAD, "the rectangle leaves the frame"),
    ("pt_image_error", dict(eps=0.0, **RECT_EMPTY), {}, BAD, "eps must be finite and >= 2^-126"),
    ("pt_image_error", dict(eps=math.inf, flags=2), {}, BAD, "eps must be finite and >= 2^-126"),
    ("pt_image_error", dict(flags=2, **BIG), {}, BAD, "unknown flags"),
    ("pt_image_error", dict(BIG), dict(result=ADDR["result"] + 4), LARGE, "more than 2^30 pixels"),
    ("pt_image_error", dict(scratch_bytes=0), dict(scratch=ADDR["scratch"] + 4), BAD, "result and scratch must be 8-byte aligned"),
    ("pt_image_error", dict(scratch_bytes=0), dict(plane=ADDR["color"]), BAD, "scratch_bytes is less than pt_image_error_scratch_bytes()"),
    ("pt_image_error", {}, dict(plane=ADDR["ref"] + FRAME - 4, result=ADDR["scratch"]), BAD, "error_plane, result and scratch must not overlap an input"),
    ("pt_image_error", {}, dict(result=ADDR["scratch"] + 8), BAD, "error_plane, result and scratch must not overlap one another"),
    ("pt_image_error", {}, dict(plane=ADDR["result"] - PLANE + 8), BAD, "error_plane, result and scratch must not overlap one another"),
]


@pytest.mark.parametrize("entry,fields,ptrs,rc,message", CASES,
                         ids=[f"{e}-{i}" for i, (e, *_) in enumerate(CASES)])
def test_the_first_defect_in_the_entry_points_own_order_is_the_one_reported(lib, entry, fields, ptrs, rc, message):
    assert call(lib, entry, dict(fields), ptrs) == rc, lib.pt_last_error()
    text = lib.pt_last_error().decode()
    assert text.startswith(entry + ": ") and message in text, text


def test_every_entry_point_is_covered():
    assert {case[0] for case in CASES} == set(PLANES) and len(PLANES) == 8
