"""CPU tests of the display stage's boundary and definition (include/pt_render.h: PtDisplay, pt_display_meter, pt_display_apply): the library
exports the entry points, abi.py declares them as the header does, the defaults are the header's, invalid calls are refused on the host
before a device or the state is touched; and the numpy restatement of the header (tests/display_model.py, the one
tests/test_gpu_display.py holds the kernels to) has the properties the header promises: the bin edges, the LOGC table, exposures that
are exact powers of two, the reference tone's bytes, monotone curves, an exposure that follows the frame's scale.  The last test prints
the clipping record of the oracle's Cornell frame that DESIGN.md quotes.

Refusals that need a live object (a NULL state is the only one a host can judge) are in tests/test_gpu_display.py."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import display_model as D
import scenes_small as S
from path_tracer_amd import abi, scenes

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "pt_render.h"
DISPLAY = ["pt_display_params_init", "pt_display_create", "pt_display_destroy", "pt_display_reset", "pt_display_frames", "pt_display_meter",
           "pt_display_set_exposure", "pt_display_apply", "pt_display_exposure", "pt_display_histogram", "pt_debug_last_display"]
F = np.float32


def header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


# ---- the boundary -------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_display_stage(lib):
    for n in DISPLAY:
        assert hasattr(lib, n), f"libpt_render.so does not export {n}"
    assert abi.has_display(lib)
    assert set(DISPLAY) == set(abi.DISPLAY_SYMBOLS)
    assert not abi.DISPLAY_SYMBOLS & (abi.ACCUM_SYMBOLS | abi.ADAPTIVE_SYMBOLS | abi.AOV_SYMBOLS | abi.DENOISE_SYMBOLS | abi.PLAN_SYMBOLS |
                                      abi.VARIANCE_SYMBOLS | abi.TEMPORAL_SYMBOLS)
    assert lib.pt_abi_version() == 2 and "#define PT_ABI_VERSION 2" in HEADER.read_text()
    for n in DISPLAY:  # the prefixes other tests scan the header by
        assert not re.match(r"pt_(accum_|adaptive_|denoise|variance_|temporal_|aov_)", n), n


def test_struct_matches_the_header():
    body = re.search(r"typedef struct PtDisplayParams\s*\{(.*?)\}\s*PtDisplayParams;", header_text(), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = re.match(r"(int32_t|uint32_t|float)\s+(.*)", decl).groups()
            fields += [(nm.strip(), ctype) for nm in names.split(",")]
    ctypes_of = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    assert [n for n, _ in fields] == ["struct_size", "tone", "flags", "ev_bias", "ev_min", "ev_max", "lo_permille", "hi_permille", "adapt_up",
                                      "adapt_down", "white", "rect_x0", "rect_y0", "rect_x1", "rect_y1", "reserved"]
    assert abi.PtDisplayParams._fields_ == [(n, ctypes_of[t]) for n, t in fields]
    assert C.sizeof(abi.PtDisplayParams) == 64


def test_ctypes_prototypes_match_the_header():
    protos = {name: (ret, [re.sub(r"\s+", " ", a.strip()) for a in args.split(",")])
              for ret, name, args in re.findall(r"^\s*([A-Za-z_][A-Za-z0-9_]*)\s+(pt_display_\w+|pt_debug_last_display)\s*\(([^)]*)\)\s*;",
                                                header_text(), re.M)}
    assert set(protos) == set(DISPLAY)
    vp, i32 = C.c_void_p, C.c_int32
    want = {
        "pt_display_params_init": (("void", ["PtDisplayParams* params"]), (None, [C.POINTER(abi.PtDisplayParams)])),
        "pt_display_create": (("int", ["PtDisplay** out"]), (C.c_int, [C.POINTER(vp)])),
        "pt_display_destroy": (("void", ["PtDisplay* state"]), (None, [vp])),
        "pt_display_reset": (("int", ["PtDisplay* state", "void* stream"]), (C.c_int, [vp, vp])),
        "pt_display_frames": (("int32_t", ["const PtDisplay* state"]), (i32, [vp])),
        "pt_display_meter": (("int", ["PtDisplay* state", "const PtDisplayParams* params", "const float* color", "int32_t width", "int32_t height",
                                      "void* stream"]), (C.c_int, [vp, C.POINTER(abi.PtDisplayParams), vp, i32, i32, vp])),
        "pt_display_set_exposure": (("int", ["PtDisplay* state", "float ev", "void* stream"]), (C.c_int, [vp, C.c_float, vp])),
        "pt_display_apply": (("int", ["const PtDisplay* state", "const PtDisplayParams* params", "const float* color", "int32_t width",
                                      "int32_t height", "uint8_t* rgb8_out", "float* linear_out", "void* stream"]),
                             (C.c_int, [vp, C.POINTER(abi.PtDisplayParams), vp, i32, i32, vp, vp, vp])),
        "pt_display_exposure": (("int", ["const PtDisplay* state", "float* ev_host", "void* stream"]), (C.c_int, [vp, C.POINTER(C.c_float), vp])),
        "pt_display_histogram": (("int", ["const PtDisplay* state", "uint32_t host[257]", "void* stream"]), (C.c_int, [vp, C.POINTER(C.c_uint32), vp])),
        "pt_debug_last_display": (("int", ["int32_t out[8]"]), (C.c_int, [C.POINTER(i32)])),
    }
    for name, (proto, sig) in want.items():
        assert protos[name] == proto, name
        assert abi.SIGNATURES[name] == sig, name


def test_defaults_are_the_headers(lib):
    m = dict(re.findall(r"^#define (PT_DISPLAY_DEFAULT_\w+) (\S+)", HEADER.read_text(), re.M))
    p = abi.PtDisplayParams(*([7] * 16))
    lib.pt_display_params_init(C.byref(p))
    assert (p.struct_size, p.flags, p.reserved) == (C.sizeof(abi.PtDisplayParams), 0, 0)
    assert (p.rect_x0, p.rect_y0, p.rect_x1, p.rect_y1) == (0, 0, 0, 0)  # the whole frame
    assert m["PT_DISPLAY_DEFAULT_TONE"] == "PT_TONE_ACES" and p.tone == abi.PT_TONE_ACES == abi.PT_DISPLAY_DEFAULT_TONE == D.DEFAULTS["tone"] == 2
    for field in ("ev_bias", "ev_min", "ev_max", "adapt_up", "adapt_down", "white"):
        want = F(m[f"PT_DISPLAY_DEFAULT_{field.upper()}"].rstrip("f"))
        assert F(getattr(p, field)) == want == F(getattr(abi, f"PT_DISPLAY_DEFAULT_{field.upper()}")) == F(D.DEFAULTS[field]), field
    for field in ("lo_permille", "hi_permille"):
        assert getattr(p, field) == int(m[f"PT_DISPLAY_DEFAULT_{field.upper()}"]) == getattr(abi, f"PT_DISPLAY_DEFAULT_{field.upper()}") == D.DEFAULTS[field]
    assert (p.tone, p.ev_bias, p.ev_min, p.ev_max, p.lo_permille, p.hi_permille, p.adapt_up, p.adapt_down, p.white) == \
        (2, 0.0, -16.0, 16.0, 400, 950, 1.0, 1.0, 4.0)
    lib.pt_display_params_init(None)  # a NULL struct is ignored
    tones = dict(re.findall(r"^#define (PT_TONE_\w+) (\d+)", HEADER.read_text(), re.M))
    assert {k: int(v) for k, v in tones.items()} == {"PT_TONE_REFERENCE": 0, "PT_TONE_REINHARD": 1, "PT_TONE_ACES": 2}
    assert (abi.PT_TONE_REFERENCE, abi.PT_TONE_REINHARD, abi.PT_TONE_ACES) == (D.REFERENCE, D.REINHARD, D.ACES) == (0, 1, 2)
    assert abi.TONES == D.TONES


def test_header_constants_match_the_model_and_float64():
    text = HEADER.read_text()
    logc = [int(v) for v in re.search(r"#define PT_DISPLAY_LOGC \{([^}]*)\}", text).group(1).split(",")]
    want = [int(np.rint(65536.0 * np.log2(1.0 + (2 * j + 1) / 16.0))) for j in range(8)]
    assert logc == want == D.LOGC
    for j in range(8):  # no entry sits near a rounding tie: the table does not depend on the last bits of log2
        assert abs(65536.0 * np.log2(1.0 + (2 * j + 1) / 16.0) - want[j]) < 0.4
    key = float.fromhex(re.search(r"#define PT_DISPLAY_LOG2_KEY \((-0x[0-9a-fp.+-]+)f\)", text).group(1))
    assert F(key) == key == D.LOG2_KEY == F(math.log2(0.18))
    assert D.LN2 == F(math.log(2.0)) and "0x1.62e430p-1f" in text
    # bin b's value is the log2 of the centre of [2^(o + j/8) ... ): monotone, 8 per octave
    vals = [D.bin_value(b) for b in range(256)]
    assert all(b > a for a, b in zip(vals, vals[1:])) and vals[128] == logc[0] and vals[0] == -16 * 65536 + logc[0]


# Pointers that are never dereferenced: every call below is refused on the host before the state or a plane is read.
STATE, COLOR, RGB8, LINEAR = (0x10000000 + i * 0x10000000 for i in range(4))


def params(lib, **over):
    p = abi.PtDisplayParams()
    lib.pt_display_params_init(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def meter(lib, p, state=STATE, color=COLOR, w=64, h=40):
    return lib.pt_display_meter(state, C.byref(p) if p is not None else None, color, w, h, None)


def apply(lib, p, state=STATE, color=COLOR, w=64, h=40, rgb8=RGB8, linear=LINEAR):
    return lib.pt_display_apply(state, C.byref(p) if p is not None else None, color, w, h, rgb8, linear, None)


BAD_PARAMS = [dict(struct_size=0), dict(struct_size=60), dict(struct_size=68), dict(tone=-1), dict(tone=3), dict(flags=1), dict(flags=4),
              dict(flags=1 << 31), dict(lo_permille=-1), dict(hi_permille=1001), dict(lo_permille=950), dict(lo_permille=960),
              dict(lo_permille=0, hi_permille=0), dict(adapt_up=0.0), dict(adapt_up=-0.5), dict(adapt_up=1.0000001), dict(adapt_up=math.nan),
              dict(adapt_down=0.0), dict(adapt_down=2.0), dict(adapt_down=math.nan), dict(adapt_down=math.inf), dict(ev_min=1.0, ev_max=0.0),
              dict(ev_min=-32.5), dict(ev_max=33.0), dict(ev_min=math.nan), dict(ev_max=math.nan), dict(ev_min=-math.inf),
              dict(ev_bias=math.nan), dict(ev_bias=math.inf), dict(white=0.0), dict(white=math.nan), dict(white=math.inf), dict(white=1e-30),
              dict(white=1e30), dict(rect_x1=1), dict(rect_x0=5, rect_x1=5, rect_y1=3), dict(rect_x1=65, rect_y1=40), dict(rect_x1=64, rect_y1=41),
              dict(rect_x0=-1, rect_x1=4, rect_y1=4), dict(rect_y0=9, rect_x1=4, rect_y1=9), dict(rect_x0=7, rect_x1=3, rect_y1=3)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_refuses_bad_params_before_touching_a_device(lib, bad):
    assert meter(lib, params(lib, **bad)) == abi.PT_ERR_INVALID_ARG
    assert b"pt_display_meter" in lib.pt_last_error()
    assert apply(lib, params(lib, **bad)) == abi.PT_ERR_INVALID_ARG
    assert b"pt_display_apply" in lib.pt_last_error()
    assert apply(lib, params(lib, **bad), state=None) == abi.PT_ERR_INVALID_ARG


def test_refuses_bad_frames_and_null_arguments(lib):
    good = params(lib)
    for w, h in [(0, 40), (64, 0), (-1, 40), (64, -3), (1 << 16, (1 << 15) + 1), (1 << 30, 4)]:
        assert meter(lib, good, w=w, h=h) == abi.PT_ERR_INVALID_ARG and b"pt_display_meter" in lib.pt_last_error(), (w, h)
        assert apply(lib, good, w=w, h=h) == abi.PT_ERR_INVALID_ARG and b"pt_display_apply" in lib.pt_last_error(), (w, h)
    assert meter(lib, None) == abi.PT_ERR_INVALID_ARG
    assert meter(lib, good, color=None) == abi.PT_ERR_INVALID_ARG
    assert meter(lib, good, state=None) == abi.PT_ERR_INVALID_ARG and b"pt_display_meter" in lib.pt_last_error()
    assert apply(lib, None) == abi.PT_ERR_INVALID_ARG
    assert apply(lib, good, color=None) == abi.PT_ERR_INVALID_ARG
    assert apply(lib, good, rgb8=None, linear=None) == abi.PT_ERR_INVALID_ARG and b"both NULL" in lib.pt_last_error()


def test_refuses_overlapping_planes(lib):
    good = params(lib)
    n = 64 * 40 * 3
    assert apply(lib, good, rgb8=COLOR) == abi.PT_ERR_INVALID_ARG and b"rgb8_out overlaps" in lib.pt_last_error()
    assert apply(lib, good, rgb8=COLOR + 4 * n - 1) == abi.PT_ERR_INVALID_ARG       # the last byte of color
    assert apply(lib, good, rgb8=COLOR - n + 1) == abi.PT_ERR_INVALID_ARG           # its first
    assert apply(lib, good, rgb8=LINEAR + 8) == abi.PT_ERR_INVALID_ARG              # inside linear_out
    assert apply(lib, good, linear=COLOR + 4) == abi.PT_ERR_INVALID_ARG and b"linear_out overlaps" in lib.pt_last_error()
    assert apply(lib, good, linear=COLOR - 4 * n + 4) == abi.PT_ERR_INVALID_ARG


def test_refuses_null_objects(lib):
    out = C.c_void_p(0x7)
    assert lib.pt_display_create(None) == abi.PT_ERR_INVALID_ARG and b"pt_display_create" in lib.pt_last_error()
    assert lib.pt_display_frames(None) == -1
    assert lib.pt_display_reset(None, None) == abi.PT_ERR_INVALID_ARG and b"pt_display_reset" in lib.pt_last_error()
    assert lib.pt_display_set_exposure(None, 1.0, None) == abi.PT_ERR_INVALID_ARG and b"pt_display_set_exposure" in lib.pt_last_error()
    ev = C.c_float(7.0)
    assert lib.pt_display_exposure(None, C.byref(ev), None) == abi.PT_ERR_INVALID_ARG and ev.value == 7.0
    assert lib.pt_display_exposure(STATE, None, None) == abi.PT_ERR_INVALID_ARG and b"pt_display_exposure" in lib.pt_last_error()
    host = (C.c_uint32 * 257)()
    assert lib.pt_display_histogram(None, host, None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_display_histogram(STATE, None, None) == abi.PT_ERR_INVALID_ARG and b"pt_display_histogram" in lib.pt_last_error()
    assert lib.pt_debug_last_display(None) == abi.PT_ERR_INVALID_ARG and b"pt_debug_last_display" in lib.pt_last_error()
    lib.pt_display_destroy(None)  # ignored
    del out


# ---- the model: the histogram -----------------------------------------------------------------------------------------------------------

def below(v):
    return np.nextafter(F(v), F(-np.inf))


def test_bin_edges():
    b = D.bins_of
    assert b(F(2.0 ** -16)) == 0 and b(below(2.0 ** -16)) == 0 and b(F(2.0 ** -20)) == 0   # everything under the range: bin 0
    assert b(F(1e-40)) == 0 and b(np.uint32(1).view(F)) == 0                                # denormals too
    assert b(F(2.0 ** 16)) == 255 and b(below(2.0 ** 16)) == 255 and b(F(3e38)) == 255     # everything over it: bin 255
    for octave in range(-16, 16):                                                           # each octave's eight edges
        for j in range(8):
            edge = F(2.0 ** octave * (1.0 + j / 8.0))
            want = (octave + 16) * 8 + j
            assert b(edge) == want, (octave, j)
            if want > 0:
                assert b(below(edge)) == want - 1, (octave, j)
    assert b(F(1.0)) == 128 and b(F(0.18)) == 16 * 8 - 24 + 3                              # 0.18 = 2^-3 x 1.44
    for v in (np.nan, np.inf, -np.inf, -1.0, -1e-40, 0.0, -0.0):                            # the rejected classes
        assert b(F(v)) == 256, v
    with np.errstate(all="ignore"):
        h = D.histogram(np.array([[[np.nan, 1, 1], [1, np.inf, 1], [-1, -1, -1], [0, 0, 0], [1, 1, 1], [F(3e38), F(3e38), F(3e38)]]], dtype=F))
    assert h[256] == 4 and h[128 - 1] + h[128] == 1 and h[255] == 1 and h.sum() == 6  # Y(1, 1, 1) rounds to 1 or just under it; the weights sum to 1: no overflow


def test_luminance_is_three_products_and_two_sums():
    c = np.array([0.3, 0.6, 0.1], dtype=F)
    want = F(F(F(0.2126) * c[0]) + F(F(0.7152) * c[1])) + F(F(0.0722) * c[2])
    assert D.luminance(c) == F(want)


def test_rectangle_is_in_frame_coordinates():
    c = np.full((6, 8, 3), 1.0, dtype=F)
    c[1:3, 2:7] = 4.0
    h = D.histogram(c, rect=(2, 1, 7, 3))
    assert h.sum() == 10 and h[D.bins_of(D.luminance(F([4, 4, 4])))] == 10


def test_solve_takes_the_band():
    h = np.zeros(257, np.uint32)
    h[10], h[100], h[200] = 400, 550, 50  # ranks [0, 400) [400, 950) [950, 1000): the default band is bin 100 alone
    assert D.solve(h) == (550 * D.bin_value(100), 550)
    assert D.solve(h, 0, 1000) == (400 * D.bin_value(10) + 550 * D.bin_value(100) + 50 * D.bin_value(200), 1000)
    assert D.solve(h, 399, 401) == (D.bin_value(10) + D.bin_value(100), 2)
    assert D.solve(np.zeros(257, np.uint32)) == (0, 0) and D.target(np.zeros(257, np.uint32)) is None
    h[:] = 0
    h[256] = 9  # rejected pixels are not ranked
    assert D.solve(h) == (0, 0)
    h[:256] = 1 << 23  # 2^31 pixels: S stays an exact integer of binary64
    s, c = D.solve(h, 0, 1000)
    assert c == 1 << 31 and abs(s) < 1 << 53


# ---- the model: exposure and curves -------------------------------------------------------------------------------------------------------

def sweep_frame(seed=3, shape=(24, 32, 3), lo=-9.0, hi=9.0):
    r = np.random.default_rng(seed)
    return np.exp2(r.uniform(lo, hi, shape)).astype(F)


def test_integer_exposures_are_exact_powers_of_two():
    for k in range(-32, 33):
        assert D.scale_of(F(k)) == F(2.0 ** k), k
    assert D.scale_of(F(0.0)) == F(1.0) and D.scale_of(F(-0.0)) == F(1.0)
    for e in (-7.75, -0.5, 0.25, 0.3, 3.9, 15.999):  # and 2^e to pt_exp_neg's 1e-6 otherwise
        assert abs(float(D.scale_of(F(e))) / 2.0 ** float(F(e)) - 1.0) < 2e-6, e
    c = sweep_frame()
    for tone in D.TONES.values():
        for k in (-5, -1, 1, 4):
            a8, a = D.apply(c, F(k), tone)
            b8, b = D.apply(c * F(2.0 ** k), F(0.0), tone)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a8, b8), (tone, k)


def quantise_scalar(v):
    """main.cpp:33-59 for one value, spelled out on its own."""
    v = F(v)
    with np.errstate(all="ignore"):
        s = np.sqrt(v)
    if s != s:
        return 0
    s = F(0.0) if s < 0 else F(0.999) if s > F(0.999) else s
    return int(F(256.0) * s) & 255


def test_reference_tone_at_0_ev_is_the_reference_output_stage():
    c = sweep_frame(5, (9, 11, 3), -12, 3)
    c[0, 0] = [np.nan, np.inf, -np.inf]
    c[1, 1] = [-1.0, 0.0, -0.0]
    c[2, 2] = [F(1e-40), F(3e38), F(0.998001)]
    c[3, 3] = [F(2.0 ** 20), F(2.0 ** 21), 1.0]
    rgb8, lin = D.apply(c, F(0.0), D.REFERENCE)
    want = np.array([[[quantise_scalar(v) for v in px] for px in row] for row in c[::-1]], dtype=np.uint8)
    assert np.array_equal(rgb8, want)
    assert lin[0, 0, 0] == 0 and lin[0, 0, 1] == F(2.0 ** 20) and lin[0, 0, 2] == 0 and lin[1, 1, 0] == 0   # NaN, +inf, -inf, negative
    assert np.array_equal(lin[4:].view(np.uint32), c[4:].view(np.uint32))                                    # y = x


@pytest.mark.parametrize("tone", sorted(D.TONES))
def test_curves_are_monotone(tone):
    """Over x = 2^-24 ... 2^20 in steps of 1 / 64 octave.  A curve is a handful of rounded operations (ACES: eight), so where it flattens
    the computed value may dip by that many half-ulps; the bytes, which are what is shown, never go down."""
    x = np.exp2(np.arange(-24 * 64, 20 * 64 + 1, dtype=np.float64) / 64.0).astype(F)
    with np.errstate(all="ignore"):
        y = D.curve(x, D.TONES[tone]).astype(F)
    assert np.isfinite(y).all() and (y >= 0).all()
    assert (y[1:] >= y[:-1] * F(1.0 - 8 * 2.0 ** -24)).all()
    b = D.quantise(y).astype(np.int32)
    assert (np.diff(b) >= 0).all() and b[0] == 0 and b[-1] == 255
    if tone == "reinhard":
        assert D.curve(F(4.0), D.REINHARD, 4.0) == F(1.0)  # `white` maps to 1
    if tone == "aces":
        assert y.max() < 1.04  # the fit's asymptote 2.51 / 2.43


@pytest.mark.parametrize("k", [-6, -1, 3, 7])
def test_exposure_follows_the_frames_scale(k):
    """Scaling a frame by 2^k moves every bin by 8 k and S by exactly 65536 k C, so the solved exposure moves by -k up to the rounding of
    the binary64 division and of the conversion to binary32: two ulps of a value below 32, 2^-18.  Luminances within 2^-9 ... 2^9 and
    |k| <= 7: nothing reaches the ends of the bin range."""
    c = sweep_frame(11)
    y = D.luminance(c)
    assert y.min() > 2.0 ** -9 and y.max() < 2.0 ** 9
    h0, hk = D.histogram(c), D.histogram(c * F(2.0 ** k))
    assert np.array_equal(np.roll(h0[:256], 8 * k), hk[:256]) and h0[256] == hk[256] == 0
    e0, ek = D.target(h0), D.target(hk)
    print(f"k = {k}: e0 = {e0!r}, ek = {ek!r}, |ek - (e0 - k)| = {abs(float(ek) - (float(e0) - k)):.3g}")
    assert abs(float(ek) - (float(e0) - k)) <= 2.0 ** -18
    assert abs(float(e0)) < 16 and abs(float(ek)) < 16  # inside the default range: nothing clamped


def test_adaptation():
    s = D.State()
    dark, bright = np.full((4, 4, 3), 0.01, dtype=F), np.full((4, 4, 3), 10.0, dtype=F)
    e_dark, e_bright = D.target(D.histogram(dark)), D.target(D.histogram(bright))
    assert e_dark > e_bright
    assert s.meter(dark, adapt_up=0.5, adapt_down=0.25) == e_dark              # the first metering is instant
    e1 = s.meter(bright, adapt_up=0.5, adapt_down=0.25)                         # going down: a quarter of the way
    assert e1 == F(e_dark + F(F(e_bright - e_dark) * F(0.25)))
    e2 = s.meter(dark, adapt_up=0.5, adapt_down=0.25)                           # going up: half of the way
    assert e2 == F(e1 + F(F(e_dark - e1) * F(0.5)))
    with np.errstate(all="ignore"):
        assert s.meter(np.full((4, 4, 3), np.nan, dtype=F)) == e2 and s.last[256] == 16  # nothing binned: e stays
    s.reset()
    assert s.e == 0 and s.meter(bright, adapt_up=0.5, adapt_down=0.25) == e_bright
    s.set_exposure(40.0)
    assert s.e == 32 and s.meter(bright, adapt_down=0.5) == F(F(32.0) + F(F(e_bright - F(32.0)) * F(0.5)))
    assert D.target(D.histogram(bright), ev_bias=1.5) == F(e_bright + F(1.5)) and D.target(D.histogram(bright), ev_max=-7.0) == F(-7.0)
    assert D.target(D.histogram(bright), ev_min=-5.0) == F(-5.0)


# ---- hosts --------------------------------------------------------------------------------------------------------------------------

def test_display_main_compiles_against_the_facade(tmp_path, lib):
    out = tmp_path / "display_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{libdir / 'include'}", str(ROOT / "tests" / "cpp" / "display_main.cpp"), "-o", str(out), f"-L{libdir}",
                    "-lpt_render", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert out.exists()


# ---- the record DESIGN.md quotes -------------------------------------------------------------------------------------------------------

def test_clipping_record_on_the_oracles_cornell_frame(orc):
    """The oracle's small Cornell frame, 64 x 40 at 32 spp, through the reference's output stage and through auto-exposure + ACES with the
    defaults: the fraction of channel values at code 255 and at code 0.  A record (printed; DESIGN.md quotes it), not a threshold: the
    only assertions are that the model ran and that the two stages differ."""
    ps, cam = S.ALL["cornell"]()
    w, h = 64, 40
    fb = orc.render(ps, scenes.make_camera(cam, w, h).c, w, h, 32)
    ref8, _ = D.apply(fb, F(0.0), D.REFERENCE)
    e = D.State().meter(fb)
    aces8, _ = D.apply(fb, e, D.ACES)
    for name, img in (("reference stage", ref8), (f"auto-exposure ({float(e):+.3f} EV) + ACES", aces8)):
        print(f"{name}: {np.mean(img == 255):.4f} of the values at code 255, {np.mean(img == 0):.4f} at code 0, mean code {img.mean():.1f}")
    assert ref8.shape == aces8.shape == (h, w, 3) and not np.array_equal(ref8, aces8)
