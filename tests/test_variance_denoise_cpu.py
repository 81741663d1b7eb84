"""CPU tests of the variance-guided denoiser's boundary and definition (include/pt_render.h: pt_variance_estimate, pt_variance_denoise):
the library exports the entry points, abi.py declares them as the header does, pt_variance_denoise_scratch_floats gives the documented
size, every invalid call is refused before any device call; the numpy binary32 restatement of the header (tests/variance_model.py, the
one tests/test_gpu_variance_denoise.py holds the kernels to) has the properties the header promises; and the default sigma_variance is
the one a measured sweep picks — with it the filter improves 8, 32 and 128 spp frames of the oracle's alike, where pt_denoise's defaults
make the 128 spp frame worse."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import denoise_model as M
import scenes_small as S
import variance_model as V
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from test_adaptive_cpu import book_np
from test_aov_cpu import aov_np

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "pt_render.h"
VARIANCE = ["pt_variance_estimate", "pt_variance_denoise_params_init", "pt_variance_denoise_scratch_floats", "pt_variance_denoise",
            "pt_debug_last_variance_denoise"]
F = np.float32


def header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def header_macros():
    return dict(re.findall(r"^#define (PT_VDENOISE_\w+) (\S+)", HEADER.read_text(), re.M))


# ---- the boundary -------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_variance_denoiser(lib):
    for n in VARIANCE:
        assert hasattr(lib, n), f"libpt_render.so does not export {n}"
    assert abi.has_variance_denoise(lib)
    assert set(VARIANCE) == set(abi.VARIANCE_SYMBOLS)
    assert not abi.VARIANCE_SYMBOLS & (abi.ACCUM_SYMBOLS | abi.ADAPTIVE_SYMBOLS | abi.AOV_SYMBOLS | abi.DENOISE_SYMBOLS | abi.PLAN_SYMBOLS)
    assert lib.pt_abi_version() == 2 and "#define PT_ABI_VERSION 2" in HEADER.read_text()


def test_struct_matches_the_header():
    body = re.search(r"typedef struct PtVarianceDenoiseParams\s*\{(.*?)\}\s*PtVarianceDenoiseParams;", header_text(), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = re.match(r"(int32_t|uint32_t|float)\s+(.*)", decl).groups()
            fields += [(nm.strip(), ctype) for nm in names.split(",")]
    assert [f[0] for f in fields] == ["struct_size", "width", "height", "iterations", "sigma_variance", "sigma_normal", "sigma_depth",
                                      "sigma_albedo", "flags", "reserved"]
    ctypes_of = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, t) for n, t in abi.PtVarianceDenoiseParams._fields_] == [(n, ctypes_of[t]) for n, t in fields]
    assert C.sizeof(abi.PtVarianceDenoiseParams) == 4 * len(fields) == 40


def test_ctypes_prototypes_match_the_header():
    protos = {name: (ret, [re.sub(r"\s+", " ", a.strip()) for a in args.split(",")])
              for ret, name, args in re.findall(r"^\s*([A-Za-z_][A-Za-z0-9_]*)\s+(pt_variance_\w+|pt_debug_last_variance_denoise)\s*\(([^)]*)\)\s*;",
                                                header_text(), re.M)}
    assert set(protos) == set(VARIANCE)
    assert protos["pt_variance_estimate"] == ("int", ["const PtAccum* acc", "float* variance_device", "void* stream"])
    assert abi.SIGNATURES["pt_variance_estimate"] == (C.c_int, [C.c_void_p] * 3)
    assert protos["pt_variance_denoise_params_init"] == ("void", ["PtVarianceDenoiseParams* params", "int32_t width", "int32_t height"])
    assert abi.SIGNATURES["pt_variance_denoise_params_init"] == (None, [C.POINTER(abi.PtVarianceDenoiseParams), C.c_int32, C.c_int32])
    assert protos["pt_variance_denoise_scratch_floats"] == ("int64_t", ["int32_t width", "int32_t height"])
    assert abi.SIGNATURES["pt_variance_denoise_scratch_floats"] == (C.c_int64, [C.c_int32, C.c_int32])
    assert protos["pt_debug_last_variance_denoise"] == ("int", ["int32_t out[8]"])
    assert abi.SIGNATURES["pt_debug_last_variance_denoise"] == (C.c_int, [C.POINTER(C.c_int32)])
    assert protos["pt_variance_denoise"] == ("int", ["const PtVarianceDenoiseParams* params", "const float* color", "const float* variance",
                                                     "const float* albedo", "const float* normal", "const float* depth", "float* out",
                                                     "float* variance_out", "float* scratch", "void* stream"])
    assert abi.SIGNATURES["pt_variance_denoise"] == (C.c_int, [C.POINTER(abi.PtVarianceDenoiseParams)] + [C.c_void_p] * 9)


def test_defaults_are_the_headers(lib):
    m = header_macros()
    p = abi.PtVarianceDenoiseParams()
    lib.pt_variance_denoise_params_init(C.byref(p), 19, 13)
    assert (p.struct_size, p.width, p.height, p.reserved) == (C.sizeof(abi.PtVarianceDenoiseParams), 19, 13, 0)
    assert p.iterations == int(m["PT_VDENOISE_DEFAULT_ITERATIONS"]) == abi.PT_VDENOISE_DEFAULT_ITERATIONS == V.DEFAULTS["iterations"] == 5
    for term in ("variance", "normal", "depth", "albedo"):
        want = F(m[f"PT_VDENOISE_DEFAULT_SIGMA_{term.upper()}"].rstrip("f"))
        assert F(getattr(p, f"sigma_{term}")) == want == F(getattr(abi, f"PT_VDENOISE_DEFAULT_SIGMA_{term.upper()}")), term
        assert F(V.DEFAULTS[f"sigma_{term}"]) == want, term
    # the guide terms, the levels and the demodulation are pt_denoise's
    for term in ("normal", "depth", "albedo"):
        assert V.DEFAULTS[f"sigma_{term}"] == M.DEFAULTS[f"sigma_{term}"], term
    assert m["PT_VDENOISE_DEMODULATE"] == "1u" and abi.PT_VDENOISE_DEMODULATE == V.DEMODULATE == 1
    assert m["PT_VDENOISE_NO_LDS"] == "2u" and abi.PT_VDENOISE_NO_LDS == 2
    assert m["PT_VDENOISE_DEFAULT_FLAGS"] == "PT_VDENOISE_DEMODULATE" and p.flags == 1 and V.DEFAULTS["demodulate"] is True
    assert int(m["PT_VDENOISE_MAX_ITERATIONS"]) == abi.PT_VDENOISE_MAX_ITERATIONS == 8
    lib.pt_variance_denoise_params_init(None, 19, 13)  # a NULL struct is ignored


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (19, 13), (70, 45), (1920, 1080), (32768, 32768)])
def test_scratch_floats(lib, w, h):
    """Per pixel: two working planes of a 16-byte record (colour, variance.r) and an 8-byte record (variance.g, variance.b) — 2 x 6
    floats — and pt_denoise's two 16-byte guide records — 8 floats."""
    assert lib.pt_variance_denoise_scratch_floats(w, h) == (2 * (4 + 2) + 2 * 4) * w * h == 20 * w * h


def test_scratch_floats_invalid(lib):
    for w, h in [(0, 13), (19, 0), (-1, 13), (19, -5), (32768, 32769), (1 << 20, 1 << 20)]:
        assert lib.pt_variance_denoise_scratch_floats(w, h) < 0, (w, h)


# Device pointers that are never dereferenced: every call below is refused on the host.
W, H = 19, 13
PX = W * H
COLOR, VAR, ALBEDO, NORMAL, DEPTH, OUT, VOUT, SCRATCH = (0x10000000 + i * 0x1000000 for i in range(8))


def params(**over):
    p = abi.PtVarianceDenoiseParams(C.sizeof(abi.PtVarianceDenoiseParams), W, H, 5, 2.0, 0.5, 0.2, 0.0, abi.PT_VDENOISE_DEMODULATE, 0)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def call(lib, p, color=COLOR, variance=VAR, albedo=ALBEDO, normal=NORMAL, depth=DEPTH, out=OUT, variance_out=VOUT, scratch=SCRATCH):
    return lib.pt_variance_denoise(C.byref(p) if p is not None else None, color, variance, albedo, normal, depth, out, variance_out, scratch, None)


BAD_PARAMS = [dict(struct_size=0), dict(struct_size=36), dict(struct_size=44), dict(width=0), dict(width=-3), dict(height=0), dict(height=-1),
              dict(iterations=0), dict(iterations=-1), dict(iterations=9),
              dict(sigma_variance=math.nan), dict(sigma_variance=math.inf), dict(sigma_normal=math.nan), dict(sigma_normal=-math.inf),
              dict(sigma_depth=math.inf), dict(sigma_depth=math.nan), dict(sigma_albedo=math.nan), dict(sigma_albedo=math.inf),
              dict(sigma_variance=1e-30), dict(sigma_variance=1e-20), dict(sigma_variance=1e30),  # sv2 is 0, 1 / sv2 is inf, sv2 is inf
              dict(sigma_normal=1e30), dict(sigma_albedo=1e-30), dict(sigma_depth=1e-30),           # k is 0 or inf, sd2 is 0
              dict(flags=4), dict(flags=5), dict(flags=1 << 31)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_refuses_bad_params_before_touching_a_device(lib, bad):
    assert call(lib, params(**bad)) == abi.PT_ERR_INVALID_ARG
    assert b"pt_variance_denoise" in lib.pt_last_error()


def test_refuses_null_arguments(lib):
    assert call(lib, None) == abi.PT_ERR_INVALID_ARG
    for name in ("color", "variance", "out", "scratch"):
        assert call(lib, params(), **{name: None}) == abi.PT_ERR_INVALID_ARG, name
    assert call(lib, params(), albedo=None) == abi.PT_ERR_INVALID_ARG  # demodulation without an albedo plane
    out = (C.c_int32 * 8)(*([7] * 8))
    assert lib.pt_debug_last_variance_denoise(None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_debug_last_variance_denoise(out) == abi.PT_OK and set(out) <= {0, 1, 2}
    # the estimate: NULL accumulator, before any device call
    assert lib.pt_variance_estimate(None, VOUT, None) == abi.PT_ERR_INVALID_ARG
    assert b"pt_variance_estimate" in lib.pt_last_error()


def test_refuses_overlapping_buffers(lib):
    floats3, scratch_floats = PX * 3, lib.pt_variance_denoise_scratch_floats(W, H)
    for guide, size in (("albedo", floats3), ("normal", floats3), ("depth", PX)):
        base = {"albedo": ALBEDO, "normal": NORMAL, "depth": DEPTH}[guide]
        for target in ("out", "variance_out"):
            assert call(lib, params(), **{target: base}) == abi.PT_ERR_INVALID_ARG, (guide, target)
            assert call(lib, params(), **{target: base + 4 * (size - 1)}) == abi.PT_ERR_INVALID_ARG, (guide, target)      # the guide's last float
            assert call(lib, params(), **{target: base - 4 * (floats3 - 1)}) == abi.PT_ERR_INVALID_ARG, (guide, target)   # the target's last float
        assert call(lib, params(), scratch=base) == abi.PT_ERR_INVALID_ARG, guide
        assert call(lib, params(), scratch=base - 4 * (scratch_floats - 4)) == abi.PT_ERR_INVALID_ARG, guide
    for frame in (COLOR, VAR, OUT, VOUT):
        assert call(lib, params(), scratch=frame) == abi.PT_ERR_INVALID_ARG
        assert call(lib, params(), scratch=frame + 16) == abi.PT_ERR_INVALID_ARG
    assert call(lib, params(), scratch=SCRATCH + 4) == abi.PT_ERR_INVALID_ARG  # not 16-byte aligned
    assert call(lib, params(), variance_out=COLOR) == abi.PT_ERR_INVALID_ARG
    assert call(lib, params(), variance_out=OUT) == abi.PT_ERR_INVALID_ARG
    assert call(lib, params(), variance_out=OUT + 4 * (floats3 - 1)) == abi.PT_ERR_INVALID_ARG
    assert call(lib, params(), out=COLOR, variance_out=COLOR) == abi.PT_ERR_INVALID_ARG
    assert call(lib, params(width=1 << 16, height=1 << 15)) == abi.PT_ERR_TOO_LARGE  # 2^31 pixels


# ---- hosts --------------------------------------------------------------------------------------------------------------------------

def test_variance_denoise_main_compiles_against_the_facade(tmp_path, lib):
    out = tmp_path / "variance_denoise_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{libdir / 'include'}", str(ROOT / "tests" / "cpp" / "variance_denoise_main.cpp"), "-o", str(out), f"-L{libdir}",
                    "-lpt_render", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert out.exists()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "path_tracer_amd", *args], capture_output=True, text=True, cwd=ROOT,
                          env=dict(os.environ), timeout=120)


def test_cli_has_the_options():
    p = _cli("--help")
    assert p.returncode == 0, p.stderr
    for opt in ("--denoise-variance", "--denoise-sigma-variance"):
        assert opt in p.stdout, opt


ADAPTIVE = ["--noise-threshold", "0.05", "--spp", "32"]


@pytest.mark.parametrize("args,message", [(["--denoise-variance", "--denoise-out", "d.png"], "--denoise-variance needs --noise-threshold"),
                                          (["--denoise-variance", *ADAPTIVE], "--denoise-variance needs --denoise-out"),
                                          (["--denoise-sigma-variance", "3", "--denoise-out", "d.png", *ADAPTIVE],
                                           "--denoise-sigma-variance needs --denoise-variance"),
                                          (["--denoise-variance", "--denoise-out", "d.png", "--denoise-sigma-color", "2", *ADAPTIVE],
                                           "--denoise-sigma-color does not apply to --denoise-variance"),
                                          (["--denoise-variance", "--denoise-out", "d.png", "--denoise-sigma-variance", "nan", *ADAPTIVE],
                                           "--denoise-sigma-* must be finite"),
                                          (["--denoise-variance", "--denoise-out", "d.png", "--denoise-iterations", "9", *ADAPTIVE],
                                           "--denoise-iterations must be in 1 .. 8")])
def test_cli_rejects_inconsistent_options_without_a_gpu(args, message):
    p = _cli(*args)
    assert p.returncode == 2, (p.returncode, p.stdout, p.stderr)
    assert message in p.stderr, p.stderr
    assert "torch" not in p.stderr


# ---- the model: the estimate ---------------------------------------------------------------------------------------------------------

def test_estimate_definition():
    S_ = np.array([[8.0, 4.0, 2.0], [8.0, 4.0, 2.0], [8.0, 4.0, 2.0], [8.0, 4.0, 2.0], [7.0, 1.0, 0.5]], F)
    H_ = np.array([[5.0, 2.0, 0.5], [0.0, 0.0, 0.0], [8.0, 4.0, 2.0], [3.0, 1.0, 0.25], [2.0, 0.25, 0.5]], F)
    n = np.array([8, 8, 8, 8, 7], np.int32)
    a = np.array([4, 0, 8, 4, 3], np.int32)
    v = V.estimate(S_, H_, n, a)
    assert v.dtype == F and v.shape == (5, 3)
    assert np.isposinf(v[1]).all() and np.isposinf(v[2]).all()  # a == 0, a == n: no estimate yet
    # equal halves: ((A - B) / 2)^2 — exact here, every value is a small dyadic number
    for row in (0, 3):
        A, B = H_[row] / F(4), (S_[row] - H_[row]) / F(4)
        assert_bit_identical(v[row], ((A - B) / F(2)) ** 2, f"equal halves, row {row}")
    # unequal halves, the header's operations one by one: a = 3, b = 4, n = 7
    A, B = H_[4] / F(3), (S_[4] - H_[4]) / F(4)
    d = A - B
    f = (F(3) * F(4)) / (F(7) * F(7))
    assert_bit_identical(v[4], (d * d) * f, "unequal halves")
    assert abs(float(v[4, 0]) - (2 / 3 - 5 / 4) ** 2 * 12 / 49) < 1e-7
    # where the halves agree the estimate is +0
    assert_bit_identical(V.estimate(np.array([[4.0, 2.0, 0.0]], F), np.array([[2.0, 1.0, 0.0]], F), [4], [2]), np.zeros((1, 3), F), "halves agree")
    # the estimate tracks the variance of the mean: n samples of variance 1, split evenly -> E[var] = 1 / n
    r = np.random.default_rng(7)
    x = r.standard_normal((4000, 16, 3)).astype(F)
    est = V.estimate(x.sum(1), x[:, :8].sum(1), np.full(4000, 16), np.full(4000, 8))
    assert abs(float(est.mean()) * 16 - 1.0) < 0.1


# ---- the model: properties -----------------------------------------------------------------------------------------------------------

def synthetic(w, h, seed):
    r = np.random.default_rng(seed)
    return dict(color=r.random((h, w, 3), dtype=F) * 2, variance=r.random((h, w, 3), dtype=F) * F(0.05), albedo=r.random((h, w, 3), dtype=F),
                normal=r.standard_normal((h, w, 3), dtype=F), depth=r.random((h, w), dtype=F) * 5 + 1)


def test_uniform_variance_is_a_constant_sigma_color(monkeypatch):
    """One iteration, variance V everywhere, sigma_variance = s: vbar = V (an exact prefilter: the weights and their sums are dyadic and V
    is a power of two, at the frame's edges too), so iv = k = 1 / (s^2 V + 1e-8) in every channel.  On a frame whose g and b channels
    are constant, x_c = ((dr dr) k + 0) + 0 here and ((dr dr + 0) + 0) k in pt_denoise's model with k_c = k: the same bits.  The model of
    pt_denoise is given that k_c directly (its _k is what turns sigma_color into k_c; no other term that uses it is on)."""
    w, h = 19, 13
    g = synthetic(w, h, 11)
    color = g["color"].copy()
    color[..., 1:] = F(0.5)
    Vv, s = F(2.0 ** -6), 2.0
    k = F(1.0) / ((F(s) * F(s)) * Vv + F(1e-8))
    assert_bit_identical(V.prefilter(np.full((h, w, 3), Vv, F)), np.full((h, w, 3), Vv, F), "the prefilter of a constant")
    kw = dict(depth=g["depth"], iterations=1, sigma_depth=0.5, demodulate=False)
    monkeypatch.setattr(M, "_k", lambda sigma: k)
    want = M.denoise(color, sigma_color=1.0, **kw)
    monkeypatch.undo()
    got, vout = V.denoise(color, np.full((h, w, 3), Vv, F), sigma_variance=s, **kw)
    assert_bit_identical(got, want, "uniform variance against a constant k_c")
    assert np.abs(got - color).max() > 0.01  # the colour term is not so tight that nothing happens
    assert (vout > 0).all() and (vout < Vv).all()  # a weighted mean of several taps has less variance than one of them


def test_variance_out_of_a_constant_weight_region():
    """Colour constant, no guides: every tap has x = 0 and w = h, so v' = sum(h^2 v) / (sum h)^2 over the taps in the frame — for an
    interior pixel of a uniform-variance frame, V sum(h^2) / 1 with sum(h^2) = (sum K^2)^2 = (70 / 256)^2."""
    w, h = 9, 7
    color = np.full((h, w, 3), 0.25, F)
    var = synthetic(w, h, 12)["variance"]
    out, vout = V.denoise(color, var, iterations=1, sigma_variance=2.0, demodulate=False)
    assert_bit_identical(out, color, "a constant frame stays constant: sum = 0.25 wsum exactly (wsum is dyadic)")
    K = np.array([float(k) for k in M.KERNEL])
    for (x, y) in [(4, 3), (0, 0), (8, 6), (1, 5)]:
        num, den = np.zeros(3), 0.0
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qx, qy = x + dx, y + dy
                if 0 <= qx < w and 0 <= qy < h:
                    hh = K[dy + 2] * K[dx + 2]
                    num += hh * hh * var[qy, qx].astype(np.float64)
                    den += hh
        np.testing.assert_allclose(vout[y, x], num / (den * den), rtol=2e-6)
    flat, vflat = V.denoise(color, np.full((h, w, 3), 0.5, F), iterations=1, sigma_variance=2.0, demodulate=False)
    assert_bit_identical(vflat[3, 4], np.full(3, 0.5 * (70 / 256) ** 2, F), "interior pixel, uniform variance: exact")


def test_zero_bleeding_across_a_normal_edge():
    """Two half-planes with orthogonal normals, sigma_normal = 0.1: x_n = 2 / 0.01 = 200 >= 80, so no tap crosses the edge and no colour
    is ever averaged across it.  The 3 x 3 prefilter is not edge-aware (the header says so): it carries VARIANCE, hence tolerance,
    one pixel across per level.  So: guide-only (no prefilter), nothing at all crosses, bit for bit; with the colour term on, one level
    (whose prefilter reads only v_0) leaves the left half's bits unchanged when the right half's colours change, and after five levels
    every left pixel is still a mean of left colours only, though the right half is 100 times brighter."""
    w, h = 24, 10
    g = synthetic(w, h, 1)
    normal = np.zeros((h, w, 3), F)
    normal[:, :12] = (1, 0, 0)
    normal[:, 12:] = (0, 1, 0)
    other = g["color"].copy()
    other[:, 12:] = synthetic(w, h, 2)["color"][:, 12:] * 100 + 50
    ovar = g["variance"].copy()
    ovar[:, 12:] = 7.0
    # guide-only: colours and variances of the right half changed, five levels
    kw = dict(normal=normal, iterations=5, sigma_variance=0.0, sigma_normal=0.1, demodulate=False)
    a, va = V.denoise(g["color"], g["variance"], **kw)
    b, vb = V.denoise(other, ovar, **kw)
    assert_bit_identical(a[:, :12], b[:, :12], "guide-only: left half")
    assert_bit_identical(va[:, :12], vb[:, :12], "guide-only: left half's variance")
    assert not np.array_equal(a[:, 12:], b[:, 12:])
    assert np.abs(a[:, :12] - g["color"][:, :12]).max() > 0.1  # the filter did work on each side
    # the colour term on, one level: the right half's colours changed
    kw = dict(normal=normal, iterations=1, sigma_variance=1e3, sigma_normal=0.1, demodulate=False)
    a, va = V.denoise(g["color"], g["variance"], **kw)
    b, vb = V.denoise(other, g["variance"], **kw)
    assert_bit_identical(a[:, :12], b[:, :12], "one level: left half, right half's colours changed")
    assert_bit_identical(va[:, :12], vb[:, :12], "one level: left half's variance")
    # five levels: every left pixel stays inside the range of the left half's colours (a mean of left pixels; one ulp per level of slack)
    b, _ = V.denoise(other, ovar, **dict(kw, iterations=5))
    lo, hi = g["color"][:, :12].min(axis=(0, 1)), g["color"][:, :12].max(axis=(0, 1))
    assert (b[:, :12] >= lo - 1e-5).all() and (b[:, :12] <= hi + 1e-5).all(), "the right half's colours reached the left"
    assert b[:, 12:].min() > 40
    # without the normal term the edge leaks
    c, _ = V.denoise(other, ovar, iterations=5, sigma_variance=1e3, demodulate=False)
    assert c[:, :12].max() > hi.max() + 1


@pytest.mark.parametrize("demodulate", [False, True])
def test_nan_and_inf_colours_are_contained(demodulate):
    w, h = 19, 13
    g = synthetic(w, h, 3)
    g["color"][5, 7] = np.nan
    g["color"][9, 2, 1] = np.inf
    g["color"][0, 18] = -np.inf
    out, vout = V.denoise(demodulate=demodulate, **g)
    bad = np.zeros((h, w), bool)
    bad[5, 7] = bad[9, 2] = bad[0, 18] = True
    assert np.isfinite(out[~bad]).all() and np.isfinite(vout).all(), "a non-finite pixel spread"
    assert np.isnan(out[5, 7]).all() and out[9, 2, 1] == np.inf and (out[0, 18] == -np.inf).all()
    if not demodulate:
        assert_bit_identical(out[bad], g["color"][bad], "the non-finite pixels come out as they went in")
        assert_bit_identical(vout[bad], g["variance"][bad], "and keep their variance")
    g2 = {k: v.copy() for k, v in g.items()}
    g2["color"][bad] = np.nan
    out2, vout2 = V.denoise(demodulate=demodulate, **g2)
    assert_bit_identical(out2[~bad], out[~bad], "finite pixels")
    assert_bit_identical(vout2, vout, "variance")


def test_bad_variance_is_sanitised_to_zero():
    w, h = 19, 13
    g = synthetic(w, h, 5)
    dirty = g["variance"].copy()
    spots = [(2, 3, 0), (2, 3, 1), (7, 11, 2), (12, 18, 0), (0, 0, 1)]
    for (y, x, ch), bad in zip(spots, (-1.0, np.nan, np.inf, -np.inf, -1e-30)):
        dirty[y, x, ch] = bad
    clean = dirty.copy()
    for y, x, ch in spots:
        clean[y, x, ch] = 0.0
    a, va = V.denoise(**dict(g, variance=dirty))
    b, vb = V.denoise(**dict(g, variance=clean))
    assert_bit_identical(a, b, "sanitised variance: colour")
    assert_bit_identical(va, vb, "sanitised variance: variance")
    assert np.isfinite(a).all() and np.isfinite(va).all() and (va >= 0).all()
    assert_bit_identical(V.sanitise(np.array([-1.0, np.nan, np.inf, -np.inf, 0.0, 3e38, 1e-45], F)), np.array([0, 0, 0, 0, 0, 3e38, 1e-45], F), "sanitise")


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2)])
def test_frames_smaller_than_the_filter(w, h):
    g = synthetic(w, h, 4)
    kw = dict(g, demodulate=False)
    out, vout = V.denoise(iterations=5, **kw)
    assert out.shape == vout.shape == (h, w, 3) and np.isfinite(out).all() and np.isfinite(vout).all()
    if (w, h) == (1, 1):
        # only the centre tap, the prefilter's too: c' = (w c) / w, v' = (w w v) / (w w) with w = 9/64 — within an ulp, five times
        assert np.abs(out - g["color"]).max() <= 8 * np.spacing(g["color"].max())
        assert np.abs(vout - g["variance"]).max() <= 16 * np.spacing(g["variance"].max())
    else:
        two = V.denoise(iterations=2, **kw)  # steps 1, 2: from step 4 on every off-centre tap is outside the frame
        assert np.abs(out - two[0]).max() <= 4 * np.spacing(np.abs(two[0]).max())
    flat = np.full((h, w, 3), 0.75, F)
    assert np.abs(V.denoise(flat, g["variance"], iterations=5, demodulate=False)[0] - flat).max() <= 5 * np.spacing(F(0.75))


def test_terms_switch_off():
    g = synthetic(19, 13, 5)
    base = V.denoise(g["color"], g["variance"], iterations=2, sigma_variance=1.5, demodulate=False)
    off = V.denoise(sigma_normal=0.0, sigma_depth=-1.0, sigma_albedo=0.0, iterations=2, sigma_variance=1.5, demodulate=False, **g)
    assert_bit_identical(base[0], off[0], "a sigma <= 0 is a NULL plane")
    assert_bit_identical(base[1], off[1], "a sigma <= 0 is a NULL plane: variance")
    on = V.denoise(iterations=2, sigma_variance=1.5, sigma_albedo=0.3, demodulate=False, **g)
    assert not np.array_equal(on[0], base[0])
    # the colour term off: the variance plays no part in the weights, it is only propagated
    a = V.denoise(iterations=2, sigma_variance=0.0, **g)
    b = V.denoise(iterations=2, sigma_variance=-1.0, **dict(g, variance=g["variance"] * F(4)))
    assert_bit_identical(a[0], b[0], "guide-only: the colour does not depend on the variance")
    assert_bit_identical(a[1] * F(4), b[1], "guide-only: the variance is propagated linearly (a power of two: exactly)")


# ---- quality --------------------------------------------------------------------------------------------------------------------------

REFERENCE_SPP = 4096
SWEEP = (2.0, 3.0, 4.0)
# measured once (this test prints the table; profiles/variance_denoise_bench.txt records it): MSE(filtered) / MSE(noisy) against the
# 4096 spp frame, for the 8, 32 and 128 spp frames
RECORDED = {2.0: (0.6387, 0.6872, 0.7529), 3.0: (0.4167, 0.5266, 0.7865), 4.0: (0.3269, 0.4704, 0.9413)}
RECORDED_PLAIN = (0.3073, 0.6282, 2.6465)  # pt_denoise's model with its DEFAULTS on the same inputs


def test_default_sigma_variance_improves_8_32_and_128_spp_frames(orc):
    """The oracle renders the small Cornell scene at 64 x 40: the reference at 4096 spp, and for n = 8, 32, 128 the noisy frame as two
    windows of n / 2 (the sums are mean x count, exact for these powers of two), bookkept with book_np into (H, n, a); the model's
    estimator gives the variance, aov_np the guides at 6 spp.  r_n = MSE(filtered) / MSE(noisy).  The default sigma_variance is the one
    of {2, 3, 4} with the smallest max_n r_n; with it r_n < min(1, 1.5 x the recorded r_n) at every n — the run is deterministic, the
    margin is the project's convention — while pt_denoise's defaults leave the 128 spp frame worse than they found it (r_128 > 1):
    the gap this filter closes."""
    w, h = 64, 40
    ps, cam = S.ALL["cornell"]()
    c = scenes.make_camera(cam, w, h)
    orc.set_math(True)
    clean = orc.render(ps, c.c, w, h, REFERENCE_SPP)
    g = aov_np(orc, ps, c.c, w, h, 6)
    guides = dict(albedo=g["albedo"], normal=g["normal"], depth=g["depth"])

    def mse(a, b):
        return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))

    r = {sv: [] for sv in SWEEP}
    plain = []
    for n in (8, 32, 128):
        half = orc.render(ps, c.c, w, h, n // 2) * F(n // 2)
        noisy = orc.render(ps, c.c, w, h, n)
        full = noisy * F(n)
        Hh, cn, ca = np.zeros((h, w, 3), F), np.zeros((h, w), np.int32), np.zeros((h, w), np.int32)
        Hh, cn, ca = book_np(np.zeros_like(half), half, Hh, cn, ca, n // 2)
        Hh, cn, ca = book_np(half, full, Hh, cn, ca, n // 2)
        assert (cn == n).all() and (ca == n // 2).all()
        var = V.estimate(full, Hh, cn, ca)
        base = mse(noisy, clean)
        plain.append(mse(M.denoise(noisy, **guides, **M.DEFAULTS), clean) / base)
        for sv in SWEEP:
            out, _ = V.denoise(noisy, var, **guides, **dict(V.DEFAULTS, sigma_variance=sv))
            r[sv].append(mse(out, clean) / base)
    print(f"reference {REFERENCE_SPP} spp; r_8, r_32, r_128:")
    print("  pt_denoise defaults   " + "  ".join(f"{x:.4f}" for x in plain))
    for sv in SWEEP:
        print(f"  sigma_variance = {sv:g}    " + "  ".join(f"{x:.4f}" for x in r[sv]) + f"    max {max(r[sv]):.4f}")
    best = min(SWEEP, key=lambda sv: max(r[sv]))
    assert best == V.DEFAULTS["sigma_variance"] == abi.PT_VDENOISE_DEFAULT_SIGMA_VARIANCE
    for got, rec in zip(r[best], RECORDED[best]):
        assert got < min(1.0, 1.5 * rec), (got, rec)
    assert plain[2] > 1.0, plain
