"""CPU tests of the spatial variance estimate's boundary and definition (include/pt_spatial_variance.h: pt_spatial_variance).  The new
header is held to the rules include/pt_render.h is held to by tests/test_abi_cpu.py and tests/test_stream_contract_cpu.py, as
tests/test_firefly_cpu.py holds pt_post.h: abi.SPATIAL_VARIANCE_SIGNATURES is exactly what it declares, the library exports all of it, and
every prototype with a `void* stream` has a row in the contract table below and a comment that says what the row says.  The struct and
the defaults are the header's, invalid calls are refused on the host before a device is touched, the CLI option parses, and the numpy
restatement of the header (tests/spatial_variance_model.py, the one tests/test_gpu_spatial_variance.py holds the kernel to) has the
properties the header promises.  The last test is the quality record DESIGN.md and profiles/spatial_variance_bench.txt quote."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import scenes_small as S
import spatial_variance_model as SV
import variance_model as V
from path_tracer_amd import abi, scenes
from test_aov_cpu import aov_np
from test_variance_denoise_cpu import REFERENCE_SPP

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "pt_spatial_variance.h"
OTHER_HEADERS = [ROOT / "include" / "pt_render.h", ROOT / "include" / "pt_post.h"]
F = np.float32
INF = F(np.inf)

# The stream contract of include/pt_spatial_variance.h, one row per prototype with a `void* stream` parameter (tests/stream_contract.py:
# CONTRACT is pt_render.h's): "async" — the call is asynchronous on `stream` —, or "sync" — it synchronises `stream`.
SPATIAL_VARIANCE_CONTRACT = {
    "pt_spatial_variance": "async",
}
ASYNC = re.compile(r"asynchronous on `stream`", re.I)
SYNC = re.compile(r"\bsynchronis\w* `stream`", re.I)
PROTO = re.compile(r"^(?:extern\s+)?(int|void|int32_t|int64_t|uint32_t|const char\*)\s+(pt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", re.M)


def header_code(path=HEADER):
    """The header with its comments blanked in place (offsets stay the file's)."""
    return re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), path.read_text(), flags=re.S)


def prototypes(path=HEADER):
    """{name: (return type, [parameter declarations], offset)}"""
    return {m.group(2): (m.group(1), [re.sub(r"\s+", " ", a.strip()) for a in m.group(3).split(",")], m.start())
            for m in PROTO.finditer(header_code(path))}


# ---- the boundary -------------------------------------------------------------------------------------------------------------------

def ctype_of(decl):
    """The ctypes type abi.py gives a parameter declared as `decl`: pointers to device memory and streams are void pointers."""
    if re.fullmatch(r"(const )?PtSpatialVarianceParams\* \w+", decl):
        return C.POINTER(abi.PtSpatialVarianceParams)
    if re.fullmatch(r"int32_t \w+\[\d+\]", decl):
        return C.POINTER(C.c_int32)
    if re.fullmatch(r"(const )?(float|uint32_t|int32_t|void)\* \w+", decl):
        return C.c_void_p
    if re.fullmatch(r"int32_t \w+", decl):
        return C.c_int32
    raise AssertionError(f"no rule for the parameter {decl!r}")


def test_signatures_are_exactly_what_the_header_declares(lib):
    protos = prototypes()
    table = abi.SPATIAL_VARIANCE_SIGNATURES
    assert set(protos) == set(table) == set(abi.SPATIAL_VARIANCE_SYMBOLS), sorted(set(protos) ^ set(table))
    ret = {"int": C.c_int, "void": None, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "const char*": C.c_char_p}
    for name, (rtype, args, _) in protos.items():
        assert table[name] == (ret[rtype], [ctype_of(a) for a in args]), name
        assert hasattr(lib, name), f"libpt_render.so does not export {name}"
        fn = getattr(lib, name)
        assert fn.restype == table[name][0] and list(fn.argtypes) == table[name][1], name  # load_library applied the row
    assert abi.has_spatial_variance(lib)
    assert protos["pt_spatial_variance"][:2] == ("int", ["const PtSpatialVarianceParams* params", "const float* color", "const float* albedo",
                                                         "const float* normal", "const float* depth", "const int32_t* id",
                                                         "const float* variance_in", "float* variance_out", "uint32_t* counts", "void* stream"])
    assert protos["pt_spatial_variance_params_init"][:2] == ("void", ["PtSpatialVarianceParams* params", "int32_t width", "int32_t height"])
    assert protos["pt_debug_last_spatial_variance"][:2] == ("int", ["int32_t out[4]"])


def test_the_tables_and_the_headers_are_disjoint(lib):
    assert not set(abi.SPATIAL_VARIANCE_SIGNATURES) & (set(abi.SIGNATURES) | set(abi.POST_SIGNATURES))
    for other in OTHER_HEADERS:
        assert not set(prototypes()) & set(prototypes(other)), other
        assert "spatial_variance" not in other.read_text().lower(), other  # the older headers know nothing of the stage
    assert '#include "pt_render.h"' in HEADER.read_text()  # the error codes and pt_last_error are its
    assert lib.pt_abi_version() == 2                        # detected by the symbols, not by a version


def test_struct_matches_the_header():
    body = re.search(r"typedef struct PtSpatialVarianceParams\s*\{(.*?)\}\s*PtSpatialVarianceParams;", header_code(), re.S).group(1)
    fields = []
    ctypes_of = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = re.match(r"(int32_t|uint32_t|float)\s+(.*)", decl).groups()
            for nm in names.split(","):
                arr = re.fullmatch(r"(\w+)\[(\d+)\]", nm.strip())
                fields.append((arr.group(1), ctypes_of[ctype] * int(arr.group(2))) if arr else (nm.strip(), ctypes_of[ctype]))
    assert [n for n, _ in fields] == ["struct_size", "width", "height", "radius", "min_pairs", "tol_depth", "tol_normal", "flags", "reserved"]
    assert abi.PtSpatialVarianceParams._fields_ == fields
    assert C.sizeof(abi.PtSpatialVarianceParams) == 40


def test_defaults_are_the_headers(lib):
    text = HEADER.read_text()
    m = dict(re.findall(r"^#define (PT_SVAR_\w+) (\S+)", text, re.M))
    p = abi.PtSpatialVarianceParams(*([7] * 8))
    lib.pt_spatial_variance_params_init(C.byref(p), 64, 40)
    assert (p.struct_size, p.width, p.height, list(p.reserved)) == (C.sizeof(abi.PtSpatialVarianceParams), 64, 40, [0, 0])
    assert int(m["PT_SVAR_DEMODULATE"].rstrip("u")) == abi.PT_SVAR_DEMODULATE == SV.DEMODULATE == 1
    assert int(m["PT_SVAR_NO_LDS"].rstrip("u")) == abi.PT_SVAR_NO_LDS == SV.NO_LDS == 2
    assert int(m["PT_SVAR_MAX_RADIUS"]) == abi.PT_SVAR_MAX_RADIUS == SV.MAX_RADIUS == 3
    assert p.radius == int(m["PT_SVAR_DEFAULT_RADIUS"]) == abi.PT_SVAR_DEFAULT_RADIUS == SV.DEFAULTS["radius"]
    assert p.min_pairs == int(m["PT_SVAR_DEFAULT_MIN_PAIRS"]) == abi.PT_SVAR_DEFAULT_MIN_PAIRS == SV.DEFAULTS["min_pairs"]
    assert F(p.tol_depth) == F(m["PT_SVAR_DEFAULT_TOL_DEPTH"].rstrip("f")) == F(abi.PT_SVAR_DEFAULT_TOL_DEPTH) == F(SV.DEFAULTS["tol_depth"])
    assert F(p.tol_normal) == F(m["PT_SVAR_DEFAULT_TOL_NORMAL"].rstrip("f")) == F(abi.PT_SVAR_DEFAULT_TOL_NORMAL) == F(SV.DEFAULTS["tol_normal"])
    # pt_temporal_push's tolerances
    assert (F(p.tol_depth), F(p.tol_normal)) == (F(abi.PT_TEMPORAL_DEFAULT_TOL_DEPTH), F(abi.PT_TEMPORAL_DEFAULT_TOL_NORMAL))
    assert m["PT_SVAR_DEFAULT_FLAGS"] == "PT_SVAR_DEMODULATE" and p.flags == abi.PT_SVAR_DEFAULT_FLAGS == abi.PT_SVAR_DEMODULATE
    assert SV.DEFAULTS["demodulate"] is True
    assert (int(m["PT_SVAR_TILE_W"]), int(m["PT_SVAR_TILE_H"])) == (abi.PT_SVAR_TILE_W, abi.PT_SVAR_TILE_H) == (32, 8)
    lib.pt_spatial_variance_params_init(None, 1, 1)  # a NULL struct is ignored
    assert "m(q).ch  = DEMODULATE ? albedo(q).ch + 1e-3f : 1" in text  # the constant of the definition, as the model has it


# Pointers that are never dereferenced: every call below is refused on the host before a plane is read.
COLOR, ALBEDO, NORMAL, DEPTH, ID, VIN, VOUT, COUNTS = (0x10000000 + i * 0x10000000 for i in range(8))
W, H = 64, 40
FRAME, PLANE = W * H * 12, W * H * 4


def params(lib, **over):
    p = abi.PtSpatialVarianceParams()
    lib.pt_spatial_variance_params_init(C.byref(p), W, H)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def call(lib, p, color=COLOR, albedo=ALBEDO, normal=NORMAL, depth=DEPTH, id=ID, variance_in=VIN, variance_out=VOUT, counts=COUNTS):
    return lib.pt_spatial_variance(C.byref(p) if p is not None else None, color, albedo, normal, depth, id, variance_in, variance_out, counts, None)


BAD_PARAMS = [dict(struct_size=0), dict(struct_size=36), dict(struct_size=44), dict(width=0), dict(height=0), dict(width=-1), dict(height=-3),
              dict(radius=0), dict(radius=4), dict(radius=-1), dict(min_pairs=0), dict(min_pairs=-5),
              dict(tol_depth=0.0), dict(tol_depth=-1.0), dict(tol_depth=math.nan), dict(tol_depth=math.inf),
              dict(tol_normal=0.0), dict(tol_normal=-0.5), dict(tol_normal=math.nan), dict(tol_normal=-math.inf),
              dict(flags=4), dict(flags=7), dict(flags=1 << 31)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_refuses_bad_params_before_touching_a_device(lib, bad):
    assert call(lib, params(lib, **bad)) == abi.PT_ERR_INVALID_ARG
    assert b"pt_spatial_variance" in lib.pt_last_error()


def test_refuses_null_arguments_demodulation_without_albedo_and_too_many_pixels(lib):
    good = params(lib)
    assert call(lib, None) == abi.PT_ERR_INVALID_ARG
    assert call(lib, good, color=None) == abi.PT_ERR_INVALID_ARG
    assert call(lib, good, variance_out=None) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.pt_last_error()
    assert good.flags & abi.PT_SVAR_DEMODULATE
    assert call(lib, good, albedo=None) == abi.PT_ERR_INVALID_ARG and b"PT_SVAR_DEMODULATE needs albedo" in lib.pt_last_error()
    assert call(lib, params(lib, width=1 << 16, height=(1 << 14) + 1)) == abi.PT_ERR_TOO_LARGE and b"2^30" in lib.pt_last_error()
    assert call(lib, params(lib, width=1 << 16, height=1 << 15)) == abi.PT_ERR_TOO_LARGE
    assert lib.pt_debug_last_spatial_variance(None) == abi.PT_ERR_INVALID_ARG and b"pt_debug_last_spatial_variance" in lib.pt_last_error()
    last = (C.c_int32 * 4)(9, 9, 9, 9)
    assert lib.pt_debug_last_spatial_variance(last) == abi.PT_OK and 9 not in list(last)


def test_refuses_overlapping_planes(lib):
    good = params(lib)
    bad = abi.PT_ERR_INVALID_ARG
    assert call(lib, good, variance_out=COLOR) == bad and b"overlap" in lib.pt_last_error()
    assert call(lib, good, variance_out=COLOR + FRAME - 1) == bad     # the last byte of color
    assert call(lib, good, variance_out=COLOR - FRAME + 1) == bad     # its first
    assert call(lib, good, variance_out=ALBEDO + 12) == bad
    assert call(lib, good, variance_out=NORMAL - 12) == bad
    assert call(lib, good, variance_out=DEPTH + PLANE - 4) == bad     # the last value of depth
    assert call(lib, good, variance_out=ID - FRAME + 4) == bad        # the first of id
    assert call(lib, good, variance_out=VIN + 12) == bad              # overlapping variance_in without being it
    assert call(lib, good, variance_out=VIN - FRAME + 4) == bad
    for plane, size in ((COLOR, FRAME), (ALBEDO, FRAME), (NORMAL, FRAME), (DEPTH, PLANE), (ID, PLANE), (VIN, FRAME)):
        assert call(lib, good, counts=plane + 8) == bad, hex(plane)
        assert call(lib, good, counts=plane + size - 8) == bad, hex(plane)  # its last eight bytes
    assert call(lib, good, counts=COLOR - 8 + 4) == bad              # its second word is color's first (and it is not aligned)
    assert call(lib, good, counts=VOUT + 16) == bad and b"one another" in lib.pt_last_error()
    assert call(lib, good, variance_out=VIN, counts=VIN + 8) == bad   # in place: counts still may not lie in the plane
    assert call(lib, good, counts=COUNTS + 4) == bad and b"aligned" in lib.pt_last_error()


# ---- the stream contract of pt_spatial_variance.h: tests/test_stream_contract_cpu.py's rule --------------------------------------------

def test_every_stream_prototype_has_a_row_and_a_comment_that_states_it():
    text = HEADER.read_text()
    with_stream = {n: at for n, (_, args, at) in prototypes().items() if any(re.fullmatch(r"void\s*\*\s*stream", a) for a in args)}
    assert set(with_stream) == set(SPATIAL_VARIANCE_CONTRACT), sorted(set(with_stream) ^ set(SPATIAL_VARIANCE_CONTRACT))
    assert set(SPATIAL_VARIANCE_CONTRACT.values()) <= {"async", "sync"}
    for name, want in SPATIAL_VARIANCE_CONTRACT.items():
        comments = list(re.finditer(r"/\*(?:(?!\*/).)*\*/", text[:with_stream[name]], re.S))
        assert comments and text[comments[-1].end():with_stream[name]].strip() == "", f"{name}: no comment directly above its prototype"
        own = re.sub(r"\s+", " ", re.sub(r"^\s*\*", " ", comments[-1].group(0), flags=re.M))
        assert (bool(ASYNC.search(own)), bool(SYNC.search(own))) == (want == "async", want == "sync"), f"{name}: the table says {want}, its comment: {own}"
        assert abi.SPATIAL_VARIANCE_SIGNATURES[name][1][-1] is C.c_void_p, name  # abi.py passes it a stream


# ---- hosts --------------------------------------------------------------------------------------------------------------------------

def test_spatial_variance_main_compiles_against_the_facade(tmp_path, lib):
    out = tmp_path / "spatial_variance_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{libdir / 'include'}", str(ROOT / "tests" / "cpp" / "spatial_variance_main.cpp"), "-o", str(out), f"-L{libdir}",
                    "-lpt_render", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert out.exists()


def test_python_host_has_the_stage_and_its_keywords():
    import inspect

    from path_tracer_amd import render as R
    sig = inspect.signature(R.spatial_variance)
    assert list(sig.parameters)[:2] == ["fb", "variance"]
    for name in ("albedo", "normal", "depth", "id", "radius", "min_pairs", "tol_depth", "tol_normal", "demodulate", "no_lds", "out", "counts"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert (sig.parameters["radius"].default, sig.parameters["min_pairs"].default) == (abi.PT_SVAR_DEFAULT_RADIUS, abi.PT_SVAR_DEFAULT_MIN_PAIRS)
    assert inspect.signature(R.Accumulator.denoise_variance).parameters["spatial"].default is None
    assert inspect.signature(R.render_temporal).parameters["spatial_variance"].default is None


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "path_tracer_amd", *args], capture_output=True, text=True, cwd=ROOT,
                          env=dict(os.environ), timeout=120)


def test_cli_has_the_option():
    p = _cli("--help")
    assert p.returncode == 0, p.stderr
    assert "--spatial-variance [RADIUS]" in p.stdout


NEEDS_THRESHOLD = "--denoise-variance needs --noise-threshold"


@pytest.mark.parametrize("args,message", [(["--spatial-variance"], "--spatial-variance needs --denoise-variance"),
                                          (["--spatial-variance", "2", "--denoise-out", "d.png"], "--spatial-variance needs --denoise-variance"),
                                          (["--spatial-variance", "0", "--denoise-variance", "--denoise-out", "d.png"], "--spatial-variance must be in 1 .. 3"),
                                          (["--spatial-variance", "4", "--denoise-variance", "--denoise-out", "d.png"], "--spatial-variance must be in 1 .. 3"),
                                          (["--spatial-variance", "--denoise-variance"], "--denoise-variance needs --denoise-out"),
                                          (["--denoise-variance", "--denoise-out", "d.png"], NEEDS_THRESHOLD)])  # the last: without the option, as ever
def test_cli_rejects_inconsistent_options_without_a_gpu(args, message):
    p = _cli(*args)
    assert p.returncode == 2, (p.returncode, p.stdout, p.stderr)
    assert message in p.stderr, p.stderr
    assert "torch" not in p.stderr


def test_cli_accepts_denoise_variance_without_a_noise_threshold(tmp_path):
    """--export-textures returns after the options have been checked and before a device is touched."""
    for extra in ([], ["--frames", "2", "--frames-dir", str(tmp_path / "f"), "--temporal"], ["--noise-threshold", "0.05", "--spp", "32"]):
        p = _cli("--spatial-variance", "3", "--denoise-variance", "--denoise-out", str(tmp_path / "d.png"), *extra, "--export-textures", str(tmp_path / "t"))
        assert p.returncode == 0, p.stderr


# ---- the model's properties ---------------------------------------------------------------------------------------------------------

def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_a_constant_frame_gives_plus_zero(radius):
    c = np.broadcast_to(np.array([2, 3, 4], F), (9, 11, 3))
    var, (est, holes) = SV.spatial_variance(c, radius=radius)
    assert same_bits(var, np.zeros_like(var)) and (est, holes) == (99, 0)  # +0, not -0
    alb = np.full((9, 11, 3), F(0.5))
    var, counts = SV.spatial_variance(c, albedo=alb, radius=radius, demodulate=True)
    assert same_bits(var, np.zeros_like(var)) and counts == (99, 0)


def test_a_step_across_an_id_boundary_is_seen_only_without_the_id():
    h, w = 9, 16
    c = np.zeros((h, w, 3), F)
    c[:, w // 2:] = F(100)
    ids = np.zeros((h, w), np.int32)
    ids[:, w // 2:] = 1
    for r in (1, 2, 3):
        var, (est, holes) = SV.spatial_variance(c, id=ids, radius=r)
        assert same_bits(var, np.zeros_like(var)) and (est, holes) == (h * w, 0), r
        blind, _ = SV.spatial_variance(c, radius=r)  # every guide NULL
        near = np.zeros((h, w), bool)
        near[:, w // 2 - r:w // 2 + r] = True  # the windows that hold a pair across the step
        assert (blind[near] > 0).all() and same_bits(blind[~near], np.zeros_like(blind[~near])), r
        assert blind.max() <= F(100 * 100 / 2)


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_a_linear_ramp_gives_the_closed_form(radius):
    """color(x, y) = g x on every channel, no guides.  A window clipped by the frame to wx columns x wy rows holds wy (wx - 1) horizontal
    pairs, each with d = -g exactly, and wx (wy - 1) vertical pairs with d = 0: ssd = wy (wx - 1) g^2, np = wy (wx - 1) + wx (wy - 1), so
    variance = ssd / (2 np) — g^2 / 4 for a whole window, whatever the radius.  With g = 0.5 every value, difference, square and sum is
    exact in binary32, so the one rounding is the division's and the comparison is bit for bit."""
    g = F(0.5)
    h, w = 8, 13
    y, x = np.mgrid[0:h, 0:w]
    c = np.repeat((g * x.astype(F))[..., None], 3, axis=2).astype(F)
    var, (est, holes) = SV.spatial_variance(c, radius=radius, min_pairs=1)
    wx = np.minimum(x + radius, w - 1) - np.maximum(x - radius, 0) + 1
    wy = np.minimum(y + radius, h - 1) - np.maximum(y - radius, 0) + 1
    nh, nv = wy * (wx - 1), wx * (wy - 1)
    want = ((nh.astype(F) * (g * g)) / (F(2) * (nh + nv).astype(F))).astype(F)
    assert (est, holes) == (h * w, 0)
    for ch in range(3):
        assert same_bits(var[..., ch], want)
    whole = (wx == 2 * radius + 1) & (wy == 2 * radius + 1)
    assert whole.any() and (var[whole] == g * g / F(4)).all()


def test_a_pixel_of_unique_id_is_a_hole_and_min_pairs_makes_holes():
    c = np.random.default_rng(3).random((9, 11, 3), dtype=F)
    ids = np.zeros((9, 11), np.int32)
    ids[4, 5] = 7
    var, (est, holes) = SV.spatial_variance(c, id=ids, min_pairs=1)
    assert (var[4, 5] == INF).all() and holes == 1 and est == 98
    assert np.isfinite(np.delete(var.reshape(-1, 3), 4 * 11 + 5, axis=0)).all()
    one = np.ones((1, 1, 3), F)
    var, counts = SV.spatial_variance(one, min_pairs=1)
    assert (var == INF).all() and counts == (0, 1)  # a 1 x 1 frame: one hole
    # a corner's window at radius 1 holds 2 x 2 pixels = 4 pairs; an edge's 2 x 3 = 7; the interior's 3 x 3 = 12
    var, (est, holes) = SV.spatial_variance(c, radius=1, min_pairs=5)
    assert holes == 4 and all((var[y, x] == INF).all() for y in (0, 8) for x in (0, 10))
    assert SV.spatial_variance(c, radius=1, min_pairs=8)[1] == (7 * 9, 99 - 63)
    assert SV.spatial_variance(c, radius=1, min_pairs=13)[1] == (0, 99)


def test_an_iid_gaussian_frame_gives_its_variance():
    """Flat 64 x 64, sigma^2 = 1, no guides, radius 3: the mean of the estimates over the frame is a weighted mean of (X - Y)^2 / 2 over the
    frame's 2 x 64 x 63 = 8064 distinct adjacent pairs, each of expectation sigma^2 and relative deviation sqrt(2): standard error
    sqrt(2 / 8064) = 1.6 % (the pairs share pixels, which correlates them only weakly).  5 % is three of them."""
    c = np.random.default_rng(20171).normal(0.0, 1.0, (64, 64, 3)).astype(F)
    var, (est, holes) = SV.spatial_variance(c, radius=3)
    assert (est, holes) == (64 * 64, 0)
    for ch in range(3):
        mean = float(var[..., ch].astype(np.float64).mean())
        print(f"channel {ch}: mean estimate {mean:.4f}")
        assert abs(mean - 1.0) < 0.05, (ch, mean)


def test_fill_mode_keeps_finite_values_and_estimates_the_rest():
    r = np.random.default_rng(5)
    c = r.random((10, 12, 3), dtype=F)
    v = r.random((10, 12, 3), dtype=F)
    v[1, 1] = [F(-0.0), F(0), F(1e-30)]       # -0 is >= 0: kept, the -0 with it
    v[2, 3, 1] = np.nan                       # one bad channel: the whole pixel is estimated
    v[3, 4] = INF
    v[5, 6, 2] = F(-1)
    v[7, 8, 0] = -INF
    free, _ = SV.spatial_variance(c)
    out, (est, holes) = SV.spatial_variance(c, v)
    bad = np.zeros((10, 12), bool)
    for y, x in ((2, 3), (3, 4), (5, 6), (7, 8)):
        bad[y, x] = True
    assert same_bits(out[~bad], v[~bad]) and np.signbit(out[1, 1, 0])
    assert same_bits(out[bad], free[bad]) and np.isfinite(out[bad]).all()
    assert (est, holes) == (4, 0)
    inplace = v.copy()
    res, counts = SV.spatial_variance(c, inplace)
    assert same_bits(res, out) and counts == (est, holes)  # (the model is functional; the kernel's in-place call is held to this)
    assert SV.spatial_variance(c, np.zeros_like(c))[1] == (0, 0)  # everything kept


def test_non_finite_colours_never_enter_a_pair_and_are_holes_themselves():
    r = np.random.default_rng(6)
    c = r.random((9, 11, 3), dtype=F)
    clean, _ = SV.spatial_variance(c, radius=1)
    d = c.copy()
    d[4, 5, 1] = np.nan
    d[0, 0] = INF
    var, (est, holes) = SV.spatial_variance(d, radius=1)
    assert (var[4, 5] == INF).all() and (var[0, 0] == INF).all() and holes == 2 and est == 97
    ok = np.ones((9, 11), bool)
    ok[4, 5] = ok[0, 0] = False
    assert np.isfinite(var[ok]).all()
    far = np.ones((9, 11), bool)
    far[3:6, 4:7] = False
    far[0:2, 0:2] = False
    assert same_bits(var[far], clean[far])  # out of reach of the two pixels: untouched
    assert not same_bits(var[3, 4], clean[3, 4])  # within reach: pairs were dropped
    # demodulation: a colour that is finite but whose e overflows is not usable either
    alb = np.full((9, 11, 3), F(0.5))
    alb[2, 2] = F(-1e-3)  # m = 0: e = c / 0 = inf
    var, (est, holes) = SV.spatial_variance(c, albedo=alb, demodulate=True, radius=1)
    assert (var[2, 2] == INF).all() and holes == 1


def test_the_guides_follow_pt_temporal_pushs_tests():
    c = np.random.default_rng(7).random((9, 11, 3), dtype=F)
    z = np.full((9, 11), F(10))
    z[:, 6:] = F(11.5)  # a depth step of 15 % against tol_depth 0.1
    var, (est, holes) = SV.spatial_variance(c, depth=z, radius=1, min_pairs=1)
    one_sided, _ = SV.spatial_variance(c[:, :6], radius=1, min_pairs=1)
    assert same_bits(var[:, :6], one_sided)  # the left part sees nothing of the right
    assert not same_bits(SV.spatial_variance(c, depth=z, radius=1, min_pairs=1, tol_depth=0.2)[0][:, :6], one_sided)
    z2 = z.copy()
    z2[4, 2] = np.nan  # a z_p that is NaN: a miss, consistent only with the q whose z is not > 0 — itself: no pair
    z2[4, 8] = F(0)
    var, _ = SV.spatial_variance(c, depth=z2, radius=1, min_pairs=1)
    assert (var[4, 2] == INF).all() and (var[4, 8] == INF).all()
    n = np.zeros((9, 11, 3), F)
    n[..., 2] = 1
    n[:, 6:] = [F(1), F(0), F(0)]  # |dn|^2 = 2 > 0.25
    var, _ = SV.spatial_variance(c, normal=n, radius=1, min_pairs=1)
    assert same_bits(var[:, :6], one_sided)
    n[4, 2] = np.nan  # fails every normal test, its own too
    assert (SV.spatial_variance(c, normal=n, radius=1, min_pairs=1)[0][4, 2] == INF).all()


# ---- the quality record ------------------------------------------------------------------------------------------------------------------

SWEEP = [(r, mp) for r in (2, 3) for mp in (2, 4, 8)]
# r_8, r_32, r_128 per (radius, min_pairs) on the Cornell scene, as this test printed them when the defaults were chosen
RECORDED = {(2, 2): (0.7380, 0.5823, 0.7521), (2, 4): (0.7409, 0.5892, 0.7396), (2, 8): (0.7497, 0.5983, 0.7444),
            (3, 2): (0.7494, 0.5958, 0.7623), (3, 4): (0.7505, 0.5998, 0.7569), (3, 8): (0.7607, 0.6091, 0.7569)}


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_quality_record_and_the_defaults(orc):
    """tests/test_variance_denoise_cpu.py::test_default_sigma_variance_improves_8_32_and_128_spp_frames' set-up: the oracle's Cornell scene
    at 64 x 40, the reference at its REFERENCE_SPP, n = 8, 32, 128, guides of 6 camera rays per pixel (here with `id`).  The frame carries
    nothing but its guides: the spatial estimate (every guide, the temporal stage's tolerances, demodulated — the header's defaults) is
    the whole variance plane, fed to variance_model.denoise at its own defaults.  r_n = MSE(filtered) / MSE(noisy).  Asserted: the
    header's (radius, min_pairs) is the setting of {2, 3} x {2, 4, 8} with the smallest max_n r_n, and with it r_n < min(1, 1.5 x the
    recorded r_n) at every n — the run is deterministic, the margin is the project's convention.  Printed, never asserted: the same table
    for the "mixed" scene, whose mirrors and glass vary where no guide does — the estimate takes that signal for noise, and the filter
    then blurs it (DESIGN.md section 1 records the table as the stage's stated limit) — and each setting's fraction of holes."""
    w, h = 64, 40
    orc.set_math(True)
    tables = {}
    for name in ("cornell", "mixed"):
        ps, cam = S.ALL[name]()
        c = scenes.make_camera(cam, w, h)
        clean = orc.render(ps, c.c, w, h, REFERENCE_SPP)
        g = aov_np(orc, ps, c.c, w, h, 6)
        guides = dict(albedo=g["albedo"], normal=g["normal"], depth=g["depth"])
        r = {s: [] for s in SWEEP}
        holes = {}
        for n in (8, 32, 128):
            noisy = orc.render(ps, c.c, w, h, n)
            base = mse(noisy, clean)
            for radius, mp in SWEEP:
                var, (_, n_holes) = SV.spatial_variance(noisy, **guides, id=g["id"], radius=radius, min_pairs=mp, tol_depth=SV.DEFAULTS["tol_depth"],
                                                        tol_normal=SV.DEFAULTS["tol_normal"], demodulate=SV.DEFAULTS["demodulate"])
                out, _ = V.denoise(noisy, var, **guides, **V.DEFAULTS)
                r[radius, mp].append(mse(out, clean) / base)
                holes[radius, mp] = n_holes / (w * h)  # (the guides decide it: the same at every n, but for non-finite colours)
        tables[name] = r
        print(f"\n{name}: reference {REFERENCE_SPP} spp; r_8, r_32, r_128, worst, holes:")
        for s in SWEEP:
            print(f"  radius {s[0]}, min_pairs {s[1]}    " + "  ".join(f"{x:.4f}" for x in r[s]) + f"    max {max(r[s]):.4f}    holes {100 * holes[s]:.1f} %")
    r = tables["cornell"]
    best = min(SWEEP, key=lambda s: max(r[s]))
    assert best == (SV.DEFAULTS["radius"], SV.DEFAULTS["min_pairs"]) == (abi.PT_SVAR_DEFAULT_RADIUS, abi.PT_SVAR_DEFAULT_MIN_PAIRS)
    for got, rec in zip(r[best], RECORDED[best]):
        assert got < min(1.0, 1.5 * rec), (got, rec)
