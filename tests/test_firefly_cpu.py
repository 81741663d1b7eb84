"""CPU tests of the firefly stage's boundary and definition (include/pt_post.h: pt_firefly).  The new header is held to the rules
include/pt_render.h is held to by tests/test_abi_cpu.py and tests/test_stream_contract_cpu.py: abi.POST_SIGNATURES is exactly what it
declares, the library exports all of it, and every prototype with a `void* stream` has a row in the contract table below and a comment that
says what the row says.  The struct and the defaults are the header's, invalid calls are refused on the host before a device is
touched, the CLI options parse, and the numpy restatement of the header (tests/firefly_model.py, the one tests/test_gpu_firefly.py holds
the kernel to) has the properties the header promises.  The last test is the quality record DESIGN.md and profiles/firefly_bench.txt
quote: it asserts the SENSE of the stage's effect on the oracle's frames, never a size."""
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
import firefly_model as FM
import scenes_small as S
from path_tracer_amd import abi, scenes
from test_aov_cpu import aov_np

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "pt_post.h"
RENDER_HEADER = ROOT / "include" / "pt_render.h"
F = np.float32
INF = F(np.inf)

# The stream contract of include/pt_post.h, one row per prototype with a `void* stream` parameter (tests/stream_contract.py: CONTRACT is
# pt_render.h's): "async" — the call is asynchronous on `stream` —, or "sync" — it synchronises `stream`.
POST_CONTRACT = {
    "pt_firefly": "async",
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
    if re.fullmatch(r"const PtFireflyParams\* \w+|PtFireflyParams\* \w+", decl):
        return C.POINTER(abi.PtFireflyParams)
    if re.fullmatch(r"int32_t \w+\[\d+\]", decl):
        return C.POINTER(C.c_int32)
    if re.fullmatch(r"(const )?(float|uint32_t|void)\* \w+", decl):
        return C.c_void_p
    if re.fullmatch(r"int32_t \w+", decl):
        return C.c_int32
    raise AssertionError(f"no rule for the parameter {decl!r}")


def test_post_signatures_are_exactly_what_the_header_declares(lib):
    protos = prototypes()
    assert set(protos) == set(abi.POST_SIGNATURES) == set(abi.FIREFLY_SYMBOLS), sorted(set(protos) ^ set(abi.POST_SIGNATURES))
    ret = {"int": C.c_int, "void": None, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "const char*": C.c_char_p}
    for name, (rtype, args, _) in protos.items():
        assert abi.POST_SIGNATURES[name] == (ret[rtype], [ctype_of(a) for a in args]), name
        assert hasattr(lib, name), f"libpt_render.so does not export {name}"
        fn = getattr(lib, name)
        assert fn.restype == abi.POST_SIGNATURES[name][0] and list(fn.argtypes) == abi.POST_SIGNATURES[name][1], name  # load_library applied the row
    assert abi.has_firefly(lib)
    assert protos["pt_firefly"][:2] == ("int", ["const PtFireflyParams* params", "const float* color", "const float* variance", "float* out",
                                                "float* variance_out", "uint32_t* counts", "void* stream"])
    assert protos["pt_firefly_params_init"][:2] == ("void", ["PtFireflyParams* params", "int32_t width", "int32_t height"])
    assert protos["pt_debug_last_firefly"][:2] == ("int", ["int32_t out[4]"])


def test_the_two_tables_and_the_two_headers_are_disjoint(lib):
    assert not set(abi.POST_SIGNATURES) & set(abi.SIGNATURES)
    assert not set(prototypes()) & set(prototypes(RENDER_HEADER))
    assert "firefly" not in RENDER_HEADER.read_text().lower()  # pt_render.h knows nothing of the stage
    assert '#include "pt_render.h"' in HEADER.read_text()       # the error codes and pt_last_error are its
    assert lib.pt_abi_version() == 2                            # detected by the symbols, not by a version


def test_struct_matches_the_header():
    body = re.search(r"typedef struct PtFireflyParams\s*\{(.*?)\}\s*PtFireflyParams;", header_code(), re.S).group(1)
    fields = []
    ctypes_of = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = re.match(r"(int32_t|uint32_t|float)\s+(.*)", decl).groups()
            for nm in names.split(","):
                arr = re.fullmatch(r"(\w+)\[(\d+)\]", nm.strip())
                fields.append((arr.group(1), ctypes_of[ctype] * int(arr.group(2))) if arr else (nm.strip(), ctypes_of[ctype]))
    assert [n for n, _ in fields] == ["struct_size", "width", "height", "rank", "k", "flags", "reserved"]
    assert abi.PtFireflyParams._fields_ == fields
    assert C.sizeof(abi.PtFireflyParams) == 32


def test_defaults_are_the_headers(lib):
    text = HEADER.read_text()
    m = dict(re.findall(r"^#define (PT_FIREFLY_\w+) (\S+)", text, re.M))
    p = abi.PtFireflyParams(*([7] * 6))
    lib.pt_firefly_params_init(C.byref(p), 64, 40)
    assert (p.struct_size, p.width, p.height, list(p.reserved)) == (C.sizeof(abi.PtFireflyParams), 64, 40, [0, 0])
    assert int(m["PT_FIREFLY_REPAIR"].rstrip("u")) == abi.PT_FIREFLY_REPAIR == FM.REPAIR == 1
    assert int(m["PT_FIREFLY_NO_LDS"].rstrip("u")) == abi.PT_FIREFLY_NO_LDS == FM.NO_LDS == 2
    assert p.rank == int(m["PT_FIREFLY_DEFAULT_RANK"]) == abi.PT_FIREFLY_DEFAULT_RANK == FM.DEFAULTS["rank"] == 1
    assert F(p.k) == F(m["PT_FIREFLY_DEFAULT_K"].rstrip("f")) == F(abi.PT_FIREFLY_DEFAULT_K) == F(FM.DEFAULTS["k"]) == 1
    assert m["PT_FIREFLY_DEFAULT_FLAGS"] == "PT_FIREFLY_REPAIR" and p.flags == abi.PT_FIREFLY_DEFAULT_FLAGS == abi.PT_FIREFLY_REPAIR
    assert FM.DEFAULTS["repair"] is True
    assert (int(m["PT_FIREFLY_TILE_W"]), int(m["PT_FIREFLY_TILE_H"])) == (abi.PT_FIREFLY_TILE_W, abi.PT_FIREFLY_TILE_H)
    lib.pt_firefly_params_init(None, 1, 1)  # a NULL struct is ignored
    # the constants of the definition, as the model has them
    assert "Y(c)      = (0.2126f * R + 0.7152f * G) + 0.0722f * B" in text


# Pointers that are never dereferenced: every call below is refused on the host before a plane is read.
COLOR, VARIANCE, OUT, VOUT, COUNTS = (0x10000000 + i * 0x10000000 for i in range(5))
W, H = 64, 40
FRAME = W * H * 12


def params(lib, **over):
    p = abi.PtFireflyParams()
    lib.pt_firefly_params_init(C.byref(p), W, H)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def call(lib, p, color=COLOR, variance=VARIANCE, out=OUT, variance_out=VOUT, counts=COUNTS):
    return lib.pt_firefly(C.byref(p) if p is not None else None, color, variance, out, variance_out, counts, None)


BAD_PARAMS = [dict(struct_size=0), dict(struct_size=28), dict(struct_size=36), dict(width=0), dict(height=0), dict(width=-1), dict(height=-3),
              dict(rank=0), dict(rank=3), dict(rank=-1), dict(k=0.0), dict(k=-1.0), dict(k=math.nan), dict(k=math.inf), dict(k=-math.inf),
              dict(flags=4), dict(flags=7), dict(flags=1 << 31)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_refuses_bad_params_before_touching_a_device(lib, bad):
    assert call(lib, params(lib, **bad)) == abi.PT_ERR_INVALID_ARG
    assert b"pt_firefly" in lib.pt_last_error()


def test_refuses_null_arguments_and_too_many_pixels(lib):
    good = params(lib)
    assert call(lib, None) == abi.PT_ERR_INVALID_ARG
    assert call(lib, good, color=None) == abi.PT_ERR_INVALID_ARG
    assert call(lib, good, out=None) == abi.PT_ERR_INVALID_ARG and b"NULL" in lib.pt_last_error()
    assert call(lib, good, variance=None) == abi.PT_ERR_INVALID_ARG and b"variance_out needs variance" in lib.pt_last_error()
    assert call(lib, params(lib, width=1 << 16, height=(1 << 14) + 1)) == abi.PT_ERR_TOO_LARGE and b"2^30" in lib.pt_last_error()
    assert call(lib, params(lib, width=1 << 16, height=1 << 15)) == abi.PT_ERR_TOO_LARGE
    assert lib.pt_debug_last_firefly(None) == abi.PT_ERR_INVALID_ARG and b"pt_debug_last_firefly" in lib.pt_last_error()
    last = (C.c_int32 * 4)(9, 9, 9, 9)
    assert lib.pt_debug_last_firefly(last) == abi.PT_OK and 9 not in list(last)


def test_refuses_overlapping_planes(lib):
    good = params(lib)
    bad = abi.PT_ERR_INVALID_ARG
    assert call(lib, good, out=COLOR) == bad and b"overlap" in lib.pt_last_error()
    assert call(lib, good, out=COLOR + FRAME - 1) == bad           # the last byte of color
    assert call(lib, good, out=COLOR - FRAME + 1) == bad           # its first
    assert call(lib, good, out=VARIANCE + 12) == bad               # out inside an input
    assert call(lib, good, variance_out=COLOR + 4) == bad
    assert call(lib, good, variance_out=VARIANCE + 12) == bad      # overlapping variance without being it
    assert call(lib, good, variance_out=VARIANCE - FRAME + 4) == bad
    assert call(lib, good, counts=COLOR + 8) == bad
    assert call(lib, good, counts=VARIANCE + FRAME - 4) == bad
    assert call(lib, good, counts=COLOR - 4) == bad                # its second word is color's first
    assert call(lib, good, counts=OUT + 16) == bad and b"one another" in lib.pt_last_error()
    assert call(lib, good, counts=VOUT) == bad
    assert call(lib, good, variance_out=OUT + 24) == bad
    assert call(lib, good, out=VARIANCE, variance_out=VARIANCE) == bad  # variance_out may be variance; out may not
    assert call(lib, good, counts=COUNTS + 2) == bad and b"aligned" in lib.pt_last_error()


# ---- the stream contract of pt_post.h: tests/test_stream_contract_cpu.py's rule ----------------------------------------------------------

def test_every_stream_prototype_has_a_row_and_a_comment_that_states_it():
    text = HEADER.read_text()
    with_stream = {n: at for n, (_, args, at) in prototypes().items() if any(re.fullmatch(r"void\s*\*\s*stream", a) for a in args)}
    assert set(with_stream) == set(POST_CONTRACT), sorted(set(with_stream) ^ set(POST_CONTRACT))
    assert set(POST_CONTRACT.values()) <= {"async", "sync"}
    for name, want in POST_CONTRACT.items():
        comments = list(re.finditer(r"/\*(?:(?!\*/).)*\*/", text[:with_stream[name]], re.S))
        assert comments and text[comments[-1].end():with_stream[name]].strip() == "", f"{name}: no comment directly above its prototype"
        own = re.sub(r"\s+", " ", re.sub(r"^\s*\*", " ", comments[-1].group(0), flags=re.M))
        assert (bool(ASYNC.search(own)), bool(SYNC.search(own))) == (want == "async", want == "sync"), f"{name}: the table says {want}, its comment: {own}"
        assert abi.POST_SIGNATURES[name][1][-1] is C.c_void_p, name  # abi.py passes it a stream


# ---- hosts --------------------------------------------------------------------------------------------------------------------------

def test_firefly_main_compiles_against_the_facade(tmp_path, lib):
    out = tmp_path / "firefly_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{libdir / 'include'}", str(ROOT / "tests" / "cpp" / "firefly_main.cpp"), "-o", str(out), f"-L{libdir}",
                    "-lpt_render", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert out.exists()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "path_tracer_amd", *args], capture_output=True, text=True, cwd=ROOT,
                          env=dict(os.environ), timeout=120)


def test_cli_has_the_firefly_options():
    p = _cli("--help")
    assert p.returncode == 0, p.stderr
    assert "--firefly-clamp [K]" in p.stdout and "--firefly-rank R" in p.stdout


@pytest.mark.parametrize("args,message", [(["--firefly-clamp"], "--firefly-clamp needs --denoise-out, --display-out or --frames-dir"),
                                          (["--firefly-clamp", "2"], "--firefly-clamp needs --denoise-out, --display-out or --frames-dir"),
                                          (["--firefly-rank", "2", "--display-out", "d.png"], "--firefly-rank needs --firefly-clamp"),
                                          (["--firefly-clamp", "0", "--display-out", "d.png"], "--firefly-clamp must be finite and > 0"),
                                          (["--firefly-clamp", "nan", "--display-out", "d.png"], "--firefly-clamp must be finite and > 0"),
                                          (["--firefly-clamp", "inf", "--denoise-out", "d.png"], "--firefly-clamp must be finite and > 0"),
                                          (["--firefly-clamp", "--firefly-rank", "3", "--denoise-out", "d.png"], "--firefly-rank must be 1 or 2"),
                                          (["--firefly-clamp", "--firefly-rank", "0", "--display-out", "d.png"], "--firefly-rank must be 1 or 2")])
def test_cli_rejects_inconsistent_firefly_options_without_a_gpu(args, message):
    p = _cli(*args)
    assert p.returncode == 2, (p.returncode, p.stdout, p.stderr)
    assert message in p.stderr, p.stderr
    assert "torch" not in p.stderr


# ---- the model's properties ---------------------------------------------------------------------------------------------------------

def smooth(w=9, h=7, seed=2):
    """A frame with no outlier under rank 1, k = 1: a ramp that rises along x and y, so that every pixel but the top right corner has a
    brighter neighbour; the corner is set level with its left neighbour (a tie: not brighter)."""
    y, x = np.mgrid[0:h, 0:w].astype(F)
    c = (np.stack([x + y, x + F(2) * y, F(0.5) * x + y], -1) + F(1)).astype(F)
    c[h - 1, w - 1] = c[h - 1, w - 2]
    return c


FLAT = np.broadcast_to(np.array([2, 3, 4], F), (7, 9, 3))  # every pixel ties with every neighbour: no outlier under either rank


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def test_a_frame_without_an_outlier_comes_back_bit_for_bit():
    c = smooth()
    c[2, 3] = [F(-0.0), F(-0.0), F(-0.0)]   # zero luminance: never touched
    c[4, 1] = [F(-3), F(-2), F(-1)]         # negative luminance likewise
    v = np.random.default_rng(1).random(c.shape, dtype=F)
    out, vout, counts = FM.firefly(c, v)
    assert same_bits(out, c) and same_bits(vout, v) and counts == (0, 0)
    for rank in (1, 2):
        for k in (1.0, 2.5):
            out, vout, counts = FM.firefly(FLAT, v, rank=rank, k=k)
            assert same_bits(out, FLAT) and same_bits(vout, v) and counts == (0, 0), (rank, k)


@pytest.mark.parametrize("where", [(0, 0), (0, 8), (6, 0), (6, 8), (0, 4), (3, 0), (6, 5), (2, 8), (3, 4)],
                         ids=["corner00", "corner0w", "cornerh0", "cornerhw", "edge_bottom", "edge_left", "edge_top", "edge_right", "interior"])
def test_a_single_spike_comes_down_to_its_neighbourhoods_maximum(where):
    c = smooth()
    y, x = where
    c[y, x] = [F(900), F(500), F(100)]
    v = np.full(c.shape, F(4), F)
    out, vout, counts = FM.firefly(c, v)
    Y = FM.luminance(c)
    nb = [Y[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx or dy) and 0 <= y + dy < c.shape[0] and 0 <= x + dx < c.shape[1]]
    assert len(nb) == (3 if where in [(0, 0), (0, 8), (6, 0), (6, 8)] else 8 if where == (3, 4) else 5)
    s = F(max(nb) / Y[y, x])
    assert same_bits(out[y, x], (c[y, x] * s).astype(F)) and same_bits(vout[y, x], (v[y, x] * F(s * s)).astype(F))
    assert abs(float(FM.luminance(out[y, x])) / float(max(nb)) - 1) < 1e-6  # the luminance is the neighbourhood's maximum, to rounding
    assert np.allclose(out[y, x] / out[y, x].sum(), c[y, x] / c[y, x].sum(), rtol=1e-6)  # the chromaticity is kept
    untouched = np.ones(c.shape[:2], bool)
    untouched[y, x] = False
    assert same_bits(out[untouched], c[untouched]) and same_bits(vout[untouched], v[untouched]) and counts == (1, 0)
    out2, _, counts2 = FM.firefly(c, rank=1, k=2.0)  # k = 2: down to twice the maximum
    assert same_bits(out2[y, x], (c[y, x] * F(F(2) * max(nb) / Y[y, x])).astype(F)) and counts2 == (1, 0)


def test_two_adjacent_spikes_survive_rank_1_and_fall_to_rank_2():
    c = FLAT.copy()
    c[3, 4] = c[3, 5] = [F(700), F(700), F(700)]
    out1, _, n1 = FM.firefly(c, rank=1)
    assert same_bits(out1, c) and n1 == (0, 0)  # each is the other's largest neighbour: a tie is not brighter
    out2, _, n2 = FM.firefly(c, rank=2)
    Y = FM.luminance(c)
    second = sorted(Y[2:5, 3:6].reshape(-1))[-3]  # (3, 4)'s neighbourhood: itself, the other spike, then this
    assert second == Y[0, 0] and n2 == (2, 0)
    for x in (4, 5):
        assert same_bits(out2[3, x], (c[3, x] * F(second / Y[3, x])).astype(F))
    rest = np.ones(c.shape[:2], bool)
    rest[3, 4:6] = False
    assert same_bits(out2[rest], c[rest])
    lone = FLAT.copy()
    lone[3, 4] = [F(700), F(700), F(700)]
    assert FM.firefly(lone, rank=2)[2] == (1, 0) and FM.firefly(lone, rank=1)[2] == (1, 0)  # a lone spike falls to either


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_a_nan_or_inf_neighbour_is_ignored(poison):
    c = smooth()
    c[3, 4] = [F(900), F(500), F(100)]
    want = FM.firefly(c, repair=False)[0][3, 4]
    c[2, 3, 1] = poison  # the spike's darkest neighbour: with it gone the maximum (at (4, 5)) is the same
    out, _, counts = FM.firefly(c, repair=False)
    assert same_bits(out[3, 4], want) and counts == (1, 0)
    assert same_bits(out[2, 3], c[2, 3])  # and without repair it stays as it is
    c[4, 5, 0] = poison  # the maximum itself: the spike now comes down to the next one
    out, _, _ = FM.firefly(c, repair=False)
    Y = FM.luminance(c)
    assert same_bits(out[3, 4], (c[3, 4] * F(max(Y[4, 4], Y[3, 5]) / Y[3, 4])).astype(F))


def test_repair_replaces_a_lone_nan_by_the_mean_of_its_finite_neighbours():
    c = smooth()
    c[3, 4] = [np.nan, F(1), F(1)]
    c[2, 4] = [F(1), np.inf, F(1)]  # a neighbour that does not count
    c[0, 0] = [-np.inf, F(1), F(1)]  # a corner: three neighbours
    v = np.full(c.shape, F(4), F)
    out, vout, counts = FM.firefly(c, v)
    total = np.zeros(3, F)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dx or dy) and (3 + dy, 4 + dx) != (2, 4):
                total = (total + c[3 + dy, 4 + dx]).astype(F)
    assert same_bits(out[3, 4], (total / F(7)).astype(F)) and (vout[3, 4] == INF).all()
    assert same_bits(out[0, 0], (((c[0, 1] + c[1, 0]).astype(F) + c[1, 1]).astype(F) / F(3)).astype(F))
    assert counts[1] == 3 and np.isfinite(out).all()
    out, vout, counts = FM.firefly(c, v, repair=False)
    assert same_bits(out, c) and same_bits(vout, v) and counts == (0, 0)


def test_frames_with_nothing_to_compare_with_come_back_unchanged():
    with np.errstate(all="ignore"):
        nans = np.full((5, 6, 3), np.nan, F)
        nans[1, 2] = [np.inf, F(1), -np.inf]
        v = np.full(nans.shape, F(2), F)
        for rank in (1, 2):
            out, vout, counts = FM.firefly(nans, v, rank=rank)
            assert same_bits(out, nans) and same_bits(vout, v) and counts == (0, 0)
        for px in ([F(5), F(6), F(7)], [np.nan, F(1), F(1)]):
            one = np.array([[px]], F)
            out, vout, counts = FM.firefly(one, np.ones((1, 1, 3), F))
            assert same_bits(out, one) and same_bits(vout, np.ones((1, 1, 3), F)) and counts == (0, 0)
    two = np.array([[[1, 1, 1], [50, 50, 50]]], F)  # rank 2 needs two finite neighbours
    assert FM.firefly(two, rank=2)[2] == (0, 0) and FM.firefly(two, rank=1)[2] == (1, 0)


def test_variance_follows_the_pixel():
    c = smooth()
    c[3, 4] = [F(900), F(500), F(100)]
    c[5, 1] = [np.nan] * 3
    v = np.random.default_rng(4).random(c.shape, dtype=F)
    v[3, 4, 2] = np.nan       # a variance value is never tested: it is multiplied like any other
    out, vout, counts = FM.firefly(c, v)
    Y = FM.luminance(c)
    s = F(Y[4, 5] / Y[3, 4])  # the ramp's largest neighbour of (3, 4)
    assert counts == (1, 1) and 0 < s < 1 and same_bits(out[3, 4], (c[3, 4] * s).astype(F))
    assert same_bits(vout[3, 4, :2], (v[3, 4, :2] * F(s * s)).astype(F)) and np.isnan(vout[3, 4, 2])
    assert (vout[5, 1] == INF).all()
    rest = np.ones(c.shape[:2], bool)
    rest[3, 4] = rest[5, 1] = False
    assert same_bits(vout[rest], v[rest])
    assert FM.firefly(c)[1] is None  # no variance in, none out


# ---- the quality record ------------------------------------------------------------------------------------------------------------------

def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_quality_record_on_the_oracles_frames(orc):
    """The oracle's Cornell and mixed scenes at 64 x 40, at 4 / 8 / 32 / 128 spp against 2048 spp, through the binary32 model; every figure
    is an MSE relative to the noisy frame's.  Asserted — the sense, never a size: with the defaults each of the eight clamped / noisy ratios
    is < 1, and on Cornell at 4 / 8 / 32 spp the clamp followed by denoise_model (default parameters, guides of 16 camera rays per pixel:
    Accumulator.denoise's) has a smaller MSE than denoise_model alone.  Printed: all the ratios, and the sweep over rank 1 / 2 and
    k 1 / 2 (DESIGN.md and profiles/firefly_bench.txt quote the table)."""
    w, h = 64, 40
    orc.set_math(True)
    settings = [(1, 1.0), (1, 2.0), (2, 1.0), (2, 2.0)]
    print("\nMSE against 2048 spp, relative to the noisy frame's; per setting: clamped / clamped then denoised (pixels clamped)")
    print(f"{'scene':8s} {'spp':>4s} {'denoise':>8s}  " + "  ".join(f"{f'rank {r}, k {k:g}':>22s}" for r, k in settings))
    for name in ("cornell", "mixed"):
        ps, cam = S.ALL[name]()
        c = scenes.make_camera(cam, w, h)
        clean = orc.render(ps, c.c, w, h, 2048)
        g = aov_np(orc, ps, c.c, w, h, 16)
        filt = lambda fb: M.denoise(fb, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **M.DEFAULTS)  # noqa: E731
        for spp in (4, 8, 32, 128):
            noisy = orc.render(ps, c.c, w, h, spp)
            base = mse(noisy, clean)
            alone = mse(filt(noisy), clean) / base
            cells = {}
            for rank, k in settings:
                out, _, (n_clamped, _) = FM.firefly(noisy, rank=rank, k=k)
                cells[rank, k] = (mse(out, clean) / base, mse(filt(out), clean) / base, n_clamped)
            print(f"{name:8s} {spp:4d} {alone:8.3f}  " + "  ".join(f"{a:7.3f} / {b:7.3f} ({n:3d})" for a, b, n in cells.values()))
            clamped, chained, _ = cells[FM.DEFAULTS["rank"], FM.DEFAULTS["k"]]
            assert clamped < 1, (name, spp, clamped)
            if name == "cornell" and spp in (4, 8, 32):
                assert chained < alone, (name, spp, chained, alone)
