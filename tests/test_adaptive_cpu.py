"""CPU tests of adaptive sampling's boundary (include/pt_render.h: pt_adaptive_*): the library exports the entry points, abi.py declares
them as the header does, the exported state has the documented size, invalid accumulators are refused before any device call, and the
numpy restatement of the error estimate and of the selection rule (the one tests/test_gpu_adaptive.py holds the kernels to) gives the
values the header defines.  The rendering itself is tests/test_gpu_adaptive.py."""
import ctypes as C
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from path_tracer_amd import abi

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "pt_render.h"
ADAPTIVE = ["pt_adaptive_create", "pt_adaptive_window", "pt_adaptive_counts", "pt_adaptive_error", "pt_adaptive_select",
            "pt_adaptive_state_bytes", "pt_adaptive_export", "pt_adaptive_import"]


# ---- the numpy restatement (binary32 throughout, the order of operations of include/pt_render.h) ----------------------------------

def error_np(S, H, n, a):
    """S, H: [..., 3] float32 sums; n, a: [...] int32 counts -> [...] float32 errors."""
    S = np.asarray(S, dtype=np.float32)
    H = np.asarray(H, dtype=np.float32)
    n = np.asarray(n, dtype=np.int32)
    a = np.asarray(a, dtype=np.int32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        fn = np.maximum(n, 1).astype(np.float32)[..., None]
        fa = np.maximum(a, 1).astype(np.float32)[..., None]
        I = S / fn
        A = H / fa
        d = np.abs(I - A)
        num = (d[..., 0] + d[..., 1]) + d[..., 2]
        den = np.float32(1e-4) + np.sqrt((I[..., 0] + I[..., 1]) + I[..., 2])
        err = (num / den).astype(np.float32)
    return np.where((a == 0) | (a == n), np.float32(np.inf), err).astype(np.float32)


def select_np(S, H, n, a, threshold, min_spp, max_spp, dilate):
    """Whole frames ([H][W] counts): the mask (uint8) and the active count."""
    n = np.asarray(n, dtype=np.int32)
    err = error_np(S, H, n, a)
    noisy = (n < max_spp) & ~(err <= np.float32(threshold))
    act = noisy | (n < min_spp)
    if dilate:
        h, w = n.shape
        pad = np.zeros((h + 2, w + 2), dtype=bool)
        pad[1:-1, 1:-1] = noisy
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                act |= pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    act &= n < max_spp
    return act.astype(np.uint8), int(act.sum())


def book_np(S_before, S_after, H, n, a, w, mask=None):
    """One window of w samples over the pixels of `mask` (None: all): the new (H, n, a)."""
    H, n, a = H.copy(), n.copy(), a.copy()
    on = np.ones(n.shape, dtype=bool) if mask is None else mask.astype(bool)
    to_a = on & (a < n - a)
    D = (np.asarray(S_after, dtype=np.float32) - np.asarray(S_before, dtype=np.float32)).astype(np.float32)
    H[to_a] = (H[to_a] + D[to_a]).astype(np.float32)
    a[to_a] += w
    n[on] += w
    return H, n, a


# ---- the boundary ---------------------------------------------------------------------------------------------------------------

def params(w, h, depth=50, si=0, sc=1, flags=0, samples=0):
    return abi.PtRenderParams(w, h, samples, depth, si, sc, flags, 0)


def test_library_exports_adaptive_sampling(lib):
    for n in ADAPTIVE:
        assert hasattr(lib, n), f"libpt_render.so does not export {n}"
    assert abi.has_adaptive(lib)
    assert set(ADAPTIVE) == set(abi.ADAPTIVE_SYMBOLS)
    assert not abi.ADAPTIVE_SYMBOLS & abi.ACCUM_SYMBOLS
    assert lib.pt_abi_version() == 2


_CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float, "void": None}


def test_ctypes_prototypes_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    protos = {name: (ret, [a.strip() for a in args.split(",")])
              for ret, name, args in re.findall(r"^\s*([A-Za-z_][A-Za-z0-9_]*)\s+(pt_adaptive_\w+)\s*\(([^)]*)\)\s*;", text, re.M)}
    assert set(protos) == set(ADAPTIVE)
    for name, (ret, args) in protos.items():
        res, argtypes = abi.SIGNATURES[name]
        assert res is _CTYPES[ret], (name, ret, res)
        assert len(argtypes) == len(args), (name, args, argtypes)
        for decl, t in zip(args, argtypes):
            if "*" in decl:
                if "PtRenderParams" in decl:
                    assert t is C.POINTER(abi.PtRenderParams), (name, decl)
                elif "PtCamera" in decl:
                    assert t is C.POINTER(abi.PtCamera), (name, decl)
                elif decl.startswith("int64_t"):
                    assert t is C.POINTER(C.c_int64), (name, decl)
                else:
                    assert t in (C.c_void_p, C.POINTER(C.c_void_p)), (name, decl, t)
            else:
                assert t is _CTYPES[decl.split()[-2] if decl.split()[0] == "const" else decl.split()[0]], (name, decl, t)


def test_header_constants_match_abi():
    text = HEADER.read_text()
    assert f"#define PT_ADAPTIVE_FORMAT {abi.PT_ADAPTIVE_FORMAT}" in text
    assert f"#define PT_ADAPTIVE_DILATE {abi.PT_ADAPTIVE_DILATE}u" in text
    assert "#define PT_ACCUM_FORMAT 1" in text and "#define PT_ABI_VERSION 2" in text


@pytest.mark.parametrize("w,h,sc,si", [(32, 18, 1, 0), (1920, 1080, 1, 0), (256, 192, 3, 1), (256, 192, 3, 2), (20, 20, 8, 7)])
def test_state_bytes(lib, w, h, sc, si):
    p = params(w, h, si=si, sc=sc)
    tiles = -(-w // 8) * -(-h // 8)
    shard_tiles = -(-tiles // sc)
    F = w * h * 3 if sc == 1 else shard_tiles * 64 * 3
    R, P = shard_tiles * 64, F // 3
    assert lib.pt_adaptive_state_bytes(C.byref(p)) == 160 + 4 * F + 4 * R + 4 * F + 4 * P + 4 * P
    assert lib.pt_adaptive_state_bytes(C.byref(params(w, h, si=si, sc=sc, samples=99))) == lib.pt_adaptive_state_bytes(C.byref(p))
    # the plain format is untouched
    assert lib.pt_accum_state_bytes(C.byref(p)) == 160 + 4 * F + 4 * R


BAD = [params(0, 18), params(32, -1), params(32, 18, depth=-1), params(32, 18, si=1, sc=1), params(32, 18, sc=0),
       params(32, 18, flags=abi.PT_FLAG_SINGLE_STREAM), params(32, 18, flags=abi.PT_FLAG_FAST_RNG)]


@pytest.mark.parametrize("bad", BAD)
def test_state_bytes_invalid(lib, bad):
    assert lib.pt_adaptive_state_bytes(C.byref(bad)) < 0
    assert lib.pt_adaptive_state_bytes(None) < 0


@pytest.mark.parametrize("bad", BAD)
def test_create_refuses_before_touching_a_device(lib, bad):
    out = C.c_void_p(1234)
    assert lib.pt_adaptive_create(C.c_void_p(0xdead0), C.byref(bad), C.byref(out)) == abi.PT_ERR_INVALID_ARG
    assert not out.value


def test_null_handles_are_refused(lib):
    p = params(32, 18)
    out = C.c_void_p()
    assert lib.pt_adaptive_create(None, C.byref(p), C.byref(out)) == abi.PT_ERR_INVALID_ARG and not out.value
    assert lib.pt_adaptive_create(C.c_void_p(0xdead0), None, C.byref(out)) == abi.PT_ERR_INVALID_ARG and not out.value
    assert lib.pt_adaptive_create(C.c_void_p(0xdead0), C.byref(p), None) == abi.PT_ERR_INVALID_ARG
    cam = abi.PtCamera()
    n = C.c_int64(-7)
    assert lib.pt_adaptive_window(None, C.byref(cam), 4, None, None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_adaptive_window(None, C.byref(cam), 4, C.c_void_p(16), None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_adaptive_counts(None, C.c_void_p(16), None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_adaptive_error(None, C.c_void_p(16), None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_adaptive_select(None, 0.1, 16, 64, 1, C.c_void_p(16), C.byref(n), None) == abi.PT_ERR_INVALID_ARG and n.value == -7
    buf = (C.c_uint8 * 256)()
    assert lib.pt_adaptive_export(None, buf, 256, None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_adaptive_import(None, buf, 256, None) == abi.PT_ERR_INVALID_ARG


# ---- the restatement on hand-made states -----------------------------------------------------------------------------------------

def test_error_definition():
    S = np.array([[0.5, 0.25, 1.0], [2.0, 2.0, 2.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [3.0, 0.0, 0.0]], dtype=np.float32)
    H = np.array([[0.125, 0.125, 0.5], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=np.float32)
    n = np.array([4, 4, 4, 8, 4], dtype=np.int32)
    a = np.array([2, 2, 0, 4, 4], dtype=np.int32)
    err = error_np(S, H, n, a)
    # pixel 0: I = (0.125, 0.0625, 0.25), A = (0.0625, 0.0625, 0.25): |d| = 0.0625; den = 1e-4 + sqrt(0.4375)
    want0 = np.float32(0.0625) / (np.float32(1e-4) + np.sqrt(np.float32(0.4375)))
    assert err[0] == want0
    assert err[1] == 0.0                             # both halves agree
    assert np.isinf(err[2]) and np.isinf(err[4])     # a == 0, a == n: no estimate yet
    assert err[3] == 0.0                             # black: 0 / 1e-4
    assert err.dtype == np.float32


def test_select_inf_nan_and_bounds():
    h, w = 3, 4
    n = np.full((h, w), 32, dtype=np.int32)
    a = np.full((h, w), 16, dtype=np.int32)
    S = np.ones((h, w, 3), dtype=np.float32) * 32
    H = np.ones((h, w, 3), dtype=np.float32) * 16  # err 0 everywhere
    m, k = select_np(S, H, n, a, 0.01, 16, 64, dilate=False)
    assert k == 0 and not m.any()
    a2 = a.copy()
    a2[0, 0] = 0                                     # inf: noisy
    S2 = S.copy()
    S2[1, 1, 0] = np.nan                             # NaN: noisy (!(NaN <= t))
    m, k = select_np(S2, H, n, a2, 0.01, 16, 64, dilate=False)
    assert k == 2 and m[0, 0] and m[1, 1]
    n2 = n.copy()
    n2[0, 0] = 64                                    # at max_spp: never active, and not noisy for its neighbours
    m, k = select_np(S2, H, n2, a2, 0.01, 16, 64, dilate=True)
    assert not m[0, 0]
    n3 = n.copy()
    n3[2, 3] = 8                                     # below min_spp: active whatever its error
    m, k = select_np(S, H, n3, a, 0.01, 16, 64, dilate=False)
    assert k == 1 and m[2, 3]
    m, k = select_np(S, H, n, a, -1.0, 16, 64, dilate=False)
    assert k == h * w                                # a negative threshold keeps everything below max_spp active


def test_select_dilation_at_frame_borders():
    h, w = 5, 6
    n = np.full((h, w), 32, dtype=np.int32)
    a = np.full((h, w), 16, dtype=np.int32)
    S = np.ones((h, w, 3), dtype=np.float32) * 32
    H = np.ones((h, w, 3), dtype=np.float32) * 16
    a[0, 0] = 0       # corner
    a[4, 3] = 0       # bottom edge
    m, k = select_np(S, H, n, a, 0.01, 16, 64, dilate=True)
    want = np.zeros((h, w), dtype=np.uint8)
    want[0:2, 0:2] = 1
    want[3:5, 2:5] = 1
    assert (m == want).all() and k == int(want.sum())
    m, k = select_np(S, H, n, a, 0.01, 16, 64, dilate=False)
    assert k == 2


def test_bookkeeping_alternates_halves_ties_to_b():
    n = np.zeros(3, dtype=np.int32)
    a = np.zeros(3, dtype=np.int32)
    H = np.zeros((3, 3), dtype=np.float32)
    S = np.zeros((3, 3), dtype=np.float32)
    seq = []
    for k in range(4):
        S2 = S + np.float32(k + 1)
        H, n, a = book_np(S, S2, H, n, a, 16)
        S = S2
        seq.append((int(n[0]), int(a[0]), float(H[0, 0])))
    # window 1 -> B (tie 0 = 0), 2 -> A, 3 -> B (tie 16 = 16), 4 -> A
    assert seq == [(16, 0, 0.0), (32, 16, 2.0), (48, 16, 2.0), (64, 32, 6.0)]
    m = np.array([1, 0, 1], dtype=np.uint8)
    H, n2, a2 = book_np(S, S + 1, H, n, a, 8, m)
    assert list(n2) == [72, 64, 72]


# ---- hosts -----------------------------------------------------------------------------------------------------------------------

def test_adaptive_main_compiles_against_the_facade(tmp_path, lib):
    out = tmp_path / "adaptive_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{libdir / 'include'}", str(ROOT / "tests" / "cpp" / "adaptive_main.cpp"), "-o", str(out), f"-L{libdir}",
                    "-lpt_render", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert out.exists()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "path_tracer_amd", *args], capture_output=True, text=True, cwd=ROOT,
                          env=dict(os.environ), timeout=120)


def test_cli_has_adaptive_options():
    p = _cli("--help")
    assert p.returncode == 0, p.stderr
    for opt in ("--noise-threshold", "--min-spp", "--adaptive-step", "--counts-out"):
        assert opt in p.stdout


@pytest.mark.parametrize("args,message", [
    (["--noise-threshold", "0.1", "--spp", "100"], "must be --min-spp (16) plus a multiple of --adaptive-step (16)"),  # 100 - 16
    (["--noise-threshold", "0.1", "--spp", "8"], "must be --min-spp (16) plus a multiple"),                          # below --min-spp
    (["--noise-threshold", "0.1", "--spp", "64", "--min-spp", "0"], "--min-spp and --adaptive-step must be > 0"),
    (["--noise-threshold", "0.1", "--spp", "64", "--adaptive-step", "-16"], "--min-spp and --adaptive-step must be > 0"),
    (["--noise-threshold", "0.1", "--spp", "64", "--min-spp", "16", "--adaptive-step", "20"], "plus a multiple of --adaptive-step (20)"),
    (["--noise-threshold", "0.1", "--spp", "64", "--preview-every", "16"], "cannot be combined with --preview-every"),
    (["--min-spp", "16"], "need --noise-threshold"), (["--counts-out", "c.png"], "need --noise-threshold")])
def test_cli_rejects_inconsistent_options_without_a_gpu(args, message):
    p = _cli(*args)
    assert p.returncode == 2, (p.returncode, p.stdout, p.stderr)
    assert message in p.stderr, p.stderr
    assert "torch" not in p.stderr


def test_cli_accepts_consistent_options_up_to_the_render():
    # (validated before torch is imported: a consistent set gets past the parser; --export-textures then ends the run without a GPU)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        p = _cli("--noise-threshold", "0.1", "--spp", "112", "--min-spp", "16", "--adaptive-step", "32", "--export-textures", d)
        assert p.returncode == 0, p.stderr
