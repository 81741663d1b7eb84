"""CPU tests of progressive rendering's boundary (include/pt_render.h: PtAccum): the library exports the accumulator's entry points,
abi.py declares them as the header does, the exported state has the documented size, and invalid accumulators are refused before any
device call.  The rendering itself is tests/test_gpu_progressive.py."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from path_tracer_amd import abi

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "pt_render.h"
ACCUM = ["pt_accum_create", "pt_accum_destroy", "pt_accum_reset", "pt_accum_samples", "pt_render_accumulate", "pt_accum_resolve",
         "pt_accum_tonemap_rgb8", "pt_accum_state_bytes", "pt_accum_export", "pt_accum_import"]


def params(w, h, depth=50, si=0, sc=1, flags=0, samples=0):
    return abi.PtRenderParams(w, h, samples, depth, si, sc, flags, 0)


def test_library_exports_the_accumulator(lib):
    for n in ACCUM:
        assert hasattr(lib, n), f"libpt_render.so does not export {n}"
    assert abi.has_accumulator(lib)
    assert set(ACCUM) == set(abi.ACCUM_SYMBOLS)
    assert lib.pt_abi_version() == 2  # additive: no version change (scene_io reads version-2 fixtures only)


_CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "void": None}


def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^\s*([A-Za-z_][A-Za-z0-9_]*)\s+(pt_accum_\w+|pt_render_accumulate)\s*\(([^)]*)\)\s*;", text, re.M):
        out[name] = (ret, [a.strip() for a in args.split(",")])
    return out


def test_ctypes_prototypes_match_the_header():
    protos = _prototypes()
    assert set(protos) == set(ACCUM)
    for name, (ret, args) in protos.items():
        res, argtypes = abi.SIGNATURES[name]
        assert res is _CTYPES[ret], (name, ret, res)
        assert len(argtypes) == len(args), (name, args, argtypes)
        for decl, t in zip(args, argtypes):
            if "*" in decl:  # pointers: the struct pointers are typed, handles and buffers are void*
                if "PtRenderParams" in decl:
                    assert t is C.POINTER(abi.PtRenderParams), (name, decl)
                elif "PtCamera" in decl:
                    assert t is C.POINTER(abi.PtCamera), (name, decl)
                else:
                    assert t in (C.c_void_p, C.POINTER(C.c_void_p)), (name, decl, t)
            else:
                assert t is _CTYPES[decl.split()[0]], (name, decl, t)


def test_header_constants_match_abi():
    text = HEADER.read_text()
    assert f"#define PT_ACCUM_HEADER_BYTES {abi.PT_ACCUM_HEADER_BYTES}" in text
    assert f"#define PT_ACCUM_FORMAT {abi.PT_ACCUM_FORMAT}" in text
    assert f"#define PT_ACCUM_MAGIC {abi.PT_ACCUM_MAGIC:#010x}u" in text


@pytest.mark.parametrize("w,h,sc,si", [(32, 18, 1, 0), (1920, 1080, 1, 0), (256, 192, 3, 1), (256, 192, 3, 2), (20, 20, 8, 7)])
def test_state_bytes(lib, w, h, sc, si):
    p = params(w, h, si=si, sc=sc)
    tiles = -(-w // 8) * -(-h // 8)
    shard_tiles = -(-tiles // sc)
    floats = w * h * 3 if sc == 1 else shard_tiles * 64 * 3
    assert lib.pt_framebuffer_floats(C.byref(abi.PtRenderParams(w, h, 1, 50, si, sc, 0, 0))) == floats
    assert lib.pt_accum_state_bytes(C.byref(p)) == 160 + 4 * floats + 4 * shard_tiles * 64
    # `samples` is not part of the frame
    assert lib.pt_accum_state_bytes(C.byref(params(w, h, si=si, sc=sc, samples=77))) == lib.pt_accum_state_bytes(C.byref(p))


@pytest.mark.parametrize("bad", [params(0, 18), params(32, -1), params(32, 18, depth=-1), params(32, 18, si=1, sc=1),
                                 params(32, 18, sc=0), params(32, 18, flags=abi.PT_FLAG_SINGLE_STREAM)])
def test_state_bytes_invalid(lib, bad):
    assert lib.pt_accum_state_bytes(C.byref(bad)) < 0
    assert lib.pt_accum_state_bytes(None) < 0


@pytest.mark.parametrize("bad", [params(0, 18), params(32, 0), params(-4, 18), params(32, 18, depth=-1), params(32, 18, si=2, sc=2),
                                 params(32, 18, flags=abi.PT_FLAG_SINGLE_STREAM)])
def test_create_refuses_before_touching_a_device(lib, bad):
    # the scene handle is never dereferenced when the parameters are refused: a dummy one proves no device call happened
    out = C.c_void_p(1234)
    assert lib.pt_accum_create(C.c_void_p(0xdead0), C.byref(bad), C.byref(out)) == abi.PT_ERR_INVALID_ARG
    assert not out.value


def test_create_refuses_null_pointers(lib):
    p = params(32, 18)
    out = C.c_void_p()
    assert lib.pt_accum_create(None, C.byref(p), C.byref(out)) == abi.PT_ERR_INVALID_ARG and not out.value
    assert lib.pt_accum_create(C.c_void_p(0xdead0), None, C.byref(out)) == abi.PT_ERR_INVALID_ARG and not out.value
    assert lib.pt_accum_create(C.c_void_p(0xdead0), C.byref(p), None) == abi.PT_ERR_INVALID_ARG


def test_null_accumulator_is_refused(lib):
    cam = abi.PtCamera()
    assert lib.pt_accum_samples(None) == -1
    assert lib.pt_render_accumulate(None, C.byref(cam), 4, None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_accum_resolve(None, C.c_void_p(16), None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_accum_tonemap_rgb8(None, C.c_void_p(16), None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_accum_reset(None, None) == abi.PT_ERR_INVALID_ARG
    buf = (C.c_uint8 * 256)()
    assert lib.pt_accum_export(None, buf, 256, None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_accum_import(None, buf, 256, None) == abi.PT_ERR_INVALID_ARG
    lib.pt_accum_destroy(None)  # no-op


def test_progressive_main_compiles_against_the_facade(tmp_path, lib):
    # same flags as tests/test_cpp_facade.py gives facade_main.cpp
    out = tmp_path / "progressive_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", f"-I{ROOT / 'path_tracer_amd' / 'include'}",
                    str(ROOT / "tests" / "cpp" / "progressive_main.cpp"), "-o", str(out), f"-L{libdir}", "-lpt_render",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert out.exists()


def test_cli_has_preview_options():
    import os
    import sys
    env = dict(os.environ)
    p = subprocess.run([sys.executable, "-m", "path_tracer_amd", "--help"], capture_output=True, text=True, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr
    assert "--preview-every" in p.stdout and "--preview-dir" in p.stdout
