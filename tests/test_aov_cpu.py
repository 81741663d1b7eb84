"""CPU tests of the first-hit feature buffers' boundary (include/pt_render.h: pt_render_aov): the library exports the entry points,
abi.py declares them as the header does, pt_aov_plane_elems gives the documented sizes, every invalid call is refused before any device
call, and the numpy + oracle restatement of the pass — aov_np, the one tests/test_gpu_aov.py holds the kernel to — gives a `direct` plane
that is the oracle's render at depth 1, bit for bit.  The pass itself is tests/test_gpu_aov.py."""
import ctypes as C
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import scenes_small as S
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "pt_render.h"
AOV = ["pt_aov_plane_elems", "pt_render_aov", "pt_debug_last_aov"]
PLANES = ("albedo", "normal", "direct", "depth", "coverage", "id")
W, H, N = 19, 13, 6  # 3 x 2 tiles, partial tiles on both edges


# ---- the numpy + oracle restatement ------------------------------------------------------------------------------------------------

_RAY = np.dtype([("origin", "<f4", 3), ("dir", "<f4", 3), ("time", "<f4"), ("rng_state", "<u4")])
_IN = np.dtype([("origin", "<f4", 3), ("dir", "<f4", 3), ("time", "<f4"), ("rng_state", "<u4"), ("attenuation", "<f4", 3)])
_OUT = np.dtype([("status", "<i4"), ("hittable", "<i4"), ("material", "<i4"), ("front_face", "<i4"), ("t", "<f4"), ("p", "<f4", 3),
                 ("normal", "<f4", 3), ("u", "<f4"), ("v", "<f4"), ("color", "<f4", 3), ("sc_origin", "<f4", 3), ("sc_dir", "<f4", 3),
                 ("sc_time", "<f4"), ("rng_state", "<u4")])
assert _RAY.itemsize == C.sizeof(abi.PtCameraRay) and _IN.itemsize == C.sizeof(abi.PtBounceIn) and _OUT.itemsize == C.sizeof(abi.PtBounceOut)


def aov_np(orc, packed, cam_c, w, h, n):
    """The AOV pass of n samples as include/pt_render.h defines it: per pixel, orc.camera_rays -> orc.bounce (attenuation in = 1, 1, 1)
    -> PtBounceOut.rng_state -> the next sample; every float channel a float32 sum from +0 in sample order, divided once by float32(n).
    Whole-frame planes: albedo, normal, direct [h][w][3], depth, coverage [h][w] float32, id [h][w] int32."""
    orc.set_math(True)
    y, x = np.mgrid[0:h, 0:w]
    xy = np.stack([x.reshape(-1), y.reshape(-1)], 1).astype(np.int32)
    px = w * h
    state = (xy[:, 1].astype(np.uint64) * np.uint64(w) + xy[:, 0].astype(np.uint64)).astype(np.uint32)  # render.hpp:130-132
    sums = {"albedo": np.zeros((px, 3), np.float32), "normal": np.zeros((px, 3), np.float32), "direct": np.zeros((px, 3), np.float32),
            "depth": np.zeros(px, np.float32), "coverage": np.zeros(px, np.float32)}
    first_id = np.full(px, -1, np.int32)
    for s in range(n):
        rays = np.frombuffer(bytes(orc.camera_rays(cam_c, w, h, xy, state)), dtype=_RAY, count=px)
        rin = np.zeros(px, dtype=_IN)
        for f in ("origin", "dir", "time", "rng_state"):
            rin[f] = rays[f]
        rin["attenuation"] = 1.0
        out = np.frombuffer(bytes(orc.bounce(packed, (abi.PtBounceIn * px).from_buffer_copy(rin.tobytes()))), dtype=_OUT, count=px)
        hit = out["status"] != abi.PT_BOUNCE_MISS
        scattered = out["status"] == abi.PT_BOUNCE_SCATTERED
        zero3 = np.zeros((px, 3), np.float32)
        sums["albedo"] = sums["albedo"] + out["color"]
        sums["normal"] = sums["normal"] + np.where(hit[:, None], out["normal"], zero3)
        sums["direct"] = sums["direct"] + np.where(scattered[:, None], zero3, out["color"])
        sums["depth"] = sums["depth"] + np.where(hit, out["t"], np.float32(0))
        sums["coverage"] = sums["coverage"] + np.where(hit, np.float32(1), np.float32(0))
        if s == 0:
            first_id = out["hittable"].astype(np.int32)
        state = out["rng_state"].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        planes = {k: (v / np.float32(n)).astype(np.float32).reshape((h, w, 3) if v.ndim == 2 else (h, w)) for k, v in sums.items()}
    assert all(v.dtype == np.float32 for v in sums.values())
    planes["id"] = first_id.reshape(h, w)
    return planes


def shard_layout(plane, w, h, shard_index, shard_count, pad):
    """A whole-frame plane ([h][w] or [h][w][c]) re-laid out as shard `shard_index`'s tiles: [local tile][64] (+ [c]); padding = pad."""
    tx, nt = (w + 7) // 8, ((w + 7) // 8) * ((h + 7) // 8)
    tiles = -(-nt // shard_count)
    out = np.full((tiles, 64) + plane.shape[2:], pad, dtype=plane.dtype)
    for l in range(tiles):
        g = l * shard_count + shard_index
        if g >= nt:
            continue
        for i in range(64):
            x, y = (g % tx) * 8 + i % 8, (g // tx) * 8 + i // 8
            if x < w and y < h:
                out[l, i] = plane[y, x]
    return out


_REF = {}


def aov_reference(orc, name, w=W, h=H, n=N, cam_over=None):
    """aov_np of a small scene, computed once per (scene, size, camera) and shared (read-only) by the tests of both files."""
    key = (name, w, h, n, tuple(sorted((cam_over or {}).items())))
    if key not in _REF:
        ps, cam = S.ALL[name]()
        c = scenes.make_camera(dict(cam, **(cam_over or {})), w, h)
        planes = aov_np(orc, ps, c.c, w, h, n)
        for v in planes.values():
            v.setflags(write=False)
        _REF[key] = planes
    return _REF[key]


# ---- the boundary -------------------------------------------------------------------------------------------------------------------

def params(w, h, samples=4, depth=50, si=0, sc=1, flags=0):
    return abi.PtRenderParams(w, h, samples, depth, si, sc, flags, 0)


def buffers(**planes):
    b = abi.PtAovBuffers(struct_size=C.sizeof(abi.PtAovBuffers))
    for k, v in planes.items():
        setattr(b, k, v)
    return b


def test_library_exports_the_aov_pass(lib):
    for n in AOV:
        assert hasattr(lib, n), f"libpt_render.so does not export {n}"
    assert abi.has_aov(lib)
    assert set(AOV) == set(abi.AOV_SYMBOLS)
    assert not abi.AOV_SYMBOLS & (abi.ACCUM_SYMBOLS | abi.ADAPTIVE_SYMBOLS)
    assert lib.pt_abi_version() == 2 and "#define PT_ABI_VERSION 2" in HEADER.read_text()


def test_struct_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    body = re.search(r"typedef struct PtAovBuffers\s*\{(.*?)\}\s*PtAovBuffers;", text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.match(r"(int32_t\s*\*?|float\s*\*)\s*(.*)", decl).groups()
        for nm in names.split(","):
            fields.append((nm.strip().lstrip("*").strip(), "*" in ctype or nm.strip().startswith("*"), ctype.replace("*", "").strip()))
    assert [f[0] for f in fields] == ["struct_size", "reserved", *PLANES]
    assert [n for n, _ in abi.PtAovBuffers._fields_] == [f[0] for f in fields]
    for (name, ctype), (_, is_ptr, base) in zip(abi.PtAovBuffers._fields_, fields):
        assert ctype is (C.c_void_p if is_ptr else C.c_int32), name
        assert base == ("int32_t" if name in ("struct_size", "reserved", "id") else "float"), name
    assert C.sizeof(abi.PtAovBuffers) == 8 + 6 * C.sizeof(C.c_void_p) == 56
    assert abi.AOV_PLANES == PLANES and abi.AOV_CHANNELS == {"albedo": 3, "normal": 3, "direct": 3, "depth": 1, "coverage": 1, "id": 1}


def test_ctypes_prototypes_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    protos = {name: (ret, [a.strip() for a in args.split(",")])
              for ret, name, args in re.findall(r"^\s*([A-Za-z_][A-Za-z0-9_]*)\s+(pt_aov_\w+|pt_render_aov|pt_debug_last_aov)\s*\(([^)]*)\)\s*;", text, re.M)}
    assert set(protos) == set(AOV)
    assert protos["pt_aov_plane_elems"] == ("int64_t", ["const PtRenderParams* p", "int32_t channels"])
    assert abi.SIGNATURES["pt_aov_plane_elems"] == (C.c_int64, [C.POINTER(abi.PtRenderParams), C.c_int32])
    assert protos["pt_debug_last_aov"] == ("int", ["const PtScene* scene", "int32_t out[2]"])
    assert abi.SIGNATURES["pt_debug_last_aov"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)])
    ret, args = protos["pt_render_aov"]
    assert ret == "int" and [a.split("*")[0].strip() for a in args] == ["const PtScene", "const PtCamera", "const PtRenderParams", "const PtAovBuffers", "void"]
    assert abi.SIGNATURES["pt_render_aov"] == (C.c_int, [C.c_void_p, C.POINTER(abi.PtCamera), C.POINTER(abi.PtRenderParams),
                                                         C.POINTER(abi.PtAovBuffers), C.c_void_p])


@pytest.mark.parametrize("w,h,sc,si", [(19, 13, 1, 0), (1920, 1080, 1, 0), (19, 13, 3, 0), (19, 13, 3, 2), (256, 192, 3, 1), (20, 20, 8, 7)])
def test_plane_elems(lib, w, h, sc, si):
    tiles = -(-w // 8) * -(-h // 8)
    pixels = w * h if sc == 1 else -(-tiles // sc) * 64
    for samples in (0, 4, 1 << 30):  # samples are ignored
        p = params(w, h, samples=samples, si=si, sc=sc)
        assert lib.pt_aov_plane_elems(C.byref(p), 1) == pixels
        assert lib.pt_aov_plane_elems(C.byref(p), 3) == pixels * 3
    # the layouts the header names: the frame buffer's, and pt_adaptive_counts' (one element per pixel of it)
    p = params(w, h, si=si, sc=sc)
    assert lib.pt_aov_plane_elems(C.byref(p), 3) == lib.pt_framebuffer_floats(C.byref(p))
    assert lib.pt_aov_plane_elems(C.byref(params(w, h, si=si, sc=sc, flags=abi.PT_FLAG_NO_LPT | abi.PT_FLAG_TILE_GRANULAR)), 1) == pixels


BAD_FRAMES = [params(0, 13), params(19, -1), params(19, 13, si=1, sc=1), params(19, 13, sc=0), params(19, 13, si=-1, sc=2),
              params(19, 13, si=3, sc=3), params(19, 13, flags=abi.PT_FLAG_SINGLE_STREAM), params(19, 13, flags=abi.PT_FLAG_FAST_RNG),
              params(19, 13, flags=abi.PT_FLAG_FAST_RNG | abi.PT_FLAG_NO_LPT)]
BAD_SAMPLES = [params(19, 13, samples=0), params(19, 13, samples=-3), params(19, 13, samples=(1 << 24) + 1)]


@pytest.mark.parametrize("bad", BAD_FRAMES)
def test_plane_elems_invalid(lib, bad):
    assert lib.pt_aov_plane_elems(C.byref(bad), 1) < 0 and lib.pt_aov_plane_elems(C.byref(bad), 3) < 0


def test_plane_elems_invalid_channels(lib):
    assert lib.pt_aov_plane_elems(None, 1) < 0
    for ch in (0, 2, 4, -1):
        assert lib.pt_aov_plane_elems(C.byref(params(19, 13)), ch) < 0


SCENE, PLANE = C.c_void_p(0xdead0), 0xbeef00  # never dereferenced: every case below is refused on the host


@pytest.mark.parametrize("bad", BAD_FRAMES + BAD_SAMPLES)
def test_render_aov_refuses_bad_params_before_touching_a_device(lib, bad):
    cam = abi.PtCamera()
    b = buffers(albedo=PLANE, id=PLANE)
    assert lib.pt_render_aov(SCENE, C.byref(cam), C.byref(bad), C.byref(b), None) == abi.PT_ERR_INVALID_ARG


def test_render_aov_refuses_null_arguments_and_bad_buffers(lib):
    cam, p = abi.PtCamera(), params(19, 13)
    b = buffers(albedo=PLANE)
    assert lib.pt_render_aov(None, C.byref(cam), C.byref(p), C.byref(b), None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_render_aov(SCENE, None, C.byref(p), C.byref(b), None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_render_aov(SCENE, C.byref(cam), None, C.byref(b), None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_render_aov(SCENE, C.byref(cam), C.byref(p), None, None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_render_aov(SCENE, C.byref(cam), C.byref(p), C.byref(buffers()), None) == abi.PT_ERR_INVALID_ARG  # all six planes NULL
    for size in (0, C.sizeof(abi.PtAovBuffers) - 8, C.sizeof(abi.PtAovBuffers) + 8):
        wrong = buffers(albedo=PLANE, depth=PLANE)
        wrong.struct_size = size
        assert lib.pt_render_aov(SCENE, C.byref(cam), C.byref(p), C.byref(wrong), None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_last_error()
    out = (C.c_int32 * 2)(7, 7)
    assert lib.pt_debug_last_aov(None, out) == abi.PT_ERR_INVALID_ARG and list(out) == [7, 7]
    assert lib.pt_debug_last_aov(SCENE, None) == abi.PT_ERR_INVALID_ARG


def test_samples_bound_is_two_to_the_24(lib):
    # (the largest count whose coverage sum of ones is still exact in binary32; accepted counts go on to the device, so only the
    # refusals can be shown here: 2^24 + 1 is refused above, and the header states the bound)
    assert np.float32(1 << 24) + np.float32(1) == np.float32(1 << 24) and np.float32((1 << 24) - 1) + np.float32(1) == np.float32(1 << 24)
    assert "samples < 1 or > 1 << 24" in HEADER.read_text()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(S.ALL))
def test_direct_plane_is_the_oracles_render_at_depth_1(orc, name):
    ps, cam = S.ALL[name]()
    c = scenes.make_camera(cam, W, H)
    got = aov_reference(orc, name)
    orc.set_math(True)
    assert_bit_identical(got["direct"], orc.render(ps, c.c, W, H, N, depth=1), f"{name}: direct vs orc.render(depth=1)")
    for k in ("albedo", "normal", "direct", "depth", "coverage"):
        assert np.isfinite(got[k]).all(), (name, k)
    cov = got["coverage"]
    assert ((cov >= 0) & (cov <= 1)).all() and got["id"].min() >= -1 and got["id"].max() < max(1, ps.n_hittables)
    # a pixel whose first sample missed has id -1 and less than full coverage; full coverage means every sample hit, the first included
    assert (got["id"][cov == 1] >= 0).all() and (cov[got["id"] < 0] < 1).all()
    if name == "empty":
        assert not cov.any() and (got["id"] == -1).all() and not got["normal"].any() and not got["depth"].any()
        assert_bit_identical(got["albedo"], got["direct"], "empty scene: albedo is the sky")


def test_shard_layout_covers_every_pixel_once():
    y, x = np.mgrid[0:H, 0:W]
    lin = (y * W + x).astype(np.int32)
    seen = np.concatenate([shard_layout(lin, W, H, k, 3, -1).reshape(-1) for k in range(3)])
    assert sorted(seen[seen >= 0]) == list(range(W * H)) and (seen == -1).sum() == 3 * 2 * 64 - W * H


# ---- hosts --------------------------------------------------------------------------------------------------------------------------

def test_aov_main_compiles_against_the_facade(tmp_path, lib):
    out = tmp_path / "aov_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{libdir / 'include'}", str(ROOT / "tests" / "cpp" / "aov_main.cpp"), "-o", str(out), f"-L{libdir}",
                    "-lpt_render", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert out.exists()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "path_tracer_amd", *args], capture_output=True, text=True, cwd=ROOT,
                          env=dict(os.environ), timeout=120)


def test_cli_has_aov_options():
    p = _cli("--help")
    assert p.returncode == 0, p.stderr
    assert "--aov-dir" in p.stdout and "--aov-spp" in p.stdout


@pytest.mark.parametrize("args,message", [(["--aov-spp", "8"], "--aov-spp needs --aov-dir"),
                                          (["--aov-dir", "d", "--aov-spp", "0"], "--aov-spp must be in 1 .. 16777216"),
                                          (["--aov-dir", "d", "--aov-spp", "16777217"], "--aov-spp must be in 1 .. 16777216")])
def test_cli_rejects_inconsistent_aov_options_without_a_gpu(args, message):
    p = _cli(*args)
    assert p.returncode == 2, (p.returncode, p.stdout, p.stderr)
    assert message in p.stderr, p.stderr
    assert "torch" not in p.stderr
