"""CPU tests of temporal reprojection's boundary and definition (include/pt_render.h: pt_adaptive_next_frame, PtTemporal,
pt_temporal_push): the library exports the entry points, abi.py declares them as the header does, pt_temporal_state_bytes gives the
documented size, invalid calls are refused before a device is touched; the numpy binary32 restatement of the header
(tests/temporal_model.py, the one tests/test_gpu_temporal.py holds the kernel to) has the properties the header promises; and over the
oracle's frames of a moving camera the accumulated frame is as much better than the last noisy one as recorded here — provided the
frames continue each pixel's random stream, which is what pt_adaptive_next_frame is for.

Two refusals need a live object and therefore a device, and are tested in tests/test_gpu_temporal.py: an out plane overlapping a guide
plane (the state holds the frame size the overlap is judged by; pt_temporal_push reads the state only after every argument that can be
judged without it — which is what lets the calls below pass a handle that is never dereferenced) and pt_adaptive_next_frame on a plain
accumulator."""
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
import temporal_model as T
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd.scene import camera
from test_aov_cpu import aov_np

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "pt_render.h"
TEMPORAL = ["pt_adaptive_next_frame", "pt_temporal_params_init", "pt_temporal_state_bytes", "pt_temporal_create", "pt_temporal_destroy",
            "pt_temporal_reset", "pt_temporal_frames", "pt_temporal_push"]
F = np.float32


def header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


# ---- the boundary -------------------------------------------------------------------------------------------------------------------

def test_library_exports_temporal_reprojection(lib):
    for n in TEMPORAL:
        assert hasattr(lib, n), f"libpt_render.so does not export {n}"
    assert abi.has_temporal(lib)
    assert set(TEMPORAL) == set(abi.TEMPORAL_SYMBOLS)
    assert not abi.TEMPORAL_SYMBOLS & (abi.ACCUM_SYMBOLS | abi.ADAPTIVE_SYMBOLS | abi.AOV_SYMBOLS | abi.DENOISE_SYMBOLS | abi.PLAN_SYMBOLS |
                                       abi.VARIANCE_SYMBOLS)
    assert lib.pt_abi_version() == 2 and "#define PT_ABI_VERSION 2" in HEADER.read_text()


def test_struct_matches_the_header():
    body = re.search(r"typedef struct PtTemporalParams\s*\{(.*?)\}\s*PtTemporalParams;", header_text(), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = re.match(r"(int32_t|uint32_t|float)\s+(.*)", decl).groups()
            fields += [(nm.strip(), ctype) for nm in names.split(",")]
    assert fields == [("struct_size", "int32_t"), ("alpha", "float"), ("tol_depth", "float"), ("tol_normal", "float"), ("flags", "uint32_t"),
                      ("reserved[3]", "int32_t")]
    assert abi.PtTemporalParams._fields_ == [("struct_size", C.c_int32), ("alpha", C.c_float), ("tol_depth", C.c_float),
                                             ("tol_normal", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_int32 * 3)]
    assert C.sizeof(abi.PtTemporalParams) == 32


def test_ctypes_prototypes_match_the_header():
    protos = {name: (ret, [re.sub(r"\s+", " ", a.strip()) for a in args.split(",")])
              for ret, name, args in re.findall(r"^\s*(?:extern\s+)?([A-Za-z_][A-Za-z0-9_]*)\s+(pt_temporal_\w+|pt_adaptive_next_frame)\s*\(([^)]*)\)\s*;",
                                                header_text(), re.M)}
    assert set(protos) == set(TEMPORAL)
    assert protos["pt_adaptive_next_frame"] == ("int", ["PtAccum* acc", "void* stream"])
    assert abi.SIGNATURES["pt_adaptive_next_frame"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert protos["pt_temporal_params_init"] == ("void", ["PtTemporalParams* params"])
    assert abi.SIGNATURES["pt_temporal_params_init"] == (None, [C.POINTER(abi.PtTemporalParams)])
    assert protos["pt_temporal_state_bytes"] == ("int64_t", ["int32_t width", "int32_t height"])
    assert abi.SIGNATURES["pt_temporal_state_bytes"] == (C.c_int64, [C.c_int32, C.c_int32])
    assert protos["pt_temporal_create"] == ("int", ["int32_t width", "int32_t height", "PtTemporal** out"])
    assert abi.SIGNATURES["pt_temporal_create"] == (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_void_p)])
    assert protos["pt_temporal_destroy"] == ("void", ["PtTemporal* state"])
    assert abi.SIGNATURES["pt_temporal_destroy"] == (None, [C.c_void_p])
    assert protos["pt_temporal_reset"] == ("int", ["PtTemporal* state", "void* stream"])
    assert abi.SIGNATURES["pt_temporal_reset"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert protos["pt_temporal_frames"] == ("int32_t", ["const PtTemporal* state"])
    assert abi.SIGNATURES["pt_temporal_frames"] == (C.c_int32, [C.c_void_p])
    assert protos["pt_temporal_push"] == ("int", ["PtTemporal* state", "const PtTemporalParams* params", "const PtCamera* cam", "const float* color",
                                                  "const float* depth", "const float* normal", "const int32_t* id", "const float* variance_in",
                                                  "float* out_color", "float* out_variance", "float* out_history", "void* stream"])
    assert abi.SIGNATURES["pt_temporal_push"] == (C.c_int, [C.c_void_p, C.POINTER(abi.PtTemporalParams), C.POINTER(abi.PtCamera)] + [C.c_void_p] * 9)


def test_defaults_are_the_headers(lib):
    m = dict(re.findall(r"^#define (PT_TEMPORAL_\w+) (\S+)", HEADER.read_text(), re.M))
    p = abi.PtTemporalParams(7, 7.0, 7.0, 7.0, 7, (7, 7, 7))
    lib.pt_temporal_params_init(C.byref(p))
    assert (p.struct_size, p.flags, list(p.reserved)) == (C.sizeof(abi.PtTemporalParams), 0, [0, 0, 0])
    for field, macro in (("alpha", "ALPHA"), ("tol_depth", "TOL_DEPTH"), ("tol_normal", "TOL_NORMAL")):
        want = F(m[f"PT_TEMPORAL_DEFAULT_{macro}"].rstrip("f"))
        assert F(getattr(p, field)) == want == F(getattr(abi, f"PT_TEMPORAL_DEFAULT_{macro}")) == F(T.DEFAULTS[field]), field
    assert (F(p.alpha), F(p.tol_depth), F(p.tol_normal)) == (F(0.1), F(0.1), F(0.5))
    lib.pt_temporal_params_init(None)  # a NULL struct is ignored


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (19, 13), (70, 45), (1920, 1080), (32768, 32768)])
def test_state_bytes(lib, w, h):
    """Two histories of three 16-byte records per pixel."""
    assert lib.pt_temporal_state_bytes(w, h) == 2 * 3 * 16 * w * h == 96 * w * h


def test_state_bytes_invalid(lib):
    for w, h in [(0, 13), (19, 0), (-1, 13), (19, -5), (32768, 32769), (1 << 20, 1 << 20)]:
        assert lib.pt_temporal_state_bytes(w, h) < 0, (w, h)


def test_create_refuses_bad_sizes_before_touching_a_device(lib):
    out = C.c_void_p(0x7)
    for w, h in [(0, 13), (19, 0), (-1, 13), (19, -5)]:
        assert lib.pt_temporal_create(w, h, C.byref(out)) == abi.PT_ERR_INVALID_ARG and not out.value, (w, h)
        assert b"pt_temporal_create" in lib.pt_last_error()
    assert lib.pt_temporal_create(1 << 16, 1 << 15, C.byref(out)) == abi.PT_ERR_TOO_LARGE and not out.value  # 2^31 pixels
    assert lib.pt_temporal_create(19, 13, None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_temporal_frames(None) == -1
    assert lib.pt_temporal_reset(None, None) == abi.PT_ERR_INVALID_ARG
    lib.pt_temporal_destroy(None)  # ignored


# Pointers that are never dereferenced: every call below is refused on the host before the state or a plane is read.
STATE, COLOR, DEPTH, NORMAL, ID, VAR, OUT, VOUT, HOUT = (0x10000000 + i * 0x1000000 for i in range(9))


def good_camera():
    return camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0, 1.6, 0.0, 1.0, 0.0, 0.0).c


def params(**over):
    p = abi.PtTemporalParams(C.sizeof(abi.PtTemporalParams), 0.1, 0.1, 0.5, 0)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def call(lib, p, cam="good", state=STATE, color=COLOR, depth=DEPTH, out=OUT):
    cam = good_camera() if cam == "good" else cam
    return lib.pt_temporal_push(state, C.byref(p) if p is not None else None, C.byref(cam) if cam is not None else None, color, depth, NORMAL, ID,
                                VAR, out, VOUT, HOUT, None)


BAD_PARAMS = [dict(struct_size=0), dict(struct_size=28), dict(struct_size=36), dict(alpha=0.0), dict(alpha=-0.1), dict(alpha=1.0000001),
              dict(alpha=math.nan), dict(alpha=math.inf), dict(tol_depth=0.0), dict(tol_depth=-1.0), dict(tol_depth=math.nan),
              dict(tol_depth=math.inf), dict(tol_normal=0.0), dict(tol_normal=-0.5), dict(tol_normal=math.nan), dict(tol_normal=math.inf),
              dict(flags=1), dict(flags=1 << 31)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_refuses_bad_params_before_touching_a_device(lib, bad):
    assert call(lib, params(**bad)) == abi.PT_ERR_INVALID_ARG
    assert b"pt_temporal_push" in lib.pt_last_error()


def test_refuses_null_arguments(lib):
    assert call(lib, None) == abi.PT_ERR_INVALID_ARG
    assert call(lib, params(), cam=None) == abi.PT_ERR_INVALID_ARG
    for name in ("state", "color", "depth", "out"):
        assert call(lib, params(), **{name: None}) == abi.PT_ERR_INVALID_ARG, name
    assert lib.pt_adaptive_next_frame(None, None) == abi.PT_ERR_INVALID_ARG
    assert b"pt_adaptive_next_frame" in lib.pt_last_error()


def test_refuses_degenerate_cameras(lib):
    zero = abi.PtCamera()
    assert call(lib, params(), cam=zero) == abi.PT_ERR_INVALID_ARG and b"degenerate" in lib.pt_last_error()
    assert T.host_constants(zero) is None
    for field, value in (("horizontal", (0, 0, 0)), ("vertical", (0, 0, 0)), ("horizontal", (math.nan, 0, 0)), ("vertical", (math.inf, 0, 0)),
                         ("w", (0, 0, 0)), ("w", (0, 0, -1)), ("origin", (math.nan, 0, 0)), ("lower_left_corner", (0, 0, -math.inf)),  # fo = +inf
                         ("horizontal", (3e38, 3e38, 0))):         # hh overflows
        cam = good_camera()
        getattr(cam, field)[:] = value
        assert call(lib, params(), cam=cam) == abi.PT_ERR_INVALID_ARG, (field, value)
        assert T.host_constants(cam) is None, (field, value)
    fo, hh, vv = T.host_constants(good_camera())
    assert abs(fo - 1) < 1e-6 and hh > 0 and vv > 0


# ---- hosts --------------------------------------------------------------------------------------------------------------------------

def test_temporal_main_compiles_against_the_facade(tmp_path, lib):
    out = tmp_path / "temporal_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{libdir / 'include'}", str(ROOT / "tests" / "cpp" / "temporal_main.cpp"), "-o", str(out), f"-L{libdir}",
                    "-lpt_render", "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert out.exists()


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "path_tracer_amd", *args], capture_output=True, text=True, cwd=ROOT,
                          env=dict(os.environ), timeout=120)


def test_cli_has_the_options():
    p = _cli("--help")
    assert p.returncode == 0, p.stderr
    for opt in ("--frames", "--move", "--frames-dir", "--temporal"):
        assert opt in p.stdout, opt


@pytest.mark.parametrize("args,message", [(["--temporal"], "--move, --frames-dir and --temporal need --frames"),
                                          (["--move", "1,0,0"], "--move, --frames-dir and --temporal need --frames"),
                                          (["--frames-dir", "d"], "--move, --frames-dir and --temporal need --frames"),
                                          (["--frames", "3"], "--frames needs --frames-dir"),
                                          (["--frames", "0", "--frames-dir", "d"], "--frames must be >= 1"),
                                          (["--frames", "3", "--frames-dir", "d", "--move", "1,2"], "--move must be three finite numbers"),
                                          (["--frames", "3", "--frames-dir", "d", "--move", "1,x,2"], "--move must be three finite numbers"),
                                          (["--frames", "3", "--frames-dir", "d", "--move", "1,nan,2"], "--move must be three finite numbers"),
                                          (["--frames", "3", "--frames-dir", "d", "--denoise-variance"], "--denoise-variance needs --noise-threshold"),
                                          (["--frames", "3", "--frames-dir", "d", "--temporal", "--denoise-variance", "--denoise-out", "x.png"],
                                           "--denoise-out with --denoise-variance needs --noise-threshold"),
                                          (["--frames", "3", "--frames-dir", "d", "--temporal", "--denoise-variance", "--denoise-sigma-color", "2"],
                                           "--denoise-sigma-color does not apply to --denoise-variance"),
                                          (["--frames", "3", "--frames-dir", "d", "--temporal", "--denoise-iterations", "3"],
                                           "--denoise-iterations and --denoise-sigma-* need --denoise-out")])
def test_cli_rejects_inconsistent_options_without_a_gpu(args, message):
    p = _cli(*args)
    assert p.returncode == 2, (p.returncode, p.stdout, p.stderr)
    assert message in p.stderr, p.stderr
    assert "torch" not in p.stderr


# ---- the model: properties ----------------------------------------------------------------------------------------------------------

W, H = 16, 10
Z = F(5.0)  # a plane facing the camera at distance 5: with focus_dist = 1 the un-normalised ray advances 1 along the view axis per unit t


def cam_at(look_from=(0, 0, 0), look_at=None):
    look_at = (look_from[0], look_from[1], look_from[2] - 1) if look_at is None else look_at
    return camera(look_from, look_at, (0, 1, 0), 60.0, W / H, 0.0, 1.0, 0.0, 0.0).c


def flat_guides():
    return dict(depth=np.full((H, W), Z, F), normal=np.tile(np.array([0, 0, 1], F), (H, W, 1)), id=np.full((H, W), 3, np.int32))


def colours(seed):
    return np.random.default_rng(seed).random((H, W, 3), dtype=F) * F(2)


def test_static_camera_gives_the_running_mean():
    """K frames from one camera with identical guides: every pixel reprojects onto itself (to within rounding: a weight of ~1e-6 may go
    to a neighbour), N counts 1 ... K, the colour is the running mean and the variance that of the mean."""
    t, cam, g = T.Temporal(W, H), cam_at(), flat_guides()
    frames = [colours(s) for s in range(6)]
    for k, c in enumerate(frames, 1):
        out, var, hist = t.push(cam, c, alpha=0.1, **g)
        assert out.dtype == var.dtype == hist.dtype == F and t.frames == k
        np.testing.assert_allclose(hist, k, rtol=1e-5)
        mean = np.mean(frames[:k], axis=0)
        np.testing.assert_allclose(out, mean, rtol=0, atol=2e-4)
        if k < 4:
            assert np.isposinf(var).all()  # no variance_in: "no estimate"
        else:
            s2 = np.mean(np.square(frames[:k]), axis=0) - mean ** 2
            np.testing.assert_allclose(var, s2 / k, rtol=0, atol=3e-4)
    # the first push is the frame itself, bit for bit
    t.reset()
    out, var, hist = t.push(cam, frames[0], **g)
    assert_bit_identical(out, frames[0], "first push")
    assert (hist == 1).all()
    assert_bit_identical(t.m2, frames[0] * frames[0], "second moment")


def test_exponential_floor():
    """Once 1 / N < alpha the blend weight stays alpha."""
    t, cam, g = T.Temporal(W, H), cam_at(), flat_guides()
    for k in range(5):
        t.push(cam, colours(k), alpha=0.5, **g)
    before = t.c.copy()
    c = colours(9)
    out, _, hist = t.push(cam, c, alpha=0.5, **g)
    np.testing.assert_allclose(hist, 6, rtol=1e-5)
    np.testing.assert_allclose(out, before + 0.5 * (c - before), atol=2e-4)


def test_a_camera_turned_away_has_no_history():
    t, g = T.Temporal(W, H), flat_guides()
    t.push(cam_at(), colours(1), **g)
    c = colours(2)
    out, var, hist = t.push(cam_at(look_at=(0, 0, 1)), c, variance_in=np.full((H, W, 3), 0.25, F), **g)  # a 180 degree turn: cp <= 0
    assert (hist == 1).all()
    assert_bit_identical(out, c, "no history: the frame itself")
    assert (var == F(0.25)).all()


def test_taps_outside_the_frame_are_skipped_and_the_weights_renormalised():
    """The camera moves sideways by 2.5 pixels' worth at the plane: a column at the edge reprojects half outside — its one remaining tap
    column is renormalised to the full weight — and the columns beyond have no history."""
    t, g = T.Temporal(W, H), flat_guides()
    first = colours(3)
    t.push(cam_at(), first, **g)
    # horizontal extent at distance Z: |horizontal| * Z over W pixels
    px = float(np.sqrt(T.host_constants(cam_at())[1])) * float(Z) / W
    c = colours(4)
    out, _, hist = t.push(cam_at(look_from=(-2.5 * px, 0, 0)), c, **g)
    # pixel x of this frame sees the previous frame at fx = x - 2.5: columns 0, 1 have fx < -1; column 2 has fx = -0.5 (x0 = -1: one tap column)
    assert (hist[:, :2] == 1).all() and np.allclose(hist[:, 2:], 2, rtol=1e-4)
    assert_bit_identical(out[:, :2], c[:, :2], "columns without history")
    np.testing.assert_allclose(out[1:-1, 2], first[1:-1, 0] + 0.5 * (c[1:-1, 2] - first[1:-1, 0]), atol=1e-3)  # renormalised: not halved
    np.testing.assert_allclose(out[1:-1, 5], 0.5 * (first[1:-1, 2] + first[1:-1, 3]) * 0.5 + 0.5 * c[1:-1, 5], atol=1e-3)


@pytest.mark.parametrize("what", ["id", "normal", "depth"])
def test_each_guide_rejects_a_tap_on_its_own(what):
    t, g = T.Temporal(W, H), flat_guides()
    t.push(cam_at(), colours(5), **g)
    g2 = flat_guides()
    if what == "id":
        g2["id"][4, 7] = 9
    elif what == "normal":
        g2["normal"][4, 7] = (0, 0.6, 0.8)  # |dn|^2 = 0.36 + 0.04 = 0.4 > 0.25
    else:
        g2["depth"][4, 7] = Z * F(1.5)      # reprojects near its own place (static camera), 50 % deeper than the history's surface
    c = colours(6)
    out, _, hist = t.push(cam_at(), c, **g2)
    assert hist[4, 7] == 1 and (np.delete(hist.reshape(-1), 4 * W + 7) > 1.5).all()
    assert_bit_identical(out[4, 7], c[4, 7], "the rejected pixel restarts")
    # ... and without that guide plane (or within tolerance) it is accepted
    t2 = T.Temporal(W, H)
    t2.push(cam_at(), colours(5), **g)
    if what == "depth":
        g2["depth"][4, 7] = Z * F(1.05)
    else:
        g2[what] = None
    assert (t2.push(cam_at(), c, **g2)[2] > 1.5).all()


def test_a_missed_pixel_takes_history_only_from_missed_pixels():
    t, g = T.Temporal(W, H), flat_guides()
    g["depth"][:, : W // 2] = 0  # the left half misses
    g["id"][:, : W // 2] = -1
    g["normal"][:, : W // 2] = 0
    t.push(cam_at(), colours(7), **g)
    g2 = {k: v.copy() for k, v in g.items()}
    g2["depth"][3, W // 2 + 2] = 0  # a pixel of the hit half now misses: its taps are hits -> no history (id and normal off: depth alone decides)
    g2["depth"][6, 2] = Z           # and a pixel of the missed half now hits
    out, _, hist = t.push(cam_at(), colours(8), depth=g2["depth"])
    assert hist[3, W // 2 + 2] == 1 and hist[6, 2] == 1
    rest = np.ones((H, W), bool)
    rest[3, W // 2 + 2] = rest[6, 2] = False
    assert (hist[rest] > 1.5).all()  # misses continue from misses (as directions), hits from hits


def test_non_finite_colours_stay_in_place_and_out_of_the_history():
    t, cam, g = T.Temporal(W, H), cam_at(), flat_guides()
    c1 = colours(10)
    c1[2, 3] = np.nan
    c1[5, 9, 1] = np.inf
    c1[7, 0] = -np.inf
    bad = np.zeros((H, W), bool)
    bad[2, 3] = bad[5, 9] = bad[7, 0] = True
    out, var, hist = t.push(cam, c1, variance_in=np.zeros((H, W, 3), F), **g)
    assert_bit_identical(out, c1, "the first push, NaN and inf in place")
    assert (hist[bad] == 0).all() and np.isposinf(var[bad]).all() and (var[~bad] == 0).all()
    assert (t.N[bad] == 0).all() and (t.c[bad] == 0).all() and (t.m2[bad] == 0).all() and np.isfinite(t.c).all()
    c2 = colours(11)
    out2, _, hist2 = t.push(cam, c2, **g)
    assert np.isfinite(out2).all(), "a non-finite colour entered the next frame"
    assert (hist2[bad] == 1).all()  # their own history was unusable (the ~1e-6 of neighbour weight stays under the 0.01 floor)
    assert_bit_identical(out2[bad], c2[bad], "restart")
    # the same sequence with other bad values gives the same finite pixels
    t3 = T.Temporal(W, H)
    c3 = c1.copy()
    c3[bad] = np.nan
    t3.push(cam, c3, **g)
    assert_bit_identical(t3.push(cam, c2, **g)[0], out2, "the bad values themselves are absent from the sums")


def test_young_histories_pass_the_callers_variance_through():
    t, cam, g = T.Temporal(W, H), cam_at(), flat_guides()
    vin = np.random.default_rng(12).random((H, W, 3), dtype=F)
    for k in range(1, 6):
        _, with_v, hist = t.push(cam, colours(20 + k), variance_in=vin, **g)
        if k < 4:
            assert_bit_identical(with_v, vin, f"N = {k}: variance_in")
        else:
            assert np.isfinite(with_v).all() and not np.array_equal(with_v, vin) and (with_v >= 0).all()
    t2 = T.Temporal(W, H)
    for k in range(1, 4):
        assert np.isposinf(t2.push(cam, colours(20 + k), **g)[1]).all()


# ---- quality --------------------------------------------------------------------------------------------------------------------------

REFERENCE_SPP = 2048
FRAMES, SPP = 8, 4
# measured once with this model (this test prints the table): MSE(accumulated frame 7) / MSE(noisy frame 7) against the 2048 spp frame of
# camera 7, for look_from.x moving by `move` units per frame (the pixels that end with N = 1 were 0 %, 0.55 %, 0.16 % and 9.38 %)
RECORDED = {0: 0.1278, 2: 0.1126, 10: 0.1184, 40: 0.2043}


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.fixture(scope="module")
def sequences(orc):
    """Per move: the model run over FRAMES frames of the oracle's small Cornell scene at 64 x 40, SPP samples each.  Frame f is the
    oracle's samples [4f, 4f + 4) of camera f's pixels — render(4f + 4) x (4f + 4) - render(4f) x 4f, over 4 — i.e. what an adaptive
    accumulator renders after f calls of pt_adaptive_next_frame; guides from aov_np at 4 spp."""
    w, h = 64, 40
    ps, cam = S.ALL["cornell"]()
    orc.set_math(True)
    out = {}
    for move in (0, 2, 10, 40):
        t = T.Temporal(w, h)
        for f in range(FRAMES):
            lf = cam["look_from"]
            c = scenes.make_camera(dict(cam, look_from=(lf[0] + f * move, lf[1], lf[2])), w, h).c
            hi = orc.render(ps, c, w, h, SPP * f + SPP) * F(SPP * f + SPP)
            lo = orc.render(ps, c, w, h, SPP * f) * F(SPP * f) if f else np.zeros_like(hi)
            noisy = ((hi - lo) / F(SPP)).astype(F)
            g = aov_np(orc, ps, c, w, h, 4)
            color, var, hist = t.push(c, noisy, depth=g["depth"], normal=g["normal"], id=g["id"], **T.DEFAULTS)
        clean = orc.render(ps, c, w, h, REFERENCE_SPP)
        out[move] = dict(r=mse(color, clean) / mse(noisy, clean), young=float(np.mean(hist == 1)), cam=c, clean=clean, noisy=noisy)
    return out


def test_accumulated_frames_beat_the_last_noisy_frame(sequences):
    for move, s in sequences.items():
        print(f"move {move:3d}: r = {s['r']:.4f}   pixels ending with N = 1: {100 * s['young']:.2f} %")
    for move, s in sequences.items():
        assert s["r"] < min(1.0, 1.5 * RECORDED[move]), (move, s["r"], RECORDED[move])
    # the filter does not pass by rejecting everything, and disocclusion really is exercised
    assert sequences[10]["young"] <= 0.02, sequences[10]["young"]
    assert 0.02 <= sequences[40]["young"] <= 0.20, sequences[40]["young"]


def test_reseeded_frames_cannot_be_averaged(orc, sequences):
    """The same static sequence with every frame re-seeded — render(cam, 4), what pt_accum_reset or pt_render give — repeats one noise
    pattern eight times: the accumulated frame is no better than a single frame.  This is why pt_adaptive_next_frame exists."""
    w, h = 64, 40
    ps, _ = S.ALL["cornell"]()
    s = sequences[0]
    g = aov_np(orc, ps, s["cam"], w, h, 4)
    noisy = orc.render(ps, s["cam"], w, h, SPP)
    t = T.Temporal(w, h)
    for f in range(FRAMES):
        color, _, _ = t.push(s["cam"], noisy, depth=g["depth"], normal=g["normal"], id=g["id"], **T.DEFAULTS)
    r = mse(color, s["clean"]) / mse(noisy, s["clean"])
    print(f"re-seeded, move 0: r = {r:.4f}")
    assert r > 0.9
