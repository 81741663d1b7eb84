"""The image error on the GPU (include/pt_metrics.h: pt_image_error), held BIT FOR BIT to the header's restatement
(tests/metrics_model.py: numpy float32 differences, binary64 terms, exact rational sums rounded once): the sums as uint64 views, max_abs
as uint32 views, the counts, and the error plane as int32 views, under both paths — the accumulators in LDS, and global atomics only.
The frames are the smallest at which the kernels can go wrong: one pixel, one column, one row, a partial workgroup, several workgroups
(the flush across workgroups) with and without a rectangle off the 256-pixel grain, a rendered pair, magnitudes across 2^-140 ... 2^120
(terms straddling two and three accumulator words), all-ones significands (every chunk near 2^32: carries through the final fold),
subnormal differences, NaN / inf / overflowing differences (data, not faults), an all-skipped frame and a frame against itself.  Then
the property the stage exists for — a permutation of the pixels gives the same bits —, the stream contract on a non-blocking side
stream behind a slow producer (tests/stream_contract.py's harness), pt_debug_last_image_error, and the hosts: render.mse_ratio,
Accumulator.error(ref), the C++ facade and the CLI's --compare."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import metrics_model as M
import scenes_small as S
import stream_contract as SC
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F = np.float32
PATHS = pytest.mark.parametrize("no_lds", [False, True], ids=["lds", "no_lds"])


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


# ---- frames -------------------------------------------------------------------------------------------------------------------------

def lognormal(w, h, seed):
    r = np.random.default_rng(seed)
    ref = np.exp(r.normal(-1.0, 1.0, (h, w, 3))).astype(F)
    a = (ref * np.exp(r.normal(0.0, 0.3, (h, w, 3))).astype(F)).astype(F)
    a[r.random((h, w, 3)) < 0.05] = F(0)         # zero terms on one side
    same = r.random((h, w, 3)) < 0.05
    a[same] = ref[same]                          # d = +0
    return a, ref


def span(w, h, seed):
    """Magnitudes across 2^-140 ... 2^120 on both sides, either sign on `a`: |d| from subnormal to 2^121, sq from 2^-298 to 2^242, rel up
    to 2^255 — the terms land in words 0 ... 41 and straddle two and three of them."""
    r = np.random.default_rng(seed)
    a = (np.ldexp(r.random((h, w, 3)) + 1.0, r.integers(-140, 121, (h, w, 3))) * r.choice([-1.0, 1.0], (h, w, 3))).astype(F)
    ref = np.ldexp(r.random((h, w, 3)) + 1.0, r.integers(-140, 121, (h, w, 3))).astype(F)
    return a, ref


def carry(w=64, h=64):
    """Every d = 0x1.fffffep+0: all-ones significands, every pixel the same chunks near 2^32 — 4096 of them carry out of every word."""
    return np.full((h, w, 3), F(float.fromhex("0x1.fffffep+0"))), np.zeros((h, w, 3), F)


def subnormal(w, h, seed):
    """Differences that are subnormal binary32 numbers: both sides a few units of 2^-149 around the smallest normal numbers."""
    r = np.random.default_rng(seed)
    unit = 2.0 ** -149
    a = (r.integers(0, 1 << 24, (h, w, 3)) * unit).astype(F)
    ref = (a.astype(np.float64) + r.integers(-4000, 4001, (h, w, 3)) * unit).clip(0, None).astype(F)
    a[0, 0], ref[0, 0] = F(unit), F(0)           # the smallest difference there is
    d = (a - ref).astype(F)
    assert (np.abs(d) < F(2.0 ** -126)).all() and (d != 0).sum() > 0.9 * d.size  # numpy kept them
    return a, ref


def sprinkled(w, h, seed):
    """NaN, +-inf and finite values whose difference overflows, on either side, over a log-normal pair."""
    a, ref = lognormal(w, h, seed)
    r = np.random.default_rng(seed + 1)
    n = w * h
    for frame in (a, ref):
        flat = frame.reshape(n, 3)
        for v in (np.nan, np.inf, -np.inf):
            sel = np.flatnonzero(r.random(n) < 0.02)
            flat[sel, r.integers(0, 3, sel.size)] = v
    sel = np.flatnonzero(r.random(n) < 0.03)
    ch = r.integers(0, 3, sel.size)
    a.reshape(n, 3)[sel, ch] = F(3e38)
    ref.reshape(n, 3)[sel, ch] = F(-3e38)        # both finite; 3e38f - (-3e38f) is not
    a[h // 2, w // 2] = F(3e38)                  # ... and a finite giant that DOES take part (if its partner is finite)
    ref[h // 2, w // 2] = F(1.0)
    return a, ref


CASES = {
    "1x1": lambda: lognormal(1, 1, 1),
    "1x70": lambda: lognormal(1, 70, 2),
    "70x1": lambda: lognormal(70, 1, 3),
    "19x13": lambda: lognormal(19, 13, 4),
    "150x70": lambda: lognormal(150, 70, 5),
    "150x70-rect": lambda: lognormal(150, 70, 5) + ((37, 9, 141, 66),),   # off the 256-pixel grain on every side
    "19x13-empty-rect": lambda: lognormal(19, 13, 4) + ((5, 4, 5, 9),),
    "span": lambda: span(61, 37, 6),
    "carry": carry,
    "subnormal": lambda: subnormal(33, 21, 7),
    "sprinkled": lambda: sprinkled(90, 50, 8),
    "all-skipped": lambda: (np.full((9, 31, 3), np.nan, F), lognormal(31, 9, 9)[1]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(a, ref, rect, the model's result with the plane): computed once and shared by the tests of both paths."""
    a, ref, *rect = CASES[name]()
    rect = rect[0] if rect else None
    return a, ref, rect, M.image_error(a, ref, rect, plane=True)


def device_bits(e):
    """An ImageError's result as the integers the model's bits() gives."""
    raw = e.result.cpu().numpy().view(np.uint64)
    words = raw.view(np.uint32)
    return {"sum_sq": [int(v) for v in raw[0:3]], "sum_abs": [int(v) for v in raw[3:6]], "sum_rel": [int(v) for v in raw[6:9]],
            "max_abs": [int(v) for v in words[22:25]], "pixels": int(raw[9]), "skipped": int(raw[10])}


def plane_bits(p):
    return np.ascontiguousarray(p, F).view(np.int32)


def check(torch, a, ref, rect, want, no_lds, what):
    da, dr = torch.from_numpy(a).cuda(), torch.from_numpy(ref).cuda()
    e = R.image_error(da, dr, rect=rect, error_plane=True, no_lds=no_lds)
    got = device_bits(e)
    wanted = M.bits(want)
    for key in wanted:
        print(what, key, got[key], wanted[key])
    assert got == wanted, what
    assert np.array_equal(plane_bits(e.plane.cpu().numpy()), plane_bits(want["plane"])), f"{what}: the error plane"
    bare = R.image_error(da, dr, rect=rect, no_lds=no_lds)  # without the plane the walk covers the rectangle only: the same result
    assert device_bits(bare) == wanted and bare.plane is None, f"{what}: without a plane"
    return e


# ---- both paths against the model ---------------------------------------------------------------------------------------------------------

@PATHS
@pytest.mark.parametrize("name", list(CASES))
def test_shapes_and_magnitudes_on_both_paths(torch, name, no_lds):
    a, ref, rect, want = case(name)
    e = check(torch, a, ref, rect, want, no_lds, name)
    if name == "all-skipped":
        assert (e.pixels, e.skipped) == (0, 9 * 31) and e.sums() == {"sq": (0.0,) * 3, "abs": (0.0,) * 3, "rel": (0.0,) * 3}
        assert np.isnan(e.mse) and e.max_abs == (0.0, 0.0, 0.0)
    if name == "19x13-empty-rect":
        assert (e.pixels, e.skipped) == (0, 0) and np.isposinf(e.plane.cpu().numpy()).all()
    if name == "sprinkled":
        assert want["skipped"] > 100 and e.skipped == want["skipped"] and e.pixels + e.skipped == 90 * 50
        assert max(e.max_abs) == float(F(3e38) - F(1.0))  # the finite giant took part
    if name == "subnormal":
        assert 0.0 < max(e.max_abs) < 2.0 ** -126  # kept, not flushed
    if name == "carry":
        d = float.fromhex("0x1.fffffep+0")
        assert e.sums()["abs"] == (4096 * d,) * 3 and e.sums()["sq"] == (4096 * d * d,) * 3  # 4096 x a 48-bit product: exact in binary64


@PATHS
def test_a_rendered_pair(torch, no_lds):
    """R.render of the small Cornell scene at 4 and at 64 spp, 64 x 40."""
    a, ref = rendered(torch)
    want = rendered_model(torch)
    e = check(torch, a, ref, None, want, no_lds, "cornell 4 spp against 64 spp")
    assert e.mse == M.mse(want) and e.mae == M.mae(want) and e.rel_mse == M.rel_mse(want) and e.psnr() == M.psnr(want)
    assert e.pixels == 64 * 40 and e.mse > 0


_rendered = {}


def rendered(torch):
    if "pair" not in _rendered:
        ps, cam_args = S.ALL["cornell"]()
        cam = scenes.make_camera(cam_args, 64, 40)
        _rendered["pair"] = tuple(R.render(64, 40, spp, ps, cam).cpu().numpy() for spp in (4, 64))
        _rendered["scene"] = (ps, cam)
    return _rendered["pair"]


def rendered_model(torch):
    if "model" not in _rendered:
        a, ref = rendered(torch)
        _rendered["model"] = M.image_error(a, ref, plane=True)
    return _rendered["model"]


@PATHS
def test_a_frame_against_itself(torch, no_lds):
    a, _ = sprinkled(40, 30, 12)
    da = torch.from_numpy(a).cuda()
    e = R.image_error(da, da, error_plane=True, no_lds=no_lds)  # a IS ref: allowed
    want = M.image_error(a, a, plane=True)
    assert device_bits(e) == M.bits(want)
    assert e.sums() == {"sq": (0.0,) * 3, "abs": (0.0,) * 3, "rel": (0.0,) * 3} and e.max_abs == (0.0,) * 3
    assert e.skipped == int((~np.isfinite(a).all(axis=2)).sum()) > 0 and e.mse == 0.0 and e.psnr() == float("inf")
    assert np.array_equal(plane_bits(e.plane.cpu().numpy()), plane_bits(want["plane"]))


# ---- order independence -----------------------------------------------------------------------------------------------------------------

@PATHS
def test_a_permutation_of_the_pixels_gives_the_same_bits(torch, no_lds):
    """What the stage exists for: the pixels in another order reach the workgroups, the lanes and the atomics in another order, and every
    sum is the same to the bit.  (A float64 sum of the same terms differs between orders: tests/test_metrics_cpu.py.)"""
    a, ref, _, want = case("span")
    h, w, _ = a.shape
    perm = np.random.default_rng(99).permutation(h * w)
    pa = np.ascontiguousarray(a.reshape(-1, 3)[perm].reshape(h, w, 3))
    pr = np.ascontiguousarray(ref.reshape(-1, 3)[perm].reshape(h, w, 3))
    e0 = R.image_error(torch.from_numpy(a).cuda(), torch.from_numpy(ref).cuda(), no_lds=no_lds)
    e1 = R.image_error(torch.from_numpy(pa).cuda(), torch.from_numpy(pr).cuda(), no_lds=no_lds)
    assert device_bits(e0) == device_bits(e1) == M.bits(want)
    # and transposed: another width, so other pixels share a wave
    ta, tr = np.ascontiguousarray(a.transpose(1, 0, 2)), np.ascontiguousarray(ref.transpose(1, 0, 2))
    assert device_bits(R.image_error(torch.from_numpy(ta).cuda(), torch.from_numpy(tr).cuda(), no_lds=no_lds)) == M.bits(want)


def test_repeated_calls_need_no_host_step_and_report_their_path(torch, lib):
    a, ref, rect, want = case("150x70-rect")
    da, dr = torch.from_numpy(a).cuda(), torch.from_numpy(ref).cuda()
    p = abi.PtImageErrorParams()
    lib.pt_image_error_params_init(C.byref(p), 150, 70)
    p.rect_x0, p.rect_y0, p.rect_x1, p.rect_y1 = rect
    p.scratch_bytes = lib.pt_image_error_scratch_bytes()
    scratch = torch.full((p.scratch_bytes // 8,), -1, dtype=torch.int64, device="cuda")  # garbage: the call zeroes it itself
    result = torch.full((13,), -1, dtype=torch.int64, device="cuda")
    last = (C.c_int32 * 4)()
    for flags, path in ((0, 2), (abi.PT_IMAGE_ERROR_NO_LDS, 1), (0, 2), (0, 2)):  # the same scratch, call after call
        p.flags = flags
        abi.check(lib.pt_image_error(C.byref(p), C.c_void_p(da.data_ptr()), C.c_void_p(dr.data_ptr()), C.c_void_p(result.data_ptr()), None,
                                     C.c_void_p(scratch.data_ptr()), R._stream_ptr(torch)), "pt_image_error")
        assert device_bits(R.ImageError(result, None, scratch)) == M.bits(want)
        assert lib.pt_debug_last_image_error(last) == abi.PT_OK
        blocks = -(-(104 * 57) // 256)
        assert list(last) == [path, blocks, 104, 57], list(last)
    for no_lds, path in ((False, 2), (True, 1)):
        R.image_error(da, dr, no_lds=no_lds)
        lib.pt_debug_last_image_error(last)
        assert list(last) == [path, -(-(150 * 70) // 256), 150, 70]
    with pytest.raises(abi.PtError, match="rectangle"):
        R.image_error(da, dr, rect=(0, 0, 151, 70))
    with pytest.raises(ValueError, match="same shape"):
        R.image_error(da, dr[:, :100].contiguous())
    plane = torch.empty((70, 150), dtype=torch.float32, device="cuda")
    assert R.image_error(da, dr, error_plane=plane).plane is plane


# ---- the stream contract ------------------------------------------------------------------------------------------------------------------

def test_behind_pending_work_on_a_side_stream(torch):
    """pt_image_error is asynchronous on `stream`: queued on a non-blocking side stream behind the slow producer, its inputs written last,
    its plane poisoned behind the producer — the scratch it zeroes with a memset of its own on that stream —, the producer still running
    when the call has returned; what it wrote is the model's."""
    a, ref, rect, want = case("150x70")
    inp = SC.staged_inputs(torch, {"a": a, "ref": ref})
    plane = torch.empty((70, 150), dtype=torch.float32, device="cuda")
    st = SC.stream_apart_from_the_null_stream(torch)

    def call():
        return [R.image_error(inp["a"][0], inp["ref"][0], error_plane=plane).result]
    with torch.cuda.stream(st):  # warm-up on the idle stream: the first launch loads the code object, the allocator gets its blocks
        call()
    st.synchronize()
    host_ms = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        with torch.cuda.stream(st):
            call()
        host_ms = min(host_ms, (time.perf_counter() - t0) * 1e3)
        st.synchronize()
    passes = SC.passes_for(host_ms, SC.measure_pass_ms(torch))
    got, more = SC.gated(torch, st, passes, inp.values(), [plane], call)
    assert np.array_equal(plane_bits(got[0]), plane_bits(want["plane"])), "pt_image_error's plane on a side stream"
    assert device_bits(R.ImageError(torch.from_numpy(more[0]), None, None)) == M.bits(want)


# ---- hosts ----------------------------------------------------------------------------------------------------------------------------

def test_mse_ratio_and_accumulator_error(torch):
    noisy, ref = rendered(torch)
    ps, cam = _rendered["scene"]
    d_noisy, d_ref = torch.from_numpy(noisy).cuda(), torch.from_numpy(ref).cuda()
    guides = R.render_aov(64, 40, 4, ps, cam)
    filtered = R.denoise(d_noisy, albedo=guides["albedo"], normal=guides["normal"], depth=guides["depth"])
    want = M.mse(M.image_error(filtered.cpu().numpy(), ref)) / M.mse(rendered_model(torch))
    assert R.mse_ratio(filtered, d_noisy, d_ref) == want and 0.0 < want
    acc = R.Accumulator(64, 40, ps, cam)
    acc.add(4)
    assert_bit_identical(acc.resolve().cpu().numpy(), noisy, "the accumulator's frame at 4 spp")
    e = acc.error(d_ref)
    assert device_bits(e) == M.bits(rendered_model(torch)) and e.mse == M.mse(rendered_model(torch))
    part = acc.error(d_ref, rect=(3, 2, 40, 30), eps=1e-2, error_plane=True, no_lds=True)
    want = M.image_error(noisy, ref, (3, 2, 40, 30), eps=1e-2, plane=True)
    assert device_bits(part) == M.bits(want) and np.array_equal(plane_bits(part.plane.cpu().numpy()), plane_bits(want["plane"]))
    with pytest.raises(abi.PtError):
        acc.error()  # without a reference: the adaptive error estimate, which a plain accumulator does not have — as ever
    acc.close()


def test_cpp_facade(torch, tmp_path):
    exe = tmp_path / "metrics_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{libdir / 'include'}",
                    str(ROOT / "tests" / "cpp" / "metrics_main.cpp"), "-o", str(exe), f"-L{libdir}", "-lpt_render", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    a, ref, rect, want = case("150x70-rect")
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(a.tobytes() + ref.tobytes())
    p = subprocess.run([str(exe), "150", "70", *map(str, rect), str(src), str(out)], check=True, timeout=300, capture_output=True, text=True)
    raw = out.read_bytes()
    size = C.sizeof(abi.PtImageErrorResult)
    assert len(raw) == 2 * size + 150 * 70 * 4
    for at, what in ((0, "with the plane"), (size + 150 * 70 * 4, "no_lds, without")):
        res = R.ImageError(None, None, None)
        res.result = torch.from_numpy(np.frombuffer(raw, np.int64, size // 8, at).copy())
        assert device_bits(res) == M.bits(want), f"C++ pt::image_error: {what}"
    assert np.array_equal(np.frombuffer(raw, np.int32, 150 * 70, size).reshape(70, 150), plane_bits(want["plane"]))
    # the facade's derived figures: the same binary64 arithmetic (%.17g round-trips)
    m = re.search(r"MSE (\S+) MAE (\S+) relMSE (\S+) PSNR (\S+) pixels (\d+) skipped (\d+)", p.stdout)
    assert m, p.stdout
    assert [float(m.group(i)) for i in (1, 2, 3, 4)] == [M.mse(want), M.mae(want), M.rel_mse(want), M.psnr(want)]
    assert (int(m.group(5)), int(m.group(6))) == (want["pixels"], want["skipped"])


def test_cli_compare_prints_the_models_figures_and_leaves_out_png_alone(torch, tmp_path):
    base = ["--scene", "cornell", "--width", "64", "--height", "40"]

    def cli(*args):
        p = subprocess.run([sys.executable, "-m", "path_tracer_amd", *base, *args], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ), timeout=300)
        assert p.returncode == 0, p.stderr
        return p.stdout
    plain, with_option, ref_png, filtered = tmp_path / "plain.png", tmp_path / "with.png", tmp_path / "ref.png", tmp_path / "filtered.png"
    ref_npy, frame_npy = tmp_path / "ref.npy", tmp_path / "frame.npy"
    cli("--spp", "64", "--out", str(ref_png), "--save-frame", str(ref_npy))
    cli("--spp", "8", "--out", str(plain))
    text = cli("--spp", "8", "--out", str(with_option), "--compare", str(ref_npy), "--save-frame", str(frame_npy), "--denoise-out", str(filtered),
               "--aov-spp", "4")
    assert plain.read_bytes() == with_option.read_bytes()
    ps, cam_args = scenes.build("cornell")
    cam = scenes.make_camera(cam_args, 64, 40)
    ref, fb = (R.render(64, 40, spp, ps, cam) for spp in (64, 8))
    assert_bit_identical(np.load(ref_npy), ref.cpu().numpy(), "--save-frame at 64 spp")
    assert_bit_identical(np.load(frame_npy), fb.cpu().numpy(), "--save-frame at 8 spp")
    want = M.image_error(fb.cpu().numpy(), ref.cpu().numpy())
    line = (f"{with_option} vs {ref_npy}: MSE {M.mse(want)!r} relMSE {M.rel_mse(want)!r} PSNR {M.psnr(want):.4f} dB (peak 1), "
            f"{want['pixels']} pixels, {want['skipped']} skipped")
    assert line in text, text
    den = R.denoise(fb, **R.render_aov(64, 40, 4, ps, cam))
    want = M.image_error(den.cpu().numpy(), ref.cpu().numpy())
    assert f"{filtered} vs {ref_npy}: MSE {M.mse(want)!r} relMSE {M.rel_mse(want)!r} " in text, text
