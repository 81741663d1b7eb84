"""The firefly stage on the GPU (include/pt_post.h: pt_firefly), held BIT FOR BIT to the header's numpy restatement
(tests/firefly_model.py): the smallest frames, a frame one pixel past a workgroup tile in each direction, a frame higher than a launch grid's
y dimension reaches, synthetic 64 x 40 frames with spikes, NaN, +-inf, zero and negative luminance and -0 under every setting, the LDS and
PT_FIREFLY_NO_LDS paths against each other, the hosts (Accumulator.denoise, Accumulator.denoise_variance, render_temporal with and without
the `firefly` keyword), the stream contract on a non-blocking side stream behind a slow producer (tests/stream_contract.py's harness), the
C++ facade and the CLI."""
import ctypes as C
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import denoise_model as M
import firefly_model as FM
import scenes_small as S
import stream_contract as SC
import temporal_model as T
import variance_model as V
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from test_gpu_denoise import read_png
from test_gpu_temporal import STEPS, moving_cameras

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F = np.float32
TW, TH = abi.PT_FIREFLY_TILE_W, abi.PT_FIREFLY_TILE_H


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


# ---- frames -------------------------------------------------------------------------------------------------------------------------

def synthetic(w, h, seed):
    """(colour, variance): log-normal values; 2 % spikes; 1 % pixels with a NaN, +inf or -inf channel; a few pixels of zero and of negative
    luminance and -0 channels; lone spikes in the four corners and in the last and first row and column on either side of a tile
    boundary (BOUNDARY_SPIKES, as far as the frame reaches), none of them another's neighbour."""
    r = np.random.default_rng(seed)
    c = np.exp(r.normal(0.0, 1.0, (h, w, 3))).astype(F)
    spikes = r.random((h, w)) < 0.02
    c[spikes] *= np.exp(r.uniform(3.0, 9.0, (int(spikes.sum()), 1))).astype(F)
    dark = r.random((h, w))
    c[dark < 0.01] = [F(0), F(-0.0), F(0)]
    c[(dark >= 0.01) & (dark < 0.02)] = [F(-2), F(-1), F(0.5)]
    c[(dark >= 0.02) & (dark < 0.03), 1] = F(-0.0)
    if w * h > 4:
        c[h // 2, w // 2] = [F(3e38), F(3e38), F(3e38)]  # finite channels whose luminance overflows
    bad = r.random((h, w))
    for lo, v in ((0.0, np.nan), (0.004, np.inf), (0.007, -np.inf)):
        sel = np.argwhere((bad >= lo) & (bad < lo + 0.0035))
        c[sel[:, 0], sel[:, 1], r.integers(0, 3, len(sel))] = v
    for y, x in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)] + BOUNDARY_SPIKES:
        if y < h and x < w:
            c[y, x] = [F(4e5), F(2e5), F(1e5)]
    if 2 <= w * h <= 64:
        c[0, 0, 1] = np.nan  # the smallest frames have a pixel to repair as well
    if w > TW + 3 and h > TH:
        c[TH - 1, TW + 3] = c[TH, TW + 3] = [F(5e6), F(5e6), F(5e6)]  # two equal spikes across a boundary: they survive rank 1
    v = np.exp(r.normal(-2.0, 1.0, (h, w, 3))).astype(F)
    v[r.random((h, w)) < 0.02] = [np.inf, np.nan, F(-1)]  # a variance value is never tested
    return c, v


BOUNDARY_SPIKES = [(TH - 1, TW - 1), (TH, TW + 1), (TH + 2, TW), (TH - 1, TW + 6)]  # a tile's last pixel; the next tiles' first row, first column; a last row
_frames = {}


def frame(w, h, seed=1):
    if (w, h, seed) not in _frames:
        c, v = synthetic(w, h, seed)
        c.setflags(write=False)
        v.setflags(write=False)
        _frames[w, h, seed] = (c, v)
    return _frames[w, h, seed]


def last_firefly(lib=None):
    out = (C.c_int32 * 4)()
    abi.check((lib or abi.load_library()).pt_debug_last_firefly(out), "pt_debug_last_firefly")
    return list(out)


def run(torch, c, v=None, *, alias=False, **kw):
    """firefly() on the device -> (out, variance_out or None, (clamped, repaired)) as numpy, like the model's result."""
    fb = torch.from_numpy(np.array(c, dtype=F)).cuda()  # (a copy: the shared frames are read-only)
    var = torch.from_numpy(np.array(v, dtype=F)).cuda() if v is not None else None
    res = R.firefly(fb, var, counts=True, variance_out=var if alias else None, **kw)
    torch.cuda.synchronize()
    assert_bit_identical(fb.cpu().numpy(), c, "the input frame is left alone")
    if var is not None:
        assert (res[1] is var) == alias
    n = tuple(int(x) for x in res[-1].cpu().numpy())
    return res[0].cpu().numpy(), res[1].cpu().numpy() if var is not None else None, n


def check(torch, c, v, what, **kw):
    want = FM.firefly(c, v, **{k: a for k, a in kw.items() if k in ("rank", "k", "repair")})
    got = run(torch, c, v, **kw)
    assert_bit_identical(got[0], want[0], f"{what}: colour")
    if v is not None:
        assert_bit_identical(got[1], want[1], f"{what}: variance")
    else:
        assert got[1] is None
    assert got[2] == want[2], f"{what}: counts {got[2]} against the model's {want[2]}"
    return want


# ---- the kernel against the model -----------------------------------------------------------------------------------------------------

SMALL = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (TW + 1, TH + 1), (2 * TW, 2 * TH)]


@pytest.mark.parametrize("no_lds", [False, True], ids=["lds", "no_lds"])
@pytest.mark.parametrize("w,h", SMALL, ids=[f"{w}x{h}" for w, h in SMALL])
def test_small_frames_and_one_pixel_past_a_tile(torch, w, h, no_lds):
    c, v = frame(w, h, 3)
    for rank in (1, 2):
        check(torch, c, v, f"{w} x {h}, rank {rank}", rank=rank, no_lds=no_lds)
        assert last_firefly() == [1 if no_lds else 2, (w + TW - 1) // TW, (h + TH - 1) // TH, 2]
    nans = np.full((h, w, 3), np.nan, F)
    out, _, n = run(torch, nans, no_lds=no_lds)
    assert np.isnan(out).all() and n == (0, 0)  # nothing to repair from


@pytest.mark.parametrize("variance", [True, False], ids=["variance", "no_variance"])
@pytest.mark.parametrize("repair", [True, False], ids=["repair", "no_repair"])
@pytest.mark.parametrize("k", [1.0, 2.5])
@pytest.mark.parametrize("rank", [1, 2])
def test_synthetic_frames_under_every_setting(torch, rank, k, repair, variance):
    w, h = 64, 40
    c, v = frame(w, h)
    want = check(torch, c, v if variance else None, f"rank {rank}, k {k}, repair {repair}", rank=rank, k=k, repair=repair)
    clamped, repaired = want[2]
    assert clamped > 10 and (repaired > 10) == repair  # the frame exercises both
    assert last_firefly()[3] == (2 if variance else 1)
    if rank == 1 and k == 1.0:
        assert_bit_identical(want[0][TH - 1:TH + 1, TW + 3], c[TH - 1:TH + 1, TW + 3], "two equal spikes across a tile boundary survive rank 1")
        for y, x in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)] + BOUNDARY_SPIKES:
            assert want[0][y, x, 0] < c[y, x, 0], (y, x)  # the corner and boundary spikes come down


def test_variance_in_place_and_paths_agree(torch):
    w, h = 64, 40
    c, v = frame(w, h)
    for kw in (dict(rank=1, k=1.0), dict(rank=2, k=2.5, repair=False)):
        apart = run(torch, c, v, **kw)
        assert last_firefly()[0] == 2
        aliased = run(torch, c, v, alias=True, **kw)
        no_lds = run(torch, c, v, no_lds=True, **kw)
        assert last_firefly()[0] == 1
        for other, what in ((aliased, "variance_out aliasing variance"), (no_lds, "PT_FIREFLY_NO_LDS")):
            assert_bit_identical(other[0], apart[0], f"{what}: colour")
            assert_bit_identical(other[1], apart[1], f"{what}: variance")
            assert other[2] == apart[2], what


def test_a_frame_higher_than_a_grid_dimension(torch):
    """2 x (8 x 65536 + 3): 65537 rows of workgroups — more than the 65535 a launch grid's y dimension holds; the kernel's grid is linear."""
    w, h = 2, TH * 65536 + 3
    c, v = frame(w, h, 5)
    check(torch, c, None, f"{w} x {h}")
    assert last_firefly()[:3] == [2, 1, 65537]


def test_refusals_with_live_planes(torch):
    c, v = frame(9, 7, 3)
    fb = torch.from_numpy(c.copy()).cuda()
    with pytest.raises(abi.PtError, match="overlap"):
        R.firefly(fb, out=fb)
    with pytest.raises(ValueError, match="variance_out needs variance"):
        R.firefly(fb, variance_out=torch.empty_like(fb))
    with pytest.raises(ValueError, match="counts"):
        R.firefly(fb, counts=torch.empty(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(abi.PtError, match="rank"):
        R.firefly(fb, rank=3)
    with pytest.raises(ValueError, match="whole frame"):
        R.firefly(fb.reshape(-1, 3))


# ---- hosts ----------------------------------------------------------------------------------------------------------------------------

W, H, SPP, AOV_SPP = 64, 40, 4, 4
DENOISE_KW = dict(iterations=2)


@pytest.fixture(scope="module")
def cornell(torch):
    ps, cam_args = S.ALL["cornell"]()
    ds = R.DeviceScene(ps)
    yield ds, moving_cameras(cam_args, W, H, 2, STEPS["cornell"])
    torch.cuda.synchronize()
    ds.close()


def host(d):
    return {k: t.cpu().numpy() for k, t in d.items()}


def test_accumulator_denoise_with_and_without_the_keyword(torch, cornell):
    ds, cams = cornell
    acc = R.Accumulator(W, H, ds, cams[0])
    acc.add(SPP)
    noisy = acc.resolve().cpu().numpy()
    g = host(R.render_aov(W, H, AOV_SPP, ds, cams[0], planes=("albedo", "normal", "depth")))
    clamped, _, (n_clamped, _) = FM.firefly(noisy)
    assert n_clamped > 20  # a 4 spp Cornell frame has its fireflies
    want = M.denoise(clamped, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **dict(M.DEFAULTS, **DENOISE_KW))
    assert_bit_identical(acc.denoise(AOV_SPP, firefly=True, **DENOISE_KW).cpu().numpy(), want, "Accumulator.denoise(firefly=True)")
    want2 = M.denoise(FM.firefly(noisy, rank=2, k=2.0)[0], albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **dict(M.DEFAULTS, **DENOISE_KW))
    assert_bit_identical(acc.denoise(AOV_SPP, firefly=dict(rank=2, k=2.0), **DENOISE_KW).cpu().numpy(), want2, "Accumulator.denoise(firefly={...})")
    plain = M.denoise(noisy, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **dict(M.DEFAULTS, **DENOISE_KW))
    assert_bit_identical(acc.denoise(AOV_SPP, **DENOISE_KW).cpu().numpy(), plain, "Accumulator.denoise without the keyword: today's bits")
    assert_bit_identical(acc.denoise(AOV_SPP, firefly=None, **DENOISE_KW).cpu().numpy(), plain, "firefly=None")
    with pytest.raises(TypeError, match="firefly"):
        acc.denoise(AOV_SPP, firefly=dict(radius=2))
    acc.close()


def test_accumulator_denoise_variance_with_and_without_the_keyword(torch, cornell):
    ds, cams = cornell
    acc = R.Accumulator(W, H, ds, cams[0], adaptive=True)
    acc.add(SPP - SPP // 2).add(SPP // 2)
    noisy, var = acc.resolve().cpu().numpy(), acc.variance().cpu().numpy()
    g = host(R.render_aov(W, H, AOV_SPP, ds, cams[0], planes=("albedo", "normal", "depth")))
    kw = dict(V.DEFAULTS, **DENOISE_KW)
    clamped, cvar, _ = FM.firefly(noisy, var)
    want = V.denoise(clamped, cvar, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **kw)[0]
    assert_bit_identical(acc.denoise_variance(AOV_SPP, firefly=True, **DENOISE_KW).cpu().numpy(), want, "Accumulator.denoise_variance(firefly=True)")
    plain = V.denoise(noisy, var, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **kw)[0]
    assert_bit_identical(acc.denoise_variance(AOV_SPP, **DENOISE_KW).cpu().numpy(), plain, "Accumulator.denoise_variance without the keyword: today's bits")
    acc.close()


def by_hand(ds, cams):
    """render_temporal's frames up to the push, from the device: per camera (noisy, variance estimate, guides) as numpy."""
    acc, out = None, []
    for cam in cams:
        if acc is None:
            acc = R.Accumulator(W, H, ds, cam, adaptive=True)
        else:
            acc.next_frame(cam)
        acc.add(SPP - SPP // 2).add(SPP // 2)
        out.append((acc.resolve().cpu().numpy(), acc.variance().cpu().numpy(),
                    host(R.render_aov(W, H, AOV_SPP, ds, cam, planes=("albedo", "normal", "depth", "id")))))
    acc.close()
    return out


def chained(cams, inputs, clamp):
    """The models chained on the host the way stream_contract.chain_expected chains them: firefly -> temporal -> filter."""
    hist, frames = T.Temporal(W, H), []
    for cam, (noisy, var, g) in zip(cams, inputs):
        fr = dict(noisy=noisy)
        if clamp is not None:
            fr["clamped"], var, fr["firefly_counts"] = FM.firefly(noisy, var, **clamp)
        fr["temporal"], fr["variance"], fr["history"] = hist.push(cam.c, fr.get("clamped", noisy), g["depth"], normal=g["normal"], id=g["id"],
                                                                  variance_in=var, **T.DEFAULTS)
        fr["filtered"] = V.denoise(fr["temporal"], fr["variance"], albedo=g["albedo"], normal=g["normal"], depth=g["depth"],
                                   **dict(V.DEFAULTS, **DENOISE_KW))[0]
        frames.append(fr)
    return frames


@pytest.mark.parametrize("firefly", [None, True, dict(rank=2, k=2.0, repair=False)], ids=["absent", "defaults", "rank2_k2"])
def test_render_temporal_with_and_without_the_keyword(torch, cornell, firefly):
    ds, cams = cornell
    clamp = None if firefly is None else {} if firefly is True else firefly
    want = chained(cams, by_hand(ds, cams), clamp)
    extra = {} if firefly is None else dict(firefly=firefly)
    got = [dict(fr) for fr in R.render_temporal(W, H, SPP, ds, cams, aov_spp=AOV_SPP, denoise_kw=DENOISE_KW, **extra)]
    assert len(got) == len(want) == 2
    for f, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b), (f, sorted(a), sorted(b))  # without the keyword: no `clamped`, no `firefly_counts`
        for key in b:
            if key == "firefly_counts":
                assert tuple(int(x) for x in a[key].cpu().numpy()) == b[key], (f, key)
                assert b[key][0] > 20
            else:
                assert_bit_identical(a[key].cpu().numpy(), b[key], f"render_temporal(firefly={firefly}) frame {f}: {key}")


# ---- the stream contract ------------------------------------------------------------------------------------------------------------------

def test_firefly_behind_pending_work_on_a_side_stream(torch):
    """pt_firefly is asynchronous on `stream`: queued on a non-blocking side stream behind the slow producer, its inputs written last, its
    outputs — the counts included, which the call zeroes with a memset of its own — poisoned behind the producer, the producer still running
    when the call has returned; what it wrote is the model's."""
    w, h = 70, 45
    c, v = frame(w, h, 7)
    inp = SC.staged_inputs(torch, dict(color=c.copy(), variance=v.copy()))
    out, vout = (torch.empty((h, w, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    counts = torch.empty(2, dtype=torch.int32, device="cuda")
    st = SC.stream_apart_from_the_null_stream(torch)

    def call():
        R.firefly(inp["color"][0], inp["variance"][0], rank=2, k=1.0, out=out, variance_out=vout, counts=counts)
    with torch.cuda.stream(st):  # warm-up on the idle stream: the first launch loads the code object
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
    got, _ = SC.gated(torch, st, passes, inp.values(), [out, vout, counts], call)
    want = FM.firefly(c, v, rank=2, k=1.0)
    assert_bit_identical(got[0], want[0], "pt_firefly on a side stream: colour")
    assert_bit_identical(got[1], want[1], "pt_firefly on a side stream: variance")
    assert tuple(int(x) for x in got[2]) == want[2]


# ---- the C++ facade and the CLI -------------------------------------------------------------------------------------------------------------

def test_cpp_facade(torch, tmp_path):
    exe = tmp_path / "firefly_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{libdir / 'include'}",
                    str(ROOT / "tests" / "cpp" / "firefly_main.cpp"), "-o", str(exe), f"-L{libdir}", "-lpt_render", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    w, h = 64, 40
    c, v = frame(w, h)
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(c.tobytes() + v.tobytes())
    subprocess.run([str(exe), str(w), str(h), "2", "2.5", "1", str(src), str(out)], check=True, timeout=300)
    raw = out.read_bytes()
    n3 = w * h * 3
    assert len(raw) == 4 * n3 * 4 + 8
    want = FM.firefly(c, v, rank=2, k=2.5, repair=True)
    plane = lambda at: np.frombuffer(raw, F, n3, at).reshape(h, w, 3)  # noqa: E731
    assert_bit_identical(plane(0), want[0], "C++ pt::firefly: colour")
    assert_bit_identical(plane(n3 * 4), want[1], "C++ pt::firefly: variance")
    assert tuple(int(x) for x in np.frombuffer(raw, np.uint32, 2, 2 * n3 * 4)) == want[2]
    assert_bit_identical(plane(2 * n3 * 4 + 8), want[0], "C++ pt::firefly, variance in place: colour")
    assert_bit_identical(plane(3 * n3 * 4 + 8), want[1], "C++ pt::firefly, variance in place: variance")


def test_cli_clamps_what_the_display_stage_shows_and_leaves_out_png_alone(torch, tmp_path):
    import display_model as D
    base = ["--scene", "cornell", "--width", "64", "--height", "40", "--spp", "4"]

    def cli(*args):
        p = subprocess.run([sys.executable, "-m", "path_tracer_amd", *base, *args], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ), timeout=300)
        assert p.returncode == 0, p.stderr
        return p.stdout
    plain, with_clamp, shown = tmp_path / "plain.png", tmp_path / "with.png", tmp_path / "shown.png"
    cli("--out", str(plain))
    text = cli("--out", str(with_clamp), "--firefly-clamp", "--firefly-rank", "2", "--display-out", str(shown), "--tone", "reference")
    assert plain.read_bytes() == with_clamp.read_bytes()
    ps, cam_args = scenes.build("cornell")
    fb = R.render(64, 40, 4, ps, scenes.make_camera(cam_args, 64, 40)).cpu().numpy()
    clamped, _, (n_clamped, n_repaired) = FM.firefly(fb, rank=2)
    assert np.array_equal(read_png(shown), D.apply(clamped, F(0.0), D.REFERENCE)[0])
    assert f"{n_clamped} pixels clamped, {n_repaired} repaired" in text and n_clamped > 20
