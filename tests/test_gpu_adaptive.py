"""Adaptive sampling on the GPU (include/pt_render.h: pt_adaptive_*; path_tracer_amd/render.py: Accumulator(adaptive=True),
render_adaptive).

The contract: after any sequence of windows, masked or not, pixel p resolves to the bits pt_render gives at p with samples = n_p — on
every kernel family, with and without the cost probe, for shards and across a checkpoint; pixels outside a window's mask keep their sum,
generator state and counts bit for bit.  Comparisons are int32 views (bit for bit); sampled pixels are also checked against the CPU
oracle.  The error estimate and the selection rule are held to the numpy restatement of tests/test_adaptive_cpu.py."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import scenes_small as S
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from test_adaptive_cpu import book_np, error_np, select_np

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def same(a, b, what=""):
    import torch
    assert a.shape == b.shape, what
    eq = a.view(torch.int32) == b.view(torch.int32)
    assert bool(eq.all()), f"{what}: {int((~eq).sum())} of {eq.numel()} values differ"


def unpack(acc):
    """An exported adaptive state: (header words, sums [P][3], rng [R], H [P][3], n [P], a [P])."""
    st = acc.state()
    lib = abi.load_library()
    F = lib.pt_framebuffer_floats(C.byref(acc._p))
    P = F // 3
    R_ = lib.pt_shard_tiles(C.byref(acc._p)) * 64
    o = abi.PT_ACCUM_HEADER_BYTES
    hdr = np.frombuffer(st[:40].tobytes(), dtype="<i4")
    sums = np.frombuffer(st[o:o + 4 * F].tobytes(), dtype=np.float32).reshape(P, 3)
    rng = np.frombuffer(st[o + 4 * F:o + 4 * F + 4 * R_].tobytes(), dtype=np.uint32)
    o2 = o + 4 * F + 4 * R_
    H = np.frombuffer(st[o2:o2 + 4 * F].tobytes(), dtype=np.float32).reshape(P, 3)
    n = np.frombuffer(st[o2 + 4 * F:o2 + 4 * F + 4 * P].tobytes(), dtype=np.int32)
    a = np.frombuffer(st[o2 + 4 * F + 4 * P:].tobytes(), dtype=np.int32)
    assert len(a) == P
    return hdr, sums, rng, H, n, a


def rng_index(W, H, shard_count=1, shard_index=0):
    """Per pixel of the per-pixel layout: its index in the generator-state array (local tile * 64 + ly * 8 + lx)."""
    if shard_count == 1:
        y, x = np.mgrid[0:H, 0:W]
        tx = (W + 7) // 8
        return (((y // 8) * tx + x // 8) * 64 + (y % 8) * 8 + x % 8).reshape(-1)
    tiles = -(-((W + 7) // 8) * ((H + 7) // 8) // shard_count)
    return np.arange(tiles * 64)


def valid_pixels(W, H, shard_count=1, shard_index=0):
    if shard_count == 1:
        return np.ones(W * H, dtype=bool)
    tx, nt = (W + 7) // 8, ((W + 7) // 8) * ((H + 7) // 8)
    tiles = -(-nt // shard_count)
    i = np.arange(tiles * 64)
    g = (i // 64) * shard_count + shard_index
    x, y = (g % tx) * 8 + (i % 64) % 8, (g // tx) * 8 + (i % 64) // 8
    return (g < nt) & (x < W) & (y < H)


def bits_eq(x, y):
    """float32 arrays equal bit for bit (any NaN matches any NaN: a NaN's payload is not semantics)."""
    x, y = np.asarray(x), np.asarray(y)
    return (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))


def check_per_pixel(torch, ds, W, H, c, fb, counts, what, flags=0, si=0, sc=1):
    """Each pixel equals pt_render at its own count (one render per distinct count); count 0 resolves to 0."""
    cnt = counts.cpu().numpy().reshape(-1)
    got = fb.reshape(-1, 3)
    for k in np.unique(cnt):
        sel = torch.from_numpy(np.nonzero(cnt == k)[0]).cuda()
        if k == 0:
            assert not bool(got[sel].view(torch.int32).any()), f"{what}: pixels at 0 samples are not 0"
            continue
        ref = R.render(W, H, int(k), ds, c, flags=flags, shard_index=si, shard_count=sc).reshape(-1, 3)
        same(got[sel], ref[sel], f"{what}: pixels at {k} spp")


def random_mask(torch, shape, frac, seed):
    g = np.random.default_rng(seed)
    return torch.from_numpy((g.random(shape) < frac).astype(np.uint8)).cuda()


def mask_sequence(torch, shape, si=0, sc=1):
    """(samples, mask | None) windows: a plain one, random 30 %, a rectangle, one pixel, an empty mask, a full mask, a plain one, random."""
    m_rect = np.zeros(shape, dtype=np.uint8)
    m_rect[shape[0] // 4:shape[0] // 2 + 1, shape[1] // 3:shape[1] // 3 + max(1, shape[1] // 4)] = 1
    m_one = np.zeros(shape, dtype=np.uint8)
    m_one[shape[0] // 2, shape[1] // 2] = 1
    T = lambda m: torch.from_numpy(m).cuda()  # noqa: E731
    return [(16, None), (4, random_mask(torch, shape, 0.3, 1)), (8, T(m_rect)), (3, T(m_one)), (5, T(np.zeros(shape, dtype=np.uint8))),
            (2, T(np.ones(shape, dtype=np.uint8))), (16, None), (4, random_mask(torch, shape, 0.3, 2).bool())]


def run_sequence(torch, ds, W, H, c, seq, what, flags=0, si=0, sc=1, first=None):
    """Runs the windows on a new adaptive accumulator, checking the bookkeeping and that pixels outside a mask keep their state."""
    acc = R.Accumulator(W, H, ds, c, flags=flags, shard_index=si, shard_count=sc, adaptive=True)
    shape = acc._pixel_shape()
    valid = valid_pixels(W, H, sc, si)
    ridx = rng_index(W, H, sc, si)
    n_host = np.zeros(int(np.prod(shape)), dtype=np.int64)
    plain = 0
    for k, (w, m) in enumerate(first or seq):
        before = unpack(acc)
        acc.add(w, m)
        after = unpack(acc)
        on = valid if m is None else (m.cpu().numpy().reshape(-1) != 0) & valid
        n_host[on] += w
        plain += w if m is None else 0
        _, s0, r0, h0, n0, a0 = before
        _, s1, r1, h1, n1, a1 = after
        assert (n1 == n_host).all(), f"{what} window {k}: counts differ from the host's bookkeeping"
        assert acc.samples == plain, f"{what} window {k}: pt_accum_samples"
        off = ~on
        for nm, x0, x1 in (("sum", s0[off], s1[off]), ("H", h0[off], h1[off]), ("a", a0[off], a1[off]),
                           ("rng", r0[ridx[off]], r1[ridx[off]])):
            assert (x0.view(np.uint32) == x1.view(np.uint32)).all(), f"{what} window {k}: {nm} changed outside the mask"
        # the window's bookkeeping = the restatement from the states before and after it
        hb, nb, ab = book_np(s0, s1, h0, n0, a0, w, None if m is None else on)
        assert bits_eq(hb, h1).all() and (nb == n1).all() and (ab == a1).all(), f"{what} window {k}: bookkeeping"
    return acc


@pytest.mark.parametrize("name", list(S.ALL))
def test_small_frames_masked_windows(torch, name):
    ps, cam = S.ALL[name]()
    W, H = 32, 18
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    acc = run_sequence(torch, ds, W, H, c, mask_sequence(torch, (H, W)), name)
    check_per_pixel(torch, ds, W, H, c, acc.resolve(), acc.counts(), name)
    acc.close()


PROBED = [("cornell", 256, 192), ("sphere_field", 640, 400), ("mixed", 192, 128)]
VARIANTS = [("default", 0, None), ("force_coop", abi.PT_FLAG_FORCE_COOP, None), ("force_stream", abi.PT_FLAG_FORCE_STREAM, None),
            ("no_lds", abi.PT_FLAG_NO_LDS, None), ("pixel_granular", abi.PT_FLAG_PIXEL_GRANULAR, None), ("no_lpt", abi.PT_FLAG_NO_LPT, None),
            ("probe_resume_off", 0, dict(probe_resume=-1))]  # (the probe only costs, from the seeds; the window resumes from the state)


@pytest.mark.parametrize("name,W,H", PROBED, ids=[p[0] for p in PROBED])
def test_masked_windows_every_kernel_family(torch, name, W, H):
    ps, cam = scenes.build("cornell") if name == "cornell" else S.ALL[name]()
    c = scenes.make_camera(cam, W, H)
    for vname, flags, tun in VARIANTS:
        ds = R.DeviceScene(ps, tuning=abi.tuning(**tun) if tun else None)
        acc = run_sequence(torch, ds, W, H, c, mask_sequence(torch, (H, W)), f"{name} {vname}", flags=flags)
        check_per_pixel(torch, ds, W, H, c, acc.resolve(), acc.counts(), f"{name} {vname}", flags=flags)
        acc.close()


def test_triangle_pool_cache_binned(torch, orc):
    ps, cam = scenes.build("triangles", n_triangles=20_000)
    W, H = 160, 96
    c = scenes.make_camera(cam, W, H)
    seq = [(4, None), (3, random_mask(torch, (H, W), 0.3, 3)), (2, None), (5, random_mask(torch, (H, W), 0.1, 4))]
    for what, tun in (("pool", None), ("pool no cache", dict(tri_cache=-1)), ("binned", dict(tri_binned=1))):
        ds = R.DeviceScene(ps, tuning=abi.tuning(**tun) if tun else None)
        acc = run_sequence(torch, ds, W, H, c, seq, f"triangles {what}")
        fb, counts = acc.resolve(), acc.counts()
        check_per_pixel(torch, ds, W, H, c, fb, counts, f"triangles {what}")
        acc.close()
    orc.set_math(True)
    xy = np.stack(np.meshgrid(np.arange(0, W, 13), np.arange(0, H, 11)), -1).reshape(-1, 2).astype(np.int32)
    cnt = counts.cpu().numpy()
    f = fb.cpu().numpy()
    for k in np.unique(cnt[xy[:, 1], xy[:, 0]]):
        sel = xy[cnt[xy[:, 1], xy[:, 0]] == k]
        assert_bit_identical(f[sel[:, 1], sel[:, 0]], orc.render_pixels(ps, c.c, W, H, int(k), sel), f"triangles at {k} spp vs oracle")


def test_shard_local_masks(torch):
    ps, cam = scenes.build("cornell")
    W, H, si, sc = 256, 192, 1, 3
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    tiles = -(-((W + 7) // 8) * ((H + 7) // 8) // sc)
    seq = mask_sequence(torch, (tiles, 64))
    acc = run_sequence(torch, ds, W, H, c, seq, "shard 1 of 3", si=si, sc=sc)
    check_per_pixel(torch, ds, W, H, c, acc.resolve(), acc.counts(), "shard 1 of 3", si=si, sc=sc)
    with pytest.raises(abi.PtError) as e:  # dilation needs whole frames
        acc.select(0.1, 16, 64, dilate=True)
    assert e.value.code == abi.PT_ERR_INVALID_ARG
    mask, k = acc.select(-1.0, 16, 64, dilate=False)
    assert k == int(valid_pixels(W, H, sc, si).sum())
    acc.close()


def test_estimator_and_select_match_the_restatement(torch):
    ps, cam = scenes.build("cornell")
    W, H = 96, 64
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    acc = R.Accumulator(W, H, ds, c, adaptive=True)
    acc.add(8).add(8).add(4, random_mask(torch, (H, W), 0.5, 5)).add(8)
    _, s, _, h, n, a = unpack(acc)
    err = acc.error().cpu().numpy().reshape(-1)
    want = error_np(s, h, n, a)
    assert bits_eq(err, want).all()
    assert np.isfinite(err).all()  # (every pixel has samples in both halves here)
    for thr in (0.02, 0.1, 0.5, -1.0):
        for dil in (False, True):
            for lo, hi in ((16, 64), (30, 32), (40, 64)):
                mask, k = acc.select(thr, lo, hi, dilate=dil)
                wm, wk = select_np(s.reshape(H, W, 3), h.reshape(H, W, 3), n.reshape(H, W), a.reshape(H, W), thr, lo, hi, dil)
                assert k == wk and (mask.cpu().numpy() == wm).all(), (thr, dil, lo, hi)
    acc.close()


def test_render_adaptive(torch, orc):
    ps, cam = scenes.build("cornell")
    W, H = 320, 180
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    fb, counts = R.render_adaptive(W, H, ds, c, threshold=-1.0, min_spp=16, max_spp=64, step=16)
    same(fb, R.render(W, H, 64, ds, c), "negative threshold = pt_render(max_spp)")
    assert bool((counts == 64).all())
    fb, counts = R.render_adaptive(W, H, ds, c, threshold=0.05, min_spp=16, max_spp=128, step=16)
    cnt = counts.cpu().numpy()
    assert cnt.min() >= 16 and cnt.max() <= 128 and ((cnt - 16) % 16 == 0).all()
    assert len(np.unique(cnt)) > 1, "a positive threshold left every pixel at the same count"
    check_per_pixel(torch, ds, W, H, c, fb, counts, "render_adaptive 0.05")
    orc.set_math(True)
    g = np.random.default_rng(11)
    xy = np.stack([g.integers(0, W, 200), g.integers(0, H, 200)], axis=1).astype(np.int32)
    f = fb.cpu().numpy()
    for k in np.unique(cnt[xy[:, 1], xy[:, 0]]):
        sel = xy[cnt[xy[:, 1], xy[:, 0]] == k]
        assert_bit_identical(f[sel[:, 1], sel[:, 0]], orc.render_pixels(ps, c.c, W, H, int(k), sel), f"render_adaptive at {k} spp vs oracle")
    with pytest.raises(ValueError):
        R.render_adaptive(W, H, ds, c, threshold=0.1, min_spp=16, max_spp=100, step=16)


def test_checkpoints(torch, tmp_path):
    ps, cam = S.mixed_scene()
    W, H = 192, 128
    c = scenes.make_camera(cam, W, H)
    seq = [(8, None), (4, random_mask(torch, (H, W), 0.4, 7)), (16, None), (6, random_mask(torch, (H, W), 0.2, 8)), (3, None)]
    acc = R.Accumulator(W, H, R.DeviceScene(ps), c, adaptive=True)
    for w, m in seq:
        acc.add(w, m)
    want, want_n = acc.resolve(), acc.counts()
    acc.close()
    acc = R.Accumulator(W, H, R.DeviceScene(ps), c, adaptive=True)
    for w, m in seq[:2]:
        acc.add(w, m)
    path = tmp_path / "st.bin"
    acc.save(path)
    assert path.stat().st_size == abi.load_library().pt_adaptive_state_bytes(C.byref(abi.PtRenderParams(W, H, 0, 50, 0, 1, 0, 0)))
    acc.close()
    acc2 = R.Accumulator.load(path, R.DeviceScene(ps))
    assert acc2.adaptive and acc2.samples == 8
    for w, m in seq[2:]:
        acc2.add(w, m)
    same(acc2.resolve(), want, "adaptive checkpoint resumed in a new accumulator")
    assert torch.equal(acc2.counts(), want_n)
    acc2.close()
    # a plain (format 1) checkpoint continued adaptively
    plain = R.Accumulator(W, H, R.DeviceScene(ps), c)
    plain.add(8)
    plain.save(tmp_path / "plain.bin")
    plain.close()
    up = R.Accumulator.load(tmp_path / "plain.bin", R.DeviceScene(ps), adaptive=True)
    assert up.adaptive and up.samples == 8
    for w, m in seq[1:]:
        up.add(w, m)
    same(up.resolve(), want, "plain checkpoint upgraded and continued adaptively")
    assert torch.equal(up.counts(), want_n)
    up.close()
    # a plain state at 0 samples upgrades too (the generator states are the seeds)
    zero = R.Accumulator(W, H, R.DeviceScene(ps), c)
    z = R.Accumulator(W, H, R.DeviceScene(ps), c, adaptive=True)
    z.restore(zero.state())
    for w, m in seq:
        z.add(w, m)
    same(z.resolve(), want, "plain state at 0 samples upgraded")
    for a_ in (zero, z):
        a_.close()


def test_rejections_and_output_paths(torch, tmp_path):
    ps, cam = scenes.build("cornell")
    W, H = 96, 64
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    m = random_mask(torch, (H, W), 0.3, 9)
    plain = R.Accumulator(W, H, ds, c)
    with pytest.raises(abi.PtError) as e:
        plain.add(4, m)
    assert e.value.code == abi.PT_ERR_INVALID_ARG
    acc = R.Accumulator(W, H, ds, c, adaptive=True)
    for f in (acc.resolve, acc.tonemap_rgb8, lambda: acc.add(0), lambda: acc.add(-2, m)):
        with pytest.raises(abi.PtError) as e:
            f()
        assert e.value.code == abi.PT_ERR_INVALID_ARG
    acc.add(5).add(7, m)
    lib = abi.load_library()
    buf = np.empty(lib.pt_accum_state_bytes(C.byref(acc._p)), dtype=np.uint8)
    assert lib.pt_accum_export(acc.handle, buf.ctypes.data_as(C.c_void_p), buf.size, None) == abi.PT_ERR_INVALID_ARG
    assert lib.pt_accum_import(acc.handle, buf.ctypes.data_as(C.c_void_p), buf.size, None) == abi.PT_ERR_INVALID_ARG
    st = acc.state()
    fresh = R.Accumulator(W, H, ds, c, adaptive=True)
    for bad in (st[:-4], np.concatenate([st, st[:4]])):
        with pytest.raises(abi.PtError):
            fresh.restore(bad)
    wrong = st.copy()
    wrong[4] = 3  # format 3
    with pytest.raises(abi.PtError):
        fresh.restore(wrong)
    neg = st.copy()
    o = len(st) - 4 * W * H
    neg[o:o + 4] = np.frombuffer(np.int32(999).tobytes(), dtype=np.uint8)  # a > n
    with pytest.raises(abi.PtError):
        fresh.restore(neg)
    with pytest.raises(abi.PtError):
        plain.restore(st)  # a plain accumulator refuses format 2
    acc.cam = scenes.make_camera(dict(scenes.build("cornell")[1], vfov=41.0), W, H)
    with pytest.raises(abi.PtError) as e:
        acc.add(4)
    assert e.value.code == abi.PT_ERR_INVALID_ARG
    with pytest.raises(abi.PtError):
        R.Accumulator(W, H, ds, c, adaptive=True, flags=abi.PT_FLAG_FAST_RNG)
    # the fused tonemap is the tonemap of the resolve
    assert torch.equal(acc.tonemap_rgb8(), R.tonemap_rgb8(acc.resolve()))
    for a_ in (plain, acc, fresh):
        a_.close()
    env = dict(os.environ)
    base = [sys.executable, "-m", "path_tracer_amd", "--scene", "cornell", "--width", "96", "--height", "64", "--spp", "48"]
    subprocess.run(base + ["--out", str(tmp_path / "plain.png")], check=True, cwd=ROOT, env=env, timeout=300)
    p = subprocess.run(base + ["--out", str(tmp_path / "ad.png"), "--noise-threshold", "-1", "--counts-out", str(tmp_path / "n.png")],
                       check=True, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    assert (tmp_path / "plain.png").read_bytes() == (tmp_path / "ad.png").read_bytes()
    assert "mean 48.0 spp" in p.stdout, p.stdout
    subprocess.run(base + ["--out", str(tmp_path / "ad2.png"), "--noise-threshold", "0.1", "--counts-out", str(tmp_path / "n2.png")],
                   check=True, cwd=ROOT, env=env, timeout=300)
    assert (tmp_path / "n2.png").exists()


def test_cpp_facade_adaptive(torch, tmp_path):
    exe = tmp_path / "adaptive_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{libdir / 'include'}",
                    str(ROOT / "tests" / "cpp" / "adaptive_main.cpp"), "-o", str(exe), f"-L{libdir}", "-lpt_render", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    W, H = 64, 40
    ps, cam = scenes.build("cornell")
    c = scenes.make_camera(cam, W, H)
    fb, counts = R.render_adaptive(W, H, ps, c, threshold=0.08, min_spp=8, max_spp=40, step=8)
    for extra in ([], ["--checkpoint", str(tmp_path / "st.bin")], ["--plain-checkpoint", str(tmp_path / "plain.bin")]):
        out, cnt = tmp_path / "fb.f32", tmp_path / "n.i32"
        subprocess.run([str(exe), str(W), str(H), str(out), str(cnt), "0.08", "8", "40", "8", *extra], check=True, timeout=300)
        assert (np.fromfile(cnt, dtype=np.int32).reshape(H, W) == counts.cpu().numpy()).all(), f"C++ counts {extra}"
        assert_bit_identical(np.fromfile(out, dtype=np.float32).reshape(H, W, 3), fb.cpu().numpy(), f"C++ adaptive {extra}")


def test_full_size_sampled(torch, orc):
    ps, cam = scenes.build("cornell")
    W, H = 1920, 1080
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    fb, counts = R.render_adaptive(W, H, ds, c, threshold=0.05, min_spp=16, max_spp=64, step=16)
    cnt = counts.cpu().numpy()
    assert cnt.min() >= 16 and cnt.max() <= 64
    orc.set_math(True)
    g = np.random.default_rng(17)
    xy = np.stack([g.integers(0, W, 1500), g.integers(0, H, 1500)], axis=1).astype(np.int32)
    f = fb.cpu().numpy()
    for k in np.unique(cnt[xy[:, 1], xy[:, 0]]):
        sel = xy[cnt[xy[:, 1], xy[:, 0]] == k]
        assert_bit_identical(f[sel[:, 1], sel[:, 0]], orc.render_pixels(ps, c.c, W, H, int(k), sel), f"cfg2 1080p adaptive at {k} spp")
