"""The spatial variance estimate on the GPU (include/pt_spatial_variance.h: pt_spatial_variance), held BIT FOR BIT to the header's numpy
restatement (tests/spatial_variance_model.py): the smallest frames at which tiling can go wrong — 1 x 1, frames narrower than the window,
one pixel into a second tile each way, three tile columns with a partial last row of tiles — under both read paths and every radius,
every subset of the guides with and without demodulation, NaN and inf sprinkled over the colours and the guides, fill mode out of place and
in place, the counts, pt_debug_last_spatial_variance, the stream contract on a non-blocking side stream behind a slow producer
(tests/stream_contract.py's harness), and the hosts: render.spatial_variance -> render.denoise_variance against the two models chained,
Accumulator.denoise_variance(spatial=...), render_temporal(spatial_variance=...), the C++ facade and the CLI."""
import ctypes as C
import itertools
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import scenes_small as S
import spatial_variance_model as SV
import stream_contract as SC
import variance_model as V
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from test_gpu_temporal import STEPS, moving_cameras

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F = np.float32
TW, TH = abi.PT_SVAR_TILE_W, abi.PT_SVAR_TILE_H
GUIDES = ("albedo", "normal", "depth", "id")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


# ---- frames -------------------------------------------------------------------------------------------------------------------------

def synthetic(w, h, seed):
    """{color, albedo, normal, depth, id, variance}: log-normal colours over surfaces laid out in blocks of 5 x 4 pixels that cross the
    tile boundaries — per block an id, a depth level (some blocks are misses: depth 0) and one of four normals, each with a little jitter
    below the tolerances; albedo in [0.1, 1]; about 1 % of the colours and of each guide's values NaN or +-inf, a few albedos that make m
    zero or tiny, -0 depths; the variance plane: a third +inf, a few NaN, negative and -0 values, the rest finite."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    block = (y // 4) * 97 + (x // 5)
    c = np.exp(r.normal(0.0, 1.0, (h, w, 3))).astype(F)
    albedo = r.uniform(0.1, 1.0, (h, w, 3)).astype(F)
    ids = (block % 7).astype(np.int32)
    level = (F(4) + (block % 3).astype(F) * F(2)).astype(F)
    depth = (level * (F(1) + r.uniform(-0.03, 0.03, (h, w)).astype(F))).astype(F)
    depth[block % 5 == 4] = F(0)  # misses
    dirs = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0, 0.8]], F)
    normal = (dirs[block % 4] + r.uniform(-0.1, 0.1, (h, w, 3)).astype(F)).astype(F)
    n_px = w * h

    def sprinkle(a, values, frac=0.01):
        flat = a.reshape(n_px, -1)
        for v in values:
            sel = r.random(n_px) < frac / len(values)
            flat[sel, r.integers(0, flat.shape[1], int(sel.sum()))] = v
    sprinkle(c, (np.nan, np.inf, -np.inf))
    sprinkle(c, (F(3e38), F(-3e38)), 0.004)  # finite, and their difference and its square overflow
    sprinkle(albedo, (np.nan, np.inf, F(-1e-3), F(1e-30), F(0)))
    sprinkle(normal, (np.nan, np.inf))
    sprinkle(depth, (np.nan, np.inf, -np.inf, F(-0.0), F(-1)))
    var = np.exp(r.normal(-2.0, 1.0, (h, w, 3))).astype(F)
    kind = r.random((h, w))
    var[kind < 0.33] = np.inf
    var[(kind >= 0.33) & (kind < 0.36), 1] = np.nan
    var[(kind >= 0.36) & (kind < 0.39), 2] = F(-1)
    var[(kind >= 0.39) & (kind < 0.42), 0] = F(-0.0)
    return dict(color=c, albedo=albedo, normal=normal, depth=depth, id=ids, variance=var)


_frames = {}


def frame(w, h, seed=1):
    if (w, h, seed) not in _frames:
        f = synthetic(w, h, seed)
        for a in f.values():
            a.setflags(write=False)
        _frames[w, h, seed] = f
    return _frames[w, h, seed]


def last_run(lib=None):
    out = (C.c_int32 * 4)()
    abi.check((lib or abi.load_library()).pt_debug_last_spatial_variance(out), "pt_debug_last_spatial_variance")
    return list(out)


def run(torch, f, guides=GUIDES, *, fill=False, in_place=False, **kw):
    """spatial_variance() on the device -> (variance_out, (estimated, holes)) as numpy, like the model's result."""
    dev = {k: torch.from_numpy(np.array(a)).cuda() for k, a in f.items()}  # (copies: the shared frames are read-only)
    var = dev["variance"] if fill else None
    out, n = R.spatial_variance(dev["color"], var, out=var if in_place else None, counts=True, **{g: dev[g] for g in guides}, **kw)
    torch.cuda.synchronize()
    assert (out is var) == in_place
    for k, a in f.items():
        if not (in_place and k == "variance"):
            assert_bit_identical(dev[k].cpu().numpy().view(F), np.array(a).view(F), f"the input plane {k} is left alone")
    return out.cpu().numpy(), tuple(int(x) for x in n.cpu().numpy())


def check(torch, f, what, guides=GUIDES, *, fill=False, in_place=False, no_lds=False, **kw):
    want, want_n = SV.spatial_variance(f["color"], f["variance"] if fill else None, **{g: f[g] for g in guides}, **kw)
    got, got_n = run(torch, f, guides, fill=fill, in_place=in_place, no_lds=no_lds, **kw)
    assert_bit_identical(got, want, what)
    assert got_n == want_n, f"{what}: counts {got_n} against the model's {want_n}"
    h, w, _ = f["color"].shape
    assert last_run() == [1 if no_lds else 2, (w + TW - 1) // TW, (h + TH - 1) // TH, kw.get("radius", abi.PT_SVAR_DEFAULT_RADIUS)]
    return want, want_n


# ---- the kernel against the model -----------------------------------------------------------------------------------------------------

# 1 x 1: one hole; 7 x 1 and 1 x 7: the window wider than the frame; 33 x 9: one pixel into a second tile each way; 70 x 19: three tile
# columns, a partial last row of tiles, halos crossing two tiles
SHAPES = [(1, 1), (7, 1), (1, 7), (TW + 1, TH + 1), (2 * TW + 6, 2 * TH + 3)]


@pytest.mark.parametrize("no_lds", [False, True], ids=["lds", "no_lds"])
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_shapes_radii_and_paths(torch, w, h, radius, no_lds):
    f = frame(w, h, 3)
    _, (est, holes) = check(torch, f, f"{w} x {h}, radius {radius}", radius=radius, min_pairs=2, no_lds=no_lds)
    assert est + holes == w * h
    if (w, h) == (1, 1):
        assert (est, holes) == (0, 1)
    if w * h > 1000:
        assert est > 500 and holes > 20  # the frame exercises both
    check(torch, f, f"{w} x {h}, radius {radius}, fill", radius=radius, min_pairs=2, no_lds=no_lds, fill=True)


@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulate"])
@pytest.mark.parametrize("no_lds", [False, True], ids=["lds", "no_lds"])
def test_every_subset_of_the_guides(torch, demodulate, no_lds):
    w, h = SHAPES[-1]
    f = frame(w, h)
    seen = set()
    for n in range(4):
        for subset in itertools.combinations(("normal", "depth", "id"), n):
            guides = subset + (("albedo",) if demodulate else ())
            want, counts = check(torch, f, f"guides {guides}", guides, demodulate=demodulate, no_lds=no_lds, radius=3, min_pairs=4)
            seen.add(want.tobytes())
    assert len(seen) == 8  # every guide changes the result on this frame
    # an albedo plane that is given and not used changes nothing
    assert_bit_identical(run(torch, f, ("albedo", "id"), demodulate=False, no_lds=no_lds)[0], run(torch, f, ("id",), no_lds=no_lds)[0], "albedo unused")


def test_fill_mode_out_of_place_in_place_and_the_paths_agree(torch):
    w, h = SHAPES[-1]
    f = frame(w, h)
    want, (est, holes) = check(torch, f, "fill", fill=True)
    kept = SV.keep(f["variance"])
    assert 0.5 * w * h < kept.sum() < 0.7 * w * h and est + holes == int((~kept).sum()) and est > 100
    assert_bit_identical(want[kept], f["variance"][kept], "kept pixels keep their bits")
    assert np.signbit(want[kept]).any()  # a -0 among them
    for kw in (dict(in_place=True), dict(no_lds=True), dict(in_place=True, no_lds=True)):
        check(torch, f, f"fill, {kw}", fill=True, **kw)
    everything = dict(f, variance=np.zeros_like(f["variance"]))
    got, n = run(torch, everything, fill=True)
    assert n == (0, 0) and not got.any()  # every pixel kept: no window work, no counts


def test_refusals_with_live_planes(torch):
    f = frame(9, 7, 3)
    fb = torch.from_numpy(np.array(f["color"])).cuda()
    with pytest.raises(abi.PtError, match="overlap"):
        R.spatial_variance(fb, out=fb)
    with pytest.raises(abi.PtError, match="PT_SVAR_DEMODULATE needs albedo"):
        R.spatial_variance(fb, demodulate=True)
    with pytest.raises(abi.PtError, match="radius"):
        R.spatial_variance(fb, radius=4)
    with pytest.raises(ValueError, match="counts"):
        R.spatial_variance(fb, counts=torch.empty(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="id must be"):
        R.spatial_variance(fb, id=torch.zeros((7, 9), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="whole frame"):
        R.spatial_variance(fb.reshape(-1, 3))
    with pytest.raises(TypeError, match="unexpected"):
        R.spatial_variance(fb, sigma=1.0)


# ---- the stream contract ------------------------------------------------------------------------------------------------------------------

def test_behind_pending_work_on_a_side_stream(torch):
    """pt_spatial_variance is asynchronous on `stream`: queued on a non-blocking side stream behind the slow producer, its inputs written
    last, its outputs — the counts included, which the call zeroes with a memset of its own — poisoned behind the producer, the producer
    still running when the call has returned; what it wrote is the model's."""
    w, h = 70, 45
    f = frame(w, h, 7)
    inp = SC.staged_inputs(torch, {k: np.array(a) for k, a in f.items()})
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    counts = torch.empty(2, dtype=torch.int32, device="cuda")
    st = SC.stream_apart_from_the_null_stream(torch)

    def call():
        R.spatial_variance(inp["color"][0], inp["variance"][0], out=out, counts=counts, radius=3, **{g: inp[g][0] for g in GUIDES})
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
    got, _ = SC.gated(torch, st, passes, inp.values(), [out, counts], call)
    want, want_n = SV.spatial_variance(f["color"], f["variance"], radius=3, **{g: f[g] for g in GUIDES})
    assert_bit_identical(got[0], want, "pt_spatial_variance on a side stream")
    assert tuple(int(x) for x in got[1]) == want_n


# ---- hosts ----------------------------------------------------------------------------------------------------------------------------

W, H, SPP, AOV_SPP = 64, 40, 8, 4
DENOISE_KW = dict(iterations=2)


@pytest.fixture(scope="module")
def cornell(torch):
    ps, cam_args = S.ALL["cornell"]()
    ds = R.DeviceScene(ps)
    yield ds, moving_cameras(cam_args, W, H, 3, STEPS["cornell"])
    torch.cuda.synchronize()
    ds.close()


def host(d):
    return {k: t.cpu().numpy() for k, t in d.items()}


def filtered_np(color, var, g):
    return V.denoise(color, var, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **dict(V.DEFAULTS, **DENOISE_KW))[0]


def test_a_plain_frame_through_the_estimate_and_the_filter(torch, cornell):
    """render() -> render.spatial_variance -> render.denoise_variance against the two models chained: a frame that carries nothing but its
    guides is variance-filtered."""
    ds, cams = cornell
    fb = R.render(W, H, SPP, ds, cams[0])
    guides = R.render_aov(W, H, AOV_SPP, ds, cams[0])  # all six planes: the stage ignores the ones it does not take
    var, n = R.spatial_variance(fb, counts=True, **guides)
    out = R.denoise_variance(fb, var, albedo=guides["albedo"], normal=guides["normal"], depth=guides["depth"], **DENOISE_KW)
    g, noisy = host(guides), fb.cpu().numpy()
    want_var, want_n = SV.spatial_variance(noisy, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], id=g["id"], **SV.DEFAULTS)
    assert_bit_identical(var.cpu().numpy(), want_var, "render.spatial_variance on a rendered frame")
    assert tuple(int(x) for x in n.cpu().numpy()) == want_n and want_n[0] > 0.8 * W * H and want_n[1] > 0
    assert_bit_identical(out.cpu().numpy(), filtered_np(noisy, want_var, g), "spatial_variance -> denoise_variance")


def test_accumulator_denoise_variance_spatial(torch, cornell):
    ds, cams = cornell
    plain = R.Accumulator(W, H, ds, cams[0])
    plain.add(SPP)
    with pytest.raises(abi.PtError):
        plain.denoise_variance(AOV_SPP, **DENOISE_KW)  # a plain accumulator has no variance of its own: as ever
    g = host(R.render_aov(W, H, AOV_SPP, ds, cams[0], planes=GUIDES))
    noisy = plain.resolve().cpu().numpy()
    want_var, _ = SV.spatial_variance(noisy, **g, **SV.DEFAULTS)
    assert_bit_identical(plain.denoise_variance(AOV_SPP, spatial=True, **DENOISE_KW).cpu().numpy(), filtered_np(noisy, want_var, g),
                         "a plain Accumulator.denoise_variance(spatial=True)")
    want_var3, _ = SV.spatial_variance(noisy, **g, **dict(SV.DEFAULTS, radius=3, min_pairs=8))
    assert_bit_identical(plain.denoise_variance(AOV_SPP, spatial=dict(radius=3, min_pairs=8), **DENOISE_KW).cpu().numpy(),
                         filtered_np(noisy, want_var3, g), "spatial={...}")
    with pytest.raises(TypeError, match="spatial"):
        plain.denoise_variance(AOV_SPP, spatial=dict(rank=2))
    plain.close()
    acc = R.Accumulator(W, H, ds, cams[0], adaptive=True)
    acc.add(1)  # one window: the second half buffer is empty, variance() is +inf everywhere
    noisy, var = acc.resolve().cpu().numpy(), acc.variance().cpu().numpy()
    assert np.isinf(var).all()
    filled, _ = SV.spatial_variance(noisy, var, **g, **SV.DEFAULTS)
    assert_bit_identical(acc.denoise_variance(AOV_SPP, spatial=True, **DENOISE_KW).cpu().numpy(), filtered_np(noisy, filled, g),
                         "an adaptive Accumulator.denoise_variance(spatial=True): the holes of variance() filled")
    assert_bit_identical(acc.denoise_variance(AOV_SPP, **DENOISE_KW).cpu().numpy(), filtered_np(noisy, var, g), "without the keyword: today's bits")
    acc.add(3).add(4)
    noisy, var = acc.resolve().cpu().numpy(), acc.variance().cpu().numpy()
    assert np.isfinite(var).all()
    assert_bit_identical(acc.denoise_variance(AOV_SPP, spatial=True, **DENOISE_KW).cpu().numpy(), filtered_np(noisy, var, g),
                         "nothing to fill: the estimate of the half buffers is kept")
    acc.close()


@pytest.mark.parametrize("spp", [1, 4])
def test_render_temporal_fills_the_variance_the_push_leaves_open(torch, cornell, spp):
    """At 1 spp a frame has no estimate of its own, so the push writes +inf wherever the history is younger than 4 frames: all of the
    first three frames.  With the keyword every such value becomes finite or is counted a hole; the colours do not change."""
    ds, cams = cornell
    plain = [dict(fr) for fr in R.render_temporal(W, H, spp, ds, cams, aov_spp=AOV_SPP, denoise_kw=DENOISE_KW)]
    got = [dict(fr) for fr in R.render_temporal(W, H, spp, ds, cams, aov_spp=AOV_SPP, denoise_kw=DENOISE_KW, spatial_variance=True)]
    assert len(got) == len(plain) == 3
    for f, (a, b) in enumerate(zip(got, plain)):
        assert set(a) == set(b) | {"variance_counts"} and "variance_counts" not in b
        for key in ("noisy", "temporal", "history"):
            assert_bit_identical(a[key].cpu().numpy(), b[key].cpu().numpy(), f"frame {f}: {key}")
        g = host(R.render_aov(W, H, AOV_SPP, ds, cams[f], planes=GUIDES))
        color, open_var = b["temporal"].cpu().numpy(), b["variance"].cpu().numpy()
        want, want_n = SV.spatial_variance(color, open_var, **g, **SV.DEFAULTS)
        var = a["variance"].cpu().numpy()
        assert_bit_identical(var, want, f"frame {f}: variance")
        counts = tuple(int(x) for x in a["variance_counts"].cpu().numpy())
        assert counts == want_n
        was_open = np.isinf(open_var).all(axis=-1)
        if spp == 1:
            assert was_open.all()
        assert counts[0] + counts[1] == int((~SV.keep(open_var)).sum()) >= int(was_open.sum())
        assert int(np.isinf(var[was_open]).all(axis=-1).sum()) == counts[1] and np.isfinite(var[was_open]).any(axis=-1).sum() == counts[0]
        assert_bit_identical(a["filtered"].cpu().numpy(), filtered_np(color, want, g), f"frame {f}: filtered")


# ---- the C++ facade and the CLI -------------------------------------------------------------------------------------------------------------

def test_cpp_facade(torch, tmp_path):
    exe = tmp_path / "spatial_variance_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{libdir / 'include'}",
                    str(ROOT / "tests" / "cpp" / "spatial_variance_main.cpp"), "-o", str(exe), f"-L{libdir}", "-lpt_render", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    w, h = SHAPES[-1]
    f = frame(w, h)
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(f[k].tobytes() for k in ("color", "albedo", "normal", "variance", "depth", "id")))
    subprocess.run([str(exe), str(w), str(h), "3", "2", str(src), str(out)], check=True, timeout=300)
    raw = out.read_bytes()
    n3 = w * h * 3
    assert len(raw) == 2 * (n3 * 4 + 8)
    g = {k: f[k] for k in GUIDES}
    for at, var_in, what in ((0, None, "the whole plane"), (n3 * 4 + 8, f["variance"], "fill mode in place")):
        want, want_n = SV.spatial_variance(f["color"], var_in, radius=3, min_pairs=2, **g)
        assert_bit_identical(np.frombuffer(raw, F, n3, at).reshape(h, w, 3), want, f"C++ pt::spatial_variance: {what}")
        assert tuple(int(x) for x in np.frombuffer(raw, np.uint32, 2, at + n3 * 4)) == want_n, what


def test_cli_filters_a_plain_frame_and_leaves_out_png_alone(torch, tmp_path):
    from test_gpu_denoise import read_png
    base = ["--scene", "cornell", "--width", "64", "--height", "40", "--spp", "8"]

    def cli(*args):
        p = subprocess.run([sys.executable, "-m", "path_tracer_amd", *base, *args], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ), timeout=300)
        assert p.returncode == 0, p.stderr
        return p.stdout
    plain, with_option, filtered = tmp_path / "plain.png", tmp_path / "with.png", tmp_path / "filtered.png"
    cli("--out", str(plain))
    text = cli("--out", str(with_option), "--denoise-out", str(filtered), "--denoise-variance", "--spatial-variance", "3", "--aov-spp", "4")
    assert plain.read_bytes() == with_option.read_bytes()
    ps, cam_args = scenes.build("cornell")
    cam = scenes.make_camera(cam_args, 64, 40)
    fb = R.render(64, 40, 8, ps, cam).cpu().numpy()
    g = host(R.render_aov(64, 40, 4, ps, cam))
    var, (est, holes) = SV.spatial_variance(fb, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], id=g["id"], **dict(SV.DEFAULTS, radius=3))
    assert f"spatial variance (radius 3): {est} pixels estimated, {holes} holes" in text and est > 2000
    want = V.denoise(fb, var, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **V.DEFAULTS)[0]
    assert np.array_equal(read_png(filtered), R.tonemap_rgb8(torch.from_numpy(want).cuda()).cpu().numpy())
    assert not np.array_equal(read_png(filtered), read_png(plain))
