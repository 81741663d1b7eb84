"""The variance-guided denoiser on the GPU (include/pt_render.h: pt_variance_estimate, pt_variance_denoise; path_tracer_amd/render.py:
denoise_variance, Accumulator.variance, Accumulator.denoise_variance).

Every comparison is bit for bit against tests/variance_model.py, the numpy binary32 restatement of the header's text: synthetic planes
with special values (NaN and inf colours; negative, NaN, inf and zero variances; a zero albedo), frames smaller than the footprint,
frames that cross the 32 x 8 workgroups and their LDS halos with partial edge groups, every guide subset, both read paths, in-place
calls; the estimate over adaptive accumulators after masked windows, whole frames and a shard; the end-to-end path over a real
accumulator; the C++ facade and the CLI."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import scenes_small as S
import variance_model as V
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from test_gpu_adaptive import mask_sequence, unpack, valid_pixels
from test_gpu_denoise import planes as guide_planes
from test_gpu_denoise import read_png

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GUIDES = ("albedo", "normal", "depth")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def last_path():
    out = (C.c_int32 * 8)()
    abi.check(abi.load_library().pt_debug_last_variance_denoise(out), "pt_debug_last_variance_denoise")
    return list(out)


def planes(w, h, seed, special=True):
    """tests/test_gpu_denoise.py's synthetic planes (NaN, inf and denormal colours, a zero albedo, NaN guides among them) and a variance
    plane: mostly a few percent of the colour scale, with exact zeros and, with `special`, negative, NaN, inf and denormal values."""
    g = guide_planes(w, h, seed, special)
    r = np.random.default_rng(seed + 1000)
    var = (r.random((h, w, 3), dtype=np.float32) * np.float32(0.1)) ** 2
    var[r.random((h, w)) < 0.1] = 0
    if special and w * h >= 15:
        flat = var.reshape(-1, 3)
        px = r.choice(w * h, 6, replace=False)
        flat[px[0]] = -1.0
        flat[px[1], 0] = np.nan
        flat[px[2]] = np.inf
        flat[px[3], 2] = -np.inf
        flat[px[4]] = (1e-40, 0.0, -0.0)
        flat[px[5]] = 3e38
    g["variance"] = var
    return g


def run(torch, g, guides=GUIDES, want_variance=True, **kw):
    """render.denoise_variance over the host planes `g` -> host arrays (out, variance_out | None)."""
    dev = {k: torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("color", "variance", *guides)}
    vout = torch.full_like(dev["color"], -7.0) if want_variance else None
    out = R.denoise_variance(dev.pop("color"), dev.pop("variance"), variance_out=vout, **dev, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (vout.cpu().numpy() if want_variance else None)


def model(g, guides=GUIDES, **kw):
    return V.denoise(g["color"], g["variance"], **{k: g[k] for k in guides}, **kw)


def check(torch, g, what, guides=GUIDES, **kw):
    """Both read paths against the model, colour and variance; returns the model's pair."""
    want = model(g, guides, **kw)
    n = kw["iterations"]
    for no_lds in (False, True):
        got = run(torch, g, guides, no_lds=no_lds, **kw)
        tag = f"{what}{', PT_VDENOISE_NO_LDS' if no_lds else ''}"
        assert_bit_identical(got[0], want[0], tag + ": colour")
        assert_bit_identical(got[1], want[1], tag + ": variance")
        assert last_path() == (([1] * n if no_lds else ([2, 2] + [1] * 6)[:n]) + [0] * (8 - n)), tag
    return want


# ---- the filter against the model ---------------------------------------------------------------------------------------------------------

def test_synthetic_19x13_three_iterations(torch):
    g = planes(19, 13, 11)
    check(torch, g, "19 x 13, 3 iterations, every term, demodulated", iterations=3, sigma_variance=2.0, sigma_normal=0.6, sigma_depth=0.5,
          sigma_albedo=0.8, demodulate=True)


@pytest.mark.parametrize("demodulate", [False, True])
def test_synthetic_70x45_five_iterations(torch, demodulate):
    """3 x 6 workgroups of 32 x 8 pixels, partial on both edges; steps 1 ... 16 reach across one and two workgroup borders."""
    g = planes(70, 45, 12)
    want = check(torch, g, f"70 x 45, 5 iterations, demodulate {demodulate}", iterations=5, sigma_variance=3.0, sigma_normal=0.6,
                 sigma_depth=0.5, sigma_albedo=0.0, demodulate=demodulate)
    assert not np.array_equal(want[0], g["color"])


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (5, 70)])
def test_degenerate_frames(torch, w, h):
    g = planes(w, h, 13, special=False)
    check(torch, g, f"{w} x {h}, 5 iterations", iterations=5, sigma_variance=2.0, sigma_normal=0.6, sigma_depth=0.5, demodulate=True)


@pytest.mark.parametrize("iterations", [1, 8])
def test_iteration_bounds(torch, iterations):
    g = planes(37, 21, 14)
    check(torch, g, f"{iterations} iterations", iterations=iterations, sigma_variance=2.5, sigma_normal=0.6, sigma_depth=0.5, demodulate=False)


@pytest.mark.parametrize("guides,demodulate", [((), False), (("albedo",), False), (("albedo",), True), (("normal", "depth"), False),
                                               (("normal",), False), (("depth",), False), (("albedo", "normal", "depth"), False),
                                               (("albedo", "normal", "depth"), True)])
def test_guide_subsets(torch, guides, demodulate):
    g = planes(37, 21, 15)
    check(torch, g, f"guides {guides}, demodulate {demodulate}", guides, iterations=3, sigma_variance=2.0, sigma_normal=0.6, sigma_depth=0.5,
          sigma_albedo=0.7, demodulate=demodulate)


def test_sigmas_switch_terms_off(torch):
    g = planes(37, 21, 16)
    kw = dict(iterations=2, sigma_variance=2.0, sigma_normal=-1.0, sigma_depth=0.5, sigma_albedo=0.0, demodulate=False)
    want = check(torch, g, "normal and albedo terms off", **kw)
    got = run(torch, g, ("depth",), **kw)
    assert_bit_identical(got[0], want[0], "a sigma <= 0 is a NULL plane")
    assert_bit_identical(got[1], want[1], "a sigma <= 0 is a NULL plane: variance")
    for sv in (0.0, -3.0):  # the colour term off: guide-only, the variance only propagated
        check(torch, g, f"sigma_variance {sv}", iterations=3, sigma_variance=sv, sigma_normal=0.6, sigma_depth=0.5, demodulate=True)
    with pytest.raises(abi.PtError) as e:
        run(torch, g, ("normal",), demodulate=True)
    assert e.value.code == abi.PT_ERR_INVALID_ARG


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_in_place(torch, iterations):
    """out = color and variance_out = variance: the prepass has read both planes completely before the last level writes them."""
    g = planes(37, 21, 17)
    kw = dict(iterations=iterations, sigma_variance=2.0, sigma_normal=0.6, sigma_depth=0.5, demodulate=True)
    want = model(g, **kw)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in g.items()}
    fb, var = dev.pop("color"), dev.pop("variance")
    out = R.denoise_variance(fb, var, out=fb, variance_out=var, **dev, **kw)
    torch.cuda.synchronize()
    assert out is fb
    assert_bit_identical(fb.cpu().numpy(), want[0], f"in place, {iterations} iterations: colour")
    assert_bit_identical(var.cpu().numpy(), want[1], f"in place, {iterations} iterations: variance")
    for k, v in dev.items():
        assert_bit_identical(v.cpu().numpy(), g[k], f"guide {k} untouched")


def test_variance_out_is_optional(torch):
    g = planes(37, 21, 18)
    kw = dict(iterations=4, sigma_variance=2.0, sigma_normal=0.6, sigma_depth=0.5, demodulate=True)
    with_v, _ = run(torch, g, **kw)
    without, none = run(torch, g, want_variance=False, **kw)
    assert none is None
    assert_bit_identical(with_v, without, "variance_out NULL or not: the same out")
    assert_bit_identical(with_v, model(g, **kw)[0], "against the model")


# ---- the estimate --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell", "mixed"])
@pytest.mark.parametrize("w,h,si,sc", [(24, 16, 0, 1), (24, 16, 1, 3), (21, 13, 3, 4)])
def test_estimate_after_masked_windows(torch, name, w, h, si, sc):
    """24 x 16: the whole frame and one shard of 3 (two whole tiles each); 21 x 13, shard 3 of 4: partial edge tiles and a padded last
    tile, whose padding pixels get 0."""
    ps, cam = S.ALL[name]()
    c = scenes.make_camera(cam, w, h)
    acc = R.Accumulator(w, h, ps, c, shard_index=si, shard_count=sc, adaptive=True)
    with pytest.raises(abi.PtError) as e:  # before the first window
        acc.variance()
    assert e.value.code == abi.PT_ERR_INVALID_ARG
    for n, m in mask_sequence(torch, acc._pixel_shape(), si, sc):
        acc.add(n, m)
    got = acc.variance()
    torch.cuda.synchronize()
    assert tuple(got.shape) == tuple(acc.resolve().shape)
    _, sums, _, Hh, n, a = unpack(acc)
    want = V.estimate(sums, Hh, n, a)
    valid = valid_pixels(w, h, sc, si)
    want[~valid] = 0  # padding pixels of a shard
    assert_bit_identical(got.cpu().numpy().reshape(-1, 3), want, f"{name} shard {si}/{sc}")
    assert np.isfinite(want[valid]).any() and (a[valid] > 0).all()
    assert bool((~valid).any()) == ((w, h) == (21, 13)), "the 21 x 13 shard has padding pixels to check"
    acc.close()


def test_estimate_is_refused_on_a_plain_accumulator(torch):
    ps, cam = S.ALL["cornell"]()
    acc = R.Accumulator(24, 16, ps, scenes.make_camera(cam, 24, 16))
    acc.add(4)
    with pytest.raises(abi.PtError) as e:
        acc.variance()
    assert e.value.code == abi.PT_ERR_INVALID_ARG
    assert abi.load_library().pt_variance_estimate(acc.handle, None, None) == abi.PT_ERR_INVALID_ARG
    acc.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cornell(torch):
    w, h = 64, 40
    ps, cam = S.ALL["cornell"]()
    c = scenes.make_camera(cam, w, h)
    ds = R.DeviceScene(ps)
    return dict(w=w, h=h, ds=ds, cam=c)


def test_accumulator_denoise_variance(torch, cornell):
    w, h, ds, c = cornell["w"], cornell["h"], cornell["ds"], cornell["cam"]
    before = R.render(w, h, 16, ds, c).cpu().numpy()
    acc = R.Accumulator(w, h, ds, c, adaptive=True)
    acc.add(4).add(4)
    got = acc.denoise_variance(aov_spp=6)
    fb1 = R.render(w, h, 16, ds, c)  # queued behind the filter without a synchronisation
    by_hand = R.denoise_variance(acc.resolve(), acc.variance(), **R.render_aov(w, h, 6, ds, c))
    torch.cuda.synchronize()
    _, sums, _, Hh, n, a = unpack(acc)
    assert (n == 8).all() and (a == 4).all()
    var = V.estimate(sums, Hh, n, a).reshape(h, w, 3)
    assert_bit_identical(acc.variance().cpu().numpy(), var, "Accumulator.variance")
    aov = R.render_aov(w, h, 6, ds, c, planes=GUIDES)
    want, _ = V.denoise(acc.resolve().cpu().numpy(), var, **{k: v.cpu().numpy() for k, v in aov.items()}, **V.DEFAULTS)
    assert_bit_identical(got.cpu().numpy(), want, "Accumulator.denoise_variance, default parameters")
    assert_bit_identical(by_hand.cpu().numpy(), want, "denoise_variance(resolve(), variance(), **render_aov())")
    assert np.isfinite(want).all() and not np.array_equal(want, acc.resolve().cpu().numpy())
    assert_bit_identical(fb1.cpu().numpy(), before, "a render of the scene queued behind the filter")
    assert_bit_identical(R.render(w, h, 16, ds, c).cpu().numpy(), before, "a render of the scene afterwards")
    assert_bit_identical(acc.resolve().cpu().numpy(), R.render(w, h, 8, ds, c).cpu().numpy(), "the accumulator still resolves to 8 spp")
    with pytest.raises(TypeError):
        R.denoise_variance(acc.resolve(), acc.variance(), beauty=acc.resolve())
    acc.close()
    shard = R.Accumulator(w, h, ds, c, shard_index=0, shard_count=2, adaptive=True)
    shard.add(2)
    with pytest.raises(ValueError):
        shard.denoise_variance()
    shard.close()


# ---- hosts -----------------------------------------------------------------------------------------------------------------------------

def test_cpp_facade(torch, tmp_path):
    exe = tmp_path / "variance_denoise_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{libdir / 'include'}",
                    str(ROOT / "tests" / "cpp" / "variance_denoise_main.cpp"), "-o", str(exe), f"-L{libdir}", "-lpt_render", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    w, h = 64, 40
    ps, cam = scenes.build("cornell")
    c = scenes.make_camera(cam, w, h)
    acc = R.Accumulator(w, h, ps, c, adaptive=True)
    acc.add(4).add(4)
    fb, var = acc.resolve(), acc.variance()
    aov = R.render_aov(w, h, 6, ps, c, planes=GUIDES)
    res, res_plain = torch.empty_like(fb), torch.empty_like(fb)
    want = R.denoise_variance(fb, var, variance_out=res, **aov).cpu().numpy()
    want_plain = R.denoise_variance(fb, var, iterations=3, demodulate=False, variance_out=res_plain, **aov).cpu().numpy()
    out = tmp_path / "filtered.bin"
    subprocess.run([str(exe), str(w), str(h), "4", "6", str(out)], check=True, timeout=300)
    raw = np.fromfile(out, dtype=np.float32)
    assert raw.size == 4 * w * h * 3
    got = raw.reshape(4, h, w, 3)
    assert_bit_identical(got[0], want, "C++ pt::variance_denoise, defaults")
    assert_bit_identical(got[1], res.cpu().numpy(), "C++ pt::variance_denoise, defaults: residual variance")
    assert_bit_identical(got[2], want_plain, "C++ pt::variance_denoise in place, 3 iterations, no demodulation")
    assert_bit_identical(got[3], res_plain.cpu().numpy(), "C++ pt::variance_denoise in place: variance")
    acc.close()


def test_cli_writes_the_filtered_frame_and_leaves_out_png_alone(torch, tmp_path):
    base = ["--scene", "cornell", "--width", "64", "--height", "40", "--spp", "32", "--noise-threshold", "0.05", "--min-spp", "8"]

    def cli(*args):
        p = subprocess.run([sys.executable, "-m", "path_tracer_amd", *base, *args], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ), timeout=300)
        assert p.returncode == 0, p.stderr
    plain, with_dn, dn = tmp_path / "plain.png", tmp_path / "with.png", tmp_path / "filtered.png"
    cli("--out", str(plain))
    cli("--out", str(with_dn), "--denoise-out", str(dn), "--denoise-variance", "--aov-spp", "6", "--denoise-iterations", "4",
        "--denoise-sigma-variance", "3")
    assert plain.read_bytes() == with_dn.read_bytes()
    ps, cam = scenes.build("cornell")
    c = scenes.make_camera(cam, 64, 40)
    fb, counts, var = R.render_adaptive(64, 40, ps, c, threshold=0.05, min_spp=8, max_spp=32, step=8, variance=True)
    want = R.tonemap_rgb8(R.denoise_variance(fb, var, iterations=4, sigma_variance=3.0, **R.render_aov(64, 40, 6, ps, c)))
    assert np.array_equal(read_png(dn), want.cpu().numpy())
    assert not np.array_equal(read_png(dn), read_png(plain))
