"""The a-trous denoiser on the GPU (include/pt_render.h: pt_denoise; path_tracer_amd/render.py: denoise, Accumulator.denoise).

The header defines the filter operation by operation; tests/denoise_model.py restates it in numpy binary32; the kernel has to give the
model's bits — on synthetic planes that mix negatives, zeros, a NaN, an inf and denormals, at sizes that cross every workgroup-tile
border (32 x 8 pixels) with steps up to 16 through both read paths (LDS-staged tiles, global memory), on frames smaller than the filter, with every guide subset, demodulated or not, in place,
and on a real 8 spp frame with render_aov's guides.  All comparisons are int32 views (bit for bit); any NaN matches any NaN."""
import ctypes as C
import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

import denoise_model as M
import scenes_small as S
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def read_png(path):
    """The pixels of a PNG path_tracer_amd.png.write_png wrote (8-bit RGB, filter type 0 rows): uint8 [h][w][3], row 0 = top."""
    raw = Path(path).read_bytes()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    w, h = int.from_bytes(raw[16:20], "big"), int.from_bytes(raw[20:24], "big")
    idat, pos = b"", 8
    while pos < len(raw):
        ln, kind = int.from_bytes(raw[pos:pos + 4], "big"), raw[pos + 4:pos + 8]
        if kind == b"IDAT":
            idat += raw[pos + 8:pos + 8 + ln]
        pos += 12 + ln
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * 3)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)


def last_denoise():
    out = (C.c_int32 * 8)()
    abi.check(abi.load_library().pt_debug_last_denoise(out), "pt_debug_last_denoise")
    return list(out)


def planes(w, h, seed, special=True):
    """Seeded synthetic planes: colours with negatives and zeros, unit-ish normals, depths with zeros (misses); with `special`, a NaN, an
    inf, denormals and an exact zero albedo among them."""
    r = np.random.default_rng(seed)
    g = dict(color=(r.random((h, w, 3), dtype=np.float32) * 3 - 0.5), albedo=r.random((h, w, 3), dtype=np.float32),
             normal=r.standard_normal((h, w, 3), dtype=np.float32) * np.float32(0.4), depth=r.random((h, w), dtype=np.float32) * 4 + 1)
    g["normal"][:, : w // 2] += np.float32(1)          # two populations of normals: an edge down the middle
    g["depth"][: h // 3] = 0                           # a band of misses
    g["color"][r.random((h, w)) < 0.1] = 0
    if special and w * h >= 15:
        flat = lambda a: a.reshape(-1, a.shape[-1]) if a.ndim == 3 else a.reshape(-1)
        px = r.choice(w * h, 12, replace=False)
        flat(g["color"])[px[0]] = np.nan
        flat(g["color"])[px[1], 1] = np.inf
        flat(g["color"])[px[2]] = (1e-40, -3e-42, 1.4e-45)   # denormals
        flat(g["color"])[px[3]] = -np.inf
        flat(g["albedo"])[px[4]] = 0
        flat(g["albedo"])[px[5]] = (1e-39, 0.5, 2e-44)
        flat(g["normal"])[px[6]] = 0
        flat(g["normal"])[px[7], 0] = np.nan
        flat(g["depth"])[px[8]] = np.inf
        flat(g["depth"])[px[9]] = 1e-41
        flat(g["albedo"])[px[10], 2] = np.nan
        flat(g["color"])[px[11]] = (-0.0, 0.0, -0.0)
    return g


def run(torch, g, guides=("albedo", "normal", "depth"), **kw):
    """render.denoise over the host planes `g` -> host array."""
    dev = {k: torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("color", *guides)}
    out = R.denoise(dev.pop("color"), **dev, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def model(g, guides=("albedo", "normal", "depth"), **kw):
    return M.denoise(g["color"], **{k: g[k] for k in guides}, **kw)


# ---- against the model ------------------------------------------------------------------------------------------------------------------

def test_synthetic_19x13_three_iterations(torch):
    g = planes(19, 13, 11)
    kw = dict(iterations=3, sigma_color=1.5, sigma_normal=0.6, sigma_depth=0.5, sigma_albedo=0.8, demodulate=True)
    assert_bit_identical(run(torch, g, **kw), model(g, **kw), "19 x 13, 3 iterations, every term, demodulated")
    assert last_denoise() == [2, 2, 1, 0, 0, 0, 0, 0]  # steps 1 and 2 from LDS-staged tiles, step 4 from global memory


@pytest.mark.parametrize("demodulate", [False, True])
def test_synthetic_70x45_five_iterations(torch, demodulate):
    """3 x 6 workgroups of 32 x 8 pixels, partial on both edges; steps 1 ... 16 reach across one and two workgroup borders."""
    g = planes(70, 45, 12)
    kw = dict(iterations=5, sigma_color=2.0, sigma_normal=0.6, sigma_depth=0.5, sigma_albedo=0.0, demodulate=demodulate)
    want = model(g, **kw)
    assert_bit_identical(run(torch, g, **kw), want, f"70 x 45, 5 iterations, demodulate {demodulate}")
    assert last_denoise() == [2, 2, 1, 1, 1, 0, 0, 0]  # both read paths ran: LDS-staged tiles at the steps 1 and 2, global memory beyond
    assert_bit_identical(run(torch, g, no_lds=True, **kw), want, f"70 x 45, 5 iterations, demodulate {demodulate}, PT_DENOISE_NO_LDS")
    assert last_denoise() == [1, 1, 1, 1, 1, 0, 0, 0]


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3)])
def test_frames_smaller_than_the_filter(torch, w, h):
    g = planes(w, h, 13, special=False)
    kw = dict(iterations=5, sigma_color=2.0, sigma_normal=0.6, sigma_depth=0.5, demodulate=True)
    assert_bit_identical(run(torch, g, **kw), model(g, **kw), f"{w} x {h}, 5 iterations")
    assert_bit_identical(run(torch, g, no_lds=True, **kw), model(g, **kw), f"{w} x {h}, 5 iterations, PT_DENOISE_NO_LDS")


@pytest.mark.parametrize("iterations", [1, 8])
def test_iteration_bounds(torch, iterations):
    g = planes(37, 21, 14)
    kw = dict(iterations=iterations, sigma_color=3.0, sigma_normal=0.6, sigma_depth=0.5, demodulate=False)
    assert_bit_identical(run(torch, g, **kw), model(g, **kw), f"{iterations} iterations")
    assert last_denoise() == ([2, 2] + [1] * 6)[:iterations] + [0] * (8 - iterations)


@pytest.mark.parametrize("guides,demodulate", [((), False), (("albedo",), False), (("albedo",), True), (("normal", "depth"), False),
                                               (("normal",), False), (("depth",), False), (("albedo", "normal", "depth"), False),
                                               (("albedo", "normal", "depth"), True)])
def test_guide_subsets(torch, guides, demodulate):
    g = planes(37, 21, 15)
    kw = dict(iterations=3, sigma_color=1.5, sigma_normal=0.6, sigma_depth=0.5, sigma_albedo=0.7, demodulate=demodulate)
    want = model(g, guides, **kw)
    assert_bit_identical(run(torch, g, guides, **kw), want, f"guides {guides}, demodulate {demodulate}")
    assert_bit_identical(run(torch, g, guides, no_lds=True, **kw), want, f"guides {guides}, demodulate {demodulate}, PT_DENOISE_NO_LDS")


def test_sigmas_switch_terms_off(torch):
    g = planes(37, 21, 16)
    kw = dict(iterations=2, sigma_color=0.0, sigma_normal=-1.0, sigma_depth=0.5, sigma_albedo=0.0, demodulate=False)
    got = run(torch, g, **kw)
    assert_bit_identical(got, model(g, **kw), "colour, normal and albedo terms off")
    assert_bit_identical(got, run(torch, g, ("depth",), **kw), "a sigma <= 0 is a NULL plane")
    with pytest.raises(abi.PtError) as e:
        run(torch, g, ("normal",), demodulate=True)
    assert e.value.code == abi.PT_ERR_INVALID_ARG


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_out_may_be_color(torch, iterations):
    """Odd counts would read `color` while writing `out`: the call filters a copy; even counts start into the scratch plane."""
    g = planes(37, 21, 17)
    kw = dict(iterations=iterations, sigma_color=1.5, sigma_normal=0.6, sigma_depth=0.5, demodulate=True)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in g.items()}
    fb = dev.pop("color")
    out = R.denoise(fb, out=fb, **dev, **kw)
    torch.cuda.synchronize()
    assert out is fb
    assert_bit_identical(fb.cpu().numpy(), model(g, **kw), f"in place, {iterations} iterations")
    for k, v in dev.items():
        assert_bit_identical(v.cpu().numpy(), g[k], f"guide {k} untouched")


# ---- a real frame ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cornell(torch):
    w, h = 64, 40
    ps, cam = S.ALL["cornell"]()
    c = scenes.make_camera(cam, w, h)
    ds = R.DeviceScene(ps)
    fb = R.render(w, h, 8, ds, c)
    aov = R.render_aov(w, h, 6, ds, c)
    torch.cuda.synchronize()
    return dict(w=w, h=h, ds=ds, cam=c, fb=fb, aov=aov)


def test_cornell_8spp_with_render_aov_guides(torch, cornell):
    got = R.denoise(cornell["fb"], **cornell["aov"])  # all six planes: the filter takes albedo, normal, depth
    torch.cuda.synchronize()
    host = {k: cornell["aov"][k].cpu().numpy() for k in ("albedo", "normal", "depth")}
    want = M.denoise(cornell["fb"].cpu().numpy(), **host, **M.DEFAULTS)
    assert_bit_identical(got.cpu().numpy(), want, "Cornell 64 x 40 x 8 spp, default parameters")
    assert np.isfinite(want).all() and not np.array_equal(want, cornell["fb"].cpu().numpy())
    with pytest.raises(TypeError):
        R.denoise(cornell["fb"], beauty=cornell["fb"])


def test_accumulator_denoise(torch, cornell):
    w, h = cornell["w"], cornell["h"]
    acc = R.Accumulator(w, h, cornell["ds"], cornell["cam"])
    acc.add(3).add(5)
    got = acc.denoise(aov_spp=6, iterations=4)
    want = R.denoise(acc.resolve(), iterations=4, **R.render_aov(w, h, 6, cornell["ds"], cornell["cam"]))
    torch.cuda.synchronize()
    assert_bit_identical(got.cpu().numpy(), want.cpu().numpy(), "Accumulator.denoise vs denoise(resolve(), **render_aov())")
    assert_bit_identical(acc.resolve().cpu().numpy(), cornell["fb"].cpu().numpy(), "3 + 5 samples")
    acc.close()
    shard = R.Accumulator(w, h, cornell["ds"], cornell["cam"], shard_index=0, shard_count=2)
    shard.add(2)
    with pytest.raises(ValueError):
        shard.denoise()
    shard.close()


def test_no_interference_with_renders(torch, cornell):
    """Queued between two renders of the scene without a synchronisation, the filter leaves their bits alone (and they its own)."""
    w, h, ds, c = cornell["w"], cornell["h"], cornell["ds"], cornell["cam"]
    before = R.render(w, h, 16, ds, c).cpu().numpy()
    alone = R.denoise(cornell["fb"], **cornell["aov"]).cpu().numpy()
    fb1, d, fb2 = R.render(w, h, 16, ds, c), R.denoise(cornell["fb"], **cornell["aov"]), R.render(w, h, 16, ds, c)
    torch.cuda.synchronize()
    assert_bit_identical(fb1.cpu().numpy(), before, "render queued before the filter")
    assert_bit_identical(fb2.cpu().numpy(), before, "render queued behind the filter")
    assert_bit_identical(d.cpu().numpy(), alone, "filter queued between two renders")


# ---- hosts -----------------------------------------------------------------------------------------------------------------------------

def test_cpp_facade(torch, tmp_path):
    exe = tmp_path / "denoise_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{libdir / 'include'}",
                    str(ROOT / "tests" / "cpp" / "denoise_main.cpp"), "-o", str(exe), f"-L{libdir}", "-lpt_render", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    w, h = 64, 40
    ps, cam = scenes.build("cornell")
    c = scenes.make_camera(cam, w, h)
    fb = R.render(w, h, 8, ps, c)
    aov = R.render_aov(w, h, 6, ps, c, planes=("albedo", "normal", "depth"))
    want = R.denoise(fb, **aov).cpu().numpy()
    want_plain = R.denoise(fb, iterations=3, demodulate=False, **aov).cpu().numpy()
    out = tmp_path / "denoised.bin"
    subprocess.run([str(exe), str(w), str(h), "8", "6", str(out)], check=True, timeout=300)
    raw = np.fromfile(out, dtype=np.float32)
    assert raw.size == 2 * w * h * 3
    assert_bit_identical(raw[: w * h * 3].reshape(h, w, 3), want, "C++ pt::denoise, defaults")
    assert_bit_identical(raw[w * h * 3:].reshape(h, w, 3), want_plain, "C++ pt::denoise in place, 3 iterations, no demodulation")


def test_cli_writes_the_filtered_frame_and_leaves_out_png_alone(torch, tmp_path):
    def cli(*args):
        p = subprocess.run([sys.executable, "-m", "path_tracer_amd", "--scene", "cornell", "--width", "64", "--height", "40", "--spp", "8", *args],
                           capture_output=True, text=True, cwd=ROOT, env=dict(os.environ), timeout=300)
        assert p.returncode == 0, p.stderr
    plain, with_dn, dn = tmp_path / "plain.png", tmp_path / "with.png", tmp_path / "denoised.png"
    cli("--out", str(plain))
    cli("--out", str(with_dn), "--denoise-out", str(dn), "--aov-spp", "6", "--denoise-iterations", "4", "--denoise-sigma-color", "8")
    assert plain.read_bytes() == with_dn.read_bytes()
    ps, cam = scenes.build("cornell")
    c = scenes.make_camera(cam, 64, 40)
    want = R.tonemap_rgb8(R.denoise(R.render(64, 40, 8, ps, c), iterations=4, sigma_color=8.0, **R.render_aov(64, 40, 6, ps, c)))
    assert np.array_equal(read_png(dn), want.cpu().numpy())
    assert not np.array_equal(read_png(dn), read_png(plain))
