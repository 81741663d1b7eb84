"""The first-hit feature buffers on the GPU (include/pt_render.h: pt_render_aov; path_tracer_amd/render.py: render_aov).

The definition: the AOV pass of n samples is the reference's render at depth 1 with the first bounce's record kept — per pixel, its own
xorshift32 stream, a camera ray and ONE bounce per sample.  The kernel is held to the numpy + oracle restatement of
tests/test_aov_cpu.py (aov_np: orc.camera_rays -> orc.bounce chained through the generator state) on every small scene, and its
`direct` plane to what render() itself writes at depth 1 — on the small scenes, the bench scene with both sphere-grid walks, and a
triangle pool.  All comparisons are int32 views (bit for bit); any NaN matches any NaN."""
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
from test_aov_cpu import H, N, PLANES, W, aov_reference, shard_layout

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


@pytest.fixture(scope="module")
def smoke():
    """scenes.build("smoke") — image textures, a medium, the sphere grid — packed once for the module."""
    return scenes.build("smoke")


def last_aov(ds):
    """(sphere-grid walk, u,v tracked) of the aov_kernel the scene's last pass launched (pt_debug_last_aov)."""
    out = (C.c_int32 * 2)()
    abi.check(ds.lib.pt_debug_last_aov(ds.handle, out), "pt_debug_last_aov")
    return tuple(out)


def host(planes):
    return {k: v.cpu().numpy() for k, v in planes.items()}


def same_planes(got, want, what, planes=PLANES):
    assert set(got) == set(planes), (what, sorted(got))
    for k in planes:
        if k == "id":
            assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, (what, k)
            bad = got[k] != want[k]
            assert not bad.any(), f"{what}: id: {int(bad.sum())} of {bad.size} differ; first at {tuple(np.argwhere(bad)[0])}"
        else:
            assert_bit_identical(got[k], want[k], f"{what}: {k}")


# ---- against the oracle ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(S.ALL))
def test_oracle_parity(torch, orc, name):
    """Every plane equals aov_np at 19 x 13 x 6: 3 x 2 tiles, partial tiles on both edges."""
    ps, cam = S.ALL[name]()
    c = scenes.make_camera(cam, W, H)
    same_planes(host(R.render_aov(W, H, N, ps, c)), aov_reference(orc, name), name)


def test_oracle_parity_with_lens_and_shutter(torch, orc):
    over = dict(aperture=0.3, time0=0.0, time1=1.0)
    ps, cam = S.ALL["spheres"]()
    c = scenes.make_camera(dict(cam, **over), W, H)
    same_planes(host(R.render_aov(W, H, N, ps, c)), aov_reference(orc, "spheres", cam_over=over), "spheres, aperture 0.3, shutter 0..1")


# ---- against render() at depth 1 --------------------------------------------------------------------------------------------------------

def direct_is_depth_1(torch, ds, c, w, h, n, what):
    planes = R.render_aov(w, h, n, ds, c)
    fb = R.render(w, h, n, ds, c, depth=1)
    torch.cuda.synchronize()
    assert_bit_identical(planes["direct"].cpu().numpy(), fb.cpu().numpy(), f"{what}: direct vs render(depth=1)")
    return host(planes)


@pytest.mark.parametrize("name", sorted(S.ALL))
def test_direct_is_render_at_depth_1_small_scenes(torch, name):
    ps, cam = S.ALL[name]()
    w, h, n = 64, 40, 16
    direct_is_depth_1(torch, R.DeviceScene(ps), scenes.make_camera(cam, w, h), w, h, n, name)


@pytest.mark.parametrize("walk", [1, 2])
def test_direct_is_render_at_depth_1_bench_scene(torch, smoke, walk):
    """scenes.build("smoke"): image textures, a medium and the sphere grid, with both grid walks (PtTuning.grid_walk)."""
    ps, cam = smoke
    w, h, n = 40, 24, 4
    ds = R.DeviceScene(ps, abi.tuning(grid_walk=walk))
    assert last_aov(ds) == (0, 0)
    got = direct_is_depth_1(torch, ds, scenes.make_camera(cam, w, h), w, h, n, f"smoke, grid walk {walk}")
    assert got["coverage"].max() == 1.0 and got["id"].max() > 0
    # the pass ran the kernel of that walk — and the walk the render itself took (direct_is_depth_1 rendered last)
    assert last_aov(ds)[0] == walk, last_aov(ds)
    launch = (C.c_int32 * 4)()
    abi.check(ds.lib.pt_debug_last_launch(ds.handle, launch), "pt_debug_last_launch")
    assert launch[3] == (1 if walk == 2 else 0), list(launch)


def test_both_grid_walks_give_the_same_planes(torch, smoke):
    ps, cam = smoke
    w, h, n = 40, 24, 4
    c = scenes.make_camera(cam, w, h)
    scenes_ = [R.DeviceScene(ps, abi.tuning(grid_walk=k)) for k in (1, 2)]
    a, b = (host(R.render_aov(w, h, n, ds, c)) for ds in scenes_)
    assert [last_aov(ds)[0] for ds in scenes_] == [1, 2]
    same_planes(a, b, "smoke: grid walk 1 vs 2")
    same_planes(host(R.render_aov(w, h, n, R.DeviceScene(ps), c)), a, "smoke: the launcher's walk vs walk 1")


def test_direct_is_render_at_depth_1_triangle_pool(torch, lib):
    ps, cam = scenes.triangle_mesh_scene(4096, seed=7, n_colors=8)
    st = (C.c_int32 * 8)()
    abi.check(lib.pt_debug_tri_pool(C.byref(ps.desc), st), "pt_debug_tri_pool")
    assert st[0] > 0, "the run must get a pool"
    w, h, n = 40, 24, 4
    ds = R.DeviceScene(ps)
    got = direct_is_depth_1(torch, ds, scenes.make_camera(cam, w, h), w, h, n, "4096 triangles (pooled)")
    assert (got["id"] >= 0).any() and last_aov(ds) == (1, 0)


# ---- layout ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed", "sphere_field"])
def test_shards(torch, name):
    """shard_count = 3 on 19 x 13 (6 tiles: every shard owns 2): each shard's planes are the whole frame's, re-laid out; padding pixels are
    0, and -1 in id."""
    ps, cam = S.ALL[name]()
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    whole = host(R.render_aov(W, H, N, ds, c))
    for k in range(3):
        got = host(R.render_aov(W, H, N, ds, c, shard_index=k, shard_count=3))
        want = {p: shard_layout(whole[p], W, H, k, 3, -1 if p == "id" else 0) for p in PLANES}
        assert got["albedo"].shape == (2, 64, 3) and got["depth"].shape == (2, 64) and got["id"].shape == (2, 64)
        same_planes(got, want, f"{name}: shard {k}/3")
    # a shard whose last tile is padding altogether: 6 tiles over 4 shards -> shards 2 and 3 own one tile and one padding tile
    got = host(R.render_aov(W, H, N, ds, c, shard_index=3, shard_count=4))
    want = {p: shard_layout(whole[p], W, H, 3, 4, -1 if p == "id" else 0) for p in PLANES}
    same_planes(got, want, f"{name}: shard 3/4")
    assert (got["id"][1] == -1).all() and not got["albedo"][1].any() and not got["coverage"][1].any()


def test_plane_subsets(torch):
    ps, cam = S.ALL["mixed"]()
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    full = host(R.render_aov(W, H, N, ds, c))
    for sub in [(p,) for p in PLANES] + [("albedo", "id")]:
        same_planes(host(R.render_aov(W, H, N, ds, c, planes=sub)), full, f"planes {sub}", planes=sub)
    with pytest.raises(ValueError):
        R.render_aov(W, H, N, ds, c, planes=())
    with pytest.raises(ValueError):
        R.render_aov(W, H, N, ds, c, planes=("albedo", "beauty"))


def test_refused_on_the_device_path_too(torch):
    ps, cam = S.ALL["cornell"]()
    c = scenes.make_camera(cam, W, H)
    with pytest.raises(abi.PtError) as e:
        R.render_aov(W, H, 0, ps, c)
    assert e.value.code == abi.PT_ERR_INVALID_ARG


@pytest.mark.parametrize("name", ["cornell", "sphere_field"])
def test_no_interference_with_renders(torch, name):
    """Two passes agree, and a render (with the cost probe: 16 spp) before and after a pass on the same scene gives the same bits."""
    ps, cam = S.ALL[name]()
    w, h = 64, 40
    c = scenes.make_camera(cam, w, h)
    ds = R.DeviceScene(ps)
    before = R.render(w, h, 16, ds, c).cpu().numpy()
    a = host(R.render_aov(w, h, 5, ds, c))
    after = R.render(w, h, 16, ds, c).cpu().numpy()
    b = host(R.render_aov(w, h, 5, ds, c))
    assert_bit_identical(before, after, f"{name}: render before / after the AOV pass")
    same_planes(a, b, f"{name}: two AOV passes")
    # queued back to back on the stream, without a synchronisation in between
    fb1, p1, fb2 = R.render(w, h, 16, ds, c), R.render_aov(w, h, 5, ds, c), R.render(w, h, 16, ds, c)
    torch.cuda.synchronize()
    assert_bit_identical(fb1.cpu().numpy(), before, f"{name}: render queued before the pass")
    assert_bit_identical(fb2.cpu().numpy(), before, f"{name}: render queued behind the pass")
    same_planes(host(p1), a, f"{name}: pass queued between two renders")


# ---- hosts ----------------------------------------------------------------------------------------------------------------------------

def test_cpp_facade(torch, tmp_path):
    exe = tmp_path / "aov_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{libdir / 'include'}",
                    str(ROOT / "tests" / "cpp" / "aov_main.cpp"), "-o", str(exe), f"-L{libdir}", "-lpt_render", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    w, h, n = 64, 40, 6
    ps, cam = scenes.build("cornell")
    want = host(R.render_aov(w, h, n, ps, scenes.make_camera(cam, w, h)))
    out = tmp_path / "aov.bin"
    subprocess.run([str(exe), str(w), str(h), str(n), str(out)], check=True, timeout=300)
    raw = np.fromfile(out, dtype=np.float32)
    n1, n3 = w * h, w * h * 3
    assert raw.size == 4 * n3 + 3 * n1
    got = {"albedo": raw[:n3].reshape(h, w, 3), "normal": raw[n3:2 * n3].reshape(h, w, 3), "direct": raw[2 * n3:3 * n3].reshape(h, w, 3),
           "depth": raw[3 * n3:3 * n3 + n1].reshape(h, w), "coverage": raw[3 * n3 + n1:3 * n3 + 2 * n1].reshape(h, w),
           "id": raw[3 * n3 + 2 * n1:3 * n3 + 3 * n1].view(np.int32).reshape(h, w)}
    same_planes(got, want, "C++ pt::render_aov over a device_scene")
    assert_bit_identical(raw[3 * n3 + 3 * n1:].reshape(h, w, 3), want["albedo"], "C++ pt::render_aov from the hittables")


def test_cli_writes_the_planes_and_leaves_out_png_alone(torch, tmp_path):
    def cli(*args):
        p = subprocess.run([sys.executable, "-m", "path_tracer_amd", "--scene", "cornell", "--width", "64", "--height", "40", "--spp", "8", *args],
                           capture_output=True, text=True, cwd=ROOT, env=dict(os.environ), timeout=300)
        assert p.returncode == 0, p.stderr
    plain, with_aov, d = tmp_path / "plain.png", tmp_path / "with.png", tmp_path / "aov"
    cli("--out", str(plain))
    cli("--out", str(with_aov), "--aov-dir", str(d), "--aov-spp", "6")
    assert plain.read_bytes() == with_aov.read_bytes()
    for f in ("albedo.png", "normal.png", "coverage.png", "aov.npz"):
        assert (d / f).exists() and (d / f).stat().st_size > 0, f
    ps, cam = scenes.build("cornell")
    want = host(R.render_aov(64, 40, 6, ps, scenes.make_camera(cam, 64, 40)))
    with np.load(d / "aov.npz") as z:
        same_planes({k: z[k] for k in z.files}, want, "aov.npz")
