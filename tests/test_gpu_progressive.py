"""Progressive rendering on the GPU (include/pt_render.h: PtAccum; path_tracer_amd/render.py: Accumulator, render_progressive).

The contract: after sample windows totalling N, the accumulator resolves to the bits pt_render gives at N samples — for every split, on
every kernel family (headline slab kernels with LDS-resident cold state, cooperative lists, the LDS-streaming kernel, both sphere-grid
walks, the triangle pool with its camera-ray cache), with and without the cost probe, for shards, across a checkpoint, and in the opt-in
fast mode under its chunk rule.  Comparisons are int32 views (bit for bit); sampled pixels are also checked against the CPU oracle."""
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

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).parent / "golden"


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


def windows(ds, W, H, cam, splits, depth=50, **kw):
    acc = R.Accumulator(W, H, ds, cam, depth, **kw)
    for n in splits:
        acc.add(n)
    assert acc.samples == sum(splits)
    fb = acc.resolve()
    acc.close()
    return fb


def same(a, b, what=""):
    import torch
    assert a.shape == b.shape, what
    eq = a.view(torch.int32) == b.view(torch.int32)
    assert bool(eq.all()), f"{what}: {int((~eq).sum())} of {eq.numel()} values differ"


def sample_xy(W, H, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], axis=1).astype(np.int32)


def check_oracle(orc, ps, c, fb, W, H, spp, n, seed, what, flags=0):
    orc.set_math(True)
    xy = sample_xy(W, H, n, seed)
    assert_bit_identical(fb.cpu().numpy()[xy[:, 1], xy[:, 0]], orc.render_pixels(ps, c.c, W, H, spp, xy, flags=flags), f"{what} against the oracle")


@pytest.mark.parametrize("name", list(S.ALL))
def test_small_frames_every_split(torch, name):
    ps, cam = S.ALL[name]()
    c = scenes.make_camera(cam, 32, 18)
    ds = R.DeviceScene(ps)
    one = R.render(32, 18, 4, ds, c)
    golden = torch.from_numpy(np.load(GOLDEN / f"fb_{name}_32x18x4.npy")).cuda()
    for split in ([4], [1, 3], [1, 1, 1, 1], [3, 1]):
        fb = windows(ds, 32, 18, c, split)
        same(fb, one, f"{name} {split} vs pt_render")
        same(fb, golden, f"{name} {split} vs golden")


PROBED = [("cornell", 256, 192, [[16, 48], [40, 24]]),
          ("sphere_field", 640, 400, [[8, 8, 16]]),
          ("mixed", 192, 128, [[1] * 8 + [40], [32] + [1] * 8 + [8]])]  # (the second: short windows after a probed one take its order)
VARIANTS = [("default", 0, None), ("force_coop", abi.PT_FLAG_FORCE_COOP, None), ("force_stream", abi.PT_FLAG_FORCE_STREAM, None),
            ("no_lds", abi.PT_FLAG_NO_LDS, None), ("pixel_granular", abi.PT_FLAG_PIXEL_GRANULAR, None), ("no_lpt", abi.PT_FLAG_NO_LPT, None),
            ("probe_resume_off", 0, dict(probe_resume=-1))]


@pytest.mark.parametrize("name,W,H,splits", PROBED, ids=[p[0] for p in PROBED])
def test_windows_long_enough_to_probe(torch, orc, name, W, H, splits):
    ps, cam = scenes.build("cornell") if name == "cornell" else S.ALL[name]()
    c = scenes.make_camera(cam, W, H)
    spp = sum(splits[0])
    for vname, flags, tun in VARIANTS:
        ds = R.DeviceScene(ps, tuning=abi.tuning(**tun) if tun else None)
        one = R.render(W, H, spp, ds, c, flags=flags)
        for split in splits:
            fb = windows(ds, W, H, c, split, flags=flags)
            same(fb, one, f"{name} {vname} {split}")
        if vname == "default":
            check_oracle(orc, ps, c, fb, W, H, spp, 200, 5, f"{name} {splits[-1]}")


def test_another_render_between_windows_changes_nothing(torch):
    """The accumulator keeps its own tile order: a render of another frame on the same scene between its windows (it rewrites the scene's
    scheduling workspace) changes neither the accumulator's image nor its own."""
    ps, cam = scenes.build("cornell")
    W, H = 256, 192
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    want = R.render(W, H, 48, ds, c)
    acc = R.Accumulator(W, H, ds, c)
    acc.add(32)
    other = R.render(320, 200, 64, ds, scenes.make_camera(cam, 320, 200))
    for _ in range(8):
        acc.add(2)
    same(acc.resolve(), want, "accumulator with a render in between")
    same(other, R.render(320, 200, 64, R.DeviceScene(ps), scenes.make_camera(cam, 320, 200)), "the render in between")
    acc.close()


def test_triangle_pool_and_binned(torch, orc):
    ps, cam = scenes.build("triangles", n_triangles=20_000)
    W, H, spp = 320, 180, 16
    c = scenes.make_camera(cam, W, H)
    for what, tun in (("pool", None), ("binned", dict(tri_binned=1))):
        ds = R.DeviceScene(ps, tuning=abi.tuning(**tun) if tun else None)
        one = R.render(W, H, spp, ds, c)
        fb = windows(ds, W, H, c, [4, 12])
        same(fb, one, f"triangles {what}")
        check_oracle(orc, ps, c, fb, W, H, spp, 256, 9, f"triangles {what}")


def test_shards(torch):
    ps, cam = scenes.build("cornell")
    W, H, spp = 256, 192, 32
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    whole = R.render(W, H, spp, ds, c)
    local = []
    for si in range(3):
        fb = windows(ds, W, H, c, [8, 24], shard_index=si, shard_count=3)
        if si in (1, 2):
            same(fb, R.render(W, H, spp, ds, c, shard_index=si, shard_count=3), f"shard {si} of 3")
        local.append(fb)
    same(R.unshard(torch.stack(local), W, H, 3), whole, "unsharded windows vs the whole frame")


def test_extend_without_reset(torch):
    ps, cam = scenes.build("cornell")
    W, H = 256, 192
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    acc = R.Accumulator(W, H, ds, c)
    acc.add(16)
    same(acc.resolve(), R.render(W, H, 16, ds, c), "16 spp")
    acc.add(48)
    same(acc.resolve(), R.render(W, H, 64, ds, c), "16 + 48 spp")
    acc.reset()
    assert acc.samples == 0
    acc.add(8)
    same(acc.resolve(), R.render(W, H, 8, ds, c), "8 spp after reset")
    acc.close()


def test_checkpoint_and_rejections(torch, tmp_path):
    ps, cam = S.mixed_scene()
    W, H = 192, 128
    c = scenes.make_camera(cam, W, H)
    one = R.render(W, H, 40, R.DeviceScene(ps), c)
    acc = R.Accumulator(W, H, R.DeviceScene(ps), c)
    acc.add(8)
    path = tmp_path / "state.bin"
    acc.save(path)
    assert path.stat().st_size == abi.load_library().pt_accum_state_bytes(C.byref(abi.PtRenderParams(W, H, 0, 50, 0, 1, 0, 0)))
    acc.close()
    del acc
    acc2 = R.Accumulator.load(path, R.DeviceScene(ps))  # a new PtScene of the same tables
    assert acc2.samples == 8
    acc2.add(32)
    same(acc2.resolve(), one, "checkpointed after 8 spp, resumed in a new accumulator")
    # a different camera on a later window is refused
    acc2.cam = scenes.make_camera(dict(cam, vfov=cam["vfov"] + 1.0), W, H)
    with pytest.raises(abi.PtError) as e:
        acc2.add(4)
    assert e.value.code == abi.PT_ERR_INVALID_ARG and acc2.samples == 40
    acc2.close()
    # a state of other frame parameters is refused on import
    state = np.fromfile(path, dtype=np.uint8)
    other = R.Accumulator(W, H, R.DeviceScene(ps), c, depth=49)
    with pytest.raises(abi.PtError) as e:
        other.restore(state)
    assert e.value.code == abi.PT_ERR_INVALID_ARG and other.samples == 0
    bad = state.copy()
    bad[0] ^= 1
    fresh = R.Accumulator(W, H, R.DeviceScene(ps), c)
    with pytest.raises(abi.PtError):
        fresh.restore(bad)
    with pytest.raises(abi.PtError):
        fresh.restore(state[:-4])
    # nothing to resolve yet; no empty windows
    for f in (fresh.resolve, fresh.tonemap_rgb8, lambda: fresh.add(0), lambda: fresh.add(-3)):
        with pytest.raises(abi.PtError) as e:
            f()
        assert e.value.code == abi.PT_ERR_INVALID_ARG
    with pytest.raises(abi.PtError):
        R.Accumulator(W, H, R.DeviceScene(ps), c, flags=abi.PT_FLAG_SINGLE_STREAM)
    sh = R.Accumulator(W, H, R.DeviceScene(ps), c, shard_index=0, shard_count=2)
    sh.add(1)
    with pytest.raises(abi.PtError):
        sh.tonemap_rgb8()
    for a in (other, fresh, sh):
        a.close()


def test_fast_mode_chunk_rule(torch):
    ps, cam = scenes.build("cornell")
    W, H = 192, 128
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    F = abi.PT_FLAG_FAST_RNG
    one = R.render(W, H, 148, ds, c, flags=F)
    same(windows(ds, W, H, c, [64, 64, 20], flags=F), one, "fast mode [64, 64, 20]")
    same(windows(ds, W, H, c, [128, 20], flags=F), one, "fast mode [128, 20]")
    acc = R.Accumulator(W, H, ds, c, flags=F)
    acc.add(64).add(20)
    with pytest.raises(abi.PtError) as e:
        acc.add(8)
    assert e.value.code == abi.PT_ERR_INVALID_ARG and acc.samples == 84
    same(acc.resolve(), R.render(W, H, 84, ds, c, flags=F), "fast mode [64, 20]")
    acc.close()


def test_tonemap_and_cli_preview(torch, tmp_path):
    ps, cam = scenes.build("cornell")
    W, H = 96, 64
    c = scenes.make_camera(cam, W, H)
    acc = R.Accumulator(W, H, R.DeviceScene(ps), c)
    acc.add(5).add(7)
    assert torch.equal(acc.tonemap_rgb8(), R.tonemap_rgb8(acc.resolve()))
    acc.close()
    env = dict(os.environ)
    base = [sys.executable, "-m", "path_tracer_amd", "--scene", "cornell", "--width", "96", "--height", "64", "--spp", "24"]
    subprocess.run(base + ["--out", str(tmp_path / "plain.png")], check=True, cwd=ROOT, env=env, timeout=300)
    subprocess.run(base + ["--out", str(tmp_path / "prog.png"), "--preview-every", "10", "--preview-dir", str(tmp_path / "pv")],
                   check=True, cwd=ROOT, env=env, timeout=300)
    assert (tmp_path / "plain.png").read_bytes() == (tmp_path / "prog.png").read_bytes()
    assert sorted(p.name for p in (tmp_path / "pv").iterdir()) == ["preview_10.png", "preview_20.png", "preview_24.png"]
    assert (tmp_path / "pv" / "preview_24.png").read_bytes() == (tmp_path / "plain.png").read_bytes()


def test_render_progressive_generator(torch):
    ps, cam = scenes.build("cornell")
    W, H = 128, 96
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    got = [(n, fb) for n, fb in R.render_progressive(W, H, 20, ds, c, step=8)]
    assert [n for n, _ in got] == [8, 16, 20]
    for n, fb in got:
        same(fb, R.render(W, H, n, ds, c), f"render_progressive at {n}")


def test_cpp_facade_accumulator(torch, tmp_path, lib):
    exe = tmp_path / "progressive_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", f"-I{libdir / 'include'}", str(ROOT / "tests" / "cpp" / "progressive_main.cpp"),
                    "-o", str(exe), f"-L{libdir}", "-lpt_render", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    W, H = 64, 40
    ps, cam = scenes.build("cornell")
    want = R.render_host(W, H, 16, ps, scenes.make_camera(cam, W, H))
    for extra in ([], ["--checkpoint", str(tmp_path / "st.bin")]):
        out = tmp_path / "fb.f32"
        subprocess.run([str(exe), str(W), str(H), str(out), "4", "5", "7", *extra], check=True, timeout=300)
        assert_bit_identical(np.fromfile(out, dtype=np.float32).reshape(H, W, 3), want, f"C++ accumulator {extra}")


def test_full_size_sampled(torch, orc):
    ps, cam = scenes.build("cornell")
    W, H, spp = 1920, 1080, 64
    c = scenes.make_camera(cam, W, H)
    ds = R.DeviceScene(ps)
    fb = windows(ds, W, H, c, [4, 28, 32])
    same(fb, R.render(W, H, spp, ds, c), "cfg2 1080p x 64 [4, 28, 32]")
    check_oracle(orc, ps, c, fb, W, H, spp, 1500, 17, "cfg2 1080p x 64 [4, 28, 32]")
