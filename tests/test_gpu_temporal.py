"""Temporal reprojection on the GPU (include/pt_render.h: pt_adaptive_next_frame, PtTemporal, pt_temporal_push; path_tracer_amd/render.py:
Accumulator.next_frame, TemporalAccumulator, render_temporal).

Every comparison of the reprojection is bit for bit against tests/temporal_model.py, the numpy binary32 restatement of the header's text:
synthetic planes with special values (NaN, inf and denormal colours and variances, NaN and inf guides, a band of misses), frames of one
pixel up to 3 x 6 partial workgroups, three pushes per frame size (the same camera, a sub-pixel move, a move of several pixels that sends
taps out of the frame), a camera turned away, every subset of the optional planes, in-place outputs, a reset in the middle; then real
frames of an adaptive accumulator continued with next_frame under a moving camera, the generator, the C++ facade and the CLI.
pt_adaptive_next_frame is held to the oracle: per pixel, the reference's sample loop started from the generator state at the call."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import scenes_small as S
import temporal_model as T
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from path_tracer_amd.scene import camera
from test_aov_cpu import _IN, _OUT, _RAY
from test_gpu_adaptive import rng_index, unpack
from test_gpu_denoise import read_png
from test_gpu_variance_denoise import planes as synthetic_planes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F = np.float32


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


# ---- the reprojection against the model, synthetic planes ----------------------------------------------------------------------------

def cam_of(w, h, look_from=(0, 0, 0), look_at=None):
    look_at = (look_from[0], look_from[1], look_from[2] - 1) if look_at is None else look_at
    return camera(look_from, look_at, (0, 1, 0), 60.0, w / h, 0.0, 1.0, 0.0, 0.0)


def planes(w, h, seed):
    """tests/test_gpu_variance_denoise.py's planes (colour, variance, normal, depth with their special values; depth 0 = a band of
    misses) and an id plane: -1 where missed, else stripes of three ids with a few odd ones."""
    g = synthetic_planes(w, h, seed)
    ids = ((np.arange(w)[None, :] // 4 + np.arange(h)[:, None] // 5) % 3).astype(np.int32)
    ids[~(g["depth"] > 0)] = -1
    r = np.random.default_rng(seed + 7)
    ids[r.random((h, w)) < 0.05] = 0x7FC00001  # an id whose bits are a NaN's: compared as bits
    g["id"] = ids
    return g


class Pair:
    """One sequence pushed into the library and into the model alike."""

    def __init__(self, torch, w, h):
        self.torch, self.w, self.h = torch, w, h
        self.lib = abi.load_library()
        self.handle = C.c_void_p()
        abi.check(self.lib.pt_temporal_create(w, h, C.byref(self.handle)), "pt_temporal_create")
        self.model = T.Temporal(w, h)

    def close(self):
        self.lib.pt_temporal_destroy(self.handle)

    def raw(self, cam, g, subset=("normal", "id", "variance"), in_place=False, outputs=(True, True), **params):
        """pt_temporal_push over the host planes `g` -> host arrays (color, variance | None, history | None) and the device planes."""
        torch = self.torch
        dev = {k: torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("color", "depth", *subset)}
        ptr = lambda k: C.c_void_p(dev[k].data_ptr()) if k in dev else None  # noqa: E731
        out = dev["color"] if in_place else torch.full_like(dev["color"], -7.0)
        var = (dev["variance"] if in_place and "variance" in dev else torch.full_like(dev["color"], -7.0)) if outputs[0] else None
        hist = torch.full((self.h, self.w), -7.0, dtype=torch.float32, device="cuda") if outputs[1] else None
        kw = dict(T.DEFAULTS, **params)
        p = abi.PtTemporalParams(C.sizeof(abi.PtTemporalParams), kw["alpha"], kw["tol_depth"], kw["tol_normal"], 0)
        rc = self.lib.pt_temporal_push(self.handle, C.byref(p), C.byref(cam.c), ptr("color"), ptr("depth"), ptr("normal"), ptr("id"), ptr("variance"),
                                       C.c_void_p(out.data_ptr()), C.c_void_p(var.data_ptr()) if var is not None else None,
                                       C.c_void_p(hist.data_ptr()) if hist is not None else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        abi.check(rc, "pt_temporal_push")
        torch.cuda.synchronize()
        host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return (host(out), host(var), host(hist)), dev

    def push(self, cam, g, what, subset=("normal", "id", "variance"), **kw):
        """Both, compared bit for bit; returns the model's triple."""
        params = {k: kw.pop(k) for k in list(kw) if k in T.DEFAULTS}
        got, dev = self.raw(cam, g, subset, **kw, **params)
        want = self.model.push(cam.c, g["color"], g["depth"], normal=g["normal"] if "normal" in subset else None,
                               id=g["id"] if "id" in subset else None, variance_in=g["variance"] if "variance" in subset else None, **params)
        for name, a, b in zip(("colour", "variance", "history"), got, want):
            if a is not None:
                assert_bit_identical(a, b, f"{what}: {name}")
        assert self.lib.pt_temporal_frames(self.handle) == self.model.frames
        if not kw.get("in_place"):
            for k, t in dev.items():
                if t.dtype == self.torch.float32:
                    assert_bit_identical(t.cpu().numpy(), g[k], f"{what}: input plane {k} untouched")
        return want


def with_colour(g, seed):
    """The same guides under another frame's colours and variances (their special values move with the seed)."""
    n = synthetic_planes(g["depth"].shape[1], g["depth"].shape[0], seed)
    return dict(g, color=n["color"], variance=n["variance"])


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (19, 13), (70, 45)])
def test_three_pushes_against_the_model(torch, w, h):
    """70 x 45 is 3 x 6 workgroups of 32 x 8 pixels, partial on both edges.  The guides stay the same from push to push, so that the same
    camera finds every finite pixel's history, and the tolerances are wide enough that a moved camera still finds some."""
    g = planes(w, h, 21)
    pair = Pair(torch, w, h)
    first = pair.push(cam_of(w, h), g, f"{w} x {h}, first push")
    assert set(np.unique(first[2])) <= {0.0, 1.0}
    same = pair.push(cam_of(w, h), with_colour(g, 22), f"{w} x {h}, the same camera")
    sound = (np.isfinite(g["color"]).all(axis=2) & np.isfinite(with_colour(g, 22)["color"]).all(axis=2) & np.isfinite(g["normal"]).all(axis=2) &
             np.isfinite(g["depth"]) & ((g["depth"] == 0) | (g["depth"] > 1e-3)))  # (a denormal depth overflows fo / cp)
    assert np.allclose(same[2][sound], 2, rtol=1e-5), "the same camera and guides: every sound pixel has N = 2"
    sub = pair.push(cam_of(w, h, (0.004, -0.003, 0.0)), with_colour(g, 23), f"{w} x {h}, a sub-pixel move", tol_depth=0.5, tol_normal=1.5)
    far = pair.push(cam_of(w, h, (0.35, 0.2, -0.05), (0.3, 0.25, -1.0)), with_colour(g, 24), f"{w} x {h}, a move of several pixels",
                    tol_depth=0.9, tol_normal=1.5, alpha=0.3)
    if w * h >= 19 * 13:
        assert (sub[2] > 2.5).any() and (far[2] > 1.5).any() and (far[2] == 1).any(), "the moves must both find and lose histories"
        assert np.isfinite(far[1]).any()
    pair.close()


def test_a_camera_turned_away(torch):
    w, h = 19, 13
    g = planes(w, h, 31)
    pair = Pair(torch, w, h)
    pair.push(cam_of(w, h), g, "first")
    back = pair.push(cam_of(w, h, look_at=(0, 0, 1)), with_colour(g, 32), "a 180 degree turn")
    assert set(np.unique(back[2])) <= {0.0, 1.0}
    pair.close()


@pytest.mark.parametrize("subset", [(), ("normal",), ("id",), ("variance",), ("normal", "id"), ("normal", "variance"), ("id", "variance"),
                                    ("normal", "id", "variance")], ids=lambda s: "+".join(s) or "none")
def test_every_subset_of_the_optional_planes(torch, subset):
    w, h = 37, 21
    g = planes(w, h, 41)
    pair = Pair(torch, w, h)
    for k, cam in enumerate([cam_of(w, h), cam_of(w, h), cam_of(w, h, (0.02, 0.01, 0.0)), cam_of(w, h), cam_of(w, h)]):
        pair.push(cam, with_colour(g, 42 + k), f"subset {subset}, push {k}", subset, tol_depth=0.5, tol_normal=1.0)
    pair.close()


def test_in_place_and_optional_outputs(torch):
    w, h = 37, 21
    g = planes(w, h, 51)
    pair = Pair(torch, w, h)
    for k in range(5):  # out_color = color, out_variance = variance_in (from the fourth push on the variance is the history's)
        pair.push(cam_of(w, h, (0.003 * k, 0, 0)), with_colour(g, 52 + k), f"in place, push {k}", in_place=True, tol_depth=0.5, tol_normal=1.0)
    pair.push(cam_of(w, h), with_colour(g, 60), "no out_variance, no out_history", outputs=(False, False))
    pair.push(cam_of(w, h), with_colour(g, 61), "no out_history", outputs=(True, False))
    pair.close()


def test_reset_in_the_middle_and_frames(torch):
    w, h = 19, 13
    g = planes(w, h, 71)
    pair = Pair(torch, w, h)
    lib = pair.lib
    assert lib.pt_temporal_frames(pair.handle) == 0
    pair.push(cam_of(w, h), g, "push 1")
    pair.push(cam_of(w, h), with_colour(g, 72), "push 2")
    assert lib.pt_temporal_frames(pair.handle) == 2
    assert lib.pt_temporal_reset(pair.handle, None) == abi.PT_OK
    pair.model.reset()
    assert lib.pt_temporal_frames(pair.handle) == 0
    again = pair.push(cam_of(w, h, (0.1, 0, 0)), with_colour(g, 73), "the first push after a reset")
    assert set(np.unique(again[2])) <= {0.0, 1.0}
    pair.push(cam_of(w, h, (0.1, 0, 0)), with_colour(g, 74), "and the next")
    assert lib.pt_temporal_frames(pair.handle) == 2
    pair.close()


def test_refusals_that_need_a_live_object(torch):
    """An out plane overlapping a guide plane or another out plane (the state holds the frame size), refused with nothing written and
    the history untouched; pt_adaptive_next_frame on a plain accumulator."""
    w, h = 19, 13
    lib = abi.load_library()
    handle = C.c_void_p()
    abi.check(lib.pt_temporal_create(w, h, C.byref(handle)), "pt_temporal_create")
    buf = torch.zeros(18 * w * h, dtype=torch.float32, device="cuda")
    base, px = buf.data_ptr(), w * h
    at = lambda floats: C.c_void_p(base + 4 * floats)  # noqa: E731
    color, depth, normal, ident, var, out, vout, hout = (at(k) for k in (0, 3 * px, 4 * px, 7 * px, 8 * px, 11 * px, 14 * px, 17 * px))
    p = abi.PtTemporalParams(C.sizeof(abi.PtTemporalParams), 0.1, 0.1, 0.5, 0)
    cam = cam_of(w, h).c

    def call(**over):
        a = dict(color=color, depth=depth, normal=normal, id=ident, variance=var, out=out, vout=vout, hout=hout)
        a.update(over)
        return lib.pt_temporal_push(handle, C.byref(p), C.byref(cam), a["color"], a["depth"], a["normal"], a["id"], a["variance"], a["out"], a["vout"],
                                    a["hout"], None)

    for bad in (dict(out=depth), dict(out=at(3 * px - 1)), dict(out=at(4 * px + 1)), dict(out=ident), dict(out=at(8 * px - 1)),
                dict(vout=normal), dict(vout=at(px)), dict(hout=depth), dict(hout=at(7 * px - 1)), dict(hout=at(7 * px + 1)),
                dict(vout=out), dict(hout=at(14 * px - 1)), dict(hout=at(11 * px))):
        assert call(**bad) == abi.PT_ERR_INVALID_ARG, bad
        assert b"overlap" in lib.pt_last_error()
    assert lib.pt_temporal_frames(handle) == 0
    torch.cuda.synchronize()
    assert not bool(buf.any()), "a refused push wrote something"
    assert call() == abi.PT_OK and call(out=color, vout=var) == abi.PT_OK and lib.pt_temporal_frames(handle) == 2
    torch.cuda.synchronize()
    lib.pt_temporal_destroy(handle)
    ps, cam_args = S.ALL["cornell"]()
    acc = R.Accumulator(w, h, ps, scenes.make_camera(cam_args, w, h))
    acc.add(2)
    assert lib.pt_adaptive_next_frame(acc.handle, None) == abi.PT_ERR_INVALID_ARG and b"not an adaptive" in lib.pt_last_error()
    with pytest.raises(abi.PtError):
        acc.next_frame()
    assert acc.samples == 2
    acc.close()


# ---- end to end: real frames of an accumulator continued with next_frame ---------------------------------------------------------------

def moving_cameras(cam_args, w, h, n, step):
    lf = cam_args["look_from"]
    return [scenes.make_camera(dict(cam_args, look_from=(lf[0] + f * step[0], lf[1] + f * step[1], lf[2] + f * step[2])), w, h) for f in range(n)]


STEPS = {"cornell": (12.0, 5.0, 0.0), "mixed": (0.08, 0.03, 0.0)}


def by_hand(torch, ds, cams, w, h, spp, aov_spp, model=None):
    """Three frames through an adaptive accumulator, next_frame between them; each pushed with the GPU's guides and variance estimate.
    Returns the frames' (noisy, guides, variance, (color, variance, history)) as device tensors; checks the model where given."""
    acc, hist, out = None, R.TemporalAccumulator(w, h), []
    for f, cam in enumerate(cams):
        if acc is None:
            acc = R.Accumulator(w, h, ds, cam, adaptive=True)
        else:
            acc.next_frame(cam)
        acc.add(spp - spp // 2).add(spp // 2)
        noisy, var = acc.resolve(), acc.variance()
        guides = R.render_aov(w, h, aov_spp, ds, cam, planes=("albedo", "normal", "depth", "id"))
        got = hist.push(noisy, cam, variance=var, **guides)
        torch.cuda.synchronize()
        assert hist.frames == f + 1
        if model is not None:
            want = model.push(cam.c, noisy.cpu().numpy(), guides["depth"].cpu().numpy(), normal=guides["normal"].cpu().numpy(),
                              id=guides["id"].cpu().numpy(), variance_in=var.cpu().numpy(), **T.DEFAULTS)
            for name, a, b in zip(("colour", "variance", "history"), got, want):
                assert_bit_identical(a.cpu().numpy(), b, f"frame {f}: {name}")
        out.append((noisy, guides, var, got))
    acc.close()
    hist.close()
    return out


@pytest.mark.parametrize("w,h", [(19, 13), (70, 45)])
@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_end_to_end_against_the_model(torch, name, w, h):
    ps, cam_args = S.ALL[name]()
    ds = R.DeviceScene(ps)
    cams = moving_cameras(cam_args, w, h, 3, STEPS[name])
    model = T.Temporal(w, h)
    frames = by_hand(torch, ds, cams, w, h, 4, 4, model)
    last = frames[-1][3][2].cpu().numpy()
    assert (last > 2.5).mean() > 0.3, "most of the frame should have carried its history across the moves"
    # the frames carry independent noise: frame 1 is not frame 0's pattern under another camera — with a static camera they differ
    still = by_hand(torch, ds, [cams[0]] * 2, w, h, 4, 4)
    assert not np.array_equal(still[0][0].cpu().numpy(), still[1][0].cpu().numpy())
    # render_temporal: the same bytes as the sequence driven by hand
    for f, (frame, hand) in enumerate(zip(R.render_temporal(w, h, 4, ds, cams, aov_spp=4), frames)):
        torch.cuda.synchronize()
        assert_bit_identical(frame["noisy"].cpu().numpy(), hand[0].cpu().numpy(), f"render_temporal frame {f}: noisy")
        for key, t in zip(("temporal", "variance", "history"), hand[3]):
            assert_bit_identical(frame[key].cpu().numpy(), t.cpu().numpy(), f"render_temporal frame {f}: {key}")
        want = R.denoise_variance(hand[3][0], hand[3][1], albedo=hand[1]["albedo"], normal=hand[1]["normal"], depth=hand[1]["depth"])
        assert_bit_identical(frame["filtered"].cpu().numpy(), want.cpu().numpy(), f"render_temporal frame {f}: filtered")
    ds.close()


def test_cpp_facade(torch, tmp_path):
    exe = tmp_path / "temporal_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{libdir / 'include'}",
                    str(ROOT / "tests" / "cpp" / "temporal_main.cpp"), "-o", str(exe), f"-L{libdir}", "-lpt_render", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    w, h, n = 64, 40, 3
    ps, cam_args = scenes.build("cornell")
    frames = by_hand(torch, R.DeviceScene(ps), moving_cameras(cam_args, w, h, n, (10.0, 0.0, 0.0)), w, h, 4, 4)
    out = tmp_path / "temporal.bin"
    subprocess.run([str(exe), str(w), str(h), str(n), "4", "4", "10", str(out)], check=True, timeout=300)
    raw = np.fromfile(out, dtype=np.float32)
    assert raw.size == n * 7 * w * h
    for f, rec in enumerate(raw.reshape(n, 7 * w * h)):
        color, var, hist = frames[f][3]
        assert_bit_identical(rec[:3 * w * h].reshape(h, w, 3), color.cpu().numpy(), f"C++ pt::temporal frame {f}: colour")
        assert_bit_identical(rec[3 * w * h:6 * w * h].reshape(h, w, 3), var.cpu().numpy(), f"C++ pt::temporal frame {f}: variance")
        assert_bit_identical(rec[6 * w * h:].reshape(h, w), hist.cpu().numpy(), f"C++ pt::temporal frame {f}: history")


def test_cli_writes_the_frames_and_leaves_out_png_alone(torch, tmp_path):
    base = ["--scene", "cornell", "--width", "64", "--height", "40", "--spp", "4"]

    def cli(*args):
        p = subprocess.run([sys.executable, "-m", "path_tracer_amd", *base, *args], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ), timeout=300)
        assert p.returncode == 0, p.stderr
    plain, with_frames = tmp_path / "plain.png", tmp_path / "with.png"
    dirs = {k: tmp_path / k for k in ("plain", "temporal", "filtered")}
    move = ["--frames", "3", "--move", "10,0,0", "--aov-spp", "4"]
    cli("--out", str(plain))
    cli("--out", str(tmp_path / "p.png"), "--frames", "3", "--move", "10,0,0", "--frames-dir", str(dirs["plain"]))
    cli("--out", str(with_frames), *move, "--frames-dir", str(dirs["temporal"]), "--temporal")
    cli("--out", str(tmp_path / "f.png"), *move, "--frames-dir", str(dirs["filtered"]), "--temporal", "--denoise-variance", "--denoise-iterations", "3")
    assert plain.read_bytes() == with_frames.read_bytes() == (tmp_path / "p.png").read_bytes() == (tmp_path / "f.png").read_bytes()
    ps, cam_args = scenes.build("cornell")
    cams = moving_cameras(cam_args, 64, 40, 3, (10.0, 0.0, 0.0))
    frames = list(R.render_temporal(64, 40, 4, ps, cams, aov_spp=4, denoise_kw=dict(iterations=3)))
    for f, frame in enumerate(frames):
        assert np.array_equal(read_png(dirs["plain"] / f"frame_{f}.png"), R.tonemap_rgb8(R.render(64, 40, 4, ps, cams[f])).cpu().numpy()), f
        assert np.array_equal(read_png(dirs["temporal"] / f"frame_{f}.png"), R.tonemap_rgb8(frame["temporal"]).cpu().numpy()), f
        assert np.array_equal(read_png(dirs["filtered"] / f"frame_{f}.png"), R.tonemap_rgb8(frame["filtered"]).cpu().numpy()), f
    assert not np.array_equal(read_png(dirs["temporal"] / "frame_2.png"), read_png(dirs["plain"] / "frame_2.png"))


# ---- pt_adaptive_next_frame against the oracle -----------------------------------------------------------------------------------------

def follow(orc, ps, cam_c, w, h, xy, state, samples, depth):
    """The reference's sample loop (render.hpp:95-101) for the pixels `xy`, each started at its generator state `state` and run for its
    own `samples[i]` samples: orc.camera_rays -> orc.bounce ... up to `depth` bounces per sample.  A sample's colour is the bounce
    record's colour where the path ends (missed: attenuation x sky; absorbed: emitted) and black when `depth` bounces all scattered.
    Returns (the binary32 sums from +0 in sample order [n][3], the end states [n])."""
    n = len(xy)
    state = np.array(state, dtype=np.uint32)
    samples = np.broadcast_to(np.asarray(samples, dtype=np.int64), (n,))
    sums = np.zeros((n, 3), F)
    for s in range(int(samples.max())):
        live = np.nonzero(samples > s)[0]
        rays = np.frombuffer(bytes(orc.camera_rays(cam_c, w, h, xy[live], state[live])), dtype=_RAY, count=len(live))
        rin = np.zeros(len(live), dtype=_IN)
        for f in ("origin", "dir", "time", "rng_state"):
            rin[f] = rays[f]
        rin["attenuation"] = 1.0
        state[live] = rays["rng_state"]
        col = np.zeros((n, 3), F)
        for _ in range(depth):
            if len(live) == 0:
                break
            out = np.frombuffer(bytes(orc.bounce(ps, (abi.PtBounceIn * len(live)).from_buffer_copy(rin.tobytes()))), dtype=_OUT, count=len(live))
            state[live] = out["rng_state"]
            ended = out["status"] != abi.PT_BOUNCE_SCATTERED
            col[live[ended]] = out["color"][ended]
            on = ~ended
            rin = np.zeros(int(on.sum()), dtype=_IN)
            rin["origin"], rin["dir"], rin["time"] = out["sc_origin"][on], out["sc_dir"][on], out["sc_time"][on]
            rin["rng_state"], rin["attenuation"] = out["rng_state"][on], out["color"][on]
            live = live[on]
        active = samples > s
        sums[active] = (sums[active] + col[active]).astype(F)
    return sums, state


@pytest.mark.parametrize("depth", [50, 3])
@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_next_frame_continues_every_pixels_stream(torch, orc, name, depth):
    w, h = 19, 13
    ps, cam_args = S.ALL[name]()
    orc.set_math(True)
    ds = R.DeviceScene(ps)
    cam_a, cam_b = moving_cameras(cam_args, w, h, 2, STEPS[name])
    before = R.render(w, h, 4, ds, cam_b, depth).cpu().numpy()
    r = np.random.default_rng(5)
    px = r.choice(w * h, 24, replace=False)
    xy = np.stack([px % w, px // w], 1).astype(np.int32)
    ridx = rng_index(w, h)[px]
    acc = R.Accumulator(w, h, ds, cam_a, depth, adaptive=True)
    acc.add(3)
    # frame A is the reference's image (the accumulator's contract) and its end states are the loop's
    sums_a, s_p = follow(orc, ps, cam_a.c, w, h, xy, px.astype(np.uint32), 3, depth)
    _, sums, rng, _, n, _ = unpack(acc)
    assert_bit_identical(sums[px], sums_a, "frame A: sums")
    assert (rng[ridx] == s_p).all() and (n == 3).all()
    acc.next_frame(cam_b)
    hdr, sums, rng2, Hh, n, a = unpack(acc)
    assert acc.samples == 0 and hdr[8] == 0 and hdr[9] == 0, "the unmasked count and the camera binding are released"
    assert not sums.any() and not Hh.any() and not n.any() and not a.any()
    assert (rng2 == rng).all(), "next_frame keeps every generator state"
    # 5 samples under camera B, one window masked: the pixels of the mask get 5, the others 3
    mask = np.zeros((h, w), np.uint8)
    mask.reshape(-1)[px[::2]] = 1
    mask[:, : w // 3] = 1
    acc.add(2).add(2, torch.from_numpy(mask).cuda()).add(1)
    n_p = np.where(mask.reshape(-1)[px] != 0, 5, 3)
    want_sum, want_state = follow(orc, ps, cam_b.c, w, h, xy, s_p, n_p, depth)
    _, sums, rng3, _, n, _ = unpack(acc)
    assert (n[px] == n_p).all()
    assert_bit_identical(sums[px], want_sum, "frame B: the sums continue the stream")
    assert (rng3[ridx] == want_state).all(), "frame B: the states are where the loop left them"
    fb = acc.resolve().cpu().numpy().reshape(-1, 3)
    assert_bit_identical(fb[px], (want_sum / n_p[:, None].astype(F)).astype(F), "frame B: resolve")
    assert not np.array_equal(fb[px], R.render(w, h, 5, ds, cam_b, depth).cpu().numpy().reshape(-1, 3)[px]), "a later part of the stream, not pt_render's image"
    # a checkpoint of the continued frame restores
    state = acc.state()
    acc2 = R.Accumulator(w, h, ds, cam_b, depth, adaptive=True)
    acc2.restore(state)
    assert_bit_identical(acc2.resolve().cpu().numpy().reshape(-1, 3), fb, "pt_adaptive_export / import after next_frame")
    acc2.close()
    acc.close()
    # nothing else changed: pt_render and a fresh accumulator
    assert_bit_identical(R.render(w, h, 4, ds, cam_b, depth).cpu().numpy(), before, "pt_render afterwards")
    fresh = R.Accumulator(w, h, ds, cam_b, depth, adaptive=True)
    fresh.add(4)
    assert_bit_identical(fresh.resolve().cpu().numpy(), before, "a fresh accumulator afterwards")
    fresh.close()
    ds.close()
