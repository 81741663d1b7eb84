"""The display stage on the GPU (include/pt_render.h: PtDisplay, pt_display_meter, pt_display_apply; path_tracer_amd/render.py: Display,
display, Accumulator.display, render_temporal(display=...)).

Every comparison is bit for bit against tests/display_model.py, the numpy restatement of the header's text: the 256 bins and the rejected
count, the exposure after one metering and after a five-frame sequence with different rates up and down, the rgb8 bytes and the linear
plane under the three tones.  Frames: one pixel; 37 x 19 (nothing a multiple of anything); a 64 x 40 frame of exp2(uniform(-20, 20))
seeded with NaN, +-inf, -1, +-0, a denormal and values on both sides of 2^-16, 2^16 and an inner bin edge; a 256 x 256 constant frame (all
65 536 counts in one bin: the metering kernel's worst case); one frame just past the size at which the metering loop runs twice (the size
comes from pt_debug_last_display); a metering rectangle aligned to nothing; both paths of the metering kernel and of the apply
kernel.  Then the stateless call, a manual exposure, reset, an all-rejected frame, the in-place linear plane, refusals on a live
object, the reference tone against pt_tonemap_rgb8, the Python hosts, the C++ facade and the CLI."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import display_model as D
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from test_gpu_denoise import read_png
from test_gpu_temporal import moving_cameras

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F = np.float32
TONES = sorted(D.TONES)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


# ---- frames -------------------------------------------------------------------------------------------------------------------------

def grey(v):
    return [F(v)] * 3


def special_frame(w=64, h=40, seed=1):
    """exp2(uniform(-20, 20)) per channel, with the special values as grey pixels (and a few in one channel only) spread over the frame."""
    r = np.random.default_rng(seed)
    c = np.exp2(r.uniform(-20.0, 20.0, (h, w, 3))).astype(F)
    up, down = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(-np.inf))  # noqa: E731
    edge = F(2.0 ** -3 * 1.375)  # an inner bin edge
    specials = [grey(np.nan), grey(np.inf), grey(-np.inf), grey(-1.0), grey(0.0), grey(-0.0), grey(1e-40), [F(np.nan), 1, 1], [1, F(np.inf), 1],
                [1, 1, F(-np.inf)], [F(-1.0), F(0.25), 0], [F(1e-40), 0, 0], [F(3e38)] * 3,
                grey(2.0 ** -16 * (1 - 2.0 ** -10)), grey(2.0 ** -16 * (1 + 2.0 ** -10)), grey(down(2.0 ** -16)), grey(2.0 ** -16), grey(up(2.0 ** -16)),
                grey(2.0 ** 16 * (1 - 2.0 ** -10)), grey(2.0 ** 16 * (1 + 2.0 ** -10)), grey(down(2.0 ** 16)), grey(2.0 ** 16), grey(up(2.0 ** 16)),
                grey(edge * F(1 - 2.0 ** -10)), grey(edge * F(1 + 2.0 ** -10)), grey(down(edge)), grey(edge), grey(up(edge)), grey(2.0 ** 20), grey(2.0 ** 21)]
    for i, px in enumerate(specials):
        if i < w * h:
            c[(i * 53) // w % h, (i * 53) % w] = px
    return c


FRAMES = {
    "1x1": lambda: np.array([[[0.5, 2.0, 0.125]]], dtype=F),
    "37x19": lambda: special_frame(37, 19, 4),
    "64x40": lambda: special_frame(64, 40, 1),
    "constant": lambda: np.full((256, 256, 3), 0.7, dtype=F),
}


class Pair:
    """One display state in the library and in the model alike."""

    def __init__(self, torch, **params):
        self.torch = torch
        self.lib = abi.load_library()
        self.kw = dict(D.DEFAULTS, **params)
        self.handle = C.c_void_p()
        abi.check(self.lib.pt_display_create(C.byref(self.handle)), "pt_display_create")
        self.model = D.State()

    def close(self):
        self.lib.pt_display_destroy(self.handle)

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def params(self, rect=None, **over):
        kw = dict(self.kw, **over)
        x0, y0, x1, y1 = rect or (0, 0, 0, 0)
        return abi.PtDisplayParams(C.sizeof(abi.PtDisplayParams), kw["tone"], 0, kw["ev_bias"], kw["ev_min"], kw["ev_max"], kw["lo_permille"],
                                   kw["hi_permille"], kw["adapt_up"], kw["adapt_down"], kw["white"], x0, y0, x1, y1, 0)

    def exposure(self):
        ev = C.c_float()
        abi.check(self.lib.pt_display_exposure(self.handle, C.byref(ev), self.stream()), "pt_display_exposure")
        return F(ev.value)

    def histogram(self):
        host = np.zeros(257, np.uint32)
        abi.check(self.lib.pt_display_histogram(self.handle, host.ctypes.data_as(C.POINTER(C.c_uint32)), self.stream()), "pt_display_histogram")
        return host

    def meter(self, frame, what, rect=None, dev=None):
        """pt_display_meter and the model's metering, compared: the 257 counts and the bits of e."""
        h, w, _ = frame.shape
        dev = self.torch.from_numpy(frame).cuda() if dev is None else dev
        p = self.params(rect)
        abi.check(self.lib.pt_display_meter(self.handle, C.byref(p), C.c_void_p(dev.data_ptr()), w, h, self.stream()), "pt_display_meter")
        with np.errstate(all="ignore"):
            want = self.model.meter(frame, rect, **{k: self.kw[k] for k in ("ev_bias", "ev_min", "ev_max", "lo_permille", "hi_permille", "adapt_up", "adapt_down")})
        got_h, got_e = self.histogram(), self.exposure()
        assert np.array_equal(got_h, self.model.last), f"{what}: histogram differs in bins {np.flatnonzero(got_h != self.model.last)[:8]}"
        assert got_h.sum() == (w * h if rect is None else (rect[2] - rect[0]) * (rect[3] - rect[1])), what
        assert_bit_identical(np.array([got_e]), np.array([want]), f"{what}: exposure")
        return dev

    def apply(self, frame, what, dev=None, stateless_ev=None, in_place=False, outputs=(True, True)):
        """pt_display_apply against the model at the model's exposure (or, stateless, at ev_bias = stateless_ev)."""
        torch = self.torch
        h, w, _ = frame.shape
        dev = torch.from_numpy(frame).cuda() if dev is None else dev
        rgb8 = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda") if outputs[0] else None
        lin = (dev if in_place else torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")) if outputs[1] else None
        p = self.params(**({} if stateless_ev is None else dict(ev_bias=stateless_ev)))
        rc = self.lib.pt_display_apply(None if stateless_ev is not None else self.handle, C.byref(p), C.c_void_p(dev.data_ptr()), w, h,
                                       C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None, C.c_void_p(lin.data_ptr()) if lin is not None else None,
                                       self.stream())
        abi.check(rc, "pt_display_apply")
        torch.cuda.synchronize()
        e = self.model.e if stateless_ev is None else F(min(max(F(stateless_ev), F(-32)), F(32)))
        want8, want_lin = D.apply(frame, e, self.kw["tone"], self.kw["white"])
        if rgb8 is not None:
            got8 = rgb8.cpu().numpy()
            assert np.array_equal(got8, want8), f"{what}: {int((got8 != want8).sum())} of {want8.size} bytes differ"
        if lin is not None:
            assert_bit_identical(lin.cpu().numpy(), want_lin, f"{what}: linear plane")
        if not in_place:
            assert_bit_identical(dev.cpu().numpy(), frame, f"{what}: the frame is untouched")
        return want8, want_lin


# ---- meter + apply against the model ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tone", TONES)
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_one_metering_and_apply_against_the_model(torch, name, tone):
    frame = FRAMES[name]()
    pair = Pair(torch, tone=D.TONES[tone], white=3.0)
    try:
        dev = pair.meter(frame, f"{name}")
        assert pair.lib.pt_display_frames(pair.handle) == 1
        pair.apply(frame, f"{name} {tone}", dev=dev)
        pair.apply(frame, f"{name} {tone} rgb8 only", dev=dev, outputs=(True, False))
        pair.apply(frame, f"{name} {tone} linear only", dev=dev, outputs=(False, True))
    finally:
        pair.close()
    if name == "constant":
        assert np.count_nonzero(pair.model.last) == 1 and pair.model.last.max() == 65536
    if name == "64x40":
        assert pair.model.last[256] >= 10 and pair.model.last[0] >= 3 and pair.model.last[255] >= 3  # the specials landed where they were aimed


def last_display(lib):
    out = (C.c_int32 * 8)()
    abi.check(lib.pt_debug_last_display(out), "pt_debug_last_display")
    return list(out)


def test_both_paths_of_both_kernels(torch):
    """The metering kernel takes four pixels per trip where the metered pixels are one contiguous 16-byte aligned range, the apply kernel
    four values where the width is a multiple of 4 and the planes are 16-byte aligned; otherwise one.  The same frames through both: a
    frame that starts 4 bytes into an allocation takes the one-at-a-time paths and gives the same histogram, exposure, bytes and floats."""
    for name, (w, h) in {"64x40": (64, 40), "37x19": (37, 19), "1x1": (1, 1)}.items():
        frame = FRAMES[name]()
        pair = Pair(torch)
        try:
            pair.meter(frame, name)
            assert last_display(pair.lib)[:4] == [-(-(-(-w * h // 4)) // 256), 256, 1, 4], name  # groups of four pixels; a last group may be partial
            pair.apply(frame, name)
            assert last_display(pair.lib)[4:] == ([-(-3 * w // 4 // 256), h, 4, 3] if w % 4 == 0 else [-(-3 * w // 256), h, 1, 3]), name
            flat = torch.zeros(frame.size + 1, dtype=torch.float32, device="cuda")
            flat[1:] = torch.from_numpy(frame).cuda().reshape(-1)
            shifted = flat[1:].view(h, w, 3)
            assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
            pair.model.reset()
            abi.check(pair.lib.pt_display_reset(pair.handle, pair.stream()), "pt_display_reset")
            pair.meter(frame, f"{name} misaligned", dev=shifted)
            assert last_display(pair.lib)[:4] == [-(-w * h // 256), 256, 1, 1], name
            pair.apply(frame, f"{name} misaligned", dev=shifted)
            assert last_display(pair.lib)[4:] == [-(-3 * w // 256), h, 1, 3], name
            pair.apply(frame, f"{name} misaligned in place", dev=shifted, in_place=True)
        finally:
            pair.close()


def test_five_frame_sequence_adapts_up_and_down(torch):
    base = special_frame(64, 40, 9)
    pair = Pair(torch, adapt_up=0.5, adapt_down=0.125, ev_bias=0.25)
    try:
        es = []
        for f, k in enumerate((0, -5, 3, 3, -9)):  # the frame darkens, brightens, stays, darkens: the exposure goes up, down, down, up
            with np.errstate(over="ignore"):
                frame = (base * F(2.0 ** k)).astype(F)
            dev = pair.meter(frame, f"frame {f}")
            pair.apply(frame, f"frame {f}", dev=dev)
            es.append(float(pair.model.e))
        assert pair.lib.pt_display_frames(pair.handle) == 5
        assert es[1] > es[0] and es[2] < es[1] and es[3] < es[2] and es[4] > es[3]
    finally:
        pair.close()


def test_a_frame_that_takes_the_metering_loop_twice(torch):
    lib = abi.load_library()
    pair = Pair(torch)
    out = (C.c_int32 * 8)()
    try:
        w, h = 512, 256
        while True:  # find the grid's cap: the first size whose threads take more than one pixel
            probe = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
            p = pair.params()
            abi.check(lib.pt_display_meter(pair.handle, C.byref(p), C.c_void_p(probe.data_ptr()), w, h, pair.stream()), "pt_display_meter")
            abi.check(lib.pt_debug_last_display(out), "pt_debug_last_display")
            if out[2] > 1:
                break
            h *= 2
            assert w * h <= 1 << 26, "the metering grid never saturates"
        assert pair.histogram()[256] == w * h  # (all zeros: all rejected, e untouched)
        pair.lib.pt_display_reset(pair.handle, pair.stream())
        threads = out[0] * out[1] * out[3]  # the pixels one trip of the whole grid takes
        w = 1021
        h = threads // w + 1  # the first whole number of rows past one trip
        assert threads < w * h <= threads + w
        frame = np.exp2(np.random.default_rng(2).uniform(-12.0, 12.0, (h, w, 3))).astype(F)
        frame[h - 1, w - 1] = grey(np.nan)  # the last pixel, taken in the second trip
        frame[h - 1, w - 2] = grey(2.0 ** 17)
        dev = pair.meter(frame, f"{w}x{h}")
        abi.check(lib.pt_debug_last_display(out), "pt_debug_last_display")
        assert (out[0] * out[1] * out[3], out[2]) == (threads, 2)
        pair.apply(frame, f"{w}x{h}", dev=dev, outputs=(True, False))
        rect = (0, 3, w, h - 2)  # as wide as the frame but starting off a 16-byte boundary: one pixel per trip, so four times the trips
        assert (3 * w * 12) % 16 != 0
        pair.meter(frame, f"{w}x{h} rect {rect}", rect=rect, dev=dev)
        abi.check(lib.pt_debug_last_display(out), "pt_debug_last_display")
        assert out[3] == 1 and out[2] == -(-w * (h - 5) // (out[0] * out[1])) > 2
    finally:
        pair.close()


@pytest.mark.parametrize("rect", [(3, 5, 50, 33), (63, 39, 64, 40), (0, 0, 64, 40), (7, 0, 8, 40)])
def test_metering_rectangle(torch, rect):
    frame = special_frame(64, 40, 6)
    frame[5:33, 3:50] *= F(64.0)  # the rectangle is brighter than the rest
    pair, whole = Pair(torch), Pair(torch)
    try:
        dev = pair.meter(frame, f"rect {rect}", rect=rect)
        whole.meter(frame, "whole frame", dev=dev)
        if rect == (0, 0, 64, 40):
            assert pair.model.e == whole.model.e
        pair.apply(frame, f"rect {rect}", dev=dev)  # the whole frame is shown
    finally:
        pair.close()
        whole.close()


# ---- the state ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tone", TONES)
def test_stateless_apply(torch, tone):
    frame = special_frame(37, 19, 12)
    pair = Pair(torch, tone=D.TONES[tone])
    try:
        for ev in (0.0, -2.0, 1.0, 0.3, -3.75, 40.0, -33.0):
            pair.apply(frame, f"stateless {tone} {ev} EV", stateless_ev=ev)
    finally:
        pair.close()
    dev = torch.from_numpy(frame).cuda()
    want8, want_lin = D.apply(frame, F(0.3), D.TONES[tone])
    got8, got_lin = R.display(dev, tone, 0.3, linear=True)
    assert np.array_equal(got8.cpu().numpy(), want8)
    assert_bit_identical(got_lin.cpu().numpy(), want_lin, "R.display linear")


def test_set_exposure_reset_and_rejected_frames(torch):
    frame, dark = special_frame(37, 19, 13), (special_frame(37, 19, 13) * F(2.0 ** -6)).astype(F)
    with np.errstate(all="ignore"):
        nothing = np.stack([np.full((19, 37), v, dtype=F) for v in (np.nan, -1.0, 0.0)], axis=2)
        nothing[::2] = F(-np.inf)
    pair = Pair(torch, adapt_up=0.25, adapt_down=0.5)
    try:
        assert pair.exposure() == 0
        pair.apply(frame, "fresh state: 0 EV")
        pair.meter(nothing, "nothing binned on a fresh state")            # e stays 0 and the state stays fresh
        assert pair.exposure() == 0 and pair.histogram()[256] == 37 * 19
        pair.meter(frame, "the first metering that solves is instant")
        e0 = pair.exposure()
        pair.meter(nothing, "nothing binned")
        assert pair.exposure() == e0
        pair.apply(frame, "after an all-rejected frame")
        pair.meter(dark, "adapting up")
        assert e0 < pair.exposure() < e0 + 6 * 0.26
        for ev, want in ((1.5, 1.5), (-2.0, -2.0), (40.0, 32.0), (-1e9, -32.0), (0.3, F(0.3))):
            abi.check(pair.lib.pt_display_set_exposure(pair.handle, ev, pair.stream()), "pt_display_set_exposure")
            pair.model.set_exposure(ev)
            assert pair.exposure() == F(want) == pair.model.e
            pair.apply(frame, f"manual {ev} EV")
        pair.meter(frame, "adapting from a manual exposure")             # not instant: the manual exposure counts as a metering
        assert pair.exposure() != e0
        abi.check(pair.lib.pt_display_reset(pair.handle, pair.stream()), "pt_display_reset")
        pair.model.reset()
        assert pair.lib.pt_display_frames(pair.handle) == 0 and pair.exposure() == 0 and not pair.histogram().any()
        pair.apply(frame, "after reset: 0 EV")
        pair.meter(frame, "after reset the metering is instant")
        assert pair.exposure() == e0 and pair.lib.pt_display_frames(pair.handle) == 1
    finally:
        pair.close()


@pytest.mark.parametrize("tone", TONES)
def test_linear_plane_in_place(torch, tone):
    frame = special_frame(64, 40, 14)
    pair = Pair(torch, tone=D.TONES[tone])
    try:
        dev = pair.meter(frame, "in place")
        pair.apply(frame, f"in place {tone}", dev=dev, in_place=True)
    finally:
        pair.close()


def test_refusals_on_a_live_object(torch):
    frame = special_frame(37, 19, 15)
    pair = Pair(torch)
    try:
        dev = pair.meter(frame, "before")
        e0, h0 = pair.exposure(), pair.histogram()
        lib, st = pair.lib, pair.stream()
        rgb8 = torch.zeros((19, 37, 3), dtype=torch.uint8, device="cuda")
        ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
        for bad in (dict(tone=7), dict(lo_permille=950), dict(adapt_up=0.0), dict(ev_min=5.0, ev_max=4.0), dict(white=0.0)):
            assert lib.pt_display_meter(pair.handle, C.byref(pair.params(**bad)), ptr(dev), 37, 19, st) == abi.PT_ERR_INVALID_ARG, bad
            assert lib.pt_display_apply(pair.handle, C.byref(pair.params(**bad)), ptr(dev), 37, 19, ptr(rgb8), None, st) == abi.PT_ERR_INVALID_ARG, bad
        assert lib.pt_display_meter(pair.handle, C.byref(pair.params(rect=(0, 0, 38, 19))), ptr(dev), 37, 19, st) == abi.PT_ERR_INVALID_ARG
        assert lib.pt_display_meter(pair.handle, C.byref(pair.params(rect=(4, 4, 4, 9))), ptr(dev), 37, 19, st) == abi.PT_ERR_INVALID_ARG
        good = pair.params()
        assert lib.pt_display_apply(pair.handle, C.byref(good), ptr(dev), 37, 19, None, None, st) == abi.PT_ERR_INVALID_ARG
        assert lib.pt_display_apply(pair.handle, C.byref(good), ptr(dev), 37, 19, ptr(dev, 8), None, st) == abi.PT_ERR_INVALID_ARG   # rgb8 inside color
        assert lib.pt_display_apply(pair.handle, C.byref(good), ptr(dev), 37, 19, ptr(rgb8), ptr(dev, 12), st) == abi.PT_ERR_INVALID_ARG  # linear astride color
        assert lib.pt_display_set_exposure(pair.handle, float("nan"), st) == abi.PT_ERR_INVALID_ARG
        assert b"pt_display_set_exposure" in lib.pt_last_error()
        torch.cuda.synchronize()
        assert pair.exposure() == e0 and np.array_equal(pair.histogram(), h0) and lib.pt_display_frames(pair.handle) == 1  # nothing ran
        assert not rgb8.any()
        assert_bit_identical(dev.cpu().numpy(), frame, "the frame is untouched")
        with pytest.raises(ValueError):
            R.Display("filmic")
        with pytest.raises(ValueError):
            R.display(dev.double(), "aces")
    finally:
        pair.close()


def test_reference_tone_at_0_ev_is_pt_tonemap_rgb8(torch):
    for frame in (special_frame(64, 40, 16), special_frame(37, 19, 17), (special_frame(64, 40, 18) * F(2.0 ** -14)).astype(F)):
        dev = torch.from_numpy(frame).cuda()
        want = R.tonemap_rgb8(dev).cpu().numpy()
        assert np.array_equal(R.display(dev, "reference", 0.0).cpu().numpy(), want)
        disp = R.Display("reference")
        assert np.array_equal(disp.apply(dev).cpu().numpy(), want)                       # a fresh state is 0 EV
        assert np.array_equal(disp.set_exposure(0.0).apply(dev).cpu().numpy(), want)
        disp.close()
        assert np.array_equal(D.apply(frame, F(0.0), D.REFERENCE)[0], want)


# ---- hosts ------------------------------------------------------------------------------------------------------------------------------

def test_python_hosts(torch):
    """Display, Accumulator.display and render_temporal(display=...) over rendered frames: what they show is the model's image of what they
    were given, and a sequence carries the exposure from frame to frame."""
    w, h = 64, 40
    ps, cam_args = scenes.build("cornell")
    cams = moving_cameras(cam_args, w, h, 3, (10.0, 0.0, 0.0))
    acc = R.Accumulator(w, h, ps, cams[0])
    acc.add(4)
    disp = R.Display("aces", adapt_up=0.5, adapt_down=0.5)
    shown = acc.display(disp).cpu().numpy()
    fb = acc.resolve().cpu().numpy()
    acc.close()
    model = D.State()
    e = model.meter(fb, adapt_up=0.5, adapt_down=0.5)
    assert F(disp.exposure()) == e and np.array_equal(disp.histogram(), model.last) and disp.frames == 1
    assert np.array_equal(shown, D.apply(fb, e, D.ACES)[0])
    disp.reset()
    frames = list(R.render_temporal(w, h, 4, ps, cams, aov_spp=4, denoise_kw=dict(iterations=2), display=disp))
    assert disp.frames == 3
    model.reset()
    for f, frame in enumerate(frames):
        filtered = frame["filtered"].cpu().numpy()
        e = model.meter(filtered, adapt_up=0.5, adapt_down=0.5)
        assert np.array_equal(frame["rgb8"].cpu().numpy(), D.apply(filtered, e, D.ACES)[0]), f
    assert F(disp.exposure()) == model.e
    plain = list(R.render_temporal(w, h, 4, ps, cams, aov_spp=4, denoise_kw=dict(iterations=2)))
    assert "rgb8" not in plain[0]
    assert_bit_identical(plain[2]["filtered"].cpu().numpy(), frames[2]["filtered"].cpu().numpy(), "the display stage changes nothing upstream")
    disp.close()


def test_cpp_facade(torch, tmp_path):
    exe = tmp_path / "display_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{libdir / 'include'}",
                    str(ROOT / "tests" / "cpp" / "display_main.cpp"), "-o", str(exe), f"-L{libdir}", "-lpt_render", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    w, h, n, spp = 64, 40, 3, 4
    out = tmp_path / "display.bin"
    subprocess.run([str(exe), str(w), str(h), str(n), str(spp), "60", "1", "0.5", "0.25", str(out)], check=True, timeout=300)
    raw = out.read_bytes()
    n3 = w * h * 3
    per = 2 * n3 * 4 + 4 + 257 * 4 + n3
    assert len(raw) == n * per + n3
    ps, cam_args = scenes.build("cornell")
    model = D.State()
    for f, cam in enumerate(moving_cameras(cam_args, w, h, n, (60.0, 0.0, 0.0))):
        rec = raw[f * per:(f + 1) * per]
        fb = np.frombuffer(rec, F, n3).reshape(h, w, 3)
        assert_bit_identical(fb, R.render(w, h, spp, ps, cam).cpu().numpy(), f"C++ frame {f}")
        e = model.meter(fb, adapt_up=0.5, adapt_down=0.25)
        want8, want_lin = D.apply(fb, e, D.REINHARD)
        assert_bit_identical(np.frombuffer(rec, F, n3, n3 * 4).reshape(h, w, 3), want_lin, f"C++ pt::display frame {f}: linear")
        assert_bit_identical(np.frombuffer(rec, F, 1, 2 * n3 * 4), np.array([e]), f"C++ pt::display frame {f}: exposure")
        assert np.array_equal(np.frombuffer(rec, np.uint32, 257, 2 * n3 * 4 + 4), model.last), f
        assert np.array_equal(np.frombuffer(rec, np.uint8, n3, 2 * n3 * 4 + 4 + 257 * 4).reshape(h, w, 3), want8), f
    assert np.array_equal(np.frombuffer(raw, np.uint8, n3, n * per).reshape(h, w, 3), D.apply(fb, F(1.0), D.REINHARD)[0])  # pt::display_apply at 1 EV


def test_cli_shows_the_frame_and_leaves_out_png_alone(torch, tmp_path):
    base = ["--scene", "cornell", "--width", "64", "--height", "40", "--spp", "16"]

    def cli(*args):
        p = subprocess.run([sys.executable, "-m", "path_tracer_amd", *base, *args], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ), timeout=300)
        assert p.returncode == 0, p.stderr
    plain, with_display, shown, frames_dir = tmp_path / "plain.png", tmp_path / "with.png", tmp_path / "shown.png", tmp_path / "frames"
    cli("--out", str(plain))
    cli("--out", str(with_display), "--auto-exposure", "--tone", "aces", "--display-out", str(shown), "--frames", "3", "--move", "60,0,0",
        "--frames-dir", str(frames_dir), "--adapt-up", "0.5", "--adapt-down", "0.25")
    assert plain.read_bytes() == with_display.read_bytes()
    ps, cam_args = scenes.build("cornell")
    fb = R.render(64, 40, 16, ps, scenes.make_camera(cam_args, 64, 40)).cpu().numpy()
    assert np.array_equal(read_png(shown), D.apply(fb, D.State().meter(fb, adapt_up=0.5, adapt_down=0.25), D.ACES)[0])
    clipped = [float(np.mean(read_png(f) == 255)) for f in (plain, shown)]
    print(f"values at code 255: reference stage {clipped[0]:.4f}, auto-exposure + ACES {clipped[1]:.4f}")
    assert clipped[1] < clipped[0]  # the reference stage clips the light's surroundings; the display stage keeps them
    model = D.State()
    for f, cam in enumerate(moving_cameras(cam_args, 64, 40, 3, (60.0, 0.0, 0.0))):
        fb = R.render(64, 40, 16, ps, cam).cpu().numpy()
        e = model.meter(fb, adapt_up=0.5, adapt_down=0.25)
        assert np.array_equal(read_png(frames_dir / f"frame_{f}.png"), D.apply(fb, e, D.ACES)[0]), f
