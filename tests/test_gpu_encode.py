"""The encode stage on the GPU (include/pt_encode.h: pt_encode, pt_display_encode; path_tracer_amd/render.py: encode and the `encode=`
keyword of the display hosts).  Every comparison is byte for byte against tests/encode_model.py, the numpy restatement of the header's
text, which finds its codes another way than the kernel (np.searchsorted over the whole table against a keyed start and three compares).

Frames: a 64 x 40 threshold frame — every M[c] and L[c] with its binary32 predecessor and successor (1533 values), the specials, and a
fixed-seed draw over [0, 1.5) — in both sRGB modes and the reference transfer, on the vector path, under PT_ENCODE_NO_VEC, at width 63 and
with the input plane offset by one float, pt_debug_last_encode naming the path each time; the small frames, and one pixel past the block
of values a workgroup takes per trip (read from the debug record) with more rows than the grid has workgroups to walk them; a ramp under
the dither at three phases; the fused call on a rendered Cornell frame against pt_encode of pt_display_apply's linear_out and, with the
reference transfer, against its rgb8_out; both calls behind pending work on a side stream; the overlap refusals with live planes; the
Python hosts, the C++ facade and the CLI."""
import ctypes as C
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import display_model as D
import encode_model as E
import stream_contract as SC
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from test_gpu_temporal import moving_cameras

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F = np.float32
W, H = 64, 40
MODES = {"srgb": (abi.PT_TRANSFER_SRGB, False), "dither": (abi.PT_TRANSFER_SRGB, True), "reference": (abi.PT_TRANSFER_REFERENCE, False)}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


@pytest.fixture(scope="module")
def lib():
    lib = abi.load_library()
    assert abi.has_encode(lib), "libpt_render.so has no encode stage (pt_encode, pt_display_encode)"
    return lib


def stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def params(lib, w, h, transfer, dither=False, phase=(0, 0), no_vec=False):
    p = abi.PtEncodeParams()
    lib.pt_encode_params_init(C.byref(p), w, h)
    p.transfer = transfer
    p.flags = (abi.PT_ENCODE_DITHER if dither else 0) | (abi.PT_ENCODE_NO_VEC if no_vec else 0)
    p.phase_x, p.phase_y = phase
    return p


def last(lib):
    out = (C.c_int32 * 8)()
    assert lib.pt_debug_last_encode(out) == abi.PT_OK
    return list(out)


def run(torch, lib, dev, transfer, dither=False, phase=(0, 0), no_vec=False):
    """pt_encode over the device frame `dev` -> (the bytes on the host, the debug record)."""
    h, w, _ = dev.shape
    out = torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device="cuda")
    p = params(lib, w, h, transfer, dither, phase, no_vec)
    abi.check(lib.pt_encode(C.byref(p), C.c_void_p(dev.data_ptr()), C.c_void_p(out.data_ptr()), stream(torch)), "pt_encode")
    rec = last(lib)
    return out.cpu().numpy(), rec


def differing(got, want):
    idx = np.argwhere(got != want)
    return f"{len(idx)} of {got.size} bytes differ; first at {tuple(idx[0])}: {got[tuple(idx[0])]} vs {want[tuple(idx[0])]}" if len(idx) else ""


def check(torch, lib, frame, what, vec, dev=None, **kw):
    """Every mode over `frame` against the model; the record names the path `vec` (None: whatever the shape allows)."""
    dev = torch.from_numpy(np.ascontiguousarray(frame)).cuda() if dev is None else dev
    h, w, _ = frame.shape
    for name, (transfer, dither) in MODES.items():
        got, rec = run(torch, lib, dev, transfer, dither, **kw)
        want = E.encode(frame, transfer, dither, kw.get("phase", (0, 0)))
        assert np.array_equal(got, want), f"{what}, {name}: {differing(got, want)}"
        want_vec = (w % 4 == 0 and dev.data_ptr() % 16 == 0 and not kw.get("no_vec", False)) if vec is None else vec
        assert rec[0] == (2 if want_vec else 1) and rec[3] == (4 if want_vec else 1), (what, name, rec)
        assert rec[4] == transfer + 1 and rec[5] == 0 and rec[6] == int(dither) and rec[7] == 0, (what, name, rec)
        items = 3 * w // 4 if want_vec else 3 * w
        assert rec[1] == (items + 255) // 256 and 1 <= rec[2] <= h, (what, name, rec)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------

def threshold_values():
    """Every M[c] and L[c], its binary32 predecessor and successor: 3 * (255 + 256) = 1533 values; then the specials."""
    t = np.concatenate([E.M, E.L])
    with np.errstate(all="ignore"):
        around = np.concatenate([t, np.nextafter(t, F(-np.inf)), np.nextafter(t, F(np.inf))]).astype(F)
    assert around.size == 1533
    specials = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, -1e-30, 1e-45, -1e-45, 1e-40, 2.0 ** -126, 2.0 ** -14, 2.0 ** -13,
                         np.nextafter(F(2.0 ** -13), F(0)), 1.0, np.nextafter(F(1), F(2)), np.nextafter(F(1), F(0)), 1.5, 2.0, 255.0, 3e38, 0.18,
                         0.5, 0.25, 0.999, 0.04045, 0.0031308], dtype=F)
    return np.concatenate([around, specials])


def threshold_frame(w=W, h=H):
    """The threshold values spread over the frame's values (so that they meet every column phase and both halves of a 16-byte load), the
    rest a fixed-seed draw over [0, 1.5)."""
    r = np.random.default_rng(20240611)
    flat = (r.random(w * h * 3) * 1.5).astype(F)
    v = threshold_values()
    assert v.size <= flat.size
    flat[(np.arange(v.size) * 4 + np.arange(v.size) // 7) % flat.size] = v  # distinct: 4 i + i // 7 is increasing and stays below the size
    assert len(set(((np.arange(v.size) * 4 + np.arange(v.size) // 7) % flat.size).tolist())) == v.size
    return flat.reshape(h, w, 3)


def test_threshold_frame_on_the_vector_path(torch, lib):
    check(torch, lib, threshold_frame(), "64x40", vec=True)


def test_threshold_frame_one_value_per_lane(torch, lib):
    check(torch, lib, threshold_frame(), "64x40 NO_VEC", vec=False, no_vec=True)


def test_threshold_frame_at_width_63(torch, lib):
    check(torch, lib, threshold_frame(63, 41), "63x41", vec=False)


def test_threshold_frame_with_the_plane_offset_by_one_float(torch, lib):
    frame = threshold_frame()
    back = torch.zeros(W * H * 3 + 4, dtype=torch.float32, device="cuda")
    dev = back[1:1 + W * H * 3].view(H, W, 3)
    dev.copy_(torch.from_numpy(frame))
    assert dev.data_ptr() % 16 == 4 and dev.is_contiguous()
    check(torch, lib, frame, "64x40 + 4 bytes", vec=False, dev=dev)


def test_the_output_plane_offset_by_one_byte_takes_the_scalar_path(torch, lib):
    frame = threshold_frame()
    dev = torch.from_numpy(frame).cuda()
    back = torch.full((W * H * 3 + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    out = back[1:1 + W * H * 3]
    p = params(lib, W, H, abi.PT_TRANSFER_SRGB, True, (2, 1))
    abi.check(lib.pt_encode(C.byref(p), C.c_void_p(dev.data_ptr()), C.c_void_p(out.data_ptr()), stream(torch)), "pt_encode")
    assert last(lib)[0] == 1
    host = back.cpu().numpy()
    assert np.array_equal(host[1:-3].reshape(H, W, 3), E.encode(frame, E.SRGB, True, (2, 1)))
    assert host[0] == 0xA5 and (host[-3:] == 0xA5).all()  # nothing written outside the plane


@pytest.mark.parametrize("w,h", [(1, 1), (3, 1), (1, 5), (5, 3), (4, 1), (8, 8)])
def test_small_frames(torch, lib, w, h):
    r = np.random.default_rng(w * 100 + h)
    frame = (r.random((h, w, 3)) * 1.2).astype(F)
    frame.reshape(-1)[:: 5] = threshold_values()[r.integers(0, 1533, frame.reshape(-1)[:: 5].size)]
    check(torch, lib, frame, f"{w}x{h}", vec=None)
    check(torch, lib, frame, f"{w}x{h} phase", vec=None, phase=(-3, 6))


@pytest.mark.parametrize("no_vec", [False, True])
def test_one_pixel_past_a_workgroups_block_and_more_rows_than_the_grid_walks(torch, lib, no_vec):
    """The record says how many values of a row a workgroup takes per trip (256 * out[3]); the frame is one pixel wider than the pixels
    that holds (rounded up to the path's width rule), and has more rows than pt_debug_last_encode's grid.y of a first call, so that the
    row loop runs more than once for some workgroup."""
    probe = torch.zeros((8, 8, 3), dtype=torch.float32, device="cuda")
    _, rec = run(torch, lib, probe, abi.PT_TRANSFER_SRGB, no_vec=no_vec)
    per_trip = 256 * rec[3]
    w = -(-per_trip // 3) + 1
    if not no_vec:
        w = (w + 3) // 4 * 4  # the vector path needs a width that is a multiple of 4: 344 is past the block too
    assert 3 * w > per_trip
    frame0 = torch.zeros((1, w, 3), dtype=torch.float32, device="cuda")
    _, rec = run(torch, lib, frame0, abi.PT_TRANSFER_SRGB, no_vec=no_vec)
    assert rec[1] == 2  # two workgroups along the row
    h = 1024 + 3        # more rows than the grid walks at two workgroups a row (asserted below)
    r = np.random.default_rng(5)
    frame = (r.random((h, w, 3)) * 1.2).astype(F)
    frame[:, -1, :] = threshold_values()[r.integers(0, 1533, (h, 3))]  # the pixel past the block
    dev = torch.from_numpy(frame).cuda()
    for name, (transfer, dither) in MODES.items():
        got, rec = run(torch, lib, dev, transfer, dither, (1, 2) if dither else (0, 0), no_vec)
        assert rec[2] < h and rec[1] == 2 and rec[0] == (1 if no_vec else 2), rec
        want = E.encode(frame, transfer, dither, (1, 2) if dither else (0, 0))
        assert np.array_equal(got, want), f"{w}x{h} {name}: {differing(got, want)}"


@pytest.mark.parametrize("phase", [(0, 0), (3, 5), (-1, 9)])
def test_a_ramp_under_the_dither(torch, lib, phase):
    ramp = np.linspace(0.0, 1.2, W * 3, dtype=np.float64).astype(F).reshape(1, W, 3)
    frame = np.ascontiguousarray(np.broadcast_to(ramp, (H, W, 3)))
    dev = torch.from_numpy(frame).cuda()
    for no_vec in (False, True):
        got, _ = run(torch, lib, dev, abi.PT_TRANSFER_SRGB, True, phase, no_vec)
        want = E.encode(frame, E.SRGB, True, phase)
        assert np.array_equal(got, want), f"ramp at phase {phase}: {differing(got, want)}"
    plain = E.encode(frame, E.SRGB)
    assert (got != plain).any() and (np.abs(got.astype(int) - plain.astype(int)) <= 1).all()  # the dither moves a code by one at most


def test_huge_phases_wrap(torch, lib):
    frame = threshold_frame()
    dev = torch.from_numpy(frame).cuda()
    got, _ = run(torch, lib, dev, abi.PT_TRANSFER_SRGB, True, (2 ** 31 - 1, -2 ** 31))
    assert np.array_equal(got, E.encode(frame, E.SRGB, True, (7, 0)))


# ---- the fused call ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cornell(torch):
    ps, cam_args = scenes.build("cornell")
    return R.render(W, H, 8, ps, scenes.make_camera(cam_args, W, H))


def display_params(lib, tone, ev_bias):
    p = abi.PtDisplayParams()
    lib.pt_display_params_init(C.byref(p))
    p.tone, p.ev_bias = tone, ev_bias
    return p


@pytest.mark.parametrize("tone", sorted(D.TONES))
@pytest.mark.parametrize("metered", [True, False], ids=["metered", "stateless"])
def test_fused_is_encode_of_display_applys_linear_out(torch, lib, cornell, tone, metered):
    fb = cornell.cpu().numpy()
    dp = display_params(lib, D.TONES[tone], 0.0 if metered else 1.5)
    handle = C.c_void_p()
    model = D.State()
    if metered:
        abi.check(lib.pt_display_create(C.byref(handle)), "pt_display_create")
        abi.check(lib.pt_display_meter(handle, C.byref(dp), C.c_void_p(cornell.data_ptr()), W, H, stream(torch)), "pt_display_meter")
        e = model.meter(fb)
    else:
        e = F(1.5)
    try:
        rgb8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        linear = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        abi.check(lib.pt_display_apply(handle, C.byref(dp), C.c_void_p(cornell.data_ptr()), W, H, C.c_void_p(rgb8.data_ptr()),
                                       C.c_void_p(linear.data_ptr()), stream(torch)), "pt_display_apply")
        want8, want_lin = D.apply(fb, e, D.TONES[tone])
        lin_host = linear.cpu().numpy()
        assert np.array_equal(lin_host.view(np.uint32), want_lin.view(np.uint32)) and np.array_equal(rgb8.cpu().numpy(), want8)
        for name, (transfer, dither) in MODES.items():
            for no_vec in (False, True):
                phase = (3, 5) if dither else (0, 0)
                two_calls, _ = run(torch, lib, linear, transfer, dither, phase, no_vec)
                fused = torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device="cuda")
                ep = params(lib, W, H, transfer, dither, phase, no_vec)
                abi.check(lib.pt_display_encode(handle, C.byref(dp), C.byref(ep), C.c_void_p(cornell.data_ptr()), C.c_void_p(fused.data_ptr()),
                                                stream(torch)), "pt_display_encode")
                rec = last(lib)
                assert rec[0] == (1 if no_vec else 2) and rec[4] == transfer + 1 and rec[5] == 1 and rec[6] == int(dither), rec
                got = fused.cpu().numpy()
                assert np.array_equal(got, two_calls), f"{tone} {name}: fused vs two calls: {differing(got, two_calls)}"
                want = E.encode(lin_host, transfer, dither, phase)
                assert np.array_equal(got, want), f"{tone} {name}: fused vs the model: {differing(got, want)}"
                if transfer == abi.PT_TRANSFER_REFERENCE:
                    assert np.array_equal(got, rgb8.cpu().numpy()), f"{tone}: the reference transfer is pt_display_apply's rgb8_out"
    finally:
        if handle:
            lib.pt_display_destroy(handle)


# ---- the stream contract ----------------------------------------------------------------------------------------------------------------

def test_both_calls_behind_pending_work_on_a_side_stream(torch, lib):
    """pt_encode and pt_display_encode are asynchronous on `stream`: queued on a non-blocking side stream behind the slow producer, their
    input written last, their outputs poisoned behind the producer, the producer still running when the calls have returned; what they
    wrote is the model's."""
    frame = threshold_frame()
    inp = SC.staged_inputs(torch, dict(linear=frame.copy()))
    out1, out2 = (torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    st = SC.stream_apart_from_the_null_stream(torch)

    def call():
        R.encode(inp["linear"][0], "srgb", True, (3, 5), out=out1)
        R.display(inp["linear"][0], "aces", 0.5, out=out2, encode=dict(dither=True, phase=(3, 5)))
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
    got, _ = SC.gated(torch, st, passes, inp.values(), [out1, out2], call)
    want1 = E.encode(frame, E.SRGB, True, (3, 5))
    with np.errstate(all="ignore"):
        want2 = E.encode(D.apply(frame, F(0.5), D.ACES)[1], E.SRGB, True, (3, 5))
    assert np.array_equal(got[0], want1), differing(got[0], want1)
    assert np.array_equal(got[1], want2), differing(got[1], want2)


# ---- refusals with live planes ----------------------------------------------------------------------------------------------------------

def test_overlap_refusals_with_live_planes(torch, lib):
    n = W * H * 3
    back = torch.zeros(n * 5 + 64, dtype=torch.uint8, device="cuda")  # the float plane at [0, 4 n), bytes after it
    base = back.data_ptr()
    assert base % 16 == 0
    p = params(lib, W, H, abi.PT_TRANSFER_SRGB)
    dp = display_params(lib, abi.PT_TONE_ACES, 0.0)
    for off in (0, 1, 4 * n - 1):
        assert lib.pt_encode(C.byref(p), base, base + off, stream(torch)) == abi.PT_ERR_INVALID_ARG
        assert b"pt_encode: rgb8_out overlaps the input" in lib.pt_last_error()
        assert lib.pt_display_encode(None, C.byref(dp), C.byref(p), base, base + off, stream(torch)) == abi.PT_ERR_INVALID_ARG
        assert b"pt_display_encode: rgb8_out overlaps the input" in lib.pt_last_error()
    assert lib.pt_encode(C.byref(p), base + n, base + 1, stream(torch)) == abi.PT_ERR_INVALID_ARG  # the bytes' last one is the plane's first
    torch.cuda.synchronize()
    assert not back.cpu().numpy().any()  # a refused call wrote nothing
    # the bytes right behind the plane: no overlap
    frame = threshold_frame()
    back[:4 * n].view(torch.float32).copy_(torch.from_numpy(frame.reshape(-1)))
    abi.check(lib.pt_encode(C.byref(p), base, base + 4 * n, stream(torch)), "pt_encode")
    assert np.array_equal(back[4 * n:5 * n].cpu().numpy().reshape(H, W, 3), E.encode(frame))


# ---- hosts ------------------------------------------------------------------------------------------------------------------------------

def test_python_hosts(torch, lib, cornell):
    fb = cornell.cpu().numpy()
    assert np.array_equal(R.encode(cornell).cpu().numpy(), E.encode(fb))
    assert np.array_equal(R.encode(cornell, "srgb", True, (3, 5)).cpu().numpy(), E.encode(fb, E.SRGB, True, (3, 5)))
    assert np.array_equal(R.encode(cornell, "reference").cpu().numpy(), R.tonemap_rgb8(cornell).cpu().numpy())
    assert np.array_equal(R.encode(cornell, no_vec=True).cpu().numpy(), E.encode(fb))
    out = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    assert R.encode(cornell, out=out) is out and np.array_equal(out.cpu().numpy(), E.encode(fb))
    with pytest.raises(ValueError):
        R.encode(cornell, "rec709")
    with pytest.raises(abi.PtError):
        R.encode(cornell, "reference", dither=True)
    # Display.apply and display(): the model's bytes with the keyword, exactly today's without
    disp = R.Display("aces", adapt_up=0.5, adapt_down=0.5)
    model = D.State()
    e = model.meter(fb, adapt_up=0.5, adapt_down=0.5)
    disp.meter(cornell)
    want8, want_lin = D.apply(fb, e, D.ACES)
    assert np.array_equal(disp.apply(cornell).cpu().numpy(), want8)
    assert last(lib)[5] == 0  # (the record is of an earlier call: apply() without the keyword made no encode call)
    assert np.array_equal(disp.apply(cornell, encode="srgb").cpu().numpy(), E.encode(want_lin))
    assert last(lib)[5] == 1
    assert np.array_equal(disp.apply(cornell, encode=dict(dither=True, phase=(-1, 9))).cpu().numpy(), E.encode(want_lin, E.SRGB, True, (-1, 9)))
    assert np.array_equal(disp.apply(cornell, encode=dict(transfer="reference")).cpu().numpy(), want8)
    with pytest.raises(ValueError):
        disp.apply(cornell, linear=True, encode="srgb")
    assert np.array_equal(R.display(cornell, "reinhard", 1.0, encode="srgb").cpu().numpy(), E.encode(D.apply(fb, F(1.0), D.REINHARD)[1]))
    assert np.array_equal(R.display(cornell, "reinhard", 1.0).cpu().numpy(), D.apply(fb, F(1.0), D.REINHARD)[0])
    # Accumulator.display and render_temporal
    ps, cam_args = scenes.build("cornell")
    cams = moving_cameras(cam_args, W, H, 2, (10.0, 0.0, 0.0))
    acc = R.Accumulator(W, H, ps, cams[0])
    acc.add(4)
    disp.reset()
    shown = acc.display(disp, encode="srgb").cpu().numpy()
    res = acc.resolve().cpu().numpy()
    acc.close()
    model.reset()
    assert np.array_equal(shown, E.encode(D.apply(res, model.meter(res, adapt_up=0.5, adapt_down=0.5), D.ACES)[1]))
    kw = dict(aov_spp=4, denoise_kw=dict(iterations=2))
    disp.reset()
    with_kw = list(R.render_temporal(W, H, 4, ps, cams, display=disp, encode=dict(dither=True), **kw))
    disp.reset()
    without = list(R.render_temporal(W, H, 4, ps, cams, display=disp, **kw))
    model.reset()
    for f, (a, b) in enumerate(zip(with_kw, without)):
        filtered = a["filtered"].cpu().numpy()
        assert np.array_equal(filtered.view(np.uint32), b["filtered"].cpu().numpy().view(np.uint32)), f
        want8, want_lin = D.apply(filtered, model.meter(filtered, adapt_up=0.5, adapt_down=0.5), D.ACES)
        assert np.array_equal(a["rgb8"].cpu().numpy(), E.encode(want_lin, E.SRGB, True)), f
        assert np.array_equal(b["rgb8"].cpu().numpy(), want8), f  # without the keyword: today's bytes
    with pytest.raises(ValueError):
        next(R.render_temporal(W, H, 4, ps, cams, encode="srgb", **kw))
    disp.close()


def test_cpp_facade(torch, lib, cornell, tmp_path):
    from test_encode_cpu import png_chunks

    exe = tmp_path / "encode_main"
    libdir = ROOT / "path_tracer_amd"
    subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{libdir / 'include'}",
                    str(ROOT / "tests" / "cpp" / "encode_main.cpp"), "-o", str(exe), f"-L{libdir}", "-lpt_render", "-L/opt/rocm/lib",
                    "-lamdhip64", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    fb = cornell.cpu().numpy()
    src, out, png = tmp_path / "in.bin", tmp_path / "out.bin", tmp_path / "out.png"
    src.write_bytes(fb.tobytes())
    subprocess.run([str(exe), str(W), str(H), "0.5", str(src), str(out), str(png)], check=True, timeout=300)
    raw = np.frombuffer(out.read_bytes(), np.uint8)
    n3 = W * H * 3
    assert raw.size == 4 * n3
    images = raw.reshape(4, H, W, 3)
    assert np.array_equal(images[0], E.encode(fb))
    assert np.array_equal(images[1], E.encode(fb, E.SRGB, True, (3, 5)))
    assert np.array_equal(images[2], E.encode(D.apply(fb, F(0.5), D.ACES)[1], E.SRGB, True, (3, 5)))
    assert np.array_equal(images[3], E.encode(fb, E.REFERENCE))
    from PIL import Image
    assert [t for t, _ in png_chunks(png.read_bytes())] == [b"IHDR", b"sRGB", b"gAMA", b"IDAT", b"IEND"]
    with Image.open(png) as im:
        assert np.array_equal(np.asarray(im), images[0])


def test_cli_writes_a_tagged_display_out_and_leaves_out_png_alone(torch, lib, tmp_path):
    from PIL import Image

    from test_encode_cpu import png_chunks

    base = ["--scene", "cornell", "--width", "64", "--height", "40", "--spp", "16"]

    def cli(*args):
        p = subprocess.run([sys.executable, "-m", "path_tracer_amd", *base, *args], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ), timeout=300)
        assert p.returncode == 0, p.stderr
    plain, with_encode, shown, old_shown = (tmp_path / n for n in ("plain.png", "with.png", "shown.png", "old_shown.png"))
    frames_dir = tmp_path / "frames"
    cli("--out", str(plain), "--tone", "aces", "--exposure", "0.5", "--display-out", str(old_shown))
    cli("--out", str(with_encode), "--tone", "aces", "--exposure", "0.5", "--display-out", str(shown), "--encode", "srgb", "--dither",
        "--frames", "2", "--move", "60,0,0", "--frames-dir", str(frames_dir))
    assert plain.read_bytes() == with_encode.read_bytes()
    ps, cam_args = scenes.build("cornell")
    fb = R.render(64, 40, 16, ps, scenes.make_camera(cam_args, 64, 40)).cpu().numpy()
    want8, want_lin = D.apply(fb, F(0.5), D.ACES)
    tags = [t for t, _ in png_chunks(shown.read_bytes())]
    assert tags == [b"IHDR", b"sRGB", b"gAMA", b"IDAT", b"IEND"]
    assert [t for t, _ in png_chunks(old_shown.read_bytes())] == [b"IHDR", b"IDAT", b"IEND"] == [t for t, _ in png_chunks(plain.read_bytes())]
    with Image.open(shown) as im:
        assert np.array_equal(np.asarray(im), E.encode(want_lin, E.SRGB, True))
    with Image.open(old_shown) as im:
        assert np.array_equal(np.asarray(im), want8)
    for f, cam in enumerate(moving_cameras(cam_args, 64, 40, 2, (60.0, 0.0, 0.0))):
        fb = R.render(64, 40, 16, ps, cam).cpu().numpy()
        data = (frames_dir / f"frame_{f}.png").read_bytes()
        assert [t for t, _ in png_chunks(data)][1] == b"sRGB"
        with Image.open(frames_dir / f"frame_{f}.png") as im:
            assert np.array_equal(np.asarray(im), E.encode(D.apply(fb, F(0.5), D.ACES)[1], E.SRGB, True)), f
