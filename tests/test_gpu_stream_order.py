"""Every stream-taking entry point of include/pt_render.h on a NON-BLOCKING side stream, held to its stream contract
(tests/stream_contract.py: CONTRACT and the harness).

The other GPU tests run on torch's current stream, the legacy default stream: every blocking stream synchronises with it and every test
ends in a device-wide synchronise, so a kernel, memset or copy on the wrong stream, device work a *_create leaves on the default stream,
a hidden host synchronisation and a synchronising call that returns early are all invisible there.  Here each call runs on a
torch.cuda.Stream() behind a slow producer whose last step writes the call's inputs (stream_contract.gated), and what it wrote is compared
BIT FOR BIT with the oracle (orc.render, orc.camera_rays / orc.bounce) and the numpy models (denoise_model, variance_model,
temporal_model, display_model, test_aov_cpu.aov_np, test_adaptive_cpu's restatements) — never with a default-stream run alone.

Frames: S.ALL["cornell"] and S.ALL["mixed"] at 40 x 24 (15 tiles) x 8 spp; the image-space stages at 70 x 45 and 19 x 13."""
import ctypes as C

import numpy as np
import pytest

import denoise_model as M
import display_model as D
import kernel_variant_cases as K
import scenes_small as S
import stream_contract as SC
import temporal_model as T
import variance_model as V
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from test_aov_cpu import PLANES, aov_reference
from test_gpu_adaptive import rng_index
from test_gpu_aov import same_planes
from test_gpu_display import special_frame
from test_gpu_fuzz import random_triangle_field, tri_pools
from test_gpu_temporal import STEPS, cam_of, moving_cameras, with_colour
from test_gpu_temporal import planes as image_planes

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SPP, AOV_SPP = 40, 24, 8, 4
SCENES = ["cornell", "mixed"]
IMAGE_SIZES = [(70, 45), (19, 13)]
DENOISE_KW = dict(iterations=3, sigma_color=1.5, sigma_normal=0.6, sigma_depth=0.5, sigma_albedo=0.8, demodulate=True)
VDENOISE_KW = dict(iterations=3, sigma_variance=2.0, sigma_normal=0.6, sigma_depth=0.5, sigma_albedo=0.8, demodulate=True)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch


_worlds, _refs = {}, {}


def world(name):
    """(packed scene, the three cameras of its path at W x H): built once."""
    if name not in _worlds:
        ps, cam_args = S.ALL[name]()
        _worlds[name] = (ps, moving_cameras(cam_args, W, H, 3, STEPS[name]))
    return _worlds[name]


def ref_render(orc, name, spp, **shard):
    key = (name, spp, tuple(sorted(shard.items())))
    if key not in _refs:
        ps, cams = world(name)
        orc.set_math(True)
        _refs[key] = orc.render(ps, cams[0].c, W, H, spp, **shard)
        _refs[key].setflags(write=False)
    return _refs[key]


def ref_chain(orc, name):
    if ("chain", name) not in _refs:
        ps, cams = world(name)
        _refs["chain", name] = SC.chain_expected(orc, ps, cams, W, H)
    return _refs["chain", name]


@pytest.fixture(scope="session")
def sizing():
    """The producer's pass count, from two times measured on the otherwise idle device: the device time of one pass (HIP events) and the
    host wall time of the longest call sequence queued behind a producer (three frames of the whole chain).  The producer runs at least
    20 x that host time — headroom for a descheduled host thread on a shared box — and at least 30 ms (profiles/stream_contract.txt)."""
    import torch
    host_ms = 0.0
    for name in SCENES:
        ps, cams = world(name)
        ds = R.DeviceScene(ps)
        host_ms = max(host_ms, SC.chain_host_ms(torch, ds, cams, W, H))
        torch.cuda.synchronize()
        ds.close()
    pass_ms = SC.measure_pass_ms(torch)
    out = dict(pass_ms=pass_ms, host_ms=host_ms, passes=SC.passes_for(host_ms, pass_ms), floats=SC.PRODUCER_FLOATS)
    print(f"stream contract sizing: one pass over {out['floats']} floats {pass_ms:.4f} ms, chain host time {host_ms:.3f} ms -> {out['passes']} passes")
    return out


def warm_scene(torch, name):
    """A DeviceScene whose launch workspaces are sized for W x H (the first render of a scene at a new size allocates)."""
    ps, cams = world(name)
    ds = R.DeviceScene(ps)
    ds.reserve(W, H, SPP)
    R.render(W, H, SPP, ds, cams[0])
    torch.cuda.synchronize()
    return ds


def stream_ptr(s):
    return C.c_void_p(s.cuda_stream)


def same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} differ"


# ---- a. ordering behind pending work, one test per stage ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_render_behind_pending_work(torch, orc, sizing, name):
    ds, cam = warm_scene(torch, name), world(name)[1][0]
    out = SC.poison(torch.empty((H, W, 3), dtype=torch.float32, device="cuda"))
    st = torch.cuda.Stream()

    def call():
        R.render(W, H, SPP, ds, cam, out=out)
    (got,), _ = SC.gated(torch, st, sizing["passes"], [], [out], call)
    assert_bit_identical(got, ref_render(orc, name, SPP), f"{name}: pt_render on a side stream")
    ds.close()


@pytest.mark.parametrize("name", SCENES)
def test_render_aov_behind_pending_work(torch, orc, sizing, name):
    """All six planes, written into planes the test owns and poisons behind the producer."""
    ds, cam = warm_scene(torch, name), world(name)[1][0]
    planes = {k: torch.empty((H, W) + ((3,) if abi.AOV_CHANNELS[k] == 3 else ()), dtype=torch.int32 if k == "id" else torch.float32, device="cuda")
              for k in PLANES}
    bufs = abi.PtAovBuffers(struct_size=C.sizeof(abi.PtAovBuffers))
    for k, t in planes.items():
        setattr(bufs, k, t.data_ptr())
    p = abi.PtRenderParams(W, H, AOV_SPP, 1, 0, 1, 0, 0)
    st = torch.cuda.Stream()

    def call():
        abi.check(ds.lib.pt_render_aov(ds.handle, C.byref(cam.c), C.byref(p), C.byref(bufs), stream_ptr(st)), "pt_render_aov")
    got, _ = SC.gated(torch, st, sizing["passes"], [], [planes[k] for k in PLANES], call)
    same_planes(dict(zip(PLANES, got)), aov_reference(orc, name, W, H, AOV_SPP), f"{name}: pt_render_aov on a side stream")
    ds.close()


@pytest.mark.parametrize("w,h", IMAGE_SIZES)
def test_tonemap_behind_pending_work(torch, sizing, w, h):
    frame = special_frame(w, h, 3)
    inp = SC.staged_inputs(torch, dict(fb=frame))
    out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    st, lib = torch.cuda.Stream(), abi.load_library()

    def call():
        abi.check(lib.pt_tonemap_rgb8(C.c_void_p(inp["fb"][0].data_ptr()), w, h, C.c_void_p(out.data_ptr()), stream_ptr(st)), "pt_tonemap_rgb8")
    (got,), _ = SC.gated(torch, st, sizing["passes"], inp.values(), [out], call)
    same_bytes(got, SC.tonemap_np(frame), f"{w} x {h}: pt_tonemap_rgb8 on a side stream")


@pytest.mark.parametrize("name", SCENES)
def test_unshard_behind_pending_work(torch, orc, sizing, name):
    """The gathered buffer's shards 0 and 2 are the oracle's, copied in behind the producer; shard 1 of 3 is rendered into its slot on the
    stream, then the frame is un-interleaved: the oracle's whole frame."""
    ds, cam = warm_scene(torch, name), world(name)[1][0]
    shards = np.stack([ref_render(orc, name, SPP, shard_index=k, shard_count=3) for k in range(3)])
    shards[1] = np.nan  # (the render's to write)
    R.render(W, H, SPP, ds, cam, shard_index=1, shard_count=3)  # (sizes the workspaces of the sharded launch)
    inp = SC.staged_inputs(torch, dict(gathered=shards))
    gathered = inp["gathered"][0]
    fb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    p = abi.PtRenderParams(W, H, 1, 1, 0, 3, 0, 0)
    st = torch.cuda.Stream()

    def call():
        R.render(W, H, SPP, ds, cam, shard_index=1, shard_count=3, out=gathered[1])
        abi.check(ds.lib.pt_unshard_tiles(C.c_void_p(gathered.data_ptr()), C.byref(p), C.c_void_p(fb.data_ptr()), stream_ptr(st)), "pt_unshard_tiles")
    (got,), _ = SC.gated(torch, st, sizing["passes"], inp.values(), [fb], call)
    assert_bit_identical(got, ref_render(orc, name, SPP), f"{name}: shard 1 of 3 rendered and un-interleaved on a side stream")
    ds.close()


@pytest.mark.parametrize("w,h", IMAGE_SIZES)
def test_denoise_behind_pending_work(torch, sizing, w, h):
    g = image_planes(w, h, 11)
    inp = SC.staged_inputs(torch, {k: g[k] for k in ("color", "albedo", "normal", "depth")})
    dev = {k: v[0] for k, v in inp.items()}
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()

    def call():
        R.denoise(dev["color"], albedo=dev["albedo"], normal=dev["normal"], depth=dev["depth"], out=out, **DENOISE_KW)
    (got,), _ = SC.gated(torch, st, sizing["passes"], inp.values(), [out], call)
    assert_bit_identical(got, M.denoise(g["color"], albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **DENOISE_KW),
                         f"{w} x {h}: pt_denoise on a side stream")


@pytest.mark.parametrize("w,h", IMAGE_SIZES)
def test_variance_denoise_behind_pending_work(torch, sizing, w, h):
    g = image_planes(w, h, 12)
    inp = SC.staged_inputs(torch, {k: g[k] for k in ("color", "variance", "albedo", "normal", "depth")})
    dev = {k: v[0] for k, v in inp.items()}
    out, vout = (torch.empty((h, w, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    st = torch.cuda.Stream()

    def call():
        R.denoise_variance(dev["color"], dev["variance"], albedo=dev["albedo"], normal=dev["normal"], depth=dev["depth"], out=out, variance_out=vout,
                           **VDENOISE_KW)
    got, _ = SC.gated(torch, st, sizing["passes"], inp.values(), [out, vout], call)
    want = V.denoise(g["color"], g["variance"], albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **VDENOISE_KW)
    assert_bit_identical(got[0], want[0], f"{w} x {h}: pt_variance_denoise on a side stream, colour")
    assert_bit_identical(got[1], want[1], f"{w} x {h}: pt_variance_denoise on a side stream, variance_out")


@pytest.mark.parametrize("w,h", IMAGE_SIZES)
def test_temporal_push_behind_pending_work(torch, sizing, w, h):
    """Three pushes — the same camera, a sub-pixel move, a move of several pixels — with every optional plane."""
    g = image_planes(w, h, 21)
    frames = [g, with_colour(g, 22), with_colour(g, 23)]
    cams = [cam_of(w, h), cam_of(w, h, (0.004, -0.003, 0.0)), cam_of(w, h, (0.35, 0.2, -0.05), (0.3, 0.25, -1.0))]
    tol = dict(tol_depth=0.5, tol_normal=1.5)
    host = {k: g[k] for k in ("depth", "normal", "id")}
    for f, fr in enumerate(frames):
        host[f"color{f}"], host[f"variance{f}"] = fr["color"], fr["variance"]
    inp = SC.staged_inputs(torch, host)
    dev = {k: v[0] for k, v in inp.items()}
    outs = [torch.empty((h, w, 3), dtype=torch.float32, device="cuda") for _ in frames]
    hist, st = R.TemporalAccumulator(w, h), torch.cuda.Stream()

    def call():
        more = []
        for f, cam in enumerate(cams):
            more += hist.push(dev[f"color{f}"], cam, depth=dev["depth"], normal=dev["normal"], id=dev["id"], variance=dev[f"variance{f}"], out=outs[f],
                              **tol)[1:]
        return more
    got, more = SC.gated(torch, st, sizing["passes"], inp.values(), outs, call)
    model = T.Temporal(w, h)
    for f, (cam, fr) in enumerate(zip(cams, frames)):
        want = model.push(cam.c, fr["color"], g["depth"], normal=g["normal"], id=g["id"], variance_in=fr["variance"], **dict(T.DEFAULTS, **tol))
        for name, a, b in zip(("colour", "variance", "history"), (got[f], more[2 * f], more[2 * f + 1]), want):
            assert_bit_identical(a, b, f"{w} x {h}: push {f} on a side stream: {name}")
    assert hist.frames == 3
    if w * h >= 19 * 13:
        assert (more[3] > 1.5).any(), "the sub-pixel move must find histories"
    hist.close()


@pytest.mark.parametrize("w,h", IMAGE_SIZES)
def test_display_behind_pending_work(torch, sizing, w, h):
    """meter + apply over three frames with adaptation, a manual exposure and a reset in between; nothing comes back to the host."""
    base = special_frame(w, h, 9)
    with np.errstate(over="ignore"):
        frames = [(base * F(2.0 ** k)).astype(F) for k in (0, -5, 3)]
    kw = dict(adapt_up=0.5, adapt_down=0.125, ev_bias=0.25)
    inp = SC.staged_inputs(torch, {f"f{k}": fr for k, fr in enumerate(frames)})
    dev = [inp[f"f{k}"][0] for k in range(3)]
    disp, st = R.Display("aces", **kw), torch.cuda.Stream()
    # (which frame is shown, after which call on the state)
    script = [("meter", 0), ("meter", 1), ("set", 1), ("meter", 2), ("reset", 2), ("meter", 2)]

    def call():
        more = []
        for what, k in script:
            if what == "meter":
                disp.meter(dev[k])
            elif what == "set":
                disp.set_exposure(1.5)
            else:
                disp.reset()
            more += disp.apply(dev[k], linear=True)
        return more
    _, more = SC.gated(torch, st, sizing["passes"], inp.values(), [], call)
    model = D.State()
    for i, (what, k) in enumerate(script):
        if what == "meter":
            with np.errstate(all="ignore"):
                model.meter(frames[k], **kw)
        elif what == "set":
            model.set_exposure(1.5)
        else:
            model.reset()
        want8, want_lin = D.apply(frames[k], model.e, D.ACES)
        same_bytes(more[2 * i], want8, f"{w} x {h}: step {i} ({what}) on a side stream: rgb8")
        assert_bit_identical(more[2 * i + 1], want_lin, f"{w} x {h}: step {i} ({what}) on a side stream: linear")
    assert F(disp.exposure()) == model.e and disp.frames == 1
    disp.close()


# ---- b. object state ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_plain_accumulator_behind_pending_work(torch, orc, sizing, name):
    ds, cam = warm_scene(torch, name), world(name)[1][0]
    acc = R.Accumulator(W, H, ds, cam)
    o8, o3 = (torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    st = torch.cuda.Stream()

    def call():
        acc.add(3).add(5)
        acc.resolve(out=o8)
        rgb8 = acc.tonemap_rgb8()
        acc.reset()
        acc.add(4)
        acc.reset()
        acc.add(3)
        acc.resolve(out=o3)
        return [rgb8]
    (got8, got3), (rgb8,) = SC.gated(torch, st, sizing["passes"], [], [o8, o3], call)
    assert_bit_identical(got8, ref_render(orc, name, 8), f"{name}: add(3); add(5); resolve")
    assert_bit_identical(got3, ref_render(orc, name, 3), f"{name}: add(4); reset; add(3); resolve")
    same_bytes(rgb8, SC.tonemap_np(ref_render(orc, name, 8)), f"{name}: pt_accum_tonemap_rgb8")
    acc.close()
    ds.close()


@pytest.mark.parametrize("name", SCENES)
def test_adaptive_accumulator_behind_pending_work(torch, orc, sizing, name):
    """Two gated runs (a masked window synchronises the stream, so what follows it has nothing pending): next_frame between two images,
    all asynchronous; then unmasked, masked, unmasked windows and every read-out, against the restatements over the oracle."""
    ps, cams = world(name)
    ds = warm_scene(torch, name)
    acc = R.Accumulator(W, H, ds, cams[0], adaptive=True)
    st = torch.cuda.Stream()
    model = SC.HostAccum(orc, ps, W, H)

    def two_images():
        acc.add(4)
        first = acc.resolve()
        acc.next_frame(cams[1])
        acc.add(3).add(5)
        return [first, acc.resolve(), acc.variance(), acc.error(), acc.counts()]
    _, got = SC.gated(torch, st, sizing["passes"], [], [], two_images)
    model.window(cams[0].c, 4)
    assert_bit_identical(got[0], model.resolve(), f"{name}: the first image")
    assert_bit_identical(got[0], ref_render(orc, name, 4), f"{name}: the first image is pt_render's")
    model.next_frame().window(cams[1].c, 3).window(cams[1].c, 5)
    assert_bit_identical(got[1], model.resolve(), f"{name}: the image after next_frame continues every pixel's stream")
    assert_bit_identical(got[2], model.variance(), f"{name}: its variance estimate")
    assert_bit_identical(got[3], model.error(), f"{name}: its error estimate")
    assert np.array_equal(got[4], model.counts())

    mask = (np.random.default_rng(3).random((H, W)) < 0.4).astype(np.uint8)
    inp = SC.staged_inputs(torch, dict(mask=mask))
    acc.cam = cams[0]

    def windows():
        acc.reset()
        acc.add(4)
        acc.add(3, inp["mask"][0])
        acc.add(2)
        return [acc.counts(), acc.error(), acc.variance(), acc.resolve()]
    _, got = SC.gated(torch, st, sizing["passes"], inp.values(), [], windows, synchronises=True)
    model.reset().window(cams[0].c, 4).window(cams[0].c, 3, mask).window(cams[0].c, 2)
    assert np.array_equal(got[0], model.counts()) and set(np.unique(got[0])) == {6, 9}
    assert_bit_identical(got[1], model.error(), f"{name}: pt_adaptive_error")
    assert_bit_identical(got[2], model.variance(), f"{name}: pt_variance_estimate")
    assert_bit_identical(got[3], model.resolve(), f"{name}: pt_accum_resolve after a masked window")
    assert np.isfinite(got[1]).all()
    acc.close()
    ds.close()


# ---- c. checkpoints -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive"])
def test_checkpoints_behind_pending_work(torch, orc, sizing, adaptive):
    """export on the side stream behind the producer holds the finished window; import followed at once by add and resolve on the stream
    is the one-shot render."""
    name = "mixed"
    ps, cams = world(name)
    ds = warm_scene(torch, name)
    acc, acc2 = (R.Accumulator(W, H, ds, cams[0], adaptive=adaptive) for _ in range(2))
    st = torch.cuda.Stream()
    SC.slow_producer(torch, st, sizing["passes"])
    with torch.cuda.stream(st):
        acc.add(5)
        state = acc.state()
        assert st.query(), "an export synchronises its stream"
    model = SC.HostAccum(orc, ps, W, H).window(cams[0].c, 5)
    o, n = abi.PT_ACCUM_HEADER_BYTES, W * H * 3
    assert_bit_identical(np.frombuffer(state[o:o + 4 * n].tobytes(), dtype=F).reshape(-1, 3), model.S, "the exported sums hold the finished window")
    rng = np.frombuffer(state[o + 4 * n:o + 4 * n + 4 * 64 * 15].tobytes(), dtype=np.uint32)
    assert np.array_equal(rng[rng_index(W, H)], model.state), "the exported generator states are where the window left them"
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")

    def resume():
        acc2.restore(state)
        acc2.add(3)
        acc2.resolve(out=out)
    (got,), _ = SC.gated(torch, st, sizing["passes"], [], [out], resume, synchronises=True)
    assert_bit_identical(got, ref_render(orc, name, 8), "import; add; resolve on a side stream")
    for a in (acc, acc2):
        a.close()
    ds.close()


# ---- d. the whole chain on a side stream ----------------------------------------------------------------------------------------------

def check_chain(got, want, what):
    assert len(got) == len(want) == 3
    for f, (g, w_) in enumerate(zip(got, want)):
        for k in SC.CHAIN_OUTPUTS:
            if k == "rgb8":
                same_bytes(g[k], w_[k], f"{what}, frame {f}: rgb8")
            else:
                assert_bit_identical(g[k], w_[k], f"{what}, frame {f}: {k}")


@pytest.mark.parametrize("name", SCENES)
def test_the_whole_chain_on_a_side_stream(torch, orc, sizing, name):
    """render -> render_aov -> temporal push -> denoise_variance -> display: three frames of render_temporal inside torch.cuda.stream(s),
    behind the producer; every output of every frame against the same models chained on the host."""
    ps, cams = world(name)
    ds = warm_scene(torch, name)
    # render_temporal creates its accumulator itself, and pt_adaptive_create ends in a synchronise of the null stream (its clears run there)
    disp, st = R.Display("aces", **SC.CHAIN["display_kw"]), SC.stream_apart_from_the_null_stream(torch)
    SC.scrub(torch, st, W * H)
    SC.slow_producer(torch, st, sizing["passes"])
    marker = SC.pending_marker(torch, st)
    snaps, pending = [], []
    with torch.cuda.stream(st):
        for fr in R.render_temporal(W, H, SC.CHAIN["spp"], ds, cams, aov_spp=SC.CHAIN["aov_spp"], denoise_kw=SC.CHAIN["denoise_kw"], display=disp):
            snaps.append({k: fr[k].clone() for k in SC.CHAIN_OUTPUTS})
            pending.append(not marker.query())  # (read per frame: the generator frees its objects, which waits for the device, when it ends)
    st.synchronize()
    assert pending == [True] * 3, f"the producer had finished before frame {pending.index(False)} was queued: the chain did not run behind pending work"
    check_chain([{k: v.cpu().numpy() for k, v in fr.items()} for fr in snaps], ref_chain(orc, name), name)
    assert (snaps[2]["history"] > 2.5).float().mean() > 0.3, "most of the frame should have carried its history across the moves"
    disp.close()
    ds.close()


# ---- e. two chains at once ------------------------------------------------------------------------------------------------------------

def test_two_chains_interleaved_call_by_call(torch, orc, sizing):
    """Two side streams, each with its own DeviceScene, adaptive Accumulator, TemporalAccumulator and Display, different scenes and
    cameras; the calls alternate one by one from this one host thread (the header's rule) and nothing synchronises until the end."""
    chains = []
    for name in SCENES:
        ps, cams = world(name)
        ds = warm_scene(torch, name)
        chains.append(dict(name=name, ds=ds, cams=cams, st=torch.cuda.Stream(), acc=R.Accumulator(W, H, ds, cams[0], adaptive=True),
                           hist=R.TemporalAccumulator(W, H), disp=R.Display("aces", **SC.CHAIN["display_kw"]), frames=[]))
    torch.cuda.synchronize()
    for c in chains:
        SC.scrub(torch, c["st"], W * H)
        SC.slow_producer(torch, c["st"], sizing["passes"])
        c["marker"] = SC.pending_marker(torch, c["st"])
    gens = [SC.chain_calls(torch, c["st"], c["ds"], c["cams"], W, H, c["acc"], c["hist"], c["disp"], c["frames"]) for c in chains]
    calls = 0
    while gens:
        for g in list(gens):
            try:
                next(g)
                calls += 1
            except StopIteration:
                gens.remove(g)
    assert calls == 2 * (3 * 9 + 2)
    for c in chains:
        with torch.cuda.stream(c["st"]):
            c["snaps"] = [{k: v.clone() for k, v in fr.items()} for fr in c["frames"]]
    pending = [not c["marker"].query() for c in chains]
    torch.cuda.synchronize()
    assert all(pending), "a producer had finished before both chains were queued: they did not run behind pending work"
    for c in chains:
        check_chain([{k: v.cpu().numpy() for k, v in fr.items()} for fr in c["snaps"]], ref_chain(orc, c["name"]), f"{c['name']} beside the other chain")
        for k in ("acc", "hist", "disp", "ds"):
            c[k].close()


# ---- f. creation while the default stream is busy --------------------------------------------------------------------------------------

def test_objects_created_while_the_default_stream_is_busy(torch, orc, sizing):
    """A *_create that clears its buffers on the default stream must have finished clearing when it returns: a non-blocking stream does not
    wait for the default stream.  The producer runs on the default stream while each object is created, and each is used at once on a
    side stream."""
    name = "cornell"
    ps, cams = world(name)
    ds = warm_scene(torch, name)
    default, st = torch.cuda.default_stream(), torch.cuda.Stream()
    w, h = IMAGE_SIZES[0]
    g = image_planes(w, h, 31)
    frames = [g, with_colour(g, 32)]
    dev = [{k: torch.from_numpy(np.ascontiguousarray(fr[k])).cuda() for k in ("color", "variance", "depth", "normal", "id")} for fr in frames]
    tps, tcam_args = random_triangle_field(8003)
    tcam = scenes.make_camera(tcam_args, W, H)
    torch.cuda.synchronize()

    def busy():
        SC.slow_producer(torch, default, sizing["passes"])

    busy()
    plain = R.Accumulator(W, H, ds, cams[0])
    # A plain accumulator's FIRST window reads neither `sum` nor `rng` (it seeds and overwrites), so clears still queued behind the producer
    # would not spoil it — they would wipe what it wrote afterwards.  Hence: a first window at once, then, when the default stream has
    # drained and any late clear has landed, the windows that resume from the state, and the state itself.
    with torch.cuda.stream(st):
        plain.add(3)
    st.synchronize()
    default.synchronize()
    with torch.cuda.stream(st):
        plain_state = plain.state()
        fb_plain = plain.add(5).resolve()
    st.synchronize()  # (the scene's launch workspaces are one stream's at a time)
    busy()
    adaptive = R.Accumulator(W, H, ds, cams[0], adaptive=True)
    with torch.cuda.stream(st):
        adaptive.add(4).add(4)
        fb_adaptive, counts, var = adaptive.resolve(), adaptive.counts(), adaptive.variance()
    busy()
    hist = R.TemporalAccumulator(w, h)
    with torch.cuda.stream(st):
        pushes = [hist.push(d["color"], cam_of(w, h), depth=d["depth"], normal=d["normal"], id=d["id"], variance=d["variance"]) for d in dev]
    busy()
    disp = R.Display("reinhard", white=3.0)
    with torch.cuda.stream(st):
        shown = disp.meter(dev[0]["color"]).apply(dev[0]["color"])
    busy()
    with tri_pools():
        tds = R.DeviceScene(tps)
    with torch.cuda.stream(st):
        fb_tri = R.render(W, H, SPP, tds, tcam)
    torch.cuda.synchronize()
    assert K.ran(K.last_kernels(tds)[1], tripool=1), K.last_kernels(tds)

    first = SC.HostAccum(orc, ps, W, H).window(cams[0].c, 3)
    o, n = abi.PT_ACCUM_HEADER_BYTES, W * H * 3
    assert_bit_identical(np.frombuffer(plain_state[o:o + 4 * n].tobytes(), dtype=F).reshape(-1, 3), first.S,
                         "a plain accumulator created while the default stream is busy: its sums once the default stream has drained")
    rng = np.frombuffer(plain_state[o + 4 * n:o + 4 * n + 4 * 64 * 15].tobytes(), dtype=np.uint32)
    assert np.array_equal(rng[rng_index(W, H)], first.state), "a plain accumulator created while the default stream is busy: its generator states"
    assert_bit_identical(fb_plain.cpu().numpy(), ref_render(orc, name, SPP), "a plain accumulator created while the default stream is busy: add(3); add(5)")
    model = SC.HostAccum(orc, ps, W, H).window(cams[0].c, 4).window(cams[0].c, 4)
    assert_bit_identical(fb_adaptive.cpu().numpy(), ref_render(orc, name, SPP), "an adaptive accumulator created while the default stream is busy")
    assert_bit_identical(var.cpu().numpy(), model.variance(), "its variance estimate")
    assert bool((counts == 8).all())
    tm = T.Temporal(w, h)
    for f, (fr, got) in enumerate(zip(frames, pushes)):
        want = tm.push(cam_of(w, h).c, fr["color"], fr["depth"], normal=fr["normal"], id=fr["id"], variance_in=fr["variance"], **T.DEFAULTS)
        for what, a, b in zip(("colour", "variance", "history"), got, want):
            assert_bit_identical(a.cpu().numpy(), b, f"a TemporalAccumulator created while the default stream is busy, push {f}: {what}")
    dm = D.State()
    with np.errstate(all="ignore"):
        e = dm.meter(g["color"])
    same_bytes(shown.cpu().numpy(), D.apply(g["color"], e, D.REINHARD, 3.0)[0], "a Display created while the default stream is busy")
    orc.set_math(True)
    assert_bit_identical(fb_tri.cpu().numpy(), orc.render(tps, tcam.c, W, H, SPP), "a triangle-pool DeviceScene created while the default stream is busy")
    for o in (plain, adaptive, hist, disp, tds, ds):
        o.close()


# ---- g. the blocking contract, row by row ----------------------------------------------------------------------------------------------

class Rig:
    """Live objects and device planes for one call of every row of CONTRACT, everything allocated and warmed beforehand."""

    def __init__(self, torch):
        self.torch, self.lib = torch, abi.load_library()
        ps, cams = world("cornell")
        self.cam, self.cam2 = cams[0], cams[1]
        self.ds = warm_scene(torch, "cornell")
        self.plain = R.Accumulator(W, H, self.ds, self.cam)
        self.adaptive = R.Accumulator(W, H, self.ds, self.cam, adaptive=True)
        self.plain.add(2)
        self.adaptive.add(2).add(2)
        self.plain_state, self.adaptive_state = self.plain.state(), self.adaptive.state()
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")  # noqa: E731
        self.fb, self.fb2, self.var = f32(H, W, 3), f32(H, W, 3), f32(H, W, 3)
        self.rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        self.gathered = f32(3, 5, 64, 3)
        self.counts = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        self.err = f32(H, W)
        self.mask = torch.from_numpy((np.random.default_rng(5).random((H, W)) < 0.5).astype(np.uint8)).cuda()
        self.no_mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        self.sel = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        self.aov = R.render_aov(W, H, AOV_SPP, self.ds, self.cam)
        self.bufs = abi.PtAovBuffers(struct_size=C.sizeof(abi.PtAovBuffers))
        for k, t in self.aov.items():
            setattr(self.bufs, k, t.data_ptr())
        self.aov_p = abi.PtRenderParams(W, H, AOV_SPP, 1, 0, 1, 0, 0)
        self.unshard_p = abi.PtRenderParams(W, H, 1, 1, 0, 3, 0, 0)
        w, h = IMAGE_SIZES[0]
        self.w, self.h = w, h
        g = image_planes(w, h, 41)
        self.g = {k: torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("color", "variance", "albedo", "normal", "depth", "id")}
        self.out, self.vout, self.tout = f32(h, w, 3), f32(h, w, 3), f32(h, w, 3)
        self.out8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        self.hist, self.disp = R.TemporalAccumulator(w, h), R.Display("aces", adapt_up=0.5, adapt_down=0.5)
        self.icam = cam_of(w, h)
        torch.cuda.synchronize()

    def close(self):
        for o in (self.plain, self.adaptive, self.hist, self.disp, self.ds):
            o.close()

    def ptr(self, s):
        return stream_ptr(s)


def _p(t):
    return C.c_void_p(t.data_ptr())


# row -> (prepare | None, call): `prepare` (torch's current stream is the side stream; synchronised before the producer starts) puts the
# object into the state the call needs; `call(rig, stream)` is ONE call of the entry point.
ROWS = {
    "pt_render": (None, lambda r, s: R.render(W, H, SPP, r.ds, r.cam, out=r.fb)),
    "pt_render_timed": (None, lambda r, s: R.render(W, H, SPP, r.ds, r.cam, out=r.fb, timed=True)),
    "pt_unshard_tiles": (None, lambda r, s: abi.check(r.lib.pt_unshard_tiles(_p(r.gathered), C.byref(r.unshard_p), _p(r.fb2), r.ptr(s)), "pt_unshard_tiles")),
    "pt_tonemap_rgb8": (None, lambda r, s: abi.check(r.lib.pt_tonemap_rgb8(_p(r.fb2), W, H, _p(r.rgb8), r.ptr(s)), "pt_tonemap_rgb8")),
    "pt_accum_reset": (None, lambda r, s: r.plain.reset()),
    "pt_render_accumulate": (None, lambda r, s: r.plain.add(2)),
    "pt_accum_resolve": (lambda r: r.plain.add(2), lambda r, s: r.plain.resolve(out=r.fb2)),
    "pt_accum_tonemap_rgb8": (lambda r: r.plain.add(2), lambda r, s: abi.check(r.lib.pt_accum_tonemap_rgb8(r.plain.handle, _p(r.rgb8), r.ptr(s)),
                                                                                "pt_accum_tonemap_rgb8")),
    "pt_accum_export": (lambda r: r.plain.add(2), lambda r, s: r.plain.state()),
    "pt_accum_import": (None, lambda r, s: r.plain.restore(r.plain_state)),
    "pt_adaptive_window": (None, lambda r, s: abi.check(r.lib.pt_adaptive_window(r.adaptive.handle, C.byref(r.adaptive.cam.c), 2, None, r.ptr(s)),
                                                        "pt_adaptive_window")),
    "pt_adaptive_window+mask": (None, lambda r, s: r.adaptive.add(2, r.mask)),
    "pt_adaptive_counts": (lambda r: r.adaptive.add(2), lambda r, s: abi.check(r.lib.pt_adaptive_counts(r.adaptive.handle, _p(r.counts), r.ptr(s)),
                                                                               "pt_adaptive_counts")),
    "pt_adaptive_error": (lambda r: r.adaptive.add(2), lambda r, s: abi.check(r.lib.pt_adaptive_error(r.adaptive.handle, _p(r.err), r.ptr(s)),
                                                                              "pt_adaptive_error")),
    "pt_adaptive_select": (lambda r: r.adaptive.add(2), lambda r, s: r.adaptive.select(0.05, 4, 64)),
    "pt_adaptive_export": (lambda r: r.adaptive.add(2), lambda r, s: r.adaptive.state()),
    "pt_adaptive_import": (None, lambda r, s: r.adaptive.restore(r.adaptive_state)),
    "pt_render_aov": (None, lambda r, s: abi.check(r.lib.pt_render_aov(r.ds.handle, C.byref(r.cam.c), C.byref(r.aov_p), C.byref(r.bufs), r.ptr(s)),
                                                   "pt_render_aov")),
    "pt_denoise": (None, lambda r, s: R.denoise(r.g["color"], albedo=r.g["albedo"], normal=r.g["normal"], depth=r.g["depth"], out=r.out, **DENOISE_KW)),
    "pt_variance_estimate": (lambda r: r.adaptive.add(2), lambda r, s: r.adaptive.variance(out=r.var)),
    "pt_variance_denoise": (None, lambda r, s: R.denoise_variance(r.g["color"], r.g["variance"], albedo=r.g["albedo"], normal=r.g["normal"],
                                                                  depth=r.g["depth"], out=r.out, variance_out=r.vout, **VDENOISE_KW)),
    "pt_adaptive_next_frame": (lambda r: r.adaptive.add(2), lambda r, s: r.adaptive.next_frame()),
    "pt_temporal_reset": (None, lambda r, s: r.hist.reset()),
    "pt_temporal_push": (None, lambda r, s: r.hist.push(r.g["color"], r.icam, depth=r.g["depth"], normal=r.g["normal"], id=r.g["id"],
                                                        variance=r.g["variance"], out=r.tout)),
    "pt_display_reset": (None, lambda r, s: r.disp.reset()),
    "pt_display_meter": (None, lambda r, s: r.disp.meter(r.g["color"])),
    "pt_display_set_exposure": (None, lambda r, s: r.disp.set_exposure(0.5)),
    "pt_display_apply": (None, lambda r, s: r.disp.apply(r.g["color"], out=r.out8)),
    "pt_display_exposure": (lambda r: r.disp.meter(r.g["color"]), lambda r, s: r.disp.exposure()),
    "pt_display_histogram": (lambda r: r.disp.meter(r.g["color"]), lambda r, s: r.disp.histogram()),
}


@pytest.fixture(scope="module")
def rig(torch):
    r = Rig(torch)
    yield r
    r.close()


def test_no_row_of_the_contract_is_left_out():
    assert set(ROWS) == set(SC.CONTRACT)


@pytest.mark.parametrize("row", list(SC.CONTRACT))
def test_blocking_contract(torch, sizing, rig, row):
    """An event is recorded on the side stream right behind the producer.  When an asynchronous call returns, the event must still be
    pending — a finished event is a hidden host synchronisation (the producer is sized so that a correct library cannot have let it
    finish); when a synchronising call returns, the stream must be idle.  A masked pt_adaptive_window synchronises and THEN launches its
    window: when it returns, everything queued before it has finished (the event), and with an empty mask — a no-op — the stream is idle."""
    prepare, call = ROWS[row]
    st = torch.cuda.Stream()

    def ready():
        with torch.cuda.stream(st):
            if prepare is not None:
                prepare(rig)
        st.synchronize()

    ready()
    with torch.cuda.stream(st):
        call(rig, st)  # (warm-up: torch's allocator and the library have seen this call on this stream)
    st.synchronize()
    ready()
    SC.slow_producer(torch, st, sizing["passes"])
    event = torch.cuda.Event()
    event.record(st)
    assert not event.query(), "the producer finished while it was being queued: it is too short for this host"
    with torch.cuda.stream(st):
        call(rig, st)
    passed, idle = event.query(), st.query()
    st.synchronize()
    if SC.CONTRACT[row] == "async":
        assert not passed, f"{row} is documented as asynchronous and returned only after the work queued before it had finished"
    elif row == "pt_adaptive_window+mask":
        assert passed, f"{row} returned before the work queued before it had finished"
        SC.slow_producer(torch, st, sizing["passes"])
        with torch.cuda.stream(st):
            rig.adaptive.add(2, rig.no_mask)
            assert st.query(), "a window with an empty mask synchronises and launches nothing"
    else:
        assert passed and idle, f"{row} is documented as synchronising `stream` and returned with work pending on it"
