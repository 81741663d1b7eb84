"""The stream contract of include/pt_render.h as a table, and the harness tests/test_gpu_stream_order.py holds the library to it with.

Every entry point that takes a `void* stream` promises one of two things: the call "is asynchronous on `stream`" (it returns while the
stream still works, allocates nothing, and every kernel, memset and copy it issues is ordered on that stream), or it "synchronises
`stream`" (the work queued before it has finished when it returns).  On torch's current stream — the legacy default stream, which every
blocking stream synchronises with — neither promise can be seen to break; on a non-blocking side stream (every torch.cuda.Stream(), every
stream a C++ host creates) a break is a wrong image without an error code.  The harness makes such a break visible: the call under test
is queued on a side stream behind a slow producer whose last step writes the call's inputs, so that work on another stream, work that
starts early and work that finishes late all read or leave NaN.

Not a test file: tests/test_stream_contract_cpu.py holds CONTRACT to the header, tests/test_gpu_stream_order.py runs the harness."""
import math
import time

import numpy as np

import display_model as D
import temporal_model as T
import variance_model as V
from path_tracer_amd import abi
from path_tracer_amd import render as R
from test_adaptive_cpu import book_np, error_np
from test_aov_cpu import _IN, _OUT, _RAY, aov_np

F = np.float32

# One row per exported function whose prototype has a `void* stream` parameter ("name+mask": the same function called with a mask).
# (pt_render of a scene with PtTuning.tri_binned — the opt-in binned renderer — "returns only when the frame is done": a documented
# exception of a mode that is off by default; it has no row.)
# "sync" means that the stream is idle when the call returns — on every row but "pt_adaptive_window+mask", where it means less: the
# header promises only that "a mask synchronises `stream` once", to read the active-tile count, and the window is launched AFTER that.
# When that call returns, everything queued before it has finished, but its own window may still run; only an empty mask leaves the
# stream idle.  The blocking test asserts exactly that for this row.
CONTRACT = {
    "pt_render": "async",
    "pt_render_timed": "sync",              # waits on its own events
    "pt_unshard_tiles": "async",
    "pt_tonemap_rgb8": "async",
    "pt_accum_reset": "async",
    "pt_render_accumulate": "async",
    "pt_accum_resolve": "async",
    "pt_accum_tonemap_rgb8": "async",
    "pt_accum_export": "sync",
    "pt_accum_import": "sync",
    "pt_adaptive_window": "async",          # without a mask
    "pt_adaptive_window+mask": "sync",      # reads the active-tile count that sizes its launch
    "pt_adaptive_counts": "async",
    "pt_adaptive_error": "async",
    "pt_adaptive_select": "sync",           # n_active is a host value
    "pt_adaptive_export": "sync",
    "pt_adaptive_import": "sync",
    "pt_render_aov": "async",
    "pt_denoise": "async",
    "pt_variance_estimate": "async",
    "pt_variance_denoise": "async",
    "pt_adaptive_next_frame": "async",
    "pt_temporal_reset": "async",
    "pt_temporal_push": "async",
    "pt_display_reset": "async",
    "pt_display_meter": "async",
    "pt_display_set_exposure": "async",
    "pt_display_apply": "async",
    "pt_display_exposure": "sync",
    "pt_display_histogram": "sync",
}


def contract_functions():
    return {k.split("+")[0] for k in CONTRACT}


# ---- the slow producer -----------------------------------------------------------------------------------------------------------------

PRODUCER_FLOATS = 1 << 26  # one pass reads and writes 256 MiB: ~100 us and more of device time against ~10 us of host time to queue it
MIN_PRODUCER_MS = 30.0     # the producer runs at least this long ...
HOST_FACTOR = 20.0         # ... and at least this many times the host time of the longest call sequence queued behind it
# One tensor for every producer of the session, allocated once and kept until the process ends (allocating and freeing 256 MiB per test
# would synchronise the device).  Two producers at once — the two chains, a default-stream producer beside a side stream's — write it
# concurrently from different streams; that is harmless, because nothing ever reads its values: only the time the passes take matters.
_producer = {}


def producer_tensor(torch):
    if "t" not in _producer:
        _producer["t"] = torch.zeros(PRODUCER_FLOATS, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
    return _producer["t"]


def slow_producer(torch, stream, passes):
    """`passes` dependent element-wise passes over one large device tensor, queued on `stream`: ordinary torch ops, each of which must
    wait for the one before it."""
    t = producer_tensor(torch)
    with torch.cuda.stream(stream):
        for _ in range(int(passes)):
            t.add_(1.0)


def measure_pass_ms(torch, passes=40):
    """Device time of one producer pass on an otherwise idle device, with HIP events."""
    s = torch.cuda.Stream()
    slow_producer(torch, s, 4)
    s.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    slow_producer(torch, s, passes)
    e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) / passes


def passes_for(host_ms, pass_ms):
    return int(math.ceil(max(HOST_FACTOR * host_ms, MIN_PRODUCER_MS) / pass_ms))


# ---- the gate --------------------------------------------------------------------------------------------------------------------------

def poison(t):
    """Fill a device tensor, on the current stream, with what no correct result holds: NaN; for integers a NaN's bits / 0xA5."""
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    elif t.element_size() == 4:
        t.fill_(0x7FC00000)
    else:
        t.fill_(0xA5)
    return t


def scrub(torch, stream, pixels, count=24):
    """Poison the free blocks torch's allocator keeps for `stream`, for the plane sizes of a frame of `pixels` pixels: a host function
    that allocates its own outputs (render_temporal) gets recycled memory, and a stale block may hold a correct image of an earlier,
    identical run — which work on the wrong stream would then pass off as its own.  A heuristic (the allocator picks the blocks): the
    tests that name a stage poison the planes they own; this only makes the whole-chain tests harder to pass by accident."""
    with torch.cuda.stream(stream):
        for nbytes in (80 * pixels, 12 * pixels, 4 * pixels, 3 * pixels):
            junk = [poison(torch.empty(nbytes, dtype=torch.uint8, device="cuda")) for _ in range(count)]
            del junk


def staged_inputs(torch, host):
    """{name: host array} -> {name: (device tensor holding poison, device tensor holding the values)}, synchronised."""
    out = {}
    for k, a in host.items():
        real = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        out[k] = (poison(torch.empty_like(real)), real)
    torch.cuda.synchronize()
    return out


def pending_marker(torch, stream):
    """An event recorded on `stream` now — right behind a producer: while it has not passed, the producer is still running."""
    event = torch.cuda.Event()
    event.record(stream)
    return event


def stream_apart_from_the_null_stream(torch, tries=8, probe_ms=20.0):
    """A side stream behind whose pending work a synchronise of the NULL stream returns at once.  Streams share a few hardware queues, and
    a side stream that shares the null stream's makes hipStreamSynchronize(NULL) — what a *_create ends in — wait behind the side stream's
    packets: no ordering breaks, but a call sequence that creates an object would then no longer run behind pending work.  Probed: a
    short producer on the candidate, a synchronise of the null stream, and the producer must still be running."""
    passes = max(8, int(probe_ms / measure_pass_ms(torch, 20)))
    for _ in range(tries):
        s = torch.cuda.Stream()
        slow_producer(torch, s, passes)
        marker = pending_marker(torch, s)
        torch.cuda.default_stream().synchronize()
        apart = not marker.query()
        s.synchronize()
        if apart:
            return s
    raise AssertionError(f"none of {tries} side streams lets a synchronise of the null stream return while it has work pending")


def gated(torch, stream, passes, inputs, outputs, call, synchronises=False):
    """The pattern of every ordering test, all of it queued on the side stream `stream` without a host synchronisation in between:
    `inputs` ((tensor the call reads, staged values) pairs) hold poison from before; the slow producer runs; a last op copies the staged
    values in; `outputs` (tensors the call writes) are poisoned by an op behind the producer, so that whatever ran early on another
    stream is overwritten; `call()` issues the library calls (torch's current stream is `stream`) and may return more tensors; outputs
    and returned tensors are snapshot by clone(); the inputs are poisoned again, which catches work that runs late; one synchronise.
    Returns (snapshots of `outputs`, snapshots of what `call` returned).
    The producer must still be running when the last of it has been queued — otherwise something in the sequence waited for the device
    and nothing ran behind pending work: asserted, unless the sequence holds a call documented to synchronise (`synchronises`)."""
    inputs, outputs = list(inputs), list(outputs)
    slow_producer(torch, stream, passes)
    marker = pending_marker(torch, stream)
    with torch.cuda.stream(stream):
        for dev, real in inputs:
            dev.copy_(real)
        for o in outputs:
            poison(o)
        more = call()
        more = [] if more is None else list(more)
        snaps = [o.clone() for o in outputs]
        more_snaps = [m.clone() for m in more]
        for dev, _ in inputs:
            poison(dev)
    still_pending = not marker.query()
    stream.synchronize()
    assert synchronises or still_pending, "the producer had finished before the calls were all queued: they did not run behind pending work"
    return [s.cpu().numpy() for s in snaps], [s.cpu().numpy() for s in more_snaps]


# ---- expected values: the accumulators and the chain restated on the host over the oracle and the numpy models -------------------------

def follow_from(orc, ps, cam_c, w, h, xy, state, sums, samples, depth):
    """The reference's sample loop (render.hpp:95-101) for the pixels `xy`, continued for `samples` samples from the generator states
    `state` and the binary32 sums `sums` (tests/test_gpu_temporal.py: follow, which starts its sums at +0).  Returns (sums, states)."""
    n = len(xy)
    state = np.array(state, dtype=np.uint32)
    sums = np.array(sums, dtype=F)
    for _ in range(int(samples)):
        live = np.arange(n)
        rays = np.frombuffer(bytes(orc.camera_rays(cam_c, w, h, xy, state)), dtype=_RAY, count=n)
        rin = np.zeros(n, dtype=_IN)
        for f in ("origin", "dir", "time", "rng_state"):
            rin[f] = rays[f]
        rin["attenuation"] = 1.0
        state[:] = rays["rng_state"]
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
        sums = (sums + col).astype(F)
    return sums, state


class HostAccum:
    """An accumulator (whole frames) restated on the host: the oracle's sample loop per pixel, include/pt_render.h's bookkeeping of the
    two halves (tests/test_adaptive_cpu.py: book_np), its error estimate (error_np) and its variance estimate (variance_model)."""

    def __init__(self, orc, ps, w, h, depth=50):
        orc.set_math(True)
        self.orc, self.ps, self.w, self.h, self.depth = orc, ps, w, h, depth
        y, x = np.mgrid[0:h, 0:w]
        self.xy = np.stack([x.reshape(-1), y.reshape(-1)], 1).astype(np.int32)
        self.reset()

    def _zero(self):
        p = self.w * self.h
        self.S, self.H = np.zeros((p, 3), F), np.zeros((p, 3), F)
        self.n, self.a = np.zeros(p, np.int32), np.zeros(p, np.int32)

    def reset(self):
        self._zero()
        self.state = np.arange(self.w * self.h, dtype=np.uint32)  # render.hpp:130-132: the pixel's linear id
        return self

    def next_frame(self):
        self._zero()
        return self

    def window(self, cam_c, samples, mask=None):
        on = np.ones(self.w * self.h, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
        idx = np.nonzero(on)[0]
        after = self.S.copy()
        if len(idx):
            after[idx], self.state[idx] = follow_from(self.orc, self.ps, cam_c, self.w, self.h, self.xy[idx], self.state[idx], self.S[idx],
                                                      samples, self.depth)
        self.H, self.n, self.a = book_np(self.S, after, self.H, self.n, self.a, samples, None if mask is None else on)
        self.S = after
        return self

    def resolve(self):
        with np.errstate(all="ignore"):
            fb = (self.S / np.maximum(self.n, 1).astype(F)[:, None]).astype(F)
        return np.where((self.n > 0)[:, None], fb, F(0)).astype(F).reshape(self.h, self.w, 3)

    def counts(self):
        return self.n.reshape(self.h, self.w).copy()

    def error(self):
        return error_np(self.S, self.H, self.n, self.a).reshape(self.h, self.w)

    def variance(self):
        return V.estimate(self.S, self.H, self.n, self.a).reshape(self.h, self.w, 3)


def tonemap_np(fb):
    """pt_tonemap_rgb8's bytes: the display model's reference tone at 0 EV (tests/test_gpu_display.py holds the two to each other)."""
    return D.apply(fb, F(0.0), D.REFERENCE)[0]


CHAIN = dict(spp=8, aov_spp=4, denoise_kw=dict(iterations=2), display_kw=dict(adapt_up=0.5, adapt_down=0.25))
CHAIN_OUTPUTS = ("noisy", "temporal", "variance", "history", "filtered", "rgb8")


def chain_expected(orc, ps, cams, w, h):
    """render -> guides -> temporal -> filter -> display for the cameras `cams`, every stage the host model of it fed by the host model of
    the stage before: what render_temporal(..., display=Display("aces", **CHAIN["display_kw"])) must give, frame by frame."""
    acc, hist, disp, frames = HostAccum(orc, ps, w, h), T.Temporal(w, h), D.State(), []
    spp = CHAIN["spp"]
    for f, cam in enumerate(cams):
        if f:
            acc.next_frame()
        acc.window(cam.c, spp - spp // 2).window(cam.c, spp // 2)
        noisy, var = acc.resolve(), acc.variance()
        g = aov_np(orc, ps, cam.c, w, h, CHAIN["aov_spp"])
        color, variance, history = hist.push(cam.c, noisy, g["depth"], normal=g["normal"], id=g["id"], variance_in=var, **T.DEFAULTS)
        filtered = V.denoise(color, variance, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **dict(V.DEFAULTS, **CHAIN["denoise_kw"]))[0]
        e = disp.meter(filtered, **CHAIN["display_kw"])
        frames.append(dict(noisy=noisy, temporal=color, variance=variance, history=history, filtered=filtered, rgb8=D.apply(filtered, e, D.ACES)[0]))
    return frames


def chain_calls(torch, stream, ds, cams, w, h, acc, hist, disp, frames):
    """render_temporal's call sequence driven by hand on `stream`, as a generator that yields after EVERY library call — so that two chains
    can be interleaved call by call from one host thread.  `acc` (adaptive, bound to cams[0]), `hist` and `disp` are the chain's own;
    each finished frame's tensors are appended to `frames`."""
    spp = CHAIN["spp"]

    def on(fn):
        with torch.cuda.stream(stream):
            return fn()
    for f, cam in enumerate(cams):
        if f:
            on(lambda: acc.next_frame(cam))
            yield
        on(lambda: acc.add(spp - spp // 2))
        yield
        on(lambda: acc.add(spp // 2))
        yield
        noisy = on(acc.resolve)
        yield
        var = on(acc.variance)
        yield
        g = on(lambda: R.render_aov(w, h, CHAIN["aov_spp"], ds, cam, planes=("albedo", "normal", "depth", "id")))
        yield
        color, variance, history = on(lambda: hist.push(noisy, cam, variance=var, **g))
        yield
        filtered = on(lambda: R.denoise_variance(color, variance, albedo=g["albedo"], normal=g["normal"], depth=g["depth"], **CHAIN["denoise_kw"]))
        yield
        on(lambda: disp.meter(filtered))
        yield
        rgb8 = on(lambda: disp.apply(filtered))
        yield
        frames.append(dict(noisy=noisy, temporal=color, variance=variance, history=history, filtered=filtered, rgb8=rgb8))


def chain_host_ms(torch, ds, cams, w, h, repeats=3):
    """Host wall time of the longest call sequence the tests queue behind a producer — three frames of render_temporal with the display
    stage — issued on an idle side stream (the smallest of `repeats` runs after a warm-up: allocations and first launches excluded)."""
    s, best = torch.cuda.Stream(), float("inf")
    for _ in range(repeats + 1):
        disp = R.Display("aces", **CHAIN["display_kw"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            frames = [dict(fr) for fr in R.render_temporal(w, h, CHAIN["spp"], ds, cams, aov_spp=CHAIN["aov_spp"], denoise_kw=CHAIN["denoise_kw"], display=disp)]
        ms = (time.perf_counter() - t0) * 1e3
        s.synchronize()
        disp.close()
        del frames
        best = min(best, ms)
    return best
