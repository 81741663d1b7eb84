"""Exact culling far from the origin, and the binned renderer past 2^22 rays in one key.

Far from the origin the camera's own arithmetic (d = llc + s hor + t ver - origin, rounded at the magnitude of |origin|) moves a
camera ray by a sizeable part of a pixel, and by many pixels at large offsets.  The fuzz fields of test_gpu_fuzz.py stay near the
origin; here the same generators are moved by 1e3 .. 1e5 times their scale and looked at from close by, in frames whose pixels are
small against that rounding, and compared with the oracle bit for bit.

The camera-ray candidate cache (pt_device.hpp: tri_pool_scan, TriPrimCtx) lists the direction-map bins of a pixel once and tests
every later camera ray of the pixel against them only: every such ray's own bin must be among them.  The CPU model below evaluates
that selection in binary32 — the corner directions it used to take, and the box grown by the camera's rounding bound it takes now —
against the oracle's own camera rays.  The guard keeps the GPU tests in the regime where the old selection missed bins; the escape
test holds the new selection to zero misses up to an offset of 1e6.

The binned renderer (pt_binned.hpp) files a whole frame under ONE key when every ray is irregular (PT_FLAG_NO_FASTDIV), when the
camera is beyond the last rho class, or when the field of view lies inside one direction bin; a packet once stored its chunk in 16
bits, so a key of more than 65 536 x 64 rays wrapped.  Those tests render 2304 x 1856 pixels in a single shard."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from test_gpu_fuzz import random_sphere_field, random_triangle_field

f32 = np.float32

# ---- the cache's choice of bins, modelled in binary32 ----------------------------------------------------------------------


def _footprint(cam: abi.PtCamera, w: int, h: int):
    """KArgs::foot as the host computes it (pt_render.hip): llc - origin, hor / W, ver / H, and the camera's rounding bound."""
    o, llc = np.array(cam.origin, f32), np.array(cam.lower_left_corner, f32)
    hor, ver = np.array(cam.horizontal, f32), np.array(cam.vertical, f32)
    inv_w, inv_h = f32(1.0) / f32(w), f32(1.0) / f32(h)
    dmax = float(np.sum(np.abs(llc.astype(np.float64)) + np.abs(o.astype(np.float64)) + np.abs(hor.astype(np.float64)) + np.abs(ver.astype(np.float64))))
    return llc - o, hor * inv_w, ver * inv_h, f32(1e-5 * dmax)


def _face_pq(d):
    """tri_dir_cell's face (the largest |component|, exact comparisons) and the two other components, per row of d [n][3]."""
    a = np.abs(d)
    k = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    idx = np.arange(len(d))
    return k, d[idx, k], d[idx, (k + 1) % 3], d[idx, (k + 2) % 3]


def _cell(p, R_):
    return np.clip(np.floor((p + f32(1.0)) * f32(0.5 * R_)).astype(np.int64), 0, R_ - 1)


def ray_cells(d, R_):
    """The bin of each ray as tri_dir_cell computes it (face, ci, cj), for the reciprocal rounded three ways (the device's rcp is
    within an ulp of 1 / d_k): [3][n] each."""
    k, dk, da, db = _face_pq(d.astype(f32))
    r = f32(1.0) / dk
    out = []
    for rk in (r, np.nextafter(r, f32(np.inf)), np.nextafter(r, f32(-np.inf))):
        out.append((k, _cell(da * rk, R_), _cell(db * rk, R_)))
    return out


def old_selection(cr, fh, fv, R_):
    """The corner directions cr +- fh / 2 +- fv / 2 (the selection before it was made conservative): (face, i0, i1, j0, j1, cached)."""
    ks, cis, cjs = [], [], []
    for q in range(4):
        dq = cr + (f32(0.5) if q & 1 else f32(-0.5)) * fh + (f32(0.5) if q & 2 else f32(-0.5)) * fv
        k, dk, da, db = _face_pq(dq.astype(f32))
        ks.append(k); cis.append(_cell(da / dk, R_)); cjs.append(_cell(db / dk, R_))
    ks, cis, cjs = np.array(ks), np.array(cis), np.array(cjs)
    i0, i1, j0, j1 = cis.min(0), cis.max(0), cjs.min(0), cjs.max(0)
    cached = (ks == ks[0]).all(0) & ((i1 - i0 + 1) * (j1 - j0 + 1) <= 4)
    return ks[0], i0, i1, j0, j1, cached


def new_selection(cr, fh, fv, rr, R_):
    """pt_device.hpp, tri_pool_scan: the box cr +- (0.5 (|fh| + |fv|) x 1.001 + rr) per component, its face only if that face's
    component dominates the whole box, the cells of the corner quotients widened by 1e-5."""
    ext = f32(0.5) * (np.abs(fh) + np.abs(fv)) * f32(1.001) + rr
    lo, hi = (cr - ext).astype(f32), (cr + ext).astype(f32)
    amin = np.where(lo > 0, lo, np.where(hi < 0, -hi, f32(0.0)))
    amax = np.maximum(np.abs(lo), np.abs(hi))
    n = len(cr)
    k = np.full(n, -1)
    for c in (2, 1, 0):
        a, b = (c + 1) % 3, (c + 2) % 3
        k = np.where((amin[:, c] > amax[:, a]) & (amin[:, c] > amax[:, b]), c, k)
    idx, kk = np.arange(n), np.maximum(k, 0)
    kl, kh = lo[idx, kk], hi[idx, kk]
    res = []
    for ax in ((kk + 1) % 3, (kk + 2) % 3):
        l, u = lo[idx, ax], hi[idx, ax]
        with np.errstate(divide="ignore", invalid="ignore"):
            qs = np.stack([l / kl, l / kh, u / kl, u / kh])
        res.append((_cell(qs.min(0) - f32(1e-5), R_), _cell(qs.max(0) + f32(1e-5), R_)))
    (i0, i1), (j0, j1) = res
    cached = (k >= 0) & ((i1 - i0 + 1) * (j1 - j0 + 1) <= 4)
    return k, i0, i1, j0, j1, cached


def cache_escapes(orc, cam: abi.PtCamera, w: int, h: int, R_: int, n: int, seed: int = 1, new: bool = True):
    """(cached pixels, cached pixels with a camera ray outside their bins) over n random camera rays of the frame."""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1).astype(np.int32)
    rays = orc.camera_rays(cam, w, h, xy, rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))
    d = np.array([r.dir[:] for r in rays], f32)
    fb, fh, fv, rr = _footprint(cam, w, h)
    sc, tc = xy[:, 0].astype(f32) + f32(0.5), xy[:, 1].astype(f32) + f32(0.5)
    cr = (fb + sc[:, None] * fh + tc[:, None] * fv).astype(f32)
    k0, i0, i1, j0, j1, cached = new_selection(cr, fh, fv, rr, R_) if new else old_selection(cr, fh, fv, R_)
    out = np.zeros(n, bool)
    for k, ci, cj in ray_cells(d, R_):
        out |= (k != k0) | (ci < i0) | (ci > i1) | (cj < j0) | (cj > j1)
    return int(cached.sum()), int((cached & out).sum())


# ---- the far-offset configurations ----------------------------------------------------------------------------------------------

W, H = 320, 180
OFFSET_DIR = np.array([0.61, -0.37, 0.7])          # (a direction off every axis and plane)
TRI_FIELDS = [(8001, 1e3), (8001, 1e4), (8001, 1e5), (8005, 1e3), (8005, 1e4), (8005, 1e5)]  # 8001: seed % 3 == 0, every primary ray grazes
SPHERE_FIELDS = [(3001, 1e3), (3004, 1e4), (3007, 1e5)]


def far_triangle_field(seed, ratio):
    """A triangle field moved by `ratio` times its scale, a pinhole camera 0.6 scales from it (focus there), vfov 30."""
    return random_triangle_field(seed, offset=OFFSET_DIR * ratio, cam_dist=0.6, vfov=30.0)


@pytest.mark.parametrize("seed,ratio", TRI_FIELDS)
def test_far_offset_cameras_reach_the_regime(orc, lib, seed, ratio):
    """The guard: the far-offset tests' cameras do make camera rays leave the bins of their pixel's corner directions (the old
    selection), at R = 128; an edit to the generators that pulled them back towards the origin fails here, on the CPU."""
    _, cam = far_triangle_field(seed, ratio)
    c = scenes.make_camera(cam, W, H)
    n = 200_000
    cached, esc = cache_escapes(orc, c.c, W, H, 128, n, seed=seed, new=False)
    assert cached > n // 10, f"field {seed} x{ratio:g}: the old selection cached only {cached} of {n} pixels"
    assert esc > 0, f"field {seed} x{ratio:g}: no camera ray left its pixel's corner bins ({cached} cached) — not the far-offset regime"


@pytest.mark.parametrize("R_", [16, 128, 512])
def test_cache_bins_cover_every_camera_ray(orc, lib, R_):
    """The new selection lists the bin of every camera ray of a cached pixel — zero escapes — from the origin to an offset of 1e6
    (320 x 180, vfov 40, focus 1, as the issue's table), and still caches most pixels near the origin."""
    rows = []
    for off in (0.0, 1e3, 1e4, 1e5, 1e6):
        o = OFFSET_DIR / np.linalg.norm(OFFSET_DIR) * off
        cam = dict(look_from=tuple(o + [0.3, 0.2, 1.0]), look_at=tuple(o), vup=(0, 1, 0), vfov=40.0, aperture=0.0, focus_dist=1.0, time0=0.0, time1=1.0)
        c = scenes.make_camera(cam, W, H)
        cached, esc = cache_escapes(orc, c.c, W, H, R_, 200_000, seed=int(off) + R_)
        old_cached, old_esc = cache_escapes(orc, c.c, W, H, R_, 200_000, seed=int(off) + R_, new=False)
        rows.append((off, cached, esc, old_cached, old_esc))
        if off == 0.0:
            assert cached > 0.5 * old_cached, f"R {R_}: near the origin the new selection caches {cached}, the old {old_cached}"
    assert all(r[2] == 0 for r in rows), f"R {R_}: camera rays outside their cached bins (offset, cached, escapes, old cached, old escapes): {rows}"
    if R_ == 128:
        assert rows[-1][4] > 0 and rows[-2][4] > 0, f"the model no longer sees the old selection's escapes: {rows}"


# ---- GPU: far-offset parity ----------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("seed,ratio", TRI_FIELDS)
def test_far_offset_triangle_fields(orc, lib, seed, ratio):
    """Triangle fields 1e3 .. 1e5 scales from the origin, seen from close by: the candidate cache on (-1) and off (0), the default
    flags and PT_FLAG_FORCE_STREAM, and one shard of two — the oracle's frame bit for bit."""
    ps, cam = far_triangle_field(seed, ratio)
    spp, depth = 2, 6
    c = scenes.make_camera(cam, W, H)
    orc.set_math(True)
    ref = orc.render(ps, c.c, W, H, spp, depth)
    for cache in (-1, 0):
        ds = R.DeviceScene(ps, abi.tuning(tri_min_run=256, tri_cache=cache))
        assert_bit_identical(R.render_host(W, H, spp, ds, c, depth), ref, f"field {seed} x{ratio:g} tri_cache {cache}")
    ds = R.DeviceScene(ps, abi.tuning(tri_min_run=256))
    assert_bit_identical(R.render_host(W, H, spp, ds, c, depth, flags=abi.PT_FLAG_FORCE_STREAM), ref, f"field {seed} x{ratio:g} stream")
    assert_bit_identical(R.render_host(W, H, spp, ds, c, depth, shard_index=1, shard_count=2),
                         orc.render(ps, c.c, W, H, spp, depth, shard_index=1, shard_count=2), f"field {seed} x{ratio:g} shard 1/2")


@pytest.mark.gpu
@pytest.mark.parametrize("walk", [1, 2])
@pytest.mark.parametrize("seed,ratio", SPHERE_FIELDS)
def test_far_offset_sphere_fields(orc, lib, seed, ratio, walk, monkeypatch):
    """Sphere fields 1e3 .. 1e5 scales from the origin (the fuzz fields stay within 25 units of it), seen from close by, through
    both sphere-grid walks and the grid kernels: the oracle's frame bit for bit."""
    monkeypatch.setenv("PT_GRID_WALK", str(walk))
    ps, cam = random_sphere_field(seed, offset=OFFSET_DIR * ratio, cam_dist=0.3, vfov=35.0)
    spp, depth = 2, 8
    c = scenes.make_camera(cam, W, H)
    orc.set_math(True)
    ref = orc.render(ps, c.c, W, H, spp, depth)
    for name, flags in (("default", 0), ("grid, LDS", abi.PT_FLAG_NO_COOP), ("grid, scalar cache", abi.PT_FLAG_NO_LDS)):
        assert_bit_identical(R.render_host(W, H, spp, ps, c, depth, flags=flags), ref, f"sphere field {seed} x{ratio:g} walk {walk} {name}")


# ---- GPU: the binned renderer with more than 2^22 rays under one key ------------------------------------------------------------

BW, BH = 2304, 1856                                  # 4 276 224 pixels > 65 536 x 64


def _binned_against_persistent(orc, ps, cam, tun: dict, what: str, flags: int = 0):
    c = scenes.make_camera(cam, BW, BH)
    spp, depth = 1, 2
    binned = R.render_host(BW, BH, spp, R.DeviceScene(ps, abi.tuning(tri_min_run=256, tri_binned=1, **tun)), c, depth, flags=flags)
    persistent = R.render_host(BW, BH, spp, R.DeviceScene(ps, abi.tuning(tri_min_run=256, **tun)), c, depth, flags=flags)
    # the whole frame: which pixels land in a key's high chunks depends on the sort
    assert_bit_identical(binned, persistent, f"{what}: binned vs persistent, {BW}x{BH}")
    rng = np.random.default_rng(7)
    xs = np.concatenate([rng.integers(0, BW, 2000), np.arange(BW - 300, BW), [0, BW - 1, 0, BW - 1]])
    ys = np.concatenate([rng.integers(0, BH, 2000), np.full(300, BH - 1), [0, 0, BH - 1, BH - 1]])
    ys[2000:2150] = BH - 2
    xy = np.stack([xs, ys], axis=1).astype(np.int32)
    orc.set_math(True)
    ref = orc.render_pixels(ps, c.c, BW, BH, spp, xy, depth, flags=flags)
    assert_bit_identical(binned[xy[:, 1], xy[:, 0]], ref, f"{what}: binned vs the oracle on {len(xy)} pixels")


def _mesh():
    """One pooled run of 4 096 triangles (bin_full_slices = 2: the slice of a packet matters), cfg5's layout and camera."""
    return scenes.triangle_mesh_scene(n_triangles=4096, seed=777)


@pytest.mark.gpu
def test_binned_every_triangle_key_past_2_22_rays(orc, lib):
    """PT_FLAG_NO_FASTDIV: every ray irregular, the whole frame under the key "every triangle, exactly", sliced in two (4 096
    triangles: bin_full_slices = 2) — 133 632 packets in one key."""
    ps, cam = _mesh()
    _binned_against_persistent(orc, ps, cam, {}, "every-triangle key", flags=abi.PT_FLAG_NO_FASTDIV)


@pytest.mark.gpu
def test_binned_every_band_record_key_past_2_22_rays(orc, lib):
    """The camera beyond the last rho class (the classes cut down to rho <= 1.2, 1.4, 1.6 R — the camera is ~3 R from the mesh's
    centre): every camera ray under the key "every band record"."""
    ps, cam = _mesh()
    _binned_against_persistent(orc, ps, cam, dict(tri_rho=(1.2, 1.4), tri_rho2=1.6), "every-band-record key")


@pytest.mark.gpu
def test_binned_one_direction_bin_past_2_22_rays(orc, lib):
    """A field of view of 0.2 degrees aimed at the middle of one direction bin of the map that serves the camera: the whole frame's
    camera rays under one bin's key (checked with the model of tri_dir_cell before the render)."""
    ps, cam = _mesh()
    st = (C.c_int32 * 8)()
    abi.check(lib.pt_debug_tri_pool(C.byref(ps.desc), st), "pt_debug_tri_pool")
    assert st[0] == 4096, "the run must get a pool"
    res = [(st[4] >> 20) & 1023, (st[4] >> 10) & 1023, st[4] & 1023]
    # the camera (0, 2.5, 9) is ~3 R from the centre of the v0's (R ~ 4.5): class 1 (rho <= 4 R) unless that map is absent
    R_ = res[1] or res[2] or res[0]
    assert R_ >= 4
    p = (np.floor(0.5 * R_) + 0.5) / (0.5 * R_) - 1.0   # the middle of the cell just off the face's centre
    frm = np.array([0.0, 2.5, 9.0])
    d = np.array([p * -1.0, p * -1.0, -1.0])             # face z (k = 2): p = d_x / d_z, q = d_y / d_z
    cam = dict(cam, look_from=tuple(frm), look_at=tuple(frm + d), vfov=0.2, focus_dist=9.0)
    c = scenes.make_camera(cam, BW, BH)
    xy = np.array([[0, 0], [BW - 1, 0], [0, BH - 1], [BW - 1, BH - 1], [BW // 2, BH // 2]], np.int32)
    rays = orc.camera_rays(c.c, BW, BH, xy, np.arange(1, 6, dtype=np.uint32))
    cells = ray_cells(np.array([r.dir[:] for r in rays], f32), R_)
    assert all(len(set(zip(k.tolist(), ci.tolist(), cj.tolist()))) == 1 for k, ci, cj in cells), cells
    _binned_against_persistent(orc, ps, cam, {}, "one direction bin")
