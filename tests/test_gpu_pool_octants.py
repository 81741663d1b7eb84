"""The two forms of the slab pass (pt_device.hpp: slab_chunk_pass), whole frames against the oracle bit for bit: flags = 0 takes the LDS
kernels and with them the sign-resolved form, which reads each lane's (near, far) bounds from the pool's octant table; PT_FLAG_NO_LDS takes the
scalar-cache kernels and the scalar form.  Frames: the Cornell-style scene (8 entries, one a rect); lattice box fields of 7, 8 and 21 entries
(the pad entry, two chunks) with the camera inside nested boxes — origins on faces, edges and corners, more than three candidates, and paths
that bounce in every direction: the test itself checks, on the CPU with the oracle's own path rays, that the regular rays of each such frame
cover all eight direction octants; the scene 2^27 away whose tiles mix a zero direction component with regular rays; a closed room; and a
scene of 260 boxes whose tables would not fit the LDS image — pt_debug_flatten shows it has none, so flags = 0 must reach the scalar-cache
kernels too (an LDS kernel there would read records as bounds, and the frame would differ).  61 x 35 has padding pixels: lanes that scan
without being live, with whatever direction their registers hold."""
import ctypes as C
import functools

import numpy as np
import pytest

import kernel_variant_cases as K
import pool_octant_scenes as P
import scenes_small as S
from conftest import assert_bit_identical
from path_tracer_amd import abi, scenes
from path_tracer_amd import render as R
from path_tracer_amd.scene import box, lambertian_material, lightsource_material, pack, xy_rect

pytestmark = pytest.mark.gpu

SIZES = [(64, 36), (61, 35)]
FLAGS = [0, abi.PT_FLAG_NO_LDS]
SPP, DEPTH = 8, 50
FIELDS = {"field7": 4, "field8": 5, "field21": 18}  # n_small: + one rect and the two nested boxes


def _far_scene():
    """a pooled rect / box scene 2^27 away along x, where floats are 8 or 16 apart: camera rays whose x component is exactly 0 next to rays
    with +-8, +-16 in the same 8 x 8 tile"""
    X = float(2 ** 27)
    cols = [lambertian_material(c) for c in ((0.8, 0.8, 0.8), (0.9, 0.2, 0.2), (0.2, 0.2, 0.9))]
    hs = [box((X - 32, -10, -90), (X - 8, -2, -50), cols[0]), box((X - 8, -4, -80), (X + 16, 6, -60), cols[1]),
          box((X + 16, -10, -100), (X + 48, 10, -70), cols[2]), box((X - 64, -12, -120), (X + 64, -10, -30), cols[0]),
          xy_rect(X - 64, X + 64, -12, 12, -120, lightsource_material((3, 3, 3)))]
    cam = dict(look_from=(X, 0.5, 0.0), look_at=(X, 0.5, -64.0), vup=(0, 1, 0), vfov=24.0, aperture=0.0, focus_dist=64.0, time0=0.0, time1=0.0)
    return pack(hs), cam


def _closed_room():
    hs, cam = scenes.cornell_box()
    return pack(hs + [box((-1000, -1000, -2000), (1500, 1500, 1500), lambertian_material((0.73, 0.73, 0.73)))]), cam


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name in FIELDS:
        return P.box_field(FIELDS[name])
    return {"cornell": S.cornell_scene, "far": _far_scene, "closed_room": _closed_room, "many_boxes": P.many_boxes}[name]()


@functools.lru_cache(maxsize=None)
def _reference(name, size, spp):
    """the oracle's frame, computed once per (scene, size) and shared by both forms; read-only"""
    from oracle import binding as orc
    orc.load()
    orc.set_math(True)
    ps, cam = _scene(name)
    ref = orc.render(ps, scenes.make_camera(cam, *size).c, *size, spp, DEPTH)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("flags", FLAGS, ids=["lds", "no_lds"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["cornell", "field7", "field8", "field21", "far", "closed_room"])
def test_frame_is_the_oracles(orc, name, size, flags):
    ps, cam = _scene(name)
    got, (_, frame) = K.render_host_tagged(*size, SPP, ps, scenes.make_camera(cam, *size), DEPTH, flags=flags)
    # the rect / box-only headline kernel in both forms: the LDS one (sign-resolved slab pass), the scalar-cache one (scalar form)
    assert K.ran(frame, lds=int(flags == 0), grid=0, mats=K.MATS_RECTBOX), frame
    assert_bit_identical(got, _reference(name, size, SPP), f"{name} {size[0]}x{size[1]}x{SPP} depth {DEPTH} flags {flags}")


@pytest.mark.parametrize("flags", FLAGS, ids=["lds", "no_lds"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scene_without_tables_renders_through_the_scalar_cache_kernels(orc, lib, size, flags):
    ps, cam = _scene("many_boxes")
    blob, n_runs = P.flatten(lib, ps)
    (off, n, first), = P.pools(blob, n_runs)
    assert n == 260 and first - 1 == off + 4 * n and len(blob) * 16 <= 64 * 1024, "a pool, no octant table, a blob that fits LDS"
    got, (_, frame) = K.render_host_tagged(*size, 2, ps, scenes.make_camera(cam, *size), DEPTH, flags=flags)
    assert K.ran(frame, lds=0, grid=0, mats=K.MATS_RECTBOX), frame  # the scalar-cache kernel, with and without PT_FLAG_NO_LDS
    assert_bit_identical(got, _reference("many_boxes", size, 2), f"260 boxes {size[0]}x{size[1]}x2 flags {flags}")


_IN = np.dtype([("origin", "3f4"), ("dir", "3f4"), ("time", "f4"), ("rng", "u4"), ("att", "3f4")])
_OUT = np.dtype([("status", "i4"), ("hittable", "i4"), ("material", "i4"), ("front", "i4"), ("t", "f4"), ("p", "3f4"), ("normal", "3f4"),
                 ("u", "f4"), ("v", "f4"), ("color", "3f4"), ("sc_origin", "3f4"), ("sc_dir", "3f4"), ("sc_time", "f4"), ("rng", "u4")])
_CAMRAY = np.dtype([("origin", "3f4"), ("dir", "3f4"), ("time", "f4"), ("rng", "u4")])


def _octants_of_the_frames_rays(orc, ps, cam_c, w, h, spp, depth):
    """Direction octants (sign bits of d: x | y << 1 | z << 2) among the REGULAR rays of the frame the oracle renders: every pixel's chain
    — generator seeded with y w + x, a camera ray per sample, scattered rays until a path ends or reaches the depth — followed a generation
    at a time with orc.camera_rays / orc.bounce (the same entry points tests/path_rays.py follows paths with).  Stops once all eight are seen."""
    assert C.sizeof(abi.PtBounceIn) == _IN.itemsize and C.sizeof(abi.PtBounceOut) == _OUT.itemsize and C.sizeof(abi.PtCameraRay) == _CAMRAY.itemsize
    orc.set_math(True)
    ys, xs = np.mgrid[0:h, 0:w]
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
    state = (xy[:, 1].astype(np.uint64) * w + xy[:, 0]).astype(np.uint32)
    seen = set()
    lo, hi = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
    for _ in range(spp):
        cr = np.frombuffer(orc.camera_rays(cam_c, w, h, xy, state), dtype=_CAMRAY, count=len(xy))
        rays = np.zeros(len(xy), _IN)
        for f in ("origin", "dir", "time", "rng"):
            rays[f] = cr[f]
        rays["att"] = 1.0
        alive = np.arange(len(xy))
        for _ in range(depth):
            if len(alive) == 0:
                break
            d = rays["dir"]
            regular = ((np.abs(d) >= lo) & (np.abs(d) <= hi)).all(1) & np.isfinite(rays["origin"]).all(1)
            sign = np.signbit(d[regular])
            seen |= set(np.unique(sign[:, 0] + 2 * sign[:, 1] + 4 * sign[:, 2]).tolist())
            if len(seen) == 8:
                return seen
            recs = (abi.PtBounceIn * len(rays)).from_buffer_copy(rays.tobytes())
            out = np.frombuffer(orc.bounce(ps, recs), dtype=_OUT, count=len(rays))
            state[alive] = out["rng"]
            go = out["status"] == abi.PT_BOUNCE_SCATTERED
            nxt = np.zeros(int(go.sum()), _IN)
            nxt["origin"], nxt["dir"], nxt["time"], nxt["rng"], nxt["att"] = out["sc_origin"][go], out["sc_dir"][go], out["sc_time"][go], out["rng"][go], out["color"][go]
            rays, alive = nxt, alive[go]
    return seen


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_lattice_field_frames_cover_all_eight_octants(orc, name, size):
    """the condition the frames above rest on, from the reference alone (CPU): without it the sign-resolved form's table could go half unread"""
    ps, cam = _scene(name)
    seen = _octants_of_the_frames_rays(orc, ps, scenes.make_camera(cam, *size).c, *size, SPP, DEPTH)
    assert seen == set(range(8)), f"{name} {size}: direction octants among the frame's regular rays: {sorted(seen)}"
