"""Scenes and the read-backs shared by tests/test_pool_plan_cpu.py and tests/test_gpu_pool_plan.py: rect / box scenes whose whole list
is ONE slab pool (the pool plan claims them: pt_device.hpp PoolPlan; pt_render.hip scene_pool_plan, pass_pool_plan) and scenes
it must not claim."""
import ctypes as C

import pool_octant_scenes as P
from path_tracer_amd import abi
from path_tracer_amd.scene import box, lambertian_material, lightsource_material, pack, sphere, xy_rect

_COLS = [lambertian_material(c) for c in ((0.8, 0.8, 0.8), (0.9, 0.2, 0.2), (0.2, 0.9, 0.2), (0.2, 0.2, 0.9))]
_LIGHT = lightsource_material((4, 4, 4))


def field17():
    """17 pool entries (14 lattice boxes, a rect, two nested boxes around the camera): two chunks of 16 — the second holds one entry and the pad"""
    return P.box_field(14)


def row_of_boxes():
    """Five boxes one behind the other along the view axis inside four nested boxes that hold the camera: a camera ray's slab test admits
    the four boxes it starts in and the row behind them — more than the three candidates a lane holds, so the pool's scan repeats its pass."""
    hs = [box((-1.5 + 0.1 * i, -1.0 + 0.05 * i, -4.0 - 2 * i), (1.5 - 0.1 * i, 1.0 - 0.05 * i, -3.0 - 2 * i), _COLS[i % 4]) for i in range(5)]
    hs.insert(2, xy_rect(-2, 2, -2, 2, -14.5, _LIGHT))
    hs += [box((-5 - i, -5 - i, -15 - i), (5 + i, 5 + i, 3 + i), _LIGHT if i == 0 else _COLS[i]) for i in range(4)]
    return pack(hs), dict(P.CAM)


def _four_boxes(z):
    return [box((-3 + 1.6 * i, -1, z), (-1.9 + 1.6 * i, 0.2 * i, z + 1), _COLS[i]) for i in range(4)]


def two_pools():
    """[four boxes][a sphere][four boxes]: two maximal rect / box stretches, a pool each, an unpooled run between them"""
    return pack(_four_boxes(-6) + [sphere((0, 1.5, -5), 0.7, _COLS[1])] + _four_boxes(-9) + [xy_rect(-6, 6, -4, 6, -12, _LIGHT)]), dict(P.CAM)


def pool_then_lone_rect():
    """[four boxes][a sphere][one rect]: the rect's stretch has no box — a run of its own outside the pool"""
    return pack(_four_boxes(-6) + [sphere((0, 1.5, -5), 0.7, _COLS[1]), xy_rect(-6, 6, -4, 6, -12, _LIGHT)]), dict(P.CAM)


def derived_plan(lib, ps, w, h, spp, depth=50, flags=0, tuning=None):
    """pt_debug_pool_plan (no device) as a dict of abi.POOL_PLAN_WORDS for the frame pass of a render of these parameters"""
    p = abi.PtRenderParams(w, h, spp, depth, 0, 1, flags, 0)
    out = (C.c_int32 * 12)()
    abi.check(lib.pt_debug_pool_plan(C.byref(ps.desc), C.byref(tuning) if tuning is not None else None, C.byref(p), out), "pt_debug_pool_plan")
    return dict(zip(abi.POOL_PLAN_WORDS, (int(v) for v in out)))


def last_plan(ds):
    """(flag, entries, offset of the exact entries, offset of the octant table) the last frame pass of a DeviceScene was given"""
    out = (C.c_int32 * 4)()
    abi.check(ds.lib.pt_debug_last_pool_plan(ds.handle, out), "pt_debug_last_pool_plan")
    return tuple(int(v) for v in out)
