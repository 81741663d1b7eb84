"""Scenes and decoding shared by tests/test_pool_octants_cpu.py and tests/test_gpu_pool_octants.py: rect / box scenes whose slab pools
carry an octant table (pt_flatten.hpp), and one whose tables would not fit the LDS image."""
import ctypes as C

import numpy as np

from path_tracer_amd.scene import box, lambertian_material, lightsource_material, pack, xy_rect

CAM = dict(look_from=(0.3, 0.4, 2), look_at=(0, 0, -5), vup=(0, 1, 0), vfov=70.0, aperture=0.0, focus_dist=5.0, time0=0.0, time1=0.0)


def box_field(n_small, seed=5):
    """n_small boxes of edge 1 or 2 on the integer lattice (they overlap, share faces, edges and corners: bounce rays start there), every
    fourth a light, one rect in a lattice plane, two nested boxes around everything with the camera inside both: n_small + 3 pool entries,
    a closed scene — every path runs to a light or to the depth limit, in every direction."""
    g = np.random.default_rng(seed)
    cols = [lambertian_material(c) for c in ((0.8, 0.8, 0.8), (0.9, 0.2, 0.2), (0.2, 0.9, 0.2), (0.2, 0.2, 0.9))]
    light = lightsource_material((4, 4, 4))
    hs = []
    for i in range(n_small):
        lo = np.array([g.integers(-4, 3), g.integers(-4, 3), g.integers(-9, -2)])
        hi = lo + g.integers(1, 3, 3)
        hs.append(box(tuple(int(v) for v in lo), tuple(int(v) for v in hi), light if i % 4 == 0 else cols[i % 4]))
    hs.insert(n_small // 2, xy_rect(-3, 3, -3, 3, -9, cols[1]))
    hs += [box((-6, -6, -11), (6, 6, 3), cols[0]), box((-7, -7, -12), (7, 7, 4), cols[3])]
    return pack(hs), dict(CAM)


def many_boxes(n=260):
    """n > 256 pooled boxes: 256 bytes of octant table per entry would pass the 64 KB LDS image, so the scene gets no table (its blob
    without them, 96 bytes per box, fits) and renders through the scalar-cache kernels."""
    cols = [lambertian_material(c) for c in ((0.8, 0.8, 0.8), (0.9, 0.2, 0.2), (0.2, 0.9, 0.2), (0.2, 0.2, 0.9))]
    light = lightsource_material((4, 4, 4))
    hs = []
    for i in range(n - 1):
        x, y, z = i % 8 - 4, (i // 8) % 8 - 4, -3 - 2 * (i // 64)
        hs.append(box((x, y, z), (x + 0.5, y + 0.5, z + 0.5), light if i % 5 == 0 else cols[i % 4]))
    hs.append(box((-7, -7, -14), (7, 7, 4), cols[0]))
    return pack(hs), dict(CAM)


def flatten(lib, ps):
    """(blob [n][4] float32, n_runs) of pt_debug_flatten"""
    n_f4, n_runs = C.c_int32(), C.c_int32()
    assert lib.pt_debug_flatten(C.byref(ps.desc), None, 0, C.byref(n_f4), C.byref(n_runs), None, 0, None) == 0
    blob = np.zeros((n_f4.value, 4), np.float32)
    assert lib.pt_debug_flatten(C.byref(ps.desc), blob.ctypes.data_as(C.POINTER(C.c_float)), len(blob), None, None, None, 0, None) == 0
    return blob, n_runs.value


def flatten_tuned(lib, ps, tuning):
    """(blob, n_runs) of pt_debug_flatten_tuned: the flattening under an explicit PtTuning"""
    n_f4, n_runs = C.c_int32(), C.c_int32()
    assert lib.pt_debug_flatten_tuned(C.byref(ps.desc), C.byref(tuning), None, 0, C.byref(n_f4), C.byref(n_runs), None, 0, None) == 0
    blob = np.zeros((n_f4.value, 4), np.float32)
    assert lib.pt_debug_flatten_tuned(C.byref(ps.desc), C.byref(tuning), blob.ctypes.data_as(C.POINTER(C.c_float)), len(blob), None, None, None, 0, None) == 0
    return blob, n_runs.value


def pools(blob, n_runs):
    """[(pool offset, entries, first record of the head run)] of the blob's slab pools, from the aux records of their head runs"""
    out = []
    for r in blob[:n_runs].view(np.int32):
        if r[0] & 15 not in (1, 3):  # DK_RECT, DK_BOX
            continue
        aux = blob[r[1] - 1].view(np.int32)
        if aux[1] != 0:
            out.append((int(aux[2]), int(aux[3]), int(r[1])))
    return out
