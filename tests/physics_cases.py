"""Inputs of the physics-model comparison (tests/physics_model.py, tests/physics_compare.py): the frozen function-table
cases as they are, the primitive x material pairs they lack, engineered rays per primitive, whole lists, the cameras.
Everything is generated deterministically; nothing here is frozen in tests/golden."""
import math

import numpy as np

import function_tables as FT
import scenes_small as S
from path_tracer_amd import abi, scenes
from path_tracer_amd.scene import (TextureAtlas, box, checker_texture, constant_medium, dielectric_material,
                                   lambertian_material, lightsource_material, metal_material, pack, sphere, triangle,
                                   xy_rect, xz_rect, yz_rect)
from physics_compare import BounceCase, CameraCase
from physics_model import xorshift32_inverse

N_RAYS = FT.N_RAYS
N_LIST = 2000


def random_bounce_inputs(rng, n, center, extent):
    """Rays from a cube of side 2*extent around `center` towards one of side `extent`; every 7th direction very short,
    every 11th very long.  Shared with tests/test_gpu_parity.py."""
    recs = (abi.PtBounceIn * n)()
    o = (rng.random((n, 3), dtype=np.float32) - 0.5) * 2 * extent + center
    target = (rng.random((n, 3), dtype=np.float32) - 0.5) * extent + center
    d = (target - o).astype(np.float32)
    d[::7] *= np.float32(0.01)   # short directions: t far beyond 1
    d[::11] *= np.float32(50.0)
    tm = rng.random(n, dtype=np.float32)
    st = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    att = rng.random((n, 3), dtype=np.float32)
    for k in range(n):
        recs[k].origin[:] = o[k].tolist()
        recs[k].dir[:] = d[k].tolist()
        recs[k].time = float(tm[k])
        recs[k].rng_state = int(st[k])
        recs[k].attenuation[:] = att[k].tolist()
    return recs


def make_recs(rays, seed):
    """rays: [(origin, dir)] or [(origin, dir, time)] or [(origin, dir, time, state)] -> PtBounceIn array."""
    rng = np.random.default_rng(seed)
    recs = (abi.PtBounceIn * len(rays))()
    for k, r in enumerate(rays):
        d = [float(np.float32(x)) for x in r[1]]
        assert any(x != 0.0 for x in d), "zero-length directions are undefined in the reference"
        recs[k].origin[:] = [float(np.float32(x)) for x in r[0]]
        recs[k].dir[:] = d
        recs[k].time = float(np.float32(r[2] if len(r) > 2 else rng.random()))
        recs[k].rng_state = int(r[3]) if len(r) > 3 else int(rng.integers(1, 2 ** 32))
        recs[k].attenuation[:] = [float(np.float32(x)) for x in rng.random(3)]
    return recs


def concat(a, b):
    out = (abi.PtBounceIn * (len(a) + len(b)))()
    for k in range(len(a)):
        out[k] = a[k]
    for k in range(len(b)):
        out[len(a) + k] = b[k]
    return out


def _dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _aimed(rng, n, centre, extent, spread=0.8):
    """n random rays from around the region towards it."""
    out = []
    for _ in range(n):
        o = np.asarray(centre) + (rng.random(3) - 0.5) * 5 * extent
        tgt = np.asarray(centre) + (rng.random(3) - 0.5) * 2 * spread * extent
        out.append((o, tgt - o))
    return out


def _fill(rays, rng, centre, extent, n=N_RAYS, spread=0.8):
    assert len(rays) <= n, len(rays)
    return rays + _aimed(rng, n - len(rays), centre, extent, spread)


# ---- primitive x material pairs the function tables lack ---------------------------------------------------------------

def pair_scenes():
    atlas = TextureAtlas()
    img = FT._image(atlas)
    checker = checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))
    tri = ((-0.5, 0.6, -1.2), (0.5, 0.6, -1.2), (0.0, 1.3, -0.9))
    out = {
        "xz_rect_dielectric": ([xz_rect(-1.0, 1.0, -2.0, 0.0, 0.5, dielectric_material(1.5, (0.9, 1.0, 0.8)))], ((0.0, 0.5, -1.0), 1.6)),
        "triangle_dielectric": ([triangle(*tri, dielectric_material(1.4, (1.0, 0.9, 0.9)))], ((0.0, 0.85, -1.1), 0.9)),
        "triangle_metal": ([triangle(*tri, metal_material((0.8, 0.7, 0.6), 0.2), "badouel")], ((0.0, 0.85, -1.1), 0.9)),
        "sphere_moving_metal_mirror": ([sphere((0.0, 0.0, -1.0), (0.3, 0.5, -1.2), 0.1, 0.9, 0.6, metal_material((0.8, 0.6, 0.2), 0.0))], ((0.1, 0.2, -1.1), 1.3)),
        "sphere_light": ([sphere((0.1, 0.2, -1.0), 0.7, lightsource_material((4, 3, 2)))], ((0.1, 0.2, -1.0), 1.2)),
        "yz_rect_image": ([yz_rect(-0.5, 1.5, -2.5, -0.5, -2.2, lambertian_material(img))], ((-2.2, 0.5, -1.5), 1.6)),
        "sphere_checker": ([sphere((0.1, 0.2, -1.0), 0.7, lambertian_material(checker))], ((0.1, 0.2, -1.0), 1.2)),
        "medium_before_rect": ([constant_medium(sphere((0.8, 0.9, -1.2), 0.6, lambertian_material((1, 1, 1))), 2.5, (0.9, 0.9, 1.0)),
                                xy_rect(-0.5, 2.0, -0.3, 2.2, -1.3, lambertian_material((0.2, 0.8, 0.3)))], ((0.8, 0.9, -1.2), 1.0)),
    }
    return {k: (pack(hs, atlas), region) for k, (hs, region) in out.items()}


# ---- engineered rays ---------------------------------------------------------------------------------------------------

def _sphere_edge_rays(rng, c, r, t_of=None):
    """Inside, on the surface, tangent and just inside the tangent, scaled directions.  c may be a function of time."""
    rays = []
    centre = (lambda tm: np.asarray(c, dtype=float)) if t_of is None else t_of
    tm = 0.5
    c0 = centre(tm)
    for n in _dirs(rng, 24):                                  # origin inside
        rays.append((c0 + n * r * 0.6 * rng.random(), _dirs(rng, 1)[0], tm))
    for n in _dirs(rng, 16):                                  # origin on the surface, heading in (far root) and out (miss)
        rays.append((c0 + n * r, -n + 0.3 * _dirs(rng, 1)[0], tm))
        rays.append((c0 + n * r, n + 0.3 * _dirs(rng, 1)[0], tm))
    # tangent (the discriminant AND the face test sit on their thresholds: such rays are skipped, so only a few), then
    # inside the tangent by 1e-6 (still borderline) .. 1e-2 of r
    for eps, count in ((0.0, 2), (1e-6, 2), (1e-4, 10), (1e-3, 10), (1e-2, 10)):
        for n in _dirs(rng, count):
            tau = np.cross(n, _dirs(rng, 1)[0])
            tau /= np.linalg.norm(tau)
            rays.append((c0 + n * r * (1 - eps) - 1.5 * tau, tau, tm))
    for scale in (1e-3, 1e3):                                 # very short and very long directions
        for o, d in _aimed(rng, 16, c0, r, 0.6):
            rays.append((o, d / np.linalg.norm(d) * scale, tm))
    return rays


def _rect_edge_rays(rng, axis, a0, a1, b0, b1, k):
    ik, ia, ib = {0: (2, 0, 1), 1: (1, 0, 2), 2: (0, 1, 2)}[axis]

    def pt(a, b, kk):
        p = np.zeros(3)
        p[ia], p[ib], p[ik] = a, b, kk
        return p
    rays = []
    for i in range(12):                                       # a direction component exactly 0: the plane's (inf), both in-plane
        d = _dirs(rng, 1)[0]
        d[ik] = 0.0
        rays.append((pt((a0 + a1) / 2, (b0 + b1) / 2, k + (1.5 if i % 2 else -1.5)) - d, d))   # parallel beside the plane: +-inf
        rays.append((pt(a0 - 1.0, (b0 + b1) / 2, k), d))                                         # in the plane itself: 0/0
        d2 = _dirs(rng, 1)[0]
        d2[ia if i % 2 else ib] = 0.0
        o = pt(a0 + (a1 - a0) * rng.random(), b0 + (b1 - b0) * rng.random(), k) - 2 * d2
        rays.append((o, 2 * d2))
    corners = [(a0, b0), (a0, b1), (a1, b0), (a1, b1)]
    edges = [(a0, (b0 + b1) / 2), (a1, b0 + 0.3 * (b1 - b0)), ((a0 + a1) / 2, b0), (a0 + 0.7 * (a1 - a0), b1)]
    # through the corners (two tests on their thresholds at once: skipped rays, one per corner) and through the edges
    for i, (a, b) in enumerate(corners + edges * 5):
        for side in ((1.0, -1.0)[i % 2:i % 2 + 1] if i < 4 else (1.0, -1.0)):
            o = pt(a, b, k) + side * np.abs(_dirs(rng, 1)[0]) * pt(1, 1, 2) * 1.5
            rays.append((o, pt(a, b, k) - o))
    for scale in (1e-3, 1e3):
        for o, d in _aimed(rng, 12, pt((a0 + a1) / 2, (b0 + b1) / 2, k), max(a1 - a0, b1 - b0), 0.4):
            rays.append((o, d / np.linalg.norm(d) * scale))
    return rays


def _triangle_edge_rays(rng, v0, v1, v2):
    v0, v1, v2 = (np.asarray(v, dtype=float) for v in (v0, v1, v2))
    n = np.cross(v1 - v0, v2 - v0)
    n /= np.linalg.norm(n)
    rays = []
    edges = [(v0 + v1) / 2, (v1 + v2) / 2, (v0 + v2) / 2, 0.3 * v0 + 0.7 * v1, 0.8 * v1 + 0.2 * v2, 0.1 * v0 + 0.9 * v2]
    # through the vertices (two barycentrics on their thresholds at once: skipped rays, one per vertex) and the edges
    for i, tgt in enumerate([v0, v1, v2] + edges * 4):
        for side in ((1.0, -1.0)[i % 2:i % 2 + 1] if i < 3 else (1.0, -1.0)):
            o = tgt + side * n * (0.5 + rng.random()) + 0.5 * (rng.random(3) - 0.5)
            rays.append((o, tgt - o))
    for _ in range(16):                                       # hits very near the origin, on both sides of tmin
        w = rng.dirichlet((1, 1, 1))
        inside = w[0] * v0 + w[1] * v1 + w[2] * v2
        d = _dirs(rng, 1)[0]
        rays.append((inside - d * rng.choice([0.0005, 0.002, 0.01]), d))
    for _ in range(12):                                       # parallel and nearly parallel to the plane
        in_plane = (v1 - v0) * (rng.random() - 0.5) + (v2 - v0) * (rng.random() - 0.5)
        o = (v0 + v1 + v2) / 3 - in_plane * 3 + n * rng.choice([1e-6, 1e-4, 1e-3])
        rays.append((o, in_plane))
    for scale in (1e-3, 1e3):
        for o, d in _aimed(rng, 12, (v0 + v1 + v2) / 3, 0.5, 0.5):
            rays.append((o, d / np.linalg.norm(d) * scale))
    return rays


def _box_edge_rays(rng, lo, hi):
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    mid, ext = (lo + hi) / 2, hi - lo
    rays = []
    for _ in range(24):                                       # origin inside
        rays.append((lo + ext * (0.1 + 0.8 * rng.random(3)), _dirs(rng, 1)[0]))
    for i in range(12):                                       # origin on a face, heading in and out
        p = lo + ext * rng.random(3)
        ax = i % 3
        p[ax] = hi[ax] if i % 2 else lo[ax]
        out = np.zeros(3)
        out[ax] = 1.0 if i % 2 else -1.0
        rays.append((p, -out + 0.3 * _dirs(rng, 1)[0]))
        rays.append((p, out + 0.3 * _dirs(rng, 1)[0]))
    for i in range(18):                                       # a direction component exactly 0, origin off every face plane
        d = _dirs(rng, 1)[0]
        d[i % 3] = 0.0
        if i % 6 >= 3:
            d[(i + 1) % 3] = 0.0
        tgt = lo + ext * (0.05 + 0.9 * rng.random(3))
        if i % 2:
            tgt[i % 3] = hi[i % 3] + 0.37                     # parallel beside the box
        rays.append((tgt - 2.5 * d, d))
    # through a corner or an edge two or three faces have a test on its threshold at once (skipped rays): one corner,
    # two edges exactly; the others pass the corners and edges at 1e-4 or 1e-3 of the box's size, inside and outside
    for c in range(8):
        corner = np.where([(c >> b) & 1 for b in range(3)], hi, lo)
        tgt = corner if c == 5 else corner + (corner - mid) * rng.choice([-1e-3, 1e-4, -1e-4, 1e-3])
        o = corner + (corner - mid) * (1 + rng.random()) + 0.6 * (rng.random(3) - 0.5)
        rays.append((o, tgt - o))
    for i in range(24):
        p = lo + ext * rng.random(3)
        a, b = rng.choice(3, 2, replace=False)
        p[a] = rng.choice([lo[a], hi[a]])
        p[b] = rng.choice([lo[b], hi[b]])
        tgt = p if i < 2 else p + (p - mid) * rng.choice([-1e-3, 1e-4, -1e-4, 1e-3])
        o = p + (p - mid) * (1 + rng.random()) + 0.6 * (rng.random(3) - 0.5)
        rays.append((o, tgt - o))
    for scale in (1e-3, 1e3):
        for o, d in _aimed(rng, 12, mid, float(ext.max()), 0.4):
            rays.append((o, d / np.linalg.norm(d) * scale))
    return rays


def _dielectric_angle_rays(rng, index, n_each=10):
    """Unit sphere at the origin: normal incidence, 1 degree either side of the critical angle from inside, grazing."""
    rays = []
    crit = math.degrees(math.asin(1 / index))

    def frame():
        n = _dirs(rng, 1)[0]
        tau = np.cross(n, _dirs(rng, 1)[0])
        return n, tau / np.linalg.norm(tau)
    for _ in range(n_each):
        n, tau = frame()
        rays.append((n * 2.5, -n))                            # normal incidence from outside
        rays.append((n * 0.0 + tau * 1e-9, n))                # and from the centre
        for deg in (crit - 1, crit + 1, crit - 0.1, crit + 0.1, 20.0, 60.0):
            th = math.radians(deg)
            d = math.cos(th) * n + math.sin(th) * tau         # from inside, meeting the surface at n under `deg`
            rays.append((n - d * math.cos(th), d))
        for deg in (85.0, 88.0, 89.5):                        # grazing, from outside
            th = math.radians(deg)
            d = -math.cos(th) * n + math.sin(th) * tau
            rays.append((n - 2 * d, d))
    return rays


def unit_vec_half_states():
    """Generator states whose THIRD draw (unit_vec's sign draw, rtweekend.hpp:65) converts to exactly 0.5 in binary32, and
    their nearest neighbours on either side: integers in [2^31 - 64, 2^31 + 128] round to 2^31."""
    out = []
    for x3 in (2 ** 31, 2 ** 31 - 64, 2 ** 31 + 128, 2 ** 31 - 1, 2 ** 31 + 1, 2 ** 31 + 77, 2 ** 31 - 65, 2 ** 31 + 129):
        out.append(xorshift32_inverse(xorshift32_inverse(xorshift32_inverse(x3))))
    return out


def edge_cases():
    """name -> (hittables, rays, centre, extent, flags)"""
    lam = lambertian_material((0.7, 0.3, 0.3))
    out = {}

    def add(name, hs, rays, centre, extent, seed, spread=0.8, **flags):
        rng = np.random.default_rng(seed)
        out[name] = (hs, make_recs(_fill(rays, rng, centre, extent, spread=spread), seed + 1), flags)

    rng = np.random.default_rng(101)
    c, r = (0.1, 0.2, -1.0), 0.7
    rays = _sphere_edge_rays(rng, c, r)
    for st in unit_vec_half_states():                        # decided hits whose Lambertian sign draw sits on 0.5
        rays.append(((0.1, 0.2, 1.0), (0.0, 0.0, -1.0), 0.5, st))
        rays.append(((1.6, 1.1, 0.3), (-1.5, -0.9, -1.3), 0.5, st))
    add("edge_sphere", [sphere(c, r, lam)], rays, c, r, 102, spread=1.4)

    rng = np.random.default_rng(111)
    c0, c1, t0, t1 = np.array((0.0, 0.0, -1.0)), np.array((0.3, 0.5, -1.2)), 0.25, 0.75
    at = lambda tm: c0 + (tm - t0) / (t1 - t0) * (c1 - c0)  # noqa: E731
    rays = []
    for tm in (t0, t1, -0.5, 1.5, 0.5, 0.0, 1.0):             # shutter times at and outside [time0, time1]
        for o, d in _aimed(rng, 8, at(tm), 0.6, 0.5):
            rays.append((o, d, tm))
        for n in _dirs(rng, 4):
            rays.append((at(tm) + n * 0.3, _dirs(rng, 1)[0], tm))
    add("edge_sphere_moving", [sphere(tuple(c0), tuple(c1), t0, t1, 0.6, lam)], rays + [(o, d, 0.6) for o, d, _ in _sphere_edge_rays(rng, at(0.6), 0.6)][:120],
        (0.15, 0.25, -1.1), 0.9, 112)
    rays = [(o, d, tm) for tm in (0.0, 0.4, 2.0) for o, d in _aimed(rng, 20, c0, 0.6, 0.5) + _aimed(rng, 10, c0, 0.6, 2.5)]
    add("edge_sphere_equal_times", [sphere(tuple(c0), tuple(c1), 0.4, 0.4, 0.6, lam)], rays, tuple(c0), 0.6, 113)

    rng = np.random.default_rng(121)
    rays = _sphere_edge_rays(rng, (0.0, 0.0, 0.0), 0.8)
    add("edge_sphere_hollow", [sphere((0.0, 0.0, 0.0), -0.8, dielectric_material(1.3, (1, 1, 1)))], rays, (0, 0, 0), 0.8, 122, dielectric=True)

    for axis, (name, ctor) in enumerate((("xy", xy_rect), ("xz", xz_rect), ("yz", yz_rect))):
        rng = np.random.default_rng(131 + axis)
        a0, a1, b0, b1, k = -1.0, 1.5, -0.5, 1.0, -2.0
        ik, ia, ib = {0: (2, 0, 1), 1: (1, 0, 2), 2: (0, 1, 2)}[axis]
        centre = np.zeros(3)
        centre[ia], centre[ib], centre[ik] = 0.25, 0.25, k
        add(f"edge_{name}_rect", [ctor(a0, a1, b0, b1, k, lam)], _rect_edge_rays(rng, axis, a0, a1, b0, b1, k), tuple(centre), 1.8, 141 + axis)

    tri = ((-0.5, 0.6, -1.2), (0.5, 0.6, -1.2), (0.0, 1.3, -0.9))
    for strat in ("moller_trumbore", "badouel"):
        rng = np.random.default_rng(151)
        add(f"edge_triangle_{strat}", [triangle(*tri, lam, strat)], _triangle_edge_rays(rng, *tri), (0.0, 0.85, -1.1), 0.9, 152)

    rng = np.random.default_rng(161)
    lo, hi = (1.2, -0.5, -2.5), (1.8, 0.7, -1.9)
    add("edge_box", [box(lo, hi, lam)], _box_edge_rays(rng, lo, hi), (1.5, 0.1, -2.2), 1.0, 162)

    rng = np.random.default_rng(171)
    c, r = (0.8, 0.9, -1.2), 0.6
    add("edge_medium_sphere", [constant_medium(sphere(c, r, lam), 2.5, (0.9, 0.9, 1.0))], _sphere_edge_rays(rng, c, r), c, r, 172, medium=True)
    rng = np.random.default_rng(181)
    lo, hi = (-1.9, -0.5, -0.9), (-1.3, 0.2, -0.3)
    add("edge_medium_box", [constant_medium(box(lo, hi, lam), 2.0, (0.8, 0.9, 0.7))], _box_edge_rays(rng, lo, hi), (-1.6, -0.15, -0.6), 0.8, 182, medium=True)

    rng = np.random.default_rng(191)
    add("edge_dielectric_angles", [sphere((0.0, 0.0, 0.0), 1.0, dielectric_material(1.5, (1.0, 0.9, 0.8)))], _dielectric_angle_rays(rng, 1.5),
        (0, 0, 0), 1.2, 192, dielectric=True)
    return out


# ---- the catalogue ------------------------------------------------------------------------------------------------------

# centre and extent of random_bounce_inputs as tests/test_gpu_parity.py::test_bounce_bit_exact aims them, except "spheres":
# around the top of its radius-1000 ground sphere (x, z within 2 of the origin) the checker's sin(10 y) has |y| below the
# bound the cancellation in |oc|^2 - r^2 leaves in p, i.e. a borderline sign; aimed at the origin 14 % of the rays end there.
LISTS = {"cornell": ((278, 278, 278), 700.0), "mixed": ((0, 0.3, -1), 3.0), "spheres": ((2.5, 0.5, 2.5), 5.0),
         "triangles": ((0, 1.5, 0), 4.0), "ties": ((0, 0, -2), 3.0)}

POOLED = ("box_metal", "edge_box", "xy_rect_lambertian_image", "xz_rect_light", "yz_rect_lambertian_checker", "edge_xy_rect",
          "edge_xz_rect", "edge_yz_rect", "list_spheres", "list_triangles", "triangle_lambertian", "edge_triangle_moller_trumbore")

_cache = {}
_camera_cache = {}


def _extra_dielectric_rays(seed):
    """The frozen sphere_dielectric rays reach total internal reflection or a winning reflectance draw only ten times;
    rays from inside at shallow angles are appended so that the case has its 20 decided reflections."""
    rng = np.random.default_rng(seed)
    rays = []
    for n in _dirs(rng, 64):
        tau = np.cross(n, _dirs(rng, 1)[0])
        tau /= np.linalg.norm(tau)
        th = math.radians(45 + 40 * rng.random())
        d = math.cos(th) * n + math.sin(th) * tau
        rays.append((n - d * math.cos(th), d))
    return make_recs(rays, seed)


def _build_all():
    if _cache:
        return _cache
    for name, (ps, region) in FT.cases().items():
        recs = FT.rays(name, region)
        if name == "sphere_dielectric":
            recs = concat(recs, _extra_dielectric_rays(77))
        _cache[name] = BounceCase(name, ps, recs, dielectric="dielectric" in name, medium=name.startswith("medium"))
    for name, (ps, region) in pair_scenes().items():
        _cache[name] = BounceCase(name, ps, FT.rays(name, region), dielectric="dielectric" in name, medium=name.startswith("medium"))
    for name, (hs, recs, flags) in edge_cases().items():
        _cache[name] = BounceCase(name, pack(hs), recs, edge=True, dielectric=flags.get("dielectric", False),
                                  medium=flags.get("medium", False))
    for name, (centre, extent) in LISTS.items():
        ps, _ = S.ALL[name]()
        rng = np.random.default_rng(sum(map(ord, name)) * 7919)
        recs = random_bounce_inputs(rng, N_LIST, np.float32(centre), np.float32(extent))
        _cache["list_" + name] = BounceCase("list_" + name, ps, recs, edge=(name == "ties"))
    return _cache


BOUNCE_NAMES = (list(FT.cases()) + ["xz_rect_dielectric", "triangle_dielectric", "triangle_metal", "sphere_moving_metal_mirror",
                                    "sphere_light", "yz_rect_image", "sphere_checker", "medium_before_rect",
                                    "edge_sphere", "edge_sphere_moving", "edge_sphere_equal_times", "edge_sphere_hollow",
                                    "edge_xy_rect", "edge_xz_rect", "edge_yz_rect", "edge_triangle_moller_trumbore",
                                    "edge_triangle_badouel", "edge_box", "edge_medium_sphere", "edge_medium_box",
                                    "edge_dielectric_angles"] + ["list_" + n for n in LISTS])


def bounce_case(name) -> BounceCase:
    return _build_all()[name]


def camera_args(name):
    """The constructor arguments of FT.CAMERAS[name] as camera.hpp:67 takes them (binary32 values)."""
    look_from, look_at, vup, vfov, aperture, focus, t0, t1, w, h = FT.CAMERAS[name]
    if focus is None:
        d = np.float32(look_at) - np.float32(look_from)
        focus = float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    aspect = float(np.float32(w) / np.float32(h))
    return (look_from, look_at, vup, vfov, aspect, aperture, focus, t0, t1), w, h


def camera_case(name) -> CameraCase:
    key = "camera_" + name
    if key not in _camera_cache:
        args, w, h = camera_args(name)
        look_from, look_at, vup, vfov, _, aperture, focus, t0, t1 = args
        cam = scenes.make_camera(dict(look_from=look_from, look_at=look_at, vup=vup, vfov=vfov, aperture=aperture, focus_dist=focus,
                                      time0=t0, time1=t1), w, h)
        xy, st = FT.camera_inputs(name)
        _camera_cache[key] = CameraCase(name, args, cam.c, w, h, xy, st)
    return _camera_cache[key]


CAMERA_NAMES = list(FT.CAMERAS)
