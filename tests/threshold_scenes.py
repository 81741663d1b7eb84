"""Scenes that sit exactly ON a size threshold of the launcher (csrc/pt_render.hip: choose_variant), the flattener (csrc/pt_flatten.hpp) and
the streaming kernel (render_kernel_stream), each with its neighbour one step above.  Host only; shared by
tests/test_threshold_scenes_cpu.py (sizes, flattener facts, visibility) and tests/test_gpu_threshold_scenes.py (frames against the oracle).

Every size is what the library's own probes report (pt_debug_flatten_tuned, pt_debug_shade_table, pt_debug_tri_pool, pt_debug_pool_plan);
every limit is read from the sources by regular expression (PATTERNS: each pattern must match exactly once).  A builder is a scene
function of a few integer knobs — hittables to pad with, materials, runs — and `land` turns the knobs until the probed size EQUALS the
target; it raises where it cannot.  Padding that no ray reaches proves nothing, so every scene ends with a MARKER: the last hittable of
the list — its records end the blob, its shade record ends the shade table — with a material of its own, which therefore ends the
material table; it stands in front of the camera and must be the first hit of at least MIN_MARKER_PIXELS pixels (marker_pixels: the
oracle's id plane)."""
import collections
import contextlib
import ctypes as C
import functools
import os
import re
from pathlib import Path

import numpy as np

import kernel_variant_cases as K
from path_tracer_amd import abi
from path_tracer_amd.scene import (TextureAtlas, box, constant_medium, hittable_dtype, image_texture, lambertian_material,
                                   lightsource_material, metal_material, pack, pack_tables, sphere, triangle, xy_rect, xz_rect)

CSRC = Path(__file__).resolve().parent.parent / "path_tracer_amd" / "csrc"
MIN_MARKER_PIXELS = 8

# ---- the constants, from the sources -----------------------------------------------------------------------------------------------

_BYTES = r"([0-9][0-9 *]*)"
PATTERNS = {
    "kMaxLdsColdScene": ("pt_render.hip", r"constexpr size_t kMaxLdsColdScene = " + _BYTES + ";"),
    "kMaxLdsWithMaterials": ("pt_render.hip", r"constexpr size_t kMaxLdsWithMaterials = " + _BYTES + ";"),
    "kMaxLdsBlob": ("pt_render.hip", r"constexpr size_t kMaxLdsBlob = ptf::(kLdsImageBytes);"),
    "kLdsImageBytes": ("pt_flatten.hpp", r"constexpr size_t kLdsImageBytes = " + _BYTES + ";"),
    "octant_rule": ("pt_flatten.hpp", r"with_tables && out\.pooled > 0 && out\.blob\.size\(\) \* 16 > (kLdsImageBytes)\)"),
    "kTileF4": ("pt_render.hip", r"constexpr int kTileF4 = (\d+);"),
    "kSmallRunF4": ("pt_render.hip", r"constexpr int kSmallRunF4 = (\d+);"),
    "small_run_rule": ("pt_render.hip", r"if \(cnt \* sz <= (kSmallRunF4)\) \{"),
    "kCoopMinTraversal": ("pt_render.hip", r"constexpr float kCoopMinTraversal = ([0-9.]+)f;"),
    "kShadeMaxHittables": ("pt_flatten.hpp", r"constexpr int kShadeMaxHittables = (\d+);"),
    "grid_count": ("pt_flatten.hpp", r"if \(count < (\d+) \|\| count > (\d+) \|\| !uniform\) return g;"),
    "grid_small": ("pt_flatten.hpp", r"if \(n_small < (\d+)\) return g;"),
    "merge_count": ("pt_flatten.hpp", r"runs\[ri\]\.count <= (\d+) \|\| absorbed_by\[ri\] >= 0\) continue;"),
    "absorbed_tri": ("pt_flatten.hpp", r"if \(rr\.kind == DK_TRI && rr\.count <= (\d+) && rr\.count < tri_tune\.min_run\) continue;"),
    "absorbed_sphere": ("pt_flatten.hpp", r"absorbed_by\[rj\] >= 0 \|\| rr\.count > (\d+)\) break;"),
    "slab_pool_rule": ("pt_flatten.hpp", r"\(box_cull == 2 \? n >= 2 : (\d+) \* n_box - (\d+) \* \(n - n_box\) > (\d+)\);"),
    "record_size": ("pt_flatten.hpp", r"case DK_SPHERE: return (\d+); case DK_RECT: return (\d+); case DK_TRI: case DK_TRI_B: return (\d+); "
                                      r"case DK_BOX: return (\d+); default: return (\d+); \}"),
    "cost_sphere": ("pt_render.hip", r"case PT_HIT_SPHERE: s->traversal_cost \+= ([0-9.]+)f; break;"),
    "cost_triangle": ("pt_render.hip", r"case PT_HIT_TRIANGLE: s->traversal_cost \+= ([0-9.]+)f; break;"),
    "cost_box": ("pt_render.hip", r"case PT_HIT_BOX: s->traversal_cost \+= ([0-9.]+)f; break;"),
    "cost_medium": ("pt_render.hip", r"case PT_HIT_CONSTANT_MEDIUM: s->traversal_cost \+= ([0-9.]+)f; break;"),
    "cost_rect": ("pt_render.hip", r"default: s->traversal_cost \+= ([0-9.]+)f; break;"),
    "coop_rule": ("pt_render.hip", r"\(s->traversal_cost >= (kCoopMinTraversal) \|\| \(p->flags & PT_FLAG_FORCE_COOP\)\)"),
}


def matches(name, csrc=CSRC):
    """every match of a constant's pattern in its source file (a list of group tuples)"""
    file, pat = PATTERNS[name]
    return [m.groups() for m in re.finditer(pat, (Path(csrc) / file).read_text())]


def _value(s):
    v = 1
    for f in s.split("*"):
        v *= int(f)
    return v


def constants(csrc=CSRC):
    """{name: value} of PATTERNS, each found exactly once; sizes in bytes, counts as integers.  (csrc: another copy of the sources — the test
    that shows the recipes follow a moved constant.)"""
    found = {}
    for name in PATTERNS:
        got = matches(name, csrc)
        if len(got) != 1:
            raise LookupError(f"{name}: {len(got)} matches of its pattern in {PATTERNS[name][0]} (a renamed or moved constant?)")
        found[name] = got[0]
    c = {k: _value(found[k][0]) for k in ("kMaxLdsColdScene", "kMaxLdsWithMaterials", "kLdsImageBytes", "kTileF4", "kSmallRunF4", "kShadeMaxHittables")}
    c["kMaxLdsBlob"] = c["kLdsImageBytes"]  # (the alias, and the octant-table rule, name it: their patterns say so)
    c["kCoopMinTraversal"] = float(found["kCoopMinTraversal"][0])
    c["grid_min"], c["grid_max"] = (int(v) for v in found["grid_count"])
    assert int(found["grid_small"][0]) == c["grid_min"], "the two grid minima of build_sphere_grid"
    c["merge_max"] = int(found["merge_count"][0])          # a sphere run of at most this many spheres absorbs nothing
    c["absorbed_tri_max"] = int(found["absorbed_tri"][0])  # a triangle run of at most this many is looked past
    c["absorbed_sphere_max"] = int(found["absorbed_sphere"][0])
    c["slab_rule"] = tuple(int(v) for v in found["slab_pool_rule"])  # (per box, per rect, threshold)
    c["record_size"] = dict(zip(("sphere", "rect", "triangle", "box", "medium"), (int(v) for v in found["record_size"])))
    c["cost"] = {k: float(found["cost_" + k][0]) for k in ("sphere", "triangle", "box", "medium", "rect")}
    return c


# ---- the probes ----------------------------------------------------------------------------------------------------------------------

def library():
    """the product's library, built on demand as conftest's `lib` fixture does (the recipes probe it while the test modules are collected)"""
    if not abi.library_path().exists():
        import __graft_entry__
        __graft_entry__.build()
    return abi.load_library()


Probe = collections.namedtuple("Probe", "blob_f4 mats_f4 shade_f4 n_runs flags tri_pooled grid_spheres")
_ENV_OF = {"sphere_grid": "PT_NO_GRID", "slab_pools": "PT_NO_BOXCULL", "sphere_merge": "PT_NO_SPHERE_MERGE"}  # (their -1; tri_min_run: PT_TRI_MIN)


@contextlib.contextmanager
def _tuning_env(tuning):
    """pt_debug_tri_pool takes no PtTuning: the layout knobs of `tuning` as the environment it reads"""
    env = {"PT_TRI_MIN": str(v) for k, v in (tuning or {}).items() if k == "tri_min_run"}
    env.update({_ENV_OF[k]: "1" for k, v in (tuning or {}).items() if k in _ENV_OF and v < 0})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def probe(ps, tuning=None):
    """The sizes the library reports for a packed scene under PtTuning keywords: the blob, the material table (the smallest buffer
    pt_debug_flatten_tuned accepts), the shade table, the runs, the flags, the pooled triangles and the spheres in a grid."""
    lib = library()
    t = abi.tuning(**tuning) if tuning else abi.tuning()
    d = C.byref(ps.desc)
    n_f4, n_runs, flags = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    abi.check(lib.pt_debug_flatten_tuned(d, C.byref(t), None, 0, C.byref(n_f4), C.byref(n_runs), None, 0, C.byref(flags)), "pt_debug_flatten_tuned")
    mats_f4 = 4 * ps.n_materials
    buf = np.zeros((mats_f4 + 1, 4), np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    ok = lib.pt_debug_flatten_tuned(d, C.byref(t), None, 0, None, None, fp, mats_f4, None)
    short = lib.pt_debug_flatten_tuned(d, C.byref(t), None, 0, None, None, fp, mats_f4 - 1, None)
    if ok != 0 or short == 0:
        raise RuntimeError(f"the material table is not {mats_f4} records: {ok}, {short}")
    sh = C.c_int32(-1)
    abi.check(lib.pt_debug_shade_table(d, C.byref(t), None, 0, C.byref(sh), None), "pt_debug_shade_table")
    st = (C.c_int32 * 8)()
    with _tuning_env(tuning):
        abi.check(lib.pt_debug_tri_pool(d, st), "pt_debug_tri_pool")
    if st[6] != n_f4.value:
        raise RuntimeError(f"pt_debug_tri_pool lays out {st[6]} records, pt_debug_flatten_tuned {n_f4.value}: the environment differs from {tuning}")
    return Probe(n_f4.value, mats_f4, sh.value, n_runs.value, flags.value, int(st[0]), int(st[7]))


def pool_plan(ps, w=24, h=16, spp=4, flags=0, tuning=None):
    """pt_debug_pool_plan's words as a dict of abi.POOL_PLAN_WORDS"""
    p = abi.PtRenderParams(w, h, spp, 50, 0, 1, flags, 0)
    out = (C.c_int32 * 12)()
    lib = library()
    t = abi.tuning(**tuning) if tuning else abi.tuning()
    abi.check(lib.pt_debug_pool_plan(C.byref(ps.desc), C.byref(t), C.byref(p), out), "pt_debug_pool_plan")
    return dict(zip(abi.POOL_PLAN_WORDS, (int(v) for v in out)))


def blob(ps, tuning=None):
    """(the blob [n][4] float32, n_runs) of pt_debug_flatten_tuned"""
    lib = library()
    t = abi.tuning(**tuning) if tuning else abi.tuning()
    n = probe(ps, tuning).blob_f4
    out = np.zeros((n, 4), np.float32)
    n_runs = C.c_int32()
    abi.check(lib.pt_debug_flatten_tuned(C.byref(ps.desc), C.byref(t), out.ctypes.data_as(C.POINTER(C.c_float)), n, None, C.byref(n_runs), None, 0, None),
              "pt_debug_flatten_tuned")
    return out, n_runs.value


def run_headers(ps, tuning=None):
    """[(device kind, absorbed, first record, count, first hittable)] of the blob's runs"""
    b, n_runs = blob(ps, tuning)
    return [(int(k) & 7, bool(int(k) & 8), int(off), int(cnt), int(first)) for k, off, cnt, first in b[:n_runs].view(np.int32)]


def staged_bytes(p):
    """what choose_variant weighs against kMaxLdsColdScene and kMaxLdsWithMaterials: records + materials + shade table"""
    return 16 * (p.blob_f4 + p.mats_f4 + p.shade_f4)


def blob_bytes(p):
    return 16 * p.blob_f4


# ---- landing on a size ---------------------------------------------------------------------------------------------------------------

def land(make, size, target, knobs, back=6):
    """The knob values {name: int} at which size(make(**values)) == target.  knobs: [(name, lo, hi)], coarsest first; sizes must not
    shrink when a knob grows.  Depth first: a knob takes the largest value that does not pass the target with the finer knobs at their
    minima — found by bisection over probed sizes —, then up to `back` values below it.  Raises where no combination lands."""
    cache = {}

    def sz(vals):
        key = tuple(sorted(vals.items()))
        if key not in cache:
            cache[key] = size(make(**vals))
        return cache[key]

    def rec(i, vals):
        if i == len(knobs):
            return dict(vals) if sz(vals) == target else None
        name, lo, hi = knobs[i]
        rest = {n: l for n, l, _ in knobs[i + 1:]}
        at = lambda v: sz({**vals, name: v, **rest})  # noqa: E731
        if at(lo) > target:
            return None
        a, b = lo, hi
        while a < b:  # the largest v with at(v) <= target
            m = (a + b + 1) // 2
            a, b = (m, b) if at(m) <= target else (a, m - 1)
        for v in range(a, max(lo, a - back) - 1, -1):
            got = rec(i + 1, {**vals, name: v})
            if got is not None:
                return got
        return None

    got = rec(0, {})
    if got is None:
        raise LookupError(f"no knob setting of {[k[0] for k in knobs]} reaches {target} (probed {len(cache)} scenes)")
    return got


def land_above(make, size, limit, knobs, steps, back=6):
    """The first reachable size above `limit`: the smallest of limit + steps that `land` reaches; (values, size)"""
    for s in steps:
        try:
            return land(make, size, limit + s, knobs, back), limit + s
        except LookupError:
            continue
    raise LookupError(f"nothing lands in {limit} + {list(steps)}")


# ---- the stage: a camera, a marker in front of it, padding behind ---------------------------------------------------------------------

CAM = dict(look_from=(0.0, 0.5, 3.0), look_at=(0.0, 0.5, -3.0), vup=(0, 1, 0), vfov=60.0, aperture=0.0, focus_dist=3.0, time0=0.0, time1=1.0)
_MARK = (0.0, 0.5, 1.0)  # two units in front of the camera: 0.7 across covers about 5 x 5 pixels of a 24 x 16 frame


def _colour(j):
    return (0.15 + 0.7 * ((j * 37) % 101) / 101.0, 0.15 + 0.7 * ((j * 53) % 103) / 103.0, 0.15 + 0.7 * ((j * 71) % 107) / 107.0)


def marker(kind):
    """the last hittable of every scene, with a material no other hittable has"""
    x, y, z = _MARK
    if kind == "rect":
        return xy_rect(x - 0.35, x + 0.35, y - 0.35, y + 0.35, z, lightsource_material((7.0, 3.0, 1.0)))
    if kind == "box":
        return box((x - 0.35, y - 0.35, z - 0.2), (x + 0.35, y + 0.35, z), lightsource_material((7.0, 3.0, 1.0)))
    up = (x, y + 0.2, z)  # the marker spheres MOVE a little: a static sphere's third record — the blob's last — is never read
    if kind == "sphere":
        return sphere(_MARK, up, 0.0, 1.0, 0.35, lambertian_material((0.95, 0.35, 0.05)))
    if kind == "metal":
        return sphere(_MARK, up, 0.0, 1.0, 0.35, metal_material((0.8, 0.7, 0.6), 0.1))
    if kind == "small_sphere":  # small enough for a field's culling grid (four median radii)
        return sphere(_MARK, up, 0.0, 1.0, 0.3, lightsource_material((7.0, 3.0, 1.0)))
    if kind == "static_sphere":  # (a run with a moving sphere is never absorbed)
        return sphere(_MARK, 0.3, lightsource_material((7.0, 3.0, 1.0)))
    if kind == "triangle":
        return triangle((x - 0.45, y - 0.35, z), (x + 0.45, y - 0.35, z), (x, y + 0.45, z), lightsource_material((7.0, 3.0, 1.0)))
    if kind == "medium":  # dense: a camera ray scatters inside it with near certainty
        return constant_medium(sphere(_MARK, (x, y + 0.2, z), 0.0, 1.0, 0.35, lambertian_material((1, 1, 1))), 1.0e4, (0.95, 0.35, 0.05))
    raise KeyError(kind)


def _image(atlas):
    y, x = np.mgrid[0:13, 0:17]
    rgb = np.stack([(x * 13 + y * 5) % 256, (x * 3 + 17 * y) % 256, (x * y * 7) % 256], axis=-1).astype(np.uint8)
    return image_texture.from_array(rgb, 1.5, atlas)


def rectbox(rects=0, cols=1, splits=0, boxes=8, last="rect"):
    """A floor, a lit back wall, `boxes` boxes and `rects` small rects behind the marker, in cols lambertian colours (cols materials more);
    `splits` of the boxes stand among the rects, each cutting the rect run in two (two runs more).  Few boxes: the scan stays below the
    cooperative kernels' traversal cost.  Open to the sky."""
    mats = [lambertian_material(_colour(j)) for j in range(cols)]
    hs = [xz_rect(-6, 6, -9, 4, -1.0, lambertian_material((0.73, 0.73, 0.73))), xy_rect(-3, 3, -1, 3, -8.5, lightsource_material((4, 4, 4)))]
    bx = [box((-4.2 + 1.2 * i % 8.4, -1.0, -7.5 + 0.5 * (i % 3)), (-3.6 + 1.2 * i % 8.4, -0.2 + 0.1 * (i % 4), -6.9 + 0.5 * (i % 3)), mats[i % cols])
          for i in range(boxes)]
    cut = sorted({(s + 1) * max(1, rects) // (splits + 1) for s in range(splits)}) if splits else []
    hs += bx[splits:]
    nb = 0
    for i in range(rects):
        if nb < splits and nb < len(cut) and i == cut[nb]:
            hs.append(bx[nb])
            nb += 1
        x, y, z = -4.5 + 0.45 * (i % 21), -0.9 + 0.42 * ((i // 21) % 6), -4.0 - 0.6 * (i // 126) - 0.01 * (i % 7)
        hs.append(xy_rect(x, x + 0.4, y, y + 0.36, z, mats[(i + 1) % cols]))
    hs += bx[nb:splits]
    return pack(hs + [marker(last)]), dict(CAM)


def field(spheres=56, cols=1, rects=0, image=None):
    """`rects` rects (a run without a box: no pool) in front of the list, then ONE sphere run: the ground,
    `spheres` small spheres on a jittered lattice (every seventh moves) in six shared materials and cols lambertian colours, and the marker, a
    small sphere itself: the run's last record ends the blob.  image: "sphere" — one of the field carries an image texture (u, v of the
    winner) —, "triangle" — a triangle run of one in front of the spheres carries it (u, v tracked through the scan)."""
    atlas = TextureAtlas() if image else None
    base = [lambertian_material((0.5, 0.5, 0.5)), lambertian_material((0.2, 0.3, 0.8)), metal_material((0.8, 0.8, 0.9), 0.1),
            lightsource_material((3, 3, 2))]
    mats = base + [lambertian_material(_colour(j)) for j in range(cols)]
    hs = []
    for i in range(rects):
        x, z = -5.0 + 0.5 * (i % 21), -2.0 - 0.5 * (i // 21)
        hs.append(xz_rect(x, x + 0.4, z, z + 0.4, -0.99 + 0.0001 * (i % 5), mats[4 + i % cols]))
    if image == "triangle":
        hs.append(triangle((-2.2, -0.9, -0.5), (-0.8, -0.9, -0.5), (-1.5, 0.6, -0.8), lambertian_material(_image(atlas))))
    hs.append(sphere((0, -501, 0), 500, mats[0]))
    side = max(8, int(np.ceil(np.sqrt(max(1, spheres) / 1.5))))  # the lattice: side columns, as many rows as it takes
    rng = np.random.default_rng(11)
    jit = rng.random((max(1, spheres), 4))
    for i in range(spheres):
        c = (-0.32 * side / 2 + 0.32 * (i % side) + 0.1 * jit[i, 0], -0.86 + 0.1 * jit[i, 1], -0.6 - 0.32 * (i // side) - 0.1 * jit[i, 2])
        r = 0.09 + 0.04 * jit[i, 3]
        m = mats[i % len(mats)]
        if image == "sphere" and i == 3:
            hs.append(sphere((-1.5, -0.4, 0.3), 0.3, lambertian_material(_image(atlas))))
        elif i % 7 == 3:
            hs.append(sphere(c, (c[0], c[1] + 0.2 * jit[i, 0], c[2]), 0.0, 1.0, r, m))
        else:
            hs.append(sphere(c, r, m))
    hs.append(marker("small_sphere"))
    return (pack(hs, atlas) if image else pack(hs)), dict(CAM)


def pooled_boxes(n):
    """n - 1 small boxes and the marker box in one slab pool (lambertian + light): 2 + 2 + 16 records of tables per entry besides its own 2"""
    mats = [lambertian_material(c) for c in K._COLS] + [lightsource_material((4, 4, 4))]
    hs = []
    for i in range(n - 1):
        x, y, z = -4.4 + 0.55 * (i % 17), -1.0 + 0.5 * ((i // 17) % 6), -3.0 - 0.8 * (i // 102)
        hs.append(box((x, y, z), (x + 0.4, y + 0.35, z + 0.4), mats[i % 5]))
    return pack(hs + [marker("box")]), dict(CAM)


def run_of(kind, count):
    """ONE run of `count` hittables of a kind — small ones on a lattice behind the marker, which is the run's last —: the streaming
    kernel's tile and small-run rules count this run's records."""
    mats = [lambertian_material(_colour(j)) for j in range(3)] + [lightsource_material((3, 3, 3))]
    hs = []
    side = max(6, int(np.ceil(np.sqrt(max(1, count) / 1.5))))
    for i in range(count - 1):
        x, y, z = 0.3 * (i % side - side / 2), -0.9 + 0.02 * (i % 5), -0.5 - 0.3 * (i // side)
        m = mats[i % 4]
        if kind == "sphere":
            hs.append(sphere((x, y, z), 0.11, m))
        elif kind == "rect":
            hs.append(xy_rect(x, x + 0.22, y, y + 0.3, z, m))
        elif kind == "triangle":
            hs.append(triangle((x, y, z), (x + 0.25, y, z), (x + 0.1, y + 0.3, z - 0.05), m))
        elif kind == "medium":
            hs.append(constant_medium(sphere((x, y + 0.2, z), 0.12, mats[0]), 2.0, _colour(i)))
        else:
            raise KeyError(kind)
    hs.append(marker({"rect": "rect", "sphere": "small_sphere", "triangle": "triangle", "medium": "medium"}[kind]))
    return pack(hs), dict(CAM)


def lattice_spheres(n):
    """n equal spheres of radius 1 on a 64 x 32 x (n / 2048) lattice, the marker among them as the run's last: the sphere grid's upper bound
    counts the RUN's spheres"""
    i = np.arange(n - 1)
    hs = np.zeros(n, dtype=hittable_dtype)
    c = np.stack([2.25 * (i % 64) - 72.0, 2.25 * ((i // 64) % 32) - 40.0, -12.0 - 2.25 * (i // 2048)], 1).astype(np.float32)
    hs["kind"] = abi.PT_HIT_SPHERE
    hs["material"][:-1] = i % 3
    hs["f"][:-1, 0:3] = c
    hs["f"][:-1, 3:6] = c
    hs["f"][:-1, 6] = 1.0
    hs["material"][-1] = 3
    hs["f"][-1, 0:3], hs["f"][-1, 3:6] = (0.0, 0.5, 0.5), (0.0, 0.7, 0.5)  # (moving, like every marker sphere: shutter 0 .. 1)
    hs["f"][-1, 6:9] = (1.0, 0.0, 1.0)
    ref = pack([sphere((0, 0, 0), 1.0, lambertian_material(_colour(j))) for j in range(3)] + [sphere((0, 0, 0), 1.0, lightsource_material((7.0, 3.0, 1.0)))])
    return pack_tables(hs, list(ref.materials), list(ref.textures)), dict(CAM)


# ---- the recipes ---------------------------------------------------------------------------------------------------------------------

Recipe = collections.namedtuple("Recipe", "name threshold side make size expect tuning flags tag facts frames spp")
# side: "at" / "above"; make(): (PackedScene, camera dict); size(ps, tuning): the probed quantity the threshold weighs — bytes, or the
# count of the run under test read from the blob's run headers —; expect: (lo, hi), the inclusive range it must lie in; tag: (kernel name,
# keywords of K.ran) of the frame pass; facts: what the flattener must have done — "shade", "pool", "tables", "grid", "tri_pool": bool;
# "absorbed": the runs flagged absorbed; "plan": pt_debug_pool_plan's (lds, mats) words.

SMALL = ((24, 16), (37, 21))
STREAM_FRAMES = ((3, 2), (40, 24))
RK, ST = "render_kernel", "render_kernel_stream"
COOP, FAST, STREAM, NO_COOP = abi.PT_FLAG_FORCE_COOP, abi.PT_FLAG_FAST_RNG, abi.PT_FLAG_FORCE_STREAM, abi.PT_FLAG_NO_COOP
LAYOUT_KNOBS = ("sphere_grid", "slab_pools", "sphere_merge", "tri_min_run")  # the PtTuning fields the flattener reads
MATS_OF = {"a": K.MATS_RECTBOX, "b": K.MATS_SIMPLE, "c": K.MATS_ALL}


def staged_size(ps, tuning):
    return staged_bytes(probe(ps, tuning))


def blob_size(ps, tuning):
    return blob_bytes(probe(ps, tuning))


def run_count(index):
    """the count of run `index` (negative: from the end) in the blob's run headers"""
    return lambda ps, tuning: run_headers(ps, tuning)[index][3]


def _family(fam):
    """(scene function of the knobs, knobs coarsest first, facts) of the byte thresholds' families"""
    box_knobs = [("rects", 0, 56), ("splits", 0, 5), ("cols", 1, 40)]  # (few enough rects for the eight boxes to earn their pool)
    if fam == "a":
        return (lambda **kw: rectbox(last="rect", **kw)), box_knobs, dict(shade=True, pool=True, tables=True)
    if fam in ("b", "c"):
        last = "sphere" if fam == "b" else "metal"
        return (lambda **kw: rectbox(last=last, **kw)), box_knobs, dict(shade=False, pool=True, tables=True)
    if fam == "r":  # rects, boxes and a sphere without slab pools: two records per hittable
        return (lambda **kw: rectbox(last="sphere", **kw)), [("rects", 0, 2400), ("splits", 0, 5)], dict(shade=False, pool=False)
    image = {"d": None, "e": "sphere", "f": "triangle"}[fam]
    return (lambda **kw: field(image=image, **kw)), [("spheres", 48, 4000), ("rects", 0, 12), ("cols", 1, 12)], dict(shade=False, grid=True)


def _layout(tuning):
    return tuple(sorted((k, v) for k, v in (tuning or {}).items() if k in LAYOUT_KNOBS))


@functools.lru_cache(maxsize=None)
def _landed(fam, which, limit, side, layout=()):
    """(knob values, probed size) of a family at / above a byte threshold of `limit` bytes (cached: landing probes a few dozen scenes)"""
    make, knobs, _ = _family(fam)
    tuning = dict(layout) or None
    size = blob_size if which == "kMaxLdsBlob" else staged_size
    keeps_grid = fam in "def" and ("sphere_grid", -1) not in layout

    def sz(s):
        """(a field that lost its grid to the LDS budget counts as past every target: the layout WITH the grid is what is landed)"""
        if keeps_grid and probe(s[0], tuning).grid_spheres == 0:
            return 1 << 40
        return size(s[0], tuning)

    if side == "at":
        return land(make, sz, limit, knobs), limit
    return land_above(make, sz, limit, knobs, (16, 32, 48, 64))


def _byte_recipe(c, threshold, fam, which, side, tag, *, tuning=None, flags=0, extra="", facts=None, more=None):
    """more: knobs turned further from the landed `at` scene — {"rects": 1} is that scene and one rect"""
    make, _, fam_facts = _family(fam)
    limit = c[which]

    def build():
        vals, _ = _landed(fam, which, limit, "at" if more else side, _layout(tuning))
        return make(**{k: v + (more or {}).get(k, 0) for k, v in vals.items()})

    expect = (limit, limit) if side == "at" else (0, limit) if more else (limit + 1, limit + 64)
    return Recipe(f"{threshold}-{fam}-{side}{extra}", threshold, side, build, blob_size if which == "kMaxLdsBlob" else staged_size, expect,
                  tuning, flags, tag, dict(fam_facts, **(facts or {})), SMALL, 4)


def _count_recipe(name, threshold, side, build, size, count, tag, *, tuning=None, flags=0, facts=None, frames=SMALL, spp=4):
    return Recipe(name, threshold, side, build, size, (count, count), tuning, flags, tag, facts or {}, frames, spp)


def largest_pool_with_tables():
    """the largest n for which pooled_boxes(n) keeps its octant tables (pt_debug_pool_plan: the scene allows the plan only with tables)"""
    ok = lambda n: pool_plan(pooled_boxes(n)[0])["scene_allows"] == 1  # noqa: E731
    a, b = 3, 600
    if not ok(a) or ok(b):
        raise LookupError("the octant-table rule does not flip between 3 and 600 pooled boxes")
    while b - a > 1:
        m = (a + b) // 2
        a, b = (m, b) if ok(m) else (a, m)
    return a


def recipes(c):
    """every recipe for the constants c (constants(): the library's own)"""
    out = []
    walk1 = dict(grid_walk=1)
    # T1: cold lane state.  At the limit CL = 1; above it CL = 0 with the materials still staged.
    for fam in "abcd":
        grid = dict(grid=1) if fam == "d" else dict(grid=0, mats=MATS_OF[fam])
        tun = walk1 if fam == "d" else None
        plan = dict(plan=(1, MATS_OF[fam])) if fam == "a" else {}
        out.append(_byte_recipe(c, "T1", fam, "kMaxLdsColdScene", "at", (RK, dict(lds=1, mlds=1, cl=1, coop=0, **grid)), tuning=tun, facts=plan))
        out.append(_byte_recipe(c, "T1", fam, "kMaxLdsColdScene", "above", (RK, dict(lds=1, mlds=1, cl=0, coop=0, **grid)), tuning=tun, facts=plan))
    # T2: materials staged.  Above the limit the kernels read the hittable's and the material's records from memory.
    for fam in "abcdef":
        uv = {"e": 1, "f": 2}.get(fam, 0)
        grid = dict(grid=1, uv=uv) if fam in "def" else dict(grid=0, mats=MATS_OF[fam])
        tun = walk1 if fam in "def" else None
        plan = dict(plan=(1, MATS_OF[fam])) if fam == "a" else {}
        out.append(_byte_recipe(c, "T2", fam, "kMaxLdsWithMaterials", "at", (RK, dict(lds=1, mlds=1, cl=0, coop=0, **grid)), tuning=tun, facts=plan))
        out.append(_byte_recipe(c, "T2", fam, "kMaxLdsWithMaterials", "above", (RK, dict(lds=1, mlds=0, cl=0, coop=0, **grid)), tuning=tun, facts=plan))
    out.append(_byte_recipe(c, "T2", "d", "kMaxLdsWithMaterials", "at", (RK, dict(lds=1, mlds=1, fast=1)), tuning=walk1, flags=FAST, extra="-fast"))
    out.append(_byte_recipe(c, "T2", "d", "kMaxLdsWithMaterials", "at", (RK, dict(lds=1, mlds=1, coop=1)), flags=COOP, extra="-coop"))
    # T3: the LDS image.  A field WITH a grid that passes the limit is first laid out again without it (pt_render.hip: flatten_tuned) and,
    # the grid's tables being far larger than 64 bytes, then fits: "above-dropped" is the at scene and one rect, still resident, its grid gone
    # (its scan then long enough for the cooperative kernels).  The streaming kernel is what a field without a grid (sphere_grid = -1) gets.
    nogrid = dict(sphere_grid=-1)
    for walk in (1, 2):
        out.append(_byte_recipe(c, "T3", "d", "kMaxLdsBlob", "at", (RK, dict(lds=1, mlds=0, coop=0, grid=walk)), tuning=dict(grid_walk=walk), extra=f"-walk{walk}"))
    out.append(_byte_recipe(c, "T3", "d", "kMaxLdsBlob", "at", (RK, dict(lds=1, mlds=0, coop=1)), flags=COOP, extra="-coop"))
    out.append(_byte_recipe(c, "T3", "d", "kMaxLdsBlob", "above", (RK, dict(lds=1, mlds=0, coop=1)), extra="-dropped", more=dict(rects=1), facts=dict(grid=False)))
    out.append(_byte_recipe(c, "T3", "d", "kMaxLdsBlob", "at", (RK, dict(lds=1, mlds=0, coop=1)), tuning=nogrid, extra="-nogrid", facts=dict(grid=False)))
    out.append(_byte_recipe(c, "T3", "d", "kMaxLdsBlob", "above", (ST, dict(uv=0)), tuning=nogrid, extra="-nogrid", facts=dict(grid=False)))
    out.append(_byte_recipe(c, "T3", "f", "kMaxLdsBlob", "at", (RK, dict(uv=2, lds=1, mlds=0, coop=0, grid=1)), tuning=walk1))
    out.append(_byte_recipe(c, "T3", "f", "kMaxLdsBlob", "above", (RK, dict(uv=2, lds=1, mlds=0, coop=0)), tuning=walk1, extra="-dropped", more=dict(rects=1),
                            facts=dict(grid=False)))
    out.append(_byte_recipe(c, "T3", "f", "kMaxLdsBlob", "at", (RK, dict(uv=2, lds=1, mlds=0, coop=0)), tuning=nogrid, extra="-nogrid", facts=dict(grid=False)))
    out.append(_byte_recipe(c, "T3", "f", "kMaxLdsBlob", "above", (ST, dict(uv=2)), tuning=nogrid, extra="-nogrid", facts=dict(grid=False)))
    nopool = dict(slab_pools=-1)
    out.append(_byte_recipe(c, "T3", "r", "kMaxLdsBlob", "at", (RK, dict(lds=1, mlds=0, coop=1)), tuning=nopool))
    out.append(_byte_recipe(c, "T3", "r", "kMaxLdsBlob", "above", (ST, dict(uv=0)), tuning=nopool))
    # T4: octant tables, all pools or none: the largest pool whose blob with tables fits the LDS image, and one box more (NO_COOP: so many
    # boxes would go cooperative)
    n = largest_pool_with_tables()
    boxes_in_run = run_count(0)
    out.append(_count_recipe("T4-at", "T4", "at", lambda: pooled_boxes(n), boxes_in_run, n, (RK, dict(lds=1, mlds=0, grid=0, mats=K.MATS_RECTBOX)),
                             flags=NO_COOP, facts=dict(pool=True, tables=True, shade=True, plan=(1, K.MATS_RECTBOX))))
    out.append(_count_recipe("T4-above", "T4", "above", lambda: pooled_boxes(n + 1), boxes_in_run, n + 1, (RK, dict(lds=0, grid=0, mats=K.MATS_RECTBOX)),
                             flags=NO_COOP, facts=dict(pool=True, tables=False, shade=True, plan=(0, K.MATS_RECTBOX))))
    # T5: the streaming kernel.  A run of exactly one tile of records, one record less and more, exactly two tiles; a run that is exactly
    # kSmallRunF4 long and one record more.
    for kind in ("sphere", "rect", "triangle", "medium"):
        size = c["record_size"][kind]
        tile, small = c["kTileF4"] // size, c["kSmallRunF4"] // size  # (the kernel's own integer divisions)
        counts = [(small, "small-at", "at"), (small + 1, "small-above", "above")]
        if kind != "medium":
            counts += [(tile - 1, "tile-below", "at"), (tile, "tile-at", "at"), (tile + 1, "tile-above", "above"), (2 * tile, "two-tiles", "at")]
        for count, what, side in counts:
            out.append(_count_recipe(f"T5-{kind}-{what}", "T5", side, functools.partial(run_of, kind, count), run_count(-1), count, (ST, dict(uv=0)),
                                     flags=STREAM, frames=STREAM_FRAMES))
    # T6: the flattener's structure thresholds
    simple = dict(lds=1, mlds=1, cl=1, coop=0, grid=0, mats=K.MATS_SIMPLE)
    g = c["grid_min"]
    out.append(_count_recipe("T6-grid-at", "T6", "at", functools.partial(run_of, "sphere", g - 1), run_count(-1), g - 1, (RK, simple), facts=dict(grid=False)))
    out.append(_count_recipe("T6-grid-above", "T6", "above", functools.partial(run_of, "sphere", g), run_count(-1), g,
                             (RK, dict(lds=1, mlds=1, cl=1, coop=0, grid=1)), facts=dict(grid=True)))
    m = c["merge_max"]
    out.append(_count_recipe("T6-merge-at", "T6", "at", functools.partial(merge_scene, m), run_count(0), m, (RK, simple), facts=dict(absorbed=[])))
    out.append(_count_recipe("T6-merge-above", "T6", "above", functools.partial(merge_scene, m + 1), run_count(0), m + 1, (RK, simple), facts=dict(absorbed=[2])))
    t = c["absorbed_tri_max"]
    out.append(_count_recipe("T6-absorbed-at", "T6", "at", functools.partial(absorbed_scene, t), run_count(1), t, (RK, simple), facts=dict(absorbed=[2])))
    out.append(_count_recipe("T6-absorbed-above", "T6", "above", functools.partial(absorbed_scene, t + 1), run_count(1), t + 1, (RK, simple), facts=dict(absorbed=[])))
    per_box, per_rect, need = c["slab_rule"]
    b = next(b for b in range(1, 100) if per_box * b - per_rect * 3 > need)  # (rectbox() has three rects besides its boxes)
    headline = dict(lds=1, mlds=1, cl=1, coop=0, grid=0, mats=K.MATS_RECTBOX)
    out.append(_count_recipe("T6-slab-at", "T6", "at", functools.partial(rectbox, boxes=b - 1), run_count(1), b - 1, (RK, headline),
                             facts=dict(pool=False, shade=True, plan=(1, K.MATS_RECTBOX))))
    out.append(_count_recipe("T6-slab-above", "T6", "above", functools.partial(rectbox, boxes=b), run_count(1), b, (RK, headline),
                             facts=dict(pool=True, tables=True, shade=True, plan=(1, K.MATS_RECTBOX))))
    pooled = dict(tri_min_run=256)
    out.append(_count_recipe("T6-tripool-at", "T6", "at", functools.partial(run_of, "triangle", 255), run_count(-1), 255, (RK, dict(lds=1, tripool=0)),
                             tuning=pooled, facts=dict(tri_pool=False)))
    out.append(_count_recipe("T6-tripool-above", "T6", "above", functools.partial(run_of, "triangle", 256), run_count(-1), 256, (RK, dict(lds=0, tripool=1)),
                             tuning=pooled, facts=dict(tri_pool=True)))
    # cooperative traversal: the last scan cost below kCoopMinTraversal and the first at or above it, in spheres without a grid
    n_coop = next(k for k in range(1, 10000) if k * c["cost"]["sphere"] >= c["kCoopMinTraversal"])
    out.append(_count_recipe("T6-coop-at", "T6", "at", functools.partial(run_of, "sphere", n_coop - 1), run_count(-1), n_coop - 1, (RK, simple),
                             tuning=nogrid, facts=dict(grid=False)))
    out.append(_count_recipe("T6-coop-above", "T6", "above", functools.partial(run_of, "sphere", n_coop), run_count(-1), n_coop,
                             (RK, dict(lds=1, mlds=1, coop=1)), tuning=nogrid, facts=dict(grid=False)))
    gm = c["grid_max"]
    out.append(_count_recipe("T6-gridmax-at", "T6", "at", functools.partial(lattice_spheres, gm), run_count(-1), gm, (ST, dict(uv=0)), facts=dict(grid=True),
                             frames=((8, 8),), spp=2))
    out.append(_count_recipe("T6-gridmax-above", "T6", "above", functools.partial(lattice_spheres, gm + 1), run_count(-1), gm + 1, (ST, dict(uv=0)),
                             facts=dict(grid=False), frames=((8, 8),), spp=2))
    return out


def merge_scene(n):
    """[n spheres][a rect][two static spheres and the marker]: the first run absorbs the last one only if it has more than merge_max spheres"""
    lam = [lambertian_material(_colour(j)) for j in range(3)]
    hs = [sphere((-1.2 + 0.8 * i, -0.3, -1.5), 0.35, lam[i % 3]) for i in range(n)]
    hs.append(xz_rect(-4, 4, -6, 2, -1.0, lam[0]))
    hs += [sphere((-1.5, 0.9, -2.5), 0.4, lam[1]), sphere((1.5, 0.9, -2.5), 0.4, lam[2]), marker("static_sphere")]
    return pack(hs), dict(CAM)


def absorbed_scene(n):
    """[five spheres][n triangles][two static spheres and the marker]: the sphere run looks past a triangle run of at most absorbed_tri_max"""
    lam = [lambertian_material(_colour(j)) for j in range(3)]
    hs = [sphere((-2.0 + 1.0 * i, -0.5, -2.0), 0.4, lam[i % 3]) for i in range(5)]
    for i in range(n):
        x, y = -2.6 + 0.4 * (i % 13), -0.9 + 0.45 * (i // 13)
        hs.append(triangle((x, y, -3.5), (x + 0.35, y, -3.5), (x + 0.15, y + 0.4, -3.4), lam[i % 3]))
    hs += [sphere((-1.5, 1.2, -1.0), 0.3, lam[1]), sphere((1.5, 1.2, -1.0), 0.3, lam[2]), marker("static_sphere")]
    return pack(hs), dict(CAM)


RECIPES = recipes(constants())


def by_name(name):
    return next(r for r in RECIPES if r.name == name)


# ---- visibility ------------------------------------------------------------------------------------------------------------------------

def marker_pixels(orc, ps, cam, w, h):
    """pixels of a w x h frame whose first camera ray hits the LAST hittable of the list first (the oracle's id plane)"""
    from path_tracer_amd import scenes
    from test_aov_cpu import aov_np
    ids = aov_np(orc, ps, scenes.make_camera(cam, w, h).c, w, h, 1)["id"]
    return int((ids == ps.n_hittables - 1).sum())
