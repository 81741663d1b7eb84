"""The shade table of small rect / box-only scenes (pt_flatten.hpp: Flat::shade; read by the kernels compiled for such scenes with their
materials in LDS — pt_device.hpp: shade_record), through pt_debug_shade_table — no GPU.  One 16-byte record per hittable: the colour slot of
its material (the lambertian's attenuation, the light's emission) and a word with the rect's axis (0 for a box), the box bit, the
material kind and the hittable's index.  A kernel finds the record from the hit word alone — record (off >> 1) - base for the hittable
whose records start at blob offset off — so the rule is checked here from the blob's own run headers, for one pool of one chunk, a
pool of two chunks, a scene of several runs, a pool of rects only and a scene without any pool.  The blob itself is what it was: the
table rides behind the materials (tests/test_pool_octants_cpu.py holds the blob's layout).  A scene with any other material, texture or
hittable kind has no table and goes to the kernels it went to before."""
import ctypes as C

import numpy as np
import pytest

import kernel_variant_cases as K
import pool_octant_scenes as P
import pool_plan_scenes as PP
from path_tracer_amd import abi, scenes
from path_tracer_amd.scene import (box, checker_texture, lambertian_material, lightsource_material, metal_material, pack, sphere, xy_rect,
                                   xz_rect, yz_rect)

_WHITE, _RED = lambertian_material((0.73, 0.73, 0.73)), lambertian_material((0.65, 0.05, 0.05))
_LIGHT = lightsource_material((15.0, 14.0, 13.0))


def _rects():
    """rects of all three kinds around the camera, the light among them — with slab_pools = 1 one pool of rects only"""
    hs = [xy_rect(-3, 3, -3, 3, -6, _WHITE), xz_rect(-3, 3, -6, 2, 3, _LIGHT), xz_rect(-3, 3, -6, 2, -3, _WHITE), yz_rect(-3, 3, -6, 2, -3, _RED),
          yz_rect(-3, 3, -6, 2, 3, _WHITE)]
    return pack(hs)


def _mixed_runs():
    """[box][rect rect][box box][rect]: four runs — an aux record in front of each shifts the records behind it by one"""
    hs = [box((-4, -4, -9), (4, 4, 3), _WHITE), xy_rect(-1, 1, -1, 1, -5, _LIGHT), yz_rect(-1, 1, -5, -4, 1, _RED), box((-2, -2, -4), (-1, -1, -3), _RED),
          box((1, 1, -4), (2, 2, -3), _WHITE), xz_rect(-1, 1, -5, -4, -1.5, _LIGHT)]
    return pack(hs)


SCENES = {
    "cornell": (lambda: pack(scenes.cornell_box()[0]), None),
    "field16": (lambda: P.box_field(13)[0], None),
    "field17": (lambda: PP.field17()[0], None),
    "rect_pool": (_rects, dict(slab_pools=1)),
    "rects_unpooled": (_rects, None),
    "mixed_runs": (_mixed_runs, None),
}


def _table(lib, ps, tuning=None):
    t = C.byref(tuning) if tuning is not None else None
    n, base = C.c_int32(-1), C.c_int32(-1)
    abi.check(lib.pt_debug_shade_table(C.byref(ps.desc), t, None, 0, C.byref(n), C.byref(base)), "pt_debug_shade_table")
    table = np.zeros((n.value, 4), np.float32)
    if n.value:
        abi.check(lib.pt_debug_shade_table(C.byref(ps.desc), t, table.ctypes.data_as(C.POINTER(C.c_float)), len(table), None, None), "pt_debug_shade_table")
    return table, base.value


def _record_offsets(blob, n_runs):
    """{hittable index: (offset of its first record, device kind)} from the blob's run headers (kind, first record, count, first hittable)"""
    out = {}
    for kind, off, count, first in blob[:n_runs].view(np.int32):
        assert kind in (1, 3), "rect and box runs only"  # DK_RECT, DK_BOX: two records per hittable
        for j in range(count):
            out[first + j] = (off + 2 * j, kind)
    return out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_hittable_has_its_record_where_its_hit_word_points(lib, name):
    make, knobs = SCENES[name]
    ps = make()
    tuning = abi.tuning(**knobs) if knobs else None
    blob, n_runs = P.flatten_tuned(lib, ps, tuning) if tuning is not None else P.flatten(lib, ps)
    pools = P.pools(blob, n_runs)
    assert len(pools) == (0 if name in ("rects_unpooled",) else 1), pools
    if name == "rect_pool":
        assert pools[0][1] == 5
    table, base = _table(lib, ps, tuning)
    d = ps.desc
    where = _record_offsets(blob, n_runs)
    assert sorted(where) == list(range(d.n_hittables))
    assert base == min(o for o, _ in where.values()) >> 1, "the first record of the list"
    assert len(table) == d.n_hittables + (n_runs >> 1)
    seen = set()
    for i in range(d.n_hittables):
        off, dk = where[i]
        at = (off >> 1) - base
        assert 0 <= at < len(table) and at not in seen, (i, off, at)
        seen.add(at)
        h = d.hittables[i]
        m = d.materials[h.material]
        colour = np.array(d.textures[m.texture].color0[:3], np.float32)
        assert (table[at, :3].view(np.uint32) == colour.view(np.uint32)).all(), (i, table[at], colour)
        word = int(table[at, 3:4].view(np.int32)[0])
        axis = {abi.PT_HIT_XY_RECT: 0, abi.PT_HIT_XZ_RECT: 1, abi.PT_HIT_YZ_RECT: 2, abi.PT_HIT_BOX: 0}[h.kind]
        assert word & 3 == axis and bool(word & 4) == (h.kind == abi.PT_HIT_BOX) == (dk == 3), (i, hex(word))
        assert (word >> 4) & 7 == m.kind and m.kind in (abi.PT_MAT_LAMBERTIAN, abi.PT_MAT_LIGHTSOURCE), (i, hex(word))
        assert word >> 8 == i and word & 0x88 == 0, (i, hex(word))
    rest = np.delete(table, sorted(seen), axis=0)
    assert not rest.view(np.uint32).any(), "records no hittable maps to are zero"
    if name == "rect_pool":
        lights = [i for i in range(d.n_hittables) if d.materials[d.hittables[i].material].kind == abi.PT_MAT_LIGHTSOURCE]
        assert lights == [1] and tuple(table[(where[1][0] >> 1) - base, :3]) == (15.0, 14.0, 13.0)


def test_the_blob_and_the_materials_are_what_they_were(lib):
    """the table is a buffer of its own behind the materials: pt_debug_flatten's blob and material table do not know it"""
    ps = pack(scenes.cornell_box()[0])
    n_f4, n_runs = C.c_int32(), C.c_int32()
    assert lib.pt_debug_flatten(C.byref(ps.desc), None, 0, C.byref(n_f4), C.byref(n_runs), None, 0, None) == 0
    mats = np.zeros((4 * ps.desc.n_materials, 4), np.float32)
    blob = np.zeros((n_f4.value, 4), np.float32)
    assert lib.pt_debug_flatten(C.byref(ps.desc), blob.ctypes.data_as(C.POINTER(C.c_float)), len(blob), None, None,
                                mats.ctypes.data_as(C.POINTER(C.c_float)), len(mats), None) == 0
    (off, n, first), = P.pools(blob, n_runs.value)
    assert first - 1 == off + 2 * n + 2 * n + 16 * n, "slab entries, exact entries, octant table, aux record: nothing between them"
    table, _ = _table(lib, ps)
    assert len(table) == 8 + (n_runs.value >> 1)


def _with(hittable):
    hs, _ = scenes.cornell_box()
    return pack(list(hs) + [hittable])


@pytest.mark.parametrize("name,make", [
    ("metal", lambda: _with(box((100, 0, 100), (150, 50, 150), metal_material((0.8, 0.7, 0.6), 0.1)))),
    ("checker", lambda: _with(box((100, 0, 100), (150, 50, 150), lambertian_material(checker_texture((0.1, 0.1, 0.1), (0.9, 0.9, 0.9))))))])
def test_other_materials_get_no_table_and_the_kernels_they_had(lib, name, make):
    ps = make()
    table, base = _table(lib, ps)
    assert len(table) == 0 and base == 0
    pl = PP.derived_plan(lib, ps, 64, 48, 8)
    assert (pl["one"], pl["lds"], pl["mats"]) == (0, 0, 0), ("not the headline family's business: the generic kernels, as before", pl)


def test_other_hittables_get_no_table(lib):
    ps = _with(sphere((190, 240, 150), 60.0, _RED))
    assert len(_table(lib, ps)[0]) == 0
    pl = PP.derived_plan(lib, ps, 64, 48, 8)
    assert (pl["one"], pl["mats"]) == (0, 0), pl


def test_the_headline_kernel_is_still_chosen_and_the_entry_point_checks_its_arguments(lib):
    ps = pack(scenes.cornell_box()[0])
    for w, h in ((64, 48), (1920, 1080)):
        pl = PP.derived_plan(lib, ps, w, h, 8)
        assert (pl["one"], pl["n"], pl["lds"], pl["mats"]) == (1, 8, 1, K.MATS_RECTBOX), pl
    n = C.c_int32(7)
    assert lib.pt_debug_shade_table(None, None, None, 0, C.byref(n), None) != 0 and n.value == 7
    small = np.zeros((2, 4), np.float32)
    assert lib.pt_debug_shade_table(C.byref(ps.desc), None, small.ctypes.data_as(C.POINTER(C.c_float)), len(small), None, None) == abi.PT_ERR_INVALID_ARG
    assert "pt_debug_shade_table" in abi.SIGNATURES
