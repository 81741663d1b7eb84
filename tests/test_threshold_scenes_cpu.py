"""The recipes of tests/threshold_scenes.py, held to what they claim — no GPU.  For every recipe: the size the library's probes report is
the limit itself ("at") or lies in (limit, limit + 64] bytes / is the limit plus one record ("above"); the flattener did what the recipe
says (a slab pool or none, octant tables or none, spheres in a grid, a pooled triangle run, a shade table, the absorbed runs);
pt_debug_pool_plan's LDS / MATS words agree where the family has them; and the scene's marker — the last hittable, with the last material
and the last shade record — is the first hit of at least eight pixels of the oracle's id plane (tests/test_aov_cpu.py: aov_np), at every
frame the GPU test renders that has that many pixels.  Every constant the recipes read from the sources must be found exactly once, and
one test shows the checks are live: expectations parsed from a scratch copy of the sources with kMaxLdsColdScene or kTileF4 moved by one
record refuse the scenes built for the real constants, while the recipes built from the copy land on the moved limits."""
import ctypes as C
import re
import shutil

import numpy as np
import pytest

import pool_octant_scenes as P
import threshold_scenes as T
from path_tracer_amd import abi

IDS = [r.name for r in T.RECIPES]
_SIZES = T.constants()["record_size"]
RECORD_F4 = {0: _SIZES["sphere"], 1: _SIZES["rect"], 2: _SIZES["triangle"], 3: _SIZES["box"], 4: _SIZES["medium"]}  # by device kind


def test_names_are_unique_and_every_threshold_has_both_sides():
    assert len(set(IDS)) == len(IDS)
    for t in ("T1", "T2", "T3", "T4", "T5", "T6"):
        sides = {r.side for r in T.RECIPES if r.threshold == t}
        assert sides == {"at", "above"}, (t, sides)


@pytest.mark.parametrize("name", sorted(T.PATTERNS))
def test_every_constant_is_found_exactly_once(name):
    got = T.matches(name)
    assert len(got) == 1, f"{name}: {len(got)} matches of {T.PATTERNS[name][1]!r} in {T.PATTERNS[name][0]}"


def check_size(r, ps):
    size = r.size(ps, r.tuning)
    lo, hi = r.expect
    assert lo <= size <= hi, f"{r.name}: probed {size}, the recipe needs [{lo}, {hi}]"
    return size


def _pools(ps, tuning):
    b, n_runs = T.blob(ps, tuning)
    return b, P.pools(b, n_runs)


def check_facts(r, ps):
    p = T.probe(ps, r.tuning)
    f = r.facts
    if "shade" in f:
        assert (p.shade_f4 > 0) == f["shade"], (r.name, p)
    if "grid" in f:
        assert (p.grid_spheres > 0) == f["grid"], (r.name, p)
    if "tri_pool" in f:
        assert (p.tri_pooled > 0) == f["tri_pool"] == bool(p.flags & 4), (r.name, p)
    if "pool" in f:
        b, pools = _pools(ps, r.tuning)
        assert (len(pools) == 1) == f["pool"] and len(pools) <= 1, (r.name, pools)
        if f["pool"]:
            off, n, first = pools[0]
            entries = first - 1 - off  # between the pool's first record and the head run's aux record: slab + exact entries (+ the table)
            plain = 2 * (n + (n & 1)) + 2 * n
            assert entries == plain + (16 * (n + (n & 1)) if f["tables"] else 0), (r.name, off, n, first)
    if "absorbed" in f:
        assert [i for i, h in enumerate(T.run_headers(ps, r.tuning)) if h[1]] == f["absorbed"], (r.name, T.run_headers(ps, r.tuning))
    if "plan" in f:
        for w, h in r.frames:
            pl = T.pool_plan(ps, w, h, r.spp, r.flags, r.tuning)
            assert (pl["lds"], pl["mats"]) == f["plan"], (r.name, pl)
    return p


@pytest.mark.parametrize("name", IDS)
def test_recipe_lands_and_its_marker_is_seen(lib, orc, name):
    r = T.by_name(name)
    ps, cam = r.make()
    size = check_size(r, ps)
    p = check_facts(r, ps)
    check_marker(lib, r, ps, p)
    seen = {}
    for w, h in r.frames:
        if w * h < 4 * T.MIN_MARKER_PIXELS:  # (the 3 x 2 frame of the streaming rows: few live lanes is its point)
            continue
        seen[(w, h)] = T.marker_pixels(orc, ps, cam, w, h)
        assert seen[(w, h)] >= T.MIN_MARKER_PIXELS, f"{name} {w}x{h}: the marker is the first hit of {seen[(w, h)]} pixels"
    assert seen, name
    print(f"{name}: {ps.n_hittables} hittables, probed {size} of {r.expect}, {tuple(p)}, marker pixels {seen}")


def check_marker(lib, r, ps, p):
    """the last hittable alone uses the last material; its records end the blob; its shade record is the table's last"""
    last = ps.hittables[ps.n_hittables - 1]
    assert last.material == ps.n_materials - 1 and [h.material for h in ps.hittables[:ps.n_hittables - 1]].count(last.material) == 0, r.name
    heads = T.run_headers(ps, r.tuning)
    kind, _, off, count, first = max(heads, key=lambda h: h[2])
    size = RECORD_F4[kind]
    assert first + count == ps.n_hittables and off + size * count == p.blob_f4, (r.name, heads[-1], p)
    if p.shade_f4:
        t = abi.tuning(**r.tuning) if r.tuning else abi.tuning()
        table = np.zeros((p.shade_f4, 4), np.float32)
        base = C.c_int32()
        abi.check(lib.pt_debug_shade_table(C.byref(ps.desc), C.byref(t), table.ctypes.data_as(C.POINTER(C.c_float)), len(table), None, C.byref(base)), "pt_debug_shade_table")
        at = ((off + size * (count - 1)) >> 1) - base.value
        assert at == p.shade_f4 - 1 and int(table[at, 3:4].view(np.int32)[0]) >> 8 == ps.n_hittables - 1, (r.name, at, p.shade_f4)


def test_land_raises_where_it_cannot_reach_the_target():
    make = lambda **kw: T.rectbox(**kw)  # noqa: E731
    size = lambda s: T.staged_size(s[0], None)  # noqa: E731
    with pytest.raises(LookupError):
        T.land(make, size, 10240 + 7, [("rects", 0, 56), ("cols", 1, 40)])  # (every table is whole records of 16 bytes)


@pytest.mark.parametrize("constant,file,records,rows", [
    ("kMaxLdsColdScene", "pt_render.hip", 16, ("T1-a-at", "T1-d-at")),             # one 16-byte record
    ("kTileF4", "pt_render.hip", 3, ("T5-sphere-tile-at", "T5-triangle-tile-above")),  # one sphere / triangle record of three f4
])
def test_a_constant_moved_by_one_record_is_noticed(tmp_path, constant, file, records, rows):
    """a scratch copy of the sources with the constant one record larger: the scenes built for the library's constant miss the moved
    expectation (the size check is live), and the recipes built from the copy follow it"""
    for f in {f for f, _ in T.PATTERNS.values()}:
        shutil.copy(T.CSRC / f, tmp_path / f)
    text = (tmp_path / file).read_text()
    new, n = re.subn(r"(constexpr \w+ " + constant + r" = )([0-9][0-9 *]*);", lambda m: f"{m.group(1)}{T._value(m.group(2)) + records};", text)
    assert n == 1
    (tmp_path / file).write_text(new)
    c = T.constants(tmp_path)
    assert c[constant] == T.constants()[constant] + records
    theirs = {r.name: r for r in T.recipes(c)}
    for name in rows:
        ps, _ = T.by_name(name).make()
        with pytest.raises(AssertionError):
            check_size(theirs[name], ps)
        check_size(theirs[name], theirs[name].make()[0])
