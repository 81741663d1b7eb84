"""The octant tables of the slab pools (pt_flatten.hpp; read by the sign-resolved slab pass of the LDS kernels, pt_device.hpp: slab_chunk_pass),
through pt_debug_flatten — no GPU.  Behind a pool's exact entries and in front of its head run's aux record: per slab entry (the all-NaN pad
entry included) and direction octant q = sx | sy << 1 | sz << 2 two records, (near.xyz, 0) and (far.xyz, 0), near_c = s_c ? hi_c : lo_c;
[entry][octant][near, far], 16 records per entry.  Nothing else moves: the blob without the tables (PT_NO_POOL_OCTANTS, the experiments'
switch) is this blob with the tables cut out and the record offsets behind them shifted.  All pools of a scene get their tables or none does:
none where the blob with them would not fit the 64 KB LDS image."""
import numpy as np
import pytest

import pool_octant_scenes as P
import scenes_small as S

SCENES = {"cornell": (lambda: S.cornell_scene()[0], 8), "field7": (lambda: P.box_field(4)[0], 7), "field21": (lambda: P.box_field(18)[0], 21)}


@pytest.fixture(params=sorted(SCENES))
def flat(request, lib, monkeypatch):
    make, n = SCENES[request.param]
    ps = make()
    blob, n_runs = P.flatten(lib, ps)
    monkeypatch.setenv("PT_NO_POOL_OCTANTS", "1")
    plain, n_runs_plain = P.flatten(lib, ps)
    monkeypatch.delenv("PT_NO_POOL_OCTANTS")
    assert n_runs == n_runs_plain
    return blob, plain, n_runs, n


def test_table_sits_behind_the_exact_entries_and_holds_the_bounds_by_octant(flat):
    blob, plain, n_runs, n = flat
    (off, entries, first), = P.pools(blob, n_runs)
    assert entries == n
    ns = n + (n & 1)
    tab = off + 2 * ns + 2 * n
    assert tab + 16 * ns == first - 1, "the table ends where the head run's aux record sits"
    assert len(blob) == len(plain) + 16 * ns, "exactly 16 records per (padded) entry"
    table = blob[tab:tab + 16 * ns].reshape(ns, 8, 2, 4)
    assert (table[..., 3].view(np.uint32) == 0).all()
    slab = blob[off:off + 2 * ns].reshape(ns, 2, 4)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for e in range(ns):
        lo, hi = slab[e, 0, :3], slab[e, 1, :3]
        for q in range(8):
            for ax in range(3):
                s = (q >> ax) & 1
                assert bits(table[e, q, 0, ax]) == bits(hi[ax] if s else lo[ax]), (e, q, ax, "near")
                assert bits(table[e, q, 1, ax]) == bits(lo[ax] if s else hi[ax]), (e, q, ax, "far")
    if ns > n:
        assert np.isnan(table[n, :, :, :3]).all() and np.isnan(slab[n, :, :3]).all(), "the pad entry is all NaN"
    assert not np.isnan(table[:n]).any()
    # a rect is a slab entry with lo == hi on its own axis: its plane is in near AND far of every octant
    rects = [(e, ax) for e in range(n) for ax in range(3) if slab[e, 0, ax] == slab[e, 1, ax]]
    assert len(rects) == 1, rects
    e, ax = rects[0]
    assert (table[e, :, 0, ax] == slab[e, 0, ax]).all() and (table[e, :, 1, ax] == slab[e, 0, ax]).all()


def test_nothing_else_moves(flat):
    """slab entries, exact entries, aux record and every hittable's record are what they are without the tables; offsets behind a table shift by its size"""
    blob, plain, n_runs, n = flat
    (off, entries, first), = P.pools(blob, n_runs)
    (off_p, entries_p, first_p), = P.pools(plain, n_runs)
    ns = n + (n & 1)
    grow = 16 * ns
    assert (off, entries) == (off_p, entries_p) and first == first_p + grow
    cut = np.concatenate([blob[:off + 2 * ns + 2 * n], blob[first - 1:]]).copy()
    assert len(cut) == len(plain)
    hdr = cut[:n_runs].view(np.int32)
    hdr[:, 1] -= grow                                            # every run's records lie behind the table
    ids = cut[off + 2 * ns:off + 2 * ns + 2 * n:2].view(np.int32)
    ids[:, 3] -= grow                                            # hit ids of the exact entries: 25-bit record offsets
    assert (cut.view(np.uint32) == plain.view(np.uint32)).all()
    # where they were: slab entries at the pool offset, exact entries behind them, aux at first record - 1 with its four fields
    aux, aux_p = blob[first - 1], plain[first_p - 1]
    assert (aux.view(np.uint32) == aux_p.view(np.uint32)).all()
    assert aux.view(np.int32)[2] == off and aux.view(np.int32)[3] == n and aux.view(np.int32)[1] >= 1


def test_a_scene_whose_tables_would_not_fit_gets_none(lib, monkeypatch):
    ps, _ = P.many_boxes()
    blob, n_runs = P.flatten(lib, ps)
    (off, n, first), = P.pools(blob, n_runs)
    assert n == 260 and (len(blob) + 16 * n) * 16 > 64 * 1024 >= len(blob) * 16
    assert first - 1 == off + 2 * n + 2 * n, "aux directly behind the exact entries: no table"
    monkeypatch.setenv("PT_NO_POOL_OCTANTS", "1")
    plain, _ = P.flatten(lib, ps)
    assert (blob.view(np.uint32) == plain.view(np.uint32)).all()
