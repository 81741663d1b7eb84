"""CPU tests of the oracle itself: pinned against the reference's own xorshift.hpp (oracle/_ref, golden
fixture), the LocalPseudoRNG known answers SURVEY.md §8a/a13 recorded from the reference headers, the
committed golden framebuffers, and self-consistency properties (thread-count independence, shard
layout, tonemap)."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import scenes_small as S
from conftest import assert_bit_identical
from path_tracer_amd import scenes

GOLDEN = Path(__file__).parent / "golden"


def test_xorshift_matches_reference_golden(orc):
    kat = json.loads((GOLDEN / "xorshift32_kat.json").read_text())
    for seed, values in kat["streams"].items():
        assert orc.xorshift_stream(int(seed), len(values)) == values, f"seed {seed}"


def ref_kat_stdout(binary: Path, name: str) -> str:
    """stdout of a known-answer binary built from the reference's own headers (oracle/_ref: oracle/Makefile target `ref`, only where
    the reference tree is present): run live where it was built — and then it must equal the record — else the record of its
    output, tests/golden/ref_kat_outputs.json."""
    rec = json.loads((GOLDEN / "ref_kat_outputs.json").read_text())[name]
    if not binary.exists():
        return rec["stdout"]
    out = subprocess.run([str(binary)] + rec["args"], capture_output=True, text=True, check=True).stdout
    assert out == rec["stdout"], f"{binary.name}: output differs from tests/golden/ref_kat_outputs.json"
    return out


def test_xorshift_matches_reference_binary_live(orc):
    """oracle/_ref/xorshift_kat is the reference's own xorshift.hpp compiled from /root/reference."""
    seeds = [1, 2, 12345, 2463534242, 0xFFFFFFFF, 0x80000000, 77777]
    out = ref_kat_stdout(orc.REF_KAT, "xorshift_kat")
    assert len(out.strip().splitlines()) == len(seeds)
    for line, seed in zip(out.strip().splitlines(), seeds):
        head, vals = line.split(":")
        assert int(head) == seed
        assert orc.xorshift_stream(seed, 64) == [int(v) for v in vals.split()]


def test_dev_visit_dispatches_by_variant_index_live(orc):
    """oracle/_ref/visit_kat is the reference's own visit.hpp:51-67 compiled from /root/reference: dev_visit selects the alternative
    whose position in the variant equals index(), and hands the callable THAT alternative — so the ABI's integer tags
    (include/pt_render.h: PT_HIT_* / PT_MAT_* / PT_TEX_*, the rect axis, the medium's boundary kind), which are the reference's
    variant positions, name the code path the reference would take."""
    from path_tracer_amd import abi
    out = ref_kat_stdout(orc.REF_VISIT_KAT, "visit_kat").strip().splitlines()
    rows = [l.split() for l in out]
    fam = {}
    for name, index, tag, payload in rows:
        fam.setdefault(name, []).append((int(index), int(tag), int(payload)))
    assert {k: len(v) for k, v in fam.items()} == {"hittable": 5, "material": 5, "texture": 3, "rectangle": 3, "volume": 2}
    for name, items in fam.items():
        for pos, (index, tag, payload) in enumerate(items):
            assert index == pos and payload == 1000 + pos, (name, pos, index, payload)   # the alternative that was constructed is the one visited
            if name != "volume":
                assert tag == index, (name, index, tag)                                   # ABI tag == variant position
    assert [t for _, t, _ in fam["hittable"]] == [abi.PT_HIT_SPHERE, abi.PT_HIT_XY_RECT, abi.PT_HIT_TRIANGLE, abi.PT_HIT_BOX, abi.PT_HIT_CONSTANT_MEDIUM]
    assert [t for _, t, _ in fam["material"]] == [abi.PT_MAT_LAMBERTIAN, abi.PT_MAT_METAL, abi.PT_MAT_DIELECTRIC, abi.PT_MAT_LIGHTSOURCE, abi.PT_MAT_ISOTROPIC]
    assert [t for _, t, _ in fam["texture"]] == [abi.PT_TEX_CHECKER, abi.PT_TEX_SOLID, abi.PT_TEX_IMAGE]


def test_survey_known_answers(orc):
    """values recorded from the reference headers (glibc libm)."""
    import ctypes as C
    lib = orc.load()
    orc.set_math(False)
    assert orc.xorshift_stream(2463534242, 5) == [3025102972, 3741822969, 1677395098, 2769794366, 3968916907]
    assert orc.xorshift_stream(12345, 5) == [20675, 61662, 70600, 209832, 351486]
    assert orc.xorshift_stream(1, 5) == [3, 5, 15, 17, 51]
    assert orc.xorshift_stream(0, 4) == [0, 0, 0, 0]  # pixel 0 is stuck at 0 (render.hpp:131, xorshift.hpp:56)
    s = C.c_uint32(2463534242)
    got = [lib.orc_float_t(C.byref(s)) for _ in range(3)]
    np.testing.assert_allclose(got, [0.704336643, 0.871211052, 0.390548974], rtol=0, atol=5e-10)
    s = C.c_uint32(12345)
    v = (C.c_float * 3)()
    lib.orc_unit_vec(C.byref(s), v)
    np.testing.assert_allclose(list(v), [-0.999990344, -0.00439440506, -3.33104108e-05], rtol=2e-7)
    s = C.c_uint32(2463534242)
    lib.orc_in_unit_ball(C.byref(s), v)
    np.testing.assert_allclose(list(v), [0.457593143, -0.479916424, 0.237442195], rtol=3e-7)
    lib.orc_in_unit_disk(C.byref(s), v)  # continues the same stream, as the survey's probe did
    np.testing.assert_allclose(list(v), [0.289785981, 0.811777234, 0.0], rtol=3e-7)


def test_float_t_can_be_exactly_one(orc):
    """state >= 0xFFFFFF80 rounds to 2^32 in uint32->float (rtweekend.hpp:40-41)."""
    import ctypes as C
    lib = orc.load()
    # find a predecessor state whose successor is >= 0xFFFFFF80 by stepping the bijection backwards is hard;
    # instead check the conversion the generator relies on
    assert np.float32(np.uint32(0xFFFFFF80)) * np.float32(2.0 ** -32) == np.float32(1.0)
    assert np.float32(np.uint32(0xFFFFFF7F)) * np.float32(2.0 ** -32) < np.float32(1.0)
    s = C.c_uint32(1)
    assert lib.orc_float_t(C.byref(s)) == np.float32(3) * np.float32(2.0 ** -32)


@pytest.mark.parametrize("name", ["cornell", "mixed", "spheres", "triangles", "ties", "empty"])
def test_golden_framebuffers(orc, name):
    """The oracle reproduces the committed fixtures (portable math: independent of the host's libm)."""
    g = np.load(GOLDEN / f"fb_{name}_32x18x4.npy")
    ps, cam = S.ALL[name]()
    c = scenes.make_camera(cam, 32, 18)
    orc.set_math(True)
    fb = orc.render(ps, c.c, 32, 18, 4)
    assert_bit_identical(fb, g, name)


def test_cornell_is_libm_independent(orc):
    """The headline scene uses no transcendental at all (rects, lambertian, solid, light): both math modes agree."""
    ps, cam = S.cornell_scene()
    c = scenes.make_camera(cam, 40, 24)
    orc.set_math(False)
    a = orc.render(ps, c.c, 40, 24, 6)
    orc.set_math(True)
    b = orc.render(ps, c.c, 40, 24, 6)
    assert_bit_identical(a, b)


def test_thread_count_independent(orc, monkeypatch):
    """Per-pixel RNG => output independent of the OpenMP schedule (SURVEY.md §6 'determinism')."""
    import os
    ps, cam = S.mixed_scene()
    c = scenes.make_camera(cam, 24, 16)
    orc.set_math(True)
    a = orc.render(ps, c.c, 24, 16, 5)
    rows = [orc.render_rows(ps, c.c, 24, 16, 5, y, y + 1) for y in range(16)]
    assert_bit_identical(a, np.concatenate(rows, axis=0))


@pytest.mark.parametrize("shards", [2, 3, 8])
@pytest.mark.parametrize("size", [(24, 16), (21, 13)])
def test_shard_layout_roundtrip(orc, shards, size):
    """Any partition of pixels gives the single-device image (seed = GLOBAL linear id, render.hpp:130-131)."""
    from dist_util import unshard_reference
    w, h = size
    ps, cam = S.spheres_scene()
    c = scenes.make_camera(cam, w, h)
    orc.set_math(True)
    full = orc.render(ps, c.c, w, h, 3)
    parts = [orc.render(ps, c.c, w, h, 3, shard_index=i, shard_count=shards) for i in range(shards)]
    assert_bit_identical(unshard_reference(np.stack(parts), w, h, shards), full)


def test_depth_zero_and_one(orc):
    ps, cam = S.spheres_scene()
    c = scenes.make_camera(cam, 16, 8)
    assert not orc.render(ps, c.c, 16, 8, 2, depth=0).any()
    one = orc.render(ps, c.c, 16, 8, 2, depth=1)  # only sky / emitters / absorbed paths contribute
    assert np.isfinite(one).all()


def test_per_pixel_ray_counts(orc):
    """orc_render_pixels_rays: the colours are those of the frame, the per-pixel ray counts (the sequential chain lengths
    behind DESIGN.md section 6) add up to the frame's ray counter, and a background-only pixel traces one ray per sample."""
    ps, cam = S.cornell_scene()
    w, h, spp = 24, 16, 5
    c = scenes.make_camera(cam, w, h)
    orc.set_math(True)
    fb, ctr = orc.render(ps, c.c, w, h, spp, counters=True)
    xy = np.array([[x, y] for y in range(h) for x in range(w)], dtype=np.int32)
    col, rays = orc.render_pixels_rays(ps, c.c, w, h, spp, xy)
    assert_bit_identical(col.reshape(h, w, 3), fb)
    assert int(rays.sum()) == ctr.as_dict()["rays"]
    assert rays.min() >= spp
    pe, came = S.empty_scene()
    ce = scenes.make_camera(came, 8, 8)
    _, r0 = orc.render_pixels_rays(pe, ce.c, 8, 8, 7, np.array([[3, 4]], dtype=np.int32))
    assert int(r0[0]) == 7


def test_pixel_zero_rng_stuck(orc):
    """Pixel (0,0) has state 0 forever: u=v=0 jitter, lens sample x=-1,y=0 (render.hpp:131)."""
    ps, cam = S.empty_scene()
    c = scenes.make_camera(cam, 8, 8)
    a = orc.render(ps, c.c, 8, 8, 1)
    b = orc.render(ps, c.c, 8, 8, 2)  # (x + x) / 2 is exact
    assert_bit_identical(a[0, 0], b[0, 0])


def test_tonemap(orc):
    fb = np.array([[[0.0, 0.25, 1.0], [4.0, -1.0, np.nan]], [[0.5, 0.999 ** 2, 1e-8], [np.inf, 0.04, 0.09]]], dtype=np.float32)
    out = orc.tonemap_rgb8(fb)
    # rows flipped: output row 0 is fb row 1
    assert out[0, 0].tolist() == [int(256 * np.sqrt(np.float32(0.5))), int(np.float32(256) * np.sqrt(np.float32(0.999 ** 2))), 0]
    assert out[0, 1].tolist() == [255, 51, 76]
    assert out[1, 0].tolist() == [0, 128, 255]
    assert out[1, 1].tolist() == [255, 0, 0]  # sqrt(-1)=NaN and NaN -> 0 (defined; UB in main.cpp:45)


def test_bad_scene_rejected(orc):
    import ctypes as C
    from path_tracer_amd import abi
    ps, cam = S.cornell_scene()
    c = scenes.make_camera(cam, 8, 8)
    ps.hittables[0].material = 99
    fb = np.zeros((8, 8, 3), np.float32)
    p = orc.params(8, 8, 1)
    rc = orc.load().orc_render(C.byref(ps.desc), C.byref(c.c), C.byref(p), fb.ctypes.data_as(C.POINTER(C.c_float)), None)
    assert rc == abi.PT_ERR_BAD_SCENE


def test_fast_mode_restatement_is_deterministic_and_seeds_never_zero(orc):
    """PT_FLAG_FAST_RNG's checker (NOT the reference's image): deterministic, differs from the parity image, equals it
    nowhere by accident of a zero seed — pt_fast_seed(pixel, chunk) is never 0 (a zero xorshift32 state is stuck)."""
    import ctypes as C
    import re
    from pathlib import Path
    from path_tracer_amd import abi
    hdr = (Path(__file__).resolve().parent.parent / "include" / "pt_render.h").read_text()
    assert int(re.search(r"#define PT_FAST_CHUNK_SPP (\d+)", hdr).group(1)) == abi.PT_FAST_CHUNK_SPP == 64
    assert f"PT_FLAG_FAST_RNG = 1u << {abi.PT_FLAG_FAST_RNG.bit_length() - 1}" in hdr
    ps, cam = S.spheres_scene()
    c = scenes.make_camera(cam, 24, 14)
    orc.set_math(True)
    a = orc.render(ps, c.c, 24, 14, 70, flags=abi.PT_FLAG_FAST_RNG)
    b = orc.render(ps, c.c, 24, 14, 70, flags=abi.PT_FLAG_FAST_RNG)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a).all()
    assert not np.array_equal(a, orc.render(ps, c.c, 24, 14, 70))
    # the header's seed function, restated: murmur-style finaliser of (pixel, chunk), 0 mapped to 1
    def seed(pixel, chunk):
        h = (pixel * 0x9E3779B1 + chunk * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF
        h ^= h >> 16; h = (h * 0x7FEB352D) & 0xFFFFFFFF; h ^= h >> 15; h = (h * 0x846CA68B) & 0xFFFFFFFF; h ^= h >> 16
        return h or 1
    from path_tracer_amd import abi as _abi
    plib = _abi.load_library()
    plib.pt_fast_seed.restype = C.c_uint32
    plib.pt_fast_seed.argtypes = [C.c_uint32, C.c_uint32]
    assert all(plib.pt_fast_seed(p, k) == seed(p, k) for p in (0, 1, 77, 2073599, 0xFFFFFFFF) for k in (0, 1, 15, 126))
    seen = {seed(p, k) for p in range(0, 4000) for k in range(16)}
    assert 0 not in seen and len(seen) > 0.999 * 4000 * 16
    # pixel (0,0), one chunk: the oracle's stream starts at seed(0, 0) — first sample of pixel 0 differs from the stuck parity stream
    px = orc.render_pixels(ps, c.c, 24, 14, 3, np.array([[0, 0]], np.int32), flags=abi.PT_FLAG_FAST_RNG)
    assert np.isfinite(px).all()


def test_single_stream_executor_restatement(orc):
    """render.hpp:113-122 (USE_SINGLE_TASK): one default-seeded stream for the whole frame, x-outer / y-inner.  The first
    pixel visited is (0, 0) with state 2463534242 — so, unlike the parallel executor's pixel 0 (seed 0: stuck generator),
    its first sample is an ordinary one; swapping the loop order would change every later pixel."""
    from path_tracer_amd import abi
    ps, cam = S.cornell_scene()
    c = scenes.make_camera(cam, 6, 4)
    orc.set_math(True)
    single = orc.render(ps, c.c, 6, 4, 2, flags=abi.PT_FLAG_SINGLE_STREAM)
    parallel = orc.render(ps, c.c, 6, 4, 2)
    assert np.isfinite(single).all() and not np.array_equal(single, parallel)
    again = orc.render(ps, c.c, 6, 4, 2, flags=abi.PT_FLAG_SINGLE_STREAM)
    assert np.array_equal(single.view(np.uint32), again.view(np.uint32))
    # a 1x1 frame: pixel (0,0) of the single stream = what the parallel executor computes for a pixel seeded 2463534242;
    # use a frame whose pixel with that linear id exists: id = y * width + x with width > id is too large, so check the
    # draw count instead: one sample of the 1x1 frame advances the shared state exactly as the counters say
    _, ctr = orc.render(ps, c.c, 1, 1, 1, counters=True, flags=abi.PT_FLAG_SINGLE_STREAM)
    assert ctr.samples == 1 and ctr.rng_draws >= 5  # jitter x2 + lens disk x2 + time, then 3 per lambertian bounce
