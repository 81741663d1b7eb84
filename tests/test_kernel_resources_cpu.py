"""Register budget of the hot kernels, checked at build time (hipcc cross-compiles gfx950 without a GPU): the resident
kernels for scenes without image textures must fit 7 waves per SIMD (<= 72 VGPRs) WITHOUT scratch — a spill there sits
around every list scan and cost 4 % of the headline number when a wider triangle loop once pushed them over."""
import re

import pytest

import kernel_resource_usage
import kernel_variant_cases as K
from kernel_resource_usage import flags as _flags  # noqa: F401 (the ISA tests import the Makefile's FLAGS from here)


@pytest.fixture(scope="module")
def usage():
    return kernel_resource_usage.usage()


def test_headline_kernels_fit_seven_waves_without_scratch(usage):
    # render_kernel<UV_NONE, LDS, MLDS, COOP=false, CL, FAST=false, BADOUEL=false, GRID=0, TRIPOOL=false, MATS>: the instantiations
    # scenes without a sphere grid run — generic shading (MATS_ALL = 287) and the lambertian + light / solid-texture
    # specialisation the headline Cornell-style scene takes (MATS = 9); mangled ...render_kernelILi0ELb?ELb?ELb0ELb?ELb0ELb0ELi0ELb0ELi<MATS>E...
    # (65545 = MATS_LAMB_LIGHT_SOLID | MATS_RECTBOX_ONLY, round 4: scenes of rects and boxes only — the headline scene itself — run kernels
    # that carry no sphere / triangle / medium code at all: 64 VGPRs)
    hot = {k: v for k, v in usage.items() if re.search(r"render_kernelILi0ELb[01]ELb[01]ELb0ELb[01]ELb0ELb0ELi0ELb0ELi(9|287|65545)E", k)}
    assert len(hot) == 12, sorted(usage)
    for k, v in hot.items():
        # the kernel the headline config runs (cold lane state in LDS: CL = 1) has no scratch at all; the variants that keep
        # the cold state in registers park up to seven dwords around the slab pool (once per iteration, outside every loop)
        cold_in_lds = re.search(r"render_kernelILi0ELb1ELb1ELb0ELb1E", k) is not None
        assert v["ScratchSize [bytes/lane]"] <= (0 if cold_in_lds else 28), (k, v)
        assert v["VGPRs"] <= 72 and v["Occupancy [waves/SIMD]"] >= 7, (k, v)


def test_grid_walk_and_triangle_pool_kernels(usage):
    """The image-texture kernel cfg1 / cfg3 / cfg4 run (UV_WINNER, LDS, sphere-grid walk) holds 5 waves per SIMD — what the
    scene's 31 KB LDS image allows anyway — without scratch; the triangle-pool kernels (TRIPOOL = true: one ray at a time across the
    wave over global tables) hold 5 (round 6; rounds 3-5: 7)."""
    # GRID = 1: the wave-synchronous walk (no scratch); GRID = 2: the queued walk (64 (ray, sphere) pairs per batch) keeps five more values
    # live across a batch: 20 bytes of scratch at the 96-register budget, stored before and reloaded after the walk — none inside its loops
    k1 = [v for k, v in usage.items() if re.search(r"render_kernelILi1ELb1ELb0ELb0ELb0ELb0ELb0ELi1ELb0E", k)]
    assert len(k1) == 1 and k1[0]["Occupancy [waves/SIMD]"] >= 5 and k1[0]["ScratchSize [bytes/lane]"] == 0, k1
    k2 = [v for k, v in usage.items() if re.search(r"render_kernelILi1ELb1ELb0ELb0ELb0ELb0ELb0ELi2ELb0E", k)]
    assert len(k2) == 1 and k2[0]["Occupancy [waves/SIMD]"] >= 5 and k2[0]["ScratchSize [bytes/lane]"] <= 24, k2
    pool = {k: v for k, v in usage.items() if re.search(r"render_kernelILi[012]ELb0ELb0ELb0ELb0ELb[01]ELb0ELi1ELb1E", k)}
    assert len(pool) == 6, sorted(usage)
    for k, v in pool.items():
        # FIVE waves since round 6 (rounds 3-5: seven at 72 VGPRs): with the camera rays' candidate cache in tri_pool_scan and two pair
        # batches / two expansion trips in flight in the grid walk, the 72-register build spills 228 bytes and measures 13 % slower (1080p x
        # 32 spp: 1 116 / 986 / 978 ms at 7 / 6 / 5 waves; with the pipelined walk 1 116 at 6, 979 at 5: profiles/r06_ab_tri_cache.txt,
        # r06_ab_tri_pipe.txt); none of the scratch sits in the pool's inner loops
        assert v["Occupancy [waves/SIMD]"] >= 5 and v["ScratchSize [bytes/lane]"] <= (184 if "ILi0E" in k else 256), (k, v)   # (FAST-mode variants of the pool kernels included)
    # the binned renderer's kernels (opt-in, csrc/pt_binned.hpp): the step at four waves and the band stage without scratch
    step = [v for k, v in usage.items() if "bin_step_kernel" in k]
    band = [v for k, v in usage.items() if "band_kernel" in k]
    # (three pairs: UV_NONE with both material sets, UV_WINNER with the generic one — an image texture is never "simple")
    assert len(step) == 3 and all(v["ScratchSize [bytes/lane]"] == 0 and v["Occupancy [waves/SIMD]"] >= 4 for v in step), step
    assert len(band) == 1 and band[0]["ScratchSize [bytes/lane]"] == 0 and band[0]["Occupancy [waves/SIMD]"] >= 4, band


def test_scratch_of_the_kernels_the_five_baseline_configs_launch(usage):
    """VERDICT r04 item 6-iv, as far as it can be met: which kernel each BASELINE config launches and what scratch it carries.  cfg2 (the
    headline: cold lane state in LDS, rect / box-only, lambertian + light) and cfg1 (image textures, LDS scene, in-place grid walk): NONE.
    cfg3 and the shards of cfg4 (queued grid walk): 20 bytes, stored before / reloaded after the walk, none inside its loops.  cfg5 (triangle
    pool): ~170 bytes at the 96-register budget of five waves per SIMD (round 5: ~150 at 72 / seven) — none inside the pool's inner loops, and the spill-free 4-wave
    build measured 12 % slower (profiles/r05_ab_tripool.txt): the bound below keeps it from creeping."""
    def one(pattern):
        ks = [v for k, v in usage.items() if re.search(pattern, k)]
        assert len(ks) == 1, (pattern, len(ks))
        return ks[0]["ScratchSize [bytes/lane]"]
    assert one(r"render_kernelILi0ELb1ELb1ELb0ELb1ELb0ELb0ELi0ELb0ELi65545E") == 0        # cfg2
    assert one(r"render_kernelILi1ELb1ELb0ELb0ELb0ELb0ELb0ELi1ELb0ELi287E") == 0          # cfg1
    assert one(r"render_kernelILi1ELb1ELb0ELb0ELb0ELb0ELb0ELi2ELb0ELi287E") <= 24         # cfg3, cfg4's shards
    assert one(r"render_kernelILi0ELb0ELb0ELb0ELb0ELb0ELb0ELi1ELb1ELi287E") <= 184        # cfg5 (round 6: 168 at five waves / 96 VGPRs, with the candidate cache)


def test_streaming_and_cooperative_kernels_without_image_textures(usage):
    """The streaming kernel does not spill at all.  The cooperative kernels (5 waves per SIMD, 96 VGPRs, four spheres per
    trip in both scans) keep a few dwords of per-iteration state in scratch — stores before / reloads after a whole list
    scan, none inside a record loop; measured faster than the spill-free alternatives (two spheres per trip: -3 %; 4 waves
    per SIMD and 128 VGPRs: -7 % on the 496-hittable scene)."""
    for k, v in usage.items():
        if re.search(r"render_kernel_streamILi0ELb0ELb0E", k):
            assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
        if re.search(r"render_kernelILi0ELb1ELb[01]ELb1ELb0ELb0ELb0E", k):
            assert v["ScratchSize [bytes/lane]"] <= 64 and v["Occupancy [waves/SIMD]"] >= 5, (k, v)


def test_every_compiled_variant_has_a_case_and_every_case_a_kernel(usage):
    """tests/kernel_variant_cases.py against the compiled library: the instantiations of render_kernel, render_kernel_stream, the binned
    renderer's step / finish pair and aov_kernel, decoded from their mangled names (template arguments: L[ib]<n>E groups), plus the
    single-stream kernel, are exactly the table's tags.  An instantiation the launcher gained without a row — so without an oracle
    comparison in tests/test_gpu_kernel_variants.py — fails here, and so does a row whose kernel is no longer compiled."""
    compiled, finish = [], []
    for name in usage:
        m = re.search(r"\d+(render_kernel_stream|render_kernel|bin_step_kernel|bin_finish_kernel|aov_kernel)I((?:L[ib]\d+E)+)E", name)
        if m:
            tag = (m.group(1), *(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(2))))
            (finish if tag[0] == "bin_finish_kernel" else compiled).append(tag)
        elif "render_single_stream_kernel" in name:
            compiled.append(("render_single_stream_kernel",))
    assert len(compiled) == len(set(compiled)) and len(K.ALL_TAGS) == len(set(K.ALL_TAGS)), "a tag appears twice"
    assert sorted(t[1:] for t in finish) == sorted(t[1:] for t in compiled if t[0] == "bin_step_kernel"), "the binned step / finish kernels come in pairs"
    missing, stale = sorted(set(compiled) - set(K.ALL_TAGS)), sorted(set(K.ALL_TAGS) - set(compiled))
    assert not missing, f"compiled kernel variants without a row in tests/kernel_variant_cases.py: {missing}"
    assert not stale, f"rows of tests/kernel_variant_cases.py whose kernel is not compiled: {stale}"
    assert len([t for t in compiled if t[0] == "render_kernel"]) == 50 and len([t for t in compiled if t[0] == "render_kernel_stream"]) == 9
