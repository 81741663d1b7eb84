"""Resources of the spatial variance estimate's kernel (path_tracer_amd/csrc/pt_spatial_variance.hpp), checked at build time the way
tests/test_firefly_resources_cpu.py checks the firefly stage's (hipcc cross-compiles gfx950 without a GPU): both instantiations of
`svar_kernel` run without scratch memory at the occupancy the compiled kernel has — 8 waves per SIMD, the most a SIMD holds: 39 and 49
VGPRs, and 9 workgroups' LDS fit a CU's 160 KiB —; the staged one's LDS is its tile with the halo of PT_SVAR_MAX_RADIUS pixels —
(32 + 6) x (8 + 6) slots of two 16-byte records, (e.rgb, z) and (n.xyz, k) = 17024 bytes — and the workgroup's two counts, 8 bytes, which
the compiler rounds up to the records' 16-byte alignment: 17040 bytes per workgroup; the PT_SVAR_NO_LDS one uses none."""
import re

import pytest

import kernel_resource_usage
from path_tracer_amd import abi

# substrings other resource tests count kernels by
OTHERS = ("bin_", "band_kernel", "temporal_", "atrous", "vdn_", "variance_estimate", "aov_kernel", "render_kernel", "display_", "firefly_")
SLOTS = (abi.PT_SVAR_TILE_W + 2 * abi.PT_SVAR_MAX_RADIUS) * (abi.PT_SVAR_TILE_H + 2 * abi.PT_SVAR_MAX_RADIUS)
LDS_BYTES = (SLOTS * 2 * 16 + 2 * 4 + 15) // 16 * 16  # tile + counts, in units of the records' alignment
OCCUPANCY = 8  # waves per SIMD: what the compiled kernel has (profiles/spatial_variance_bench.txt: compiled, not measured)


@pytest.fixture(scope="module")
def usage():
    return kernel_resource_usage.usage()


def staged(name):
    """Is this mangled name svar_kernel<true> (the LDS path)?"""
    return re.search(r"svar_kernelILb([01])E", name).group(1) == "1"


def test_svar_kernels_have_no_scratch_and_the_lds_of_their_tile(usage):
    ours = {n: v for n, v in usage.items() if "svar_" in n}
    assert sorted(re.search(r"svar_[a-z]+", n).group(0) for n in ours) == ["svar_kernel"] * 2, sorted(ours)
    assert sorted(staged(n) for n in ours) == [False, True]
    assert SLOTS == 38 * 14 and LDS_BYTES == 17040
    for name, v in ours.items():
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["Occupancy [waves/SIMD]"] >= OCCUPANCY, (name, v)
        assert v["LDS Size [bytes/block]"] == (LDS_BYTES if staged(name) else 0), (name, v)


def test_names_stay_clear_of_the_other_kernel_tables(usage):
    ours = [n for n in usage if "svar_" in n]
    assert ours
    for name in ours:
        for other in OTHERS:
            assert other not in name, (name, other)
    # and the other way round: no other kernel is taken for one of these
    assert len(ours) == 2
