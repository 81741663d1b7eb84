"""Resources of the firefly stage's kernel (path_tracer_amd/csrc/pt_firefly.hpp), checked at build time the way
tests/test_display_resources_cpu.py checks the display stage's (hipcc cross-compiles gfx950 without a GPU): both instantiations of
`firefly_kernel` run without scratch memory at an occupancy of 4 waves per SIMD or more; the staged one's LDS is its tile with the halo of
one pixel — (32 + 2) x (8 + 2) slots of one 16-byte record (R, G, B, Y) = 5440 bytes — and the workgroup's two counts, 8 bytes, which the
compiler rounds up to the records' 16-byte alignment: 5456 bytes per workgroup; the PT_FIREFLY_NO_LDS one uses none."""
import re

import pytest

import kernel_resource_usage
from path_tracer_amd import abi

OTHERS = ("bin_", "band_kernel", "temporal_", "atrous", "vdn_", "variance_estimate", "aov_kernel", "render_kernel", "display_")  # substrings other resource tests count kernels by
LDS_BYTES = ((abi.PT_FIREFLY_TILE_W + 2) * (abi.PT_FIREFLY_TILE_H + 2) * 16 + 2 * 4 + 15) // 16 * 16  # tile + counts, in units of the records' alignment


@pytest.fixture(scope="module")
def usage():
    return kernel_resource_usage.usage()


def staged(name):
    """Is this mangled name firefly_kernel<true> (the LDS path)?"""
    return re.search(r"firefly_kernelILb([01])E", name).group(1) == "1"


def test_firefly_kernels_have_no_scratch_and_the_lds_of_their_tile(usage):
    ours = {n: v for n, v in usage.items() if "firefly_" in n}
    assert sorted(re.search(r"firefly_[a-z]+", n).group(0) for n in ours) == ["firefly_kernel"] * 2, sorted(ours)
    assert sorted(staged(n) for n in ours) == [False, True]
    assert LDS_BYTES == 5456
    for name, v in ours.items():
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["Occupancy [waves/SIMD]"] >= 4, (name, v)
        assert v["LDS Size [bytes/block]"] == (LDS_BYTES if staged(name) else 0), (name, v)


def test_names_stay_clear_of_the_other_kernel_tables(usage):
    ours = [n for n in usage if "firefly_" in n]
    assert ours
    for name in ours:
        for other in OTHERS:
            assert other not in name, (name, other)
