"""Resources of the temporal reprojection's kernel, checked at build time the way tests/test_variance_denoise_resources_cpu.py checks the
denoisers' (hipcc cross-compiles gfx950 without a GPU): every `temporal_` kernel runs without scratch memory at an occupancy of 4 waves
per SIMD or more; temporal_push_kernel gathers its four taps from global memory and stages nothing, so its LDS is 0."""
import re

import pytest

import kernel_resource_usage

OTHERS = ("atrous", "vdn_", "variance_estimate", "aov_kernel", "render_kernel", "bin_")  # substrings other resource tests count kernels by


@pytest.fixture(scope="module")
def usage():
    return kernel_resource_usage.usage()


def test_temporal_kernels_have_no_scratch_and_no_lds(usage):
    ours = {n: v for n, v in usage.items() if "temporal_" in n}
    assert len(ours) == 1 and "temporal_push_kernel" in next(iter(ours)), sorted(ours)
    for name, v in ours.items():
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["Occupancy [waves/SIMD]"] >= 4, (name, v)
        assert v["LDS Size [bytes/block]"] == 0, (name, v)  # the straightforward gather: nothing is staged


def test_names_stay_clear_of_the_other_kernel_tables(usage):
    for name in usage:
        if "temporal_" in name:
            for other in OTHERS:
                assert other not in name, (name, other)
