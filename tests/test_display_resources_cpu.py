"""Resources of the display stage's kernels, checked at build time the way tests/test_temporal_resources_cpu.py checks the reprojection's
(hipcc cross-compiles gfx950 without a GPU): every `display_` kernel runs without scratch memory at an occupancy of 4 waves per SIMD or
more; the metering kernel's LDS is its histogram (257 words per workgroup), the others use none."""
import re

import pytest

import kernel_resource_usage

OTHERS = ("bin_", "band_kernel", "temporal_", "atrous", "vdn_", "variance_estimate", "aov_kernel", "render_kernel")  # substrings other resource tests count kernels by


@pytest.fixture(scope="module")
def usage():
    return kernel_resource_usage.usage()


def test_display_kernels_have_no_scratch(usage):
    ours = {n: v for n, v in usage.items() if "display_" in n}
    kinds = sorted(re.search(r"display_[a-z]+_kernel", n).group(0) for n in ours)
    assert kinds == ["display_apply_kernel"] * 6 + ["display_meter_kernel"] * 2 + ["display_set_kernel", "display_solve_kernel"], sorted(ours)
    for name, v in ours.items():
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["Occupancy [waves/SIMD]"] >= 4, (name, v)
        want_lds = 257 * 4 if "display_meter_kernel" in name else 0
        assert v["LDS Size [bytes/block]"] == want_lds, (name, v)


def test_names_stay_clear_of_the_other_kernel_tables(usage):
    ours = [n for n in usage if "display_" in n]
    assert ours
    for name in ours:
        for other in OTHERS:
            assert other not in name, (name, other)
