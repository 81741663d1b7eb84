"""Resources of the encode stage's kernels (path_tracer_amd/csrc/pt_encode.hpp), checked at build time the way
tests/test_metrics_resources_cpu.py checks the image error's (hipcc cross-compiles gfx950 without a GPU): every `encode_` kernel runs
without scratch memory at the full occupancy of 8 waves per SIMD; their number is the instantiations the launcher can reach — {pt_encode,
and pt_display_encode under each of the three tones} x {reference, sRGB, sRGB + dither} x {four values per lane, one}: 24; the LDS of a
kernel is the one table its mode searches, the start bytes and the dither's thresholds — 259 + 64 floats and 416 bytes —, which the
reference transfer never touches."""
import re

import pytest

import kernel_resource_usage

# substrings other resource tests count kernels by
OTHERS = ("bin_", "band_kernel", "temporal_", "atrous", "vdn_", "variance_estimate", "aov_kernel", "render_kernel", "display_", "firefly_", "svar_",
          "imgerr_")
LDS_BYTES = (259 + 64) * 4 + 416
NAME = re.compile(r"encode_kernelILi(n?\d)ELi(\d)ELb([01])E")


@pytest.fixture(scope="module")
def usage():
    return kernel_resource_usage.usage()


def test_encode_kernels_have_no_scratch_and_are_the_instantiations_the_launcher_reaches(usage):
    ours = {n: v for n, v in usage.items() if "encode_" in n}
    got = sorted(NAME.search(n).groups() for n in ours)
    want = sorted((tone, mode, vec) for tone in ("n1", "0", "1", "2") for mode in "012" for vec in "01")  # n1: ENCODE_PLAIN = -1
    assert got == want and len(ours) == 24, sorted(ours)
    for name, v in ours.items():
        print(name, v)
        mode = NAME.search(name).group(2)
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["Occupancy [waves/SIMD]"] >= 8, (name, v)
        assert v["VGPRs"] <= 64, (name, v)
        assert v["LDS Size [bytes/block]"] == (0 if mode == "0" else LDS_BYTES), (name, v)


def test_names_stay_clear_of_the_other_kernel_tables(usage):
    ours = [n for n in usage if "encode_" in n]
    assert ours
    for name in ours:
        for other in OTHERS:
            assert other not in name, (name, other)
    for other in OTHERS:  # and no other table's kernels carry this one's name
        assert not [n for n in usage if other in n and "encode_" in n]
