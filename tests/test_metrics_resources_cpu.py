"""Resources of the image error's kernels (path_tracer_amd/csrc/pt_metrics.hpp), checked at build time the way
tests/test_spatial_variance_resources_cpu.py checks the spatial variance estimate's (hipcc cross-compiles gfx950 without a GPU): the three
kernels run without scratch memory; the accumulating kernel's LDS is its eight copies of the nine accumulators — 8 x 9 x 68 words of 8
bytes = 39168 bytes — and the workgroup's three maxima and two counts, 39192 bytes in all, of which four workgroups fit a CU's 160 KiB:
the 4 waves per SIMD the compiler reports, and PT_IMGERR_MAX_BLOCKS = 4 x 256 CUs; the PT_IMAGE_ERROR_NO_LDS one uses none; the
finishing kernel holds one copy, 4896 bytes; no kernel needs more than 64 VGPRs.  The kernels' ISA — the header compiled alone, which
takes seconds — keeps binary32 and binary64 subnormals (float_denorm_mode_32 = float_denorm_mode_16_64 = 3: the header's "a subnormal
difference is kept"), adds its chunks with 27 `ds_add_u64` in the LDS kernel and with 64-bit global vector atomics otherwise, and has no
flat atomic and no compare-and-swap loop."""
import re
import subprocess

import pytest

import kernel_resource_usage
from path_tracer_amd import abi

# substrings other resource tests count kernels by
OTHERS = ("bin_", "band_kernel", "temporal_", "atrous", "vdn_", "variance_estimate", "aov_kernel", "render_kernel", "display_", "firefly_", "svar_")
ACC_BYTES = abi.PT_IMAGE_ERROR_SUMS * abi.PT_IMAGE_ERROR_WORDS * 8
COPIES = 8


@pytest.fixture(scope="module")
def usage():
    return kernel_resource_usage.usage()


def test_imgerr_kernels_have_no_scratch_and_the_lds_of_their_accumulators(usage):
    ours = {n: v for n, v in usage.items() if "imgerr_" in n}
    assert sorted(re.search(r"imgerr_[a-z]+_kernel", n).group(0) for n in ours) == ["imgerr_accumulate_kernel"] * 2 + ["imgerr_finish_kernel"], sorted(ours)
    staged = {n: re.search(r"imgerr_accumulate_kernelILb([01])E", n).group(1) == "1" for n in ours if "accumulate" in n}
    assert sorted(staged.values()) == [False, True]
    assert ACC_BYTES == 4896
    for name, v in ours.items():
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["VGPRs"] <= 64, (name, v)
        if "finish" in name:
            assert v["LDS Size [bytes/block]"] == ACC_BYTES, (name, v)
        elif staged[name]:
            assert v["LDS Size [bytes/block]"] == COPIES * ACC_BYTES + (3 + 2) * 4 + 4, (name, v)  # (the compiler pads the 12-byte maxima to 16)
            assert v["Occupancy [waves/SIMD]"] >= 4 and 4 * v["LDS Size [bytes/block]"] <= 160 * 1024, (name, v)
        else:
            assert v["LDS Size [bytes/block]"] == 0 and v["Occupancy [waves/SIMD]"] >= 8, (name, v)


def test_names_stay_clear_of_the_other_kernel_tables(usage):
    ours = [n for n in usage if "imgerr_" in n]
    assert len(ours) == 3
    for name in ours:
        for other in OTHERS:
            assert other not in name, (name, other)


WRAPPER = """
#include <hip/hip_runtime.h>
#include <cstddef>
#include <algorithm>
#include "{root}/include/pt_metrics.h"
namespace {{
#include "{root}/path_tracer_amd/csrc/pt_metrics.hpp"
}}
void use(ImgErrArgs a, PtImageErrorResult* r) {{
  hipLaunchKernelGGL(imgerr_accumulate_kernel<true>, dim3(1), dim3(256), 0, 0, a);
  hipLaunchKernelGGL(imgerr_accumulate_kernel<false>, dim3(1), dim3(256), 0, 0, a);
  hipLaunchKernelGGL(imgerr_finish_kernel, dim3(1), dim3(64), 0, 0, a.scratch, r);
}}
"""


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    """{kernel name: its gfx950 assembly, from the label to .end_amdhsa_kernel}: pt_metrics.hpp compiled alone with the Makefile's FLAGS."""
    d = tmp_path_factory.mktemp("imgerr_isa")
    src = d / "imgerr.hip"
    src.write_text(WRAPPER.format(root=kernel_resource_usage.CSRC.parent.parent))
    p = subprocess.run(["/opt/rocm/bin/hipcc", *kernel_resource_usage.flags(), "--cuda-device-only", "-S", "-o", str(d / "imgerr.s"), str(src)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    text = (d / "imgerr.s").read_text()
    out = {}
    for m in re.finditer(r"^(_Z\w*imgerr_\w+):.*?\.end_amdhsa_kernel", text, re.S | re.M):
        out[m.group(1)] = m.group(0)
    return out


def test_the_isa_keeps_subnormals_and_adds_with_vector_atomics(isa):
    assert len(isa) == 3, sorted(isa)
    for name, text in isa.items():
        assert re.search(r"\.amdhsa_float_denorm_mode_32 3\b", text) and re.search(r"\.amdhsa_float_denorm_mode_16_64 3\b", text), name
        assert "flat_atomic" not in text and "cmpswap" not in text, name
        if "finish" in name:
            assert "atomic" not in text, name
        elif "ILb1E" in name:
            assert len(re.findall(r"\bds_add_u64\b", text)) == 27, name          # nine terms x three chunks
            assert len(re.findall(r"\bglobal_atomic_add_x2\b", text)) == 2 and len(re.findall(r"\bglobal_atomic_umax_x2\b", text)) == 1, name  # the flush
        else:
            assert "ds_add" not in text, name
            assert len(re.findall(r"\bglobal_atomic_add_x2\b", text)) == 27 + 2, name  # the chunks and the two counts
            assert len(re.findall(r"\bglobal_atomic_umax_x2\b", text)) == 3, name
