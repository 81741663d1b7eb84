"""Resources of the denoiser's kernels, checked at build time the way tests/test_kernel_resources_cpu.py checks the render kernels (hipcc
cross-compiles gfx950 without a GPU): every atrous_kernel instantiation — (normal, depth) records read or not x albedo records read or
not x taps from global memory / from an LDS tile at step 1 / at step 2 — and the guide-packing prepass run without scratch memory, and the
LDS tiles are the sizes the kernel's layout says."""
import re

import pytest

import kernel_resource_usage
from kernel_resource_usage import flags as _flags


@pytest.fixture(scope="module")
def usage():
    return kernel_resource_usage.usage()


def test_flags_keep_the_numerics_contract():
    assert "-ffp-contract=off" in _flags() and "-fhip-fp32-correctly-rounded-divide-sqrt" in _flags() and "-fno-fast-math" in _flags()


def test_atrous_kernels_have_no_scratch(usage):
    kernels = {}
    for name, v in usage.items():
        m = re.search(r"\d+atrous_kernelILb([01])ELb([01])ELi([012])EE", name)
        if m:
            kernels[tuple(int(x) for x in m.groups())] = v
    assert sorted(kernels) == [(nd, al, step) for nd in (0, 1) for al in (0, 1) for step in (0, 1, 2)], sorted(usage)
    for (nd, al, step), v in kernels.items():
        assert v["ScratchSize [bytes/lane]"] == 0, ((nd, al, step), v)
        assert v["Occupancy [waves/SIMD]"] >= 4, ((nd, al, step), v)
        # the tile: 32 x 8 pixels with a halo of 2 x step, three colour planes of floats and a 16-byte record per guide pair read
        tile = (32 + 4 * step) * (8 + 4 * step)
        want = tile * (12 + 16 * nd + 16 * al) if step else 0
        assert want <= v["LDS Size [bytes/block]"] <= want + 64, ((nd, al, step), v, want)  # (+ the one-element stand-ins of unused arrays)
    pack = [v for k, v in usage.items() if "atrous_pack_kernel" in k]
    assert len(pack) == 1 and pack[0]["ScratchSize [bytes/lane]"] == 0, pack


def test_names_stay_clear_of_the_render_kernel_table(usage):
    """tests/test_kernel_resources_cpu.py decodes render_kernel*, bin_*_kernel and aov_kernel instantiations into the variant table: the
    denoiser's kernels must not match its pattern."""
    for name in usage:
        if "atrous" in name:
            assert not re.search(r"\d+(render_kernel_stream|render_kernel|bin_step_kernel|bin_finish_kernel|aov_kernel)I((?:L[ib]\d+E)+)E", name), name
