"""Resources of the variance-guided denoiser's kernels, checked at build time the way tests/test_denoise_resources_cpu.py checks the
a-trous kernels (hipcc cross-compiles gfx950 without a GPU): every vdn_kernel instantiation — (normal, depth) records read or not x albedo
records read or not x reads from global memory / from an LDS tile at step 1 / at step 2 — the packing prepass and the variance estimate
run without scratch memory at an occupancy of 4 waves per SIMD or more, and the LDS tiles are the sizes the kernel's layout says."""
import re

import pytest

import kernel_resource_usage


@pytest.fixture(scope="module")
def usage():
    return kernel_resource_usage.usage()


def test_vdn_kernels_have_no_scratch(usage):
    kernels = {}
    for name, v in usage.items():
        m = re.search(r"\d+vdn_kernelILb([01])ELb([01])ELi([012])EE", name)
        if m:
            kernels[tuple(int(x) for x in m.groups())] = v
    assert sorted(kernels) == [(nd, al, step) for nd in (0, 1) for al in (0, 1) for step in (0, 1, 2)], sorted(usage)
    for (nd, al, step), v in kernels.items():
        print((nd, al, step), v)
        assert v["ScratchSize [bytes/lane]"] == 0, ((nd, al, step), v)
        assert v["Occupancy [waves/SIMD]"] >= 4, ((nd, al, step), v)
        # the tile: 32 x 8 pixels with a halo of 2 x step; per pixel a 16-byte record (colour, variance.r), an 8-byte record
        # (variance.g, variance.b) and a 16-byte record per guide pair read
        tile = (32 + 4 * step) * (8 + 4 * step)
        want = tile * (16 + 8 + 16 * nd + 16 * al) if step else 0
        assert want <= v["LDS Size [bytes/block]"] <= want + 64, ((nd, al, step), v, want)  # (+ the one-element stand-ins of unused arrays)
    for small in ("vdn_pack_kernel", "variance_estimate_kernel"):
        found = [v for k, v in usage.items() if small in k]
        print(small, found)
        assert len(found) == 1 and found[0]["ScratchSize [bytes/lane]"] == 0 and found[0]["Occupancy [waves/SIMD]"] >= 4, (small, found)


def test_names_stay_clear_of_the_other_kernel_tables(usage):
    """tests/test_kernel_resources_cpu.py decodes render_kernel*, bin_*_kernel and aov_kernel instantiations, and
    tests/test_denoise_resources_cpu.py counts the names that carry `atrous`: the new kernels match neither."""
    ours = [n for n in usage if "vdn_" in n or "variance_estimate" in n]
    assert len(ours) == 14, ours
    for name in ours:
        assert "atrous" not in name, name
        assert not re.search(r"\d+(render_kernel_stream|render_kernel|bin_step_kernel|bin_finish_kernel|aov_kernel)I((?:L[ib]\d+E)+)E", name), name
