"""Resources of the display stage's kernels, checked at build time the way tests/test_temporal_resources_cpu.py checks the reprojection's
(hipcc cross-compiles gfx950 without a GPU): every `display_` kernel runs without scratch memory at an occupancy of 4 waves per SIMD or
more; the metering kernel's LDS is its histogram (257 words per workgroup), the others use none."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "path_tracer_amd" / "csrc"
OTHERS = ("bin_", "band_kernel", "temporal_", "atrous", "vdn_", "variance_estimate", "aov_kernel", "render_kernel")  # substrings other resource tests count kernels by


def _flags():
    mk = (CSRC / "Makefile").read_text()
    m = re.search(r"^FLAGS\s*=\s*(.*?)(?<!\\)\n", mk, re.S | re.M)
    flags = m.group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    return [f for f in flags if f not in ("-fPIC",) and not f.startswith("-W")]


@pytest.fixture(scope="module")
def usage():
    cmd = ["/opt/rocm/bin/hipcc", *_flags(), "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", "/dev/null",
           str(CSRC / "pt_render.hip")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key in ("VGPRs", "SGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


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
