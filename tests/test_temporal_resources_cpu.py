"""Resources of the temporal reprojection's kernel, checked at build time the way tests/test_variance_denoise_resources_cpu.py checks the
denoisers' (hipcc cross-compiles gfx950 without a GPU): every `temporal_` kernel runs without scratch memory at an occupancy of 4 waves
per SIMD or more; temporal_push_kernel gathers its four taps from global memory and stages nothing, so its LDS is 0."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "path_tracer_amd" / "csrc"
OTHERS = ("atrous", "vdn_", "variance_estimate", "aov_kernel", "render_kernel", "bin_")  # substrings other resource tests count kernels by


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
