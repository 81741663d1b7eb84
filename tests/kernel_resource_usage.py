"""The compiler's resource-usage remarks for every kernel of path_tracer_amd/csrc/pt_render.hip, for the *_resources_cpu.py tests: one
cross-compile for gfx950 (no GPU needed) with the Makefile's FLAGS as they stand, run once per process and shared by all of them."""
import functools
import re
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "path_tracer_amd" / "csrc"
KEYS = ("VGPRs", "SGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def flags():
    mk = (CSRC / "Makefile").read_text()
    m = re.search(r"^FLAGS\s*=\s*(.*?)(?<!\\)\n", mk, re.S | re.M)
    flags = m.group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    return [f for f in flags if f not in ("-fPIC",) and not f.startswith("-W")]


@functools.lru_cache(maxsize=None)
def usage():
    """{mangled kernel name: {key of KEYS: value}}"""
    cmd = ["/opt/rocm/bin/hipcc", *flags(), "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", "/dev/null",
           str(CSRC / "pt_render.hip")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key in KEYS:
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out
