"""The sign-resolved slab pass (pt_device.hpp: slab_chunk_pass, the LDS kernels' form) on the CPU:
 - tests/cpp/slab_forms_main.c states both forms of one entry's arithmetic and compares L, the candidate decision and the key bit for bit over
   10^8 random and ~350 000 enumerated cases;
 - the headline kernel's gfx950 assembly (cross-compiled, no GPU): the "slab pass" phase of tools/isa_budget.py stays at or below the committed
   budget, profiles/headline_slabpass_isa_budget_after.txt, which itself is below the parent commit's beside it (..._before.txt).  The
   ceilings are READ from those files."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

from test_kernel_resources_cpu import _flags  # the Makefile's FLAGS, parsed once

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "path_tracer_amd" / "csrc"
PASS = "slab pass (per 2 entries)"


def test_both_forms_give_the_same_keys(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    src = ROOT / "tests" / "cpp" / "slab_forms_main.c"
    exe = tmp_path / "slab_forms"
    base = ["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"]
    built = subprocess.run(base[:1] + ["-fopenmp"] + base[1:], capture_output=True, text=True)
    if built.returncode != 0:  # a gcc without OpenMP: the same program on one core
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-2000:]
    assert int(p.stdout.split("checked ")[1].split()[0]) >= 100_000_000, p.stdout


def _pass_row(text):
    """(total, VALU) of the slab pass phase in a tools/isa_budget.py table"""
    for line in text.splitlines():
        m = re.match(r"(.{50})\s*(\d+)\s+(\d+)\s", line)
        if m and m.group(1).strip() == PASS:
            return int(m.group(2)), int(m.group(3))
    raise AssertionError(f"no `{PASS}` row")


def test_committed_slab_pass_budget_is_below_the_parents():
    before = _pass_row((ROOT / "profiles" / "headline_slabpass_isa_budget_before.txt").read_text())
    after = _pass_row((ROOT / "profiles" / "headline_slabpass_isa_budget_after.txt").read_text())
    assert before == (118, 93), before  # the parent commit's figures
    assert after[0] < before[0] and after[1] < before[1], (after, before)


def test_slab_pass_within_the_committed_budget(tmp_path):
    out = tmp_path / "pt_render.s"
    cmd = ["/opt/rocm/bin/hipcc", *_flags(), "-gline-tables-only", "--cuda-device-only", "-S", "-o", str(out), str(CSRC / "pt_render.hip")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_budget.py"), "--asm", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = _pass_row(p.stdout)
    after = _pass_row((ROOT / "profiles" / "headline_slabpass_isa_budget_after.txt").read_text())
    print(f"slab pass: {got[0]} instructions, {got[1]} VALU (committed budget {after[0]}, {after[1]})")
    assert got[0] <= after[0] and got[1] <= after[1], (got, after)
    # the sign-resolved form reads the octant table from LDS and nothing through the scalar cache
    row = next(line for line in p.stdout.splitlines() if line.startswith(PASS))
    cols = [int(v) for v in row[50:].split()[:11]]  # total VALU SALU v_mov v_cndmask s_nop SMEM LDS ...
    assert cols[6] == 0 and cols[7] == 8, row
