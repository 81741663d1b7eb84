"""Instruction ceilings of the headline kernel (cfg2: the Cornell-style scene's render_kernel), checked at build time on the gfx950
assembly hipcc cross-compiles without a GPU.  The kernel is bound by instruction issue, all kinds together, so its frame time follows
the instructions a wave-iteration executes; what these ceilings keep out are the register copies the compiler adds when a change to the
loop's control flow makes it merge the lane state or the traversal's (closest, hit) through a second register set (DESIGN.md §7,
profiles/headline_isa_budget_*.txt; tools/isa_budget.py shows where the instructions are)."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

from test_kernel_resources_cpu import _flags  # the Makefile's FLAGS, parsed once for both tests

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "path_tracer_amd" / "csrc"
HEADLINE = r"render_kernelILi0ELb1ELb1ELb0ELb1ELb0ELb0ELi0ELb0ELi65545E"  # the kernel tests/test_kernel_resources_cpu.py calls cfg2's

PARENT_TOTAL, PARENT_V_MOV = 2840, 286  # the commit before the bounce loop was reworked
# MAX_TOTAL is the committed budget's own total (profiles/headline_isa_budget_after.txt: 166 fewer than the parent), with no slack: a compiler
# release or an edit to an inline helper the kernel shares moves it.  When it trips, look at where the instructions went
# (`make -C path_tracer_amd/csrc asm && python tools/isa_budget.py`, against the committed budget); if the change is meant, re-derive the figure
# with `python tools/isa_budget.py --totals` (prints `total v_mov`) and commit the new budget beside it.
MAX_TOTAL = 2674
MAX_V_MOV = 226                         # 60 fewer: the copies that went are ~100; the rest is room for what the allocator legitimately needs


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "pt_render.s"
    cmd = ["/opt/rocm/bin/hipcc", *_flags(), "--cuda-device-only", "-S", "-o", str(out), str(CSRC / "pt_render.hip")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return out


def _count(asm_path):
    total = v_mov = 0
    inside = False
    found = []
    for line in open(asm_path):
        if not inside:
            m = re.match(r"(\S+):\s", line)
            if m and not m.group(1).startswith(".") and re.search(HEADLINE, m.group(1)):
                inside = True
                found.append(m.group(1))
            continue
        if line.startswith(".Lfunc_end"):
            inside = False
            continue
        m = re.match(r"\t([a-z][a-z_0-9]*)", line)
        if m:
            total += 1
            v_mov += m.group(1).startswith("v_mov_b32")
    assert len(found) == 1, found
    return total, v_mov


def test_headline_kernel_instruction_ceilings(asm):
    total, v_mov = _count(asm)
    print(f"headline kernel: {total} instructions (parent {PARENT_TOTAL}, ceiling {MAX_TOTAL}), {v_mov} v_mov_b32 (parent {PARENT_V_MOV}, ceiling {MAX_V_MOV})")
    assert v_mov <= MAX_V_MOV, (v_mov, MAX_V_MOV)
    assert total <= MAX_TOTAL, (total, MAX_TOTAL)


def test_isa_budget_tool_counts_the_same(asm):
    """tools/isa_budget.py cuts the same kernel into phases: its totals are this test's."""
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_budget.py"), "--asm", str(asm), "--totals"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert tuple(int(x) for x in p.stdout.split()) == _count(asm)
