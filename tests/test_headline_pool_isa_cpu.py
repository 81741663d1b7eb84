"""The slab pool's candidate loop in the headline kernel's gfx950 assembly (cross-compiled, no GPU): the gates are one comparison each and
the candidate queue is written in place, so the kernel and the two phases of tools/isa_budget.py that hold the loop stay at or below
the committed budget, profiles/headline_pool_isa_budget_after.txt — which itself is below the parent commit's budget beside it
(headline_pool_isa_budget_before.txt).  The ceilings are READ from those files: what this test measures against is what a reader sees there.
When it trips: `make -C path_tracer_amd/csrc asm && python tools/isa_budget.py` shows where the instructions went (docs/EXPERIMENTS.md,
"The pool scan's gates", has the ISA of each gate as it should come out)."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

from test_kernel_resources_cpu import _flags  # the Makefile's FLAGS, parsed once

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "path_tracer_amd" / "csrc"
PROOF, TRIP, WHOLE = "leaving-ray proof (inside gate)", "trip gate, record fetch, pool exit", "whole kernel"


def _rows(text):
    """{phase label: (total, v_mov)} of a tools/isa_budget.py table (columns: total VALU SALU v_mov ...)."""
    out = {}
    for line in text.splitlines():
        m = re.match(r"(.{50})\s*(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s", line)
        if m:
            out[m.group(1).strip()] = (int(m.group(2)), int(m.group(5)))
    assert {PROOF, TRIP, WHOLE} <= set(out), sorted(out)
    return out


@pytest.fixture(scope="module")
def budget(tmp_path_factory):
    out = tmp_path_factory.mktemp("pool_isa") / "pt_render.s"
    cmd = ["/opt/rocm/bin/hipcc", *_flags(), "-gline-tables-only", "--cuda-device-only", "-S", "-o", str(out), str(CSRC / "pt_render.hip")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_budget.py"), "--asm", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return _rows(p.stdout)


def test_committed_budget_is_below_the_parents():
    before = _rows((ROOT / "profiles" / "headline_pool_isa_budget_before.txt").read_text())
    after = _rows((ROOT / "profiles" / "headline_pool_isa_budget_after.txt").read_text())
    assert before[WHOLE] == (2674, 162) and before[PROOF][0] == 144 and before[TRIP][0] == 92, before  # the parent commit's figures
    assert after[WHOLE][0] < before[WHOLE][0] and after[WHOLE][1] < before[WHOLE][1], (after[WHOLE], before[WHOLE])
    assert after[PROOF][0] < before[PROOF][0] and after[TRIP][0] < before[TRIP][0], (after[PROOF], after[TRIP])


def test_headline_kernel_and_pool_phases_within_the_committed_budget(budget):
    after = _rows((ROOT / "profiles" / "headline_pool_isa_budget_after.txt").read_text())
    for label in (WHOLE, PROOF, TRIP):
        print(f"{label}: {budget[label][0]} instructions, {budget[label][1]} v_mov_b32 (committed budget {after[label][0]}, {after[label][1]})")
    assert budget[WHOLE][0] <= after[WHOLE][0], (budget[WHOLE], after[WHOLE])
    assert budget[WHOLE][1] <= after[WHOLE][1], (budget[WHOLE], after[WHOLE])
    assert budget[PROOF][0] <= after[PROOF][0], (budget[PROOF], after[PROOF])
    assert budget[TRIP][0] <= after[TRIP][0], (budget[TRIP], after[TRIP])
