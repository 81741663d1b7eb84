"""The run walk in front of the slab pool in the headline kernel's gfx950 assembly (cross-compiled, no GPU).  A scene that is ONE pool
reaches it from the pool plan in the kernel arguments — one scalar load per bounce — instead of a run header, an aux record and the table
addresses rebuilt from them, so the phase "run loop + slab_pool set-up" of tools/isa_budget.py is below the parent commit's in total and in
scalar instructions, and the kernel and its `v_mov_b32` are not above the parent's.  The figures are READ from the two committed tables,
profiles/headline_runwalk_isa_budget_{before,after}.txt: what this test measures against is what a reader sees there.
When it trips: `make -C path_tracer_amd/csrc asm && python tools/isa_budget.py` shows where the instructions went (docs/EXPERIMENTS.md,
"The run walk in front of the pool", has the phase's ISA as it should come out)."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

from test_kernel_resources_cpu import _flags  # the Makefile's FLAGS, parsed once

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "path_tracer_amd" / "csrc"
WALK, WHOLE = "run loop + slab_pool set-up", "whole kernel"
COLS = ("total", "VALU", "SALU", "v_mov")


def _rows(text):
    """{phase label: {total, VALU, SALU, v_mov}} of a tools/isa_budget.py table (columns: total VALU SALU v_mov ...)."""
    out = {}
    for line in text.splitlines():
        m = re.match(r"(.{50})\s*(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s", line)
        if m:
            out[m.group(1).strip()] = dict(zip(COLS, (int(m.group(k)) for k in (2, 3, 4, 5))))
    assert {WALK, WHOLE} <= set(out), sorted(out)
    return out


def _committed(which):
    return _rows((ROOT / "profiles" / f"headline_runwalk_isa_budget_{which}.txt").read_text())


@pytest.fixture(scope="module")
def budget(tmp_path_factory):
    out = tmp_path_factory.mktemp("runwalk_isa") / "pt_render.s"
    cmd = ["/opt/rocm/bin/hipcc", *_flags(), "-gline-tables-only", "--cuda-device-only", "-S", "-o", str(out), str(CSRC / "pt_render.hip")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_budget.py"), "--asm", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return _rows(p.stdout)


def test_committed_budget_is_below_the_parents():
    before, after = _committed("before"), _committed("after")
    assert (before[WHOLE]["total"], before[WHOLE]["v_mov"]) == (2611, 126), before[WHOLE]  # the parent commit's figures
    assert after[WALK]["total"] < before[WALK]["total"] and after[WALK]["SALU"] < before[WALK]["SALU"], (after[WALK], before[WALK])
    assert after[WHOLE]["total"] <= before[WHOLE]["total"] and after[WHOLE]["v_mov"] <= before[WHOLE]["v_mov"], (after[WHOLE], before[WHOLE])


def test_headline_kernel_and_run_walk_within_the_committed_budget(budget):
    after = _committed("after")
    for label in (WHOLE, WALK):
        print(f"{label}: {budget[label]} (committed budget {after[label]})")
    assert budget[WHOLE]["total"] <= after[WHOLE]["total"], (budget[WHOLE], after[WHOLE])
    assert budget[WHOLE]["v_mov"] <= after[WHOLE]["v_mov"], (budget[WHOLE], after[WHOLE])
    assert budget[WALK]["total"] <= after[WALK]["total"], (budget[WALK], after[WALK])
    assert budget[WALK]["SALU"] <= after[WALK]["SALU"], (budget[WALK], after[WALK])
