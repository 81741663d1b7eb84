"""The glue of a regular wave-iteration in the headline kernel's gfx950 assembly (cross-compiled, no GPU): the vote on "every live ray
regular" as scalar arithmetic on wave masks, the one-chunk pool without the chunk loop's control, the frame's size as float launch
constants and the exact trip's close inside the last side's statement.  Every
figure is READ from the two committed tables of tools/isa_budget.py, profiles/headline_flags_isa_budget_{before,after}.txt — the parent
commit's and this tree's — and the cross-compiled tree is held to the committed after-table in each of the sums.
When it trips: `make -C path_tracer_amd/csrc asm && python tools/isa_budget.py` shows where the instructions went (docs/EXPERIMENTS.md,
"Votes, the one-chunk pool and no-ops of the headline loop", has the ISA of the votes and joins as it should come out)."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

from test_kernel_resources_cpu import _flags  # the Makefile's FLAGS, parsed once

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "path_tracer_amd" / "csrc"
COLS = ("total", "VALU", "SALU", "v_mov", "v_cndmask", "s_nop")
WHOLE = "whole kernel"
HEAD, CAMERA, CONTEXT, WALK = ("loop head, back-edge, priority poll", "camera ray (lane_regenerate)", "ray context (make_ctx, wave_all_regular)",
                               "run loop + slab_pool set-up")
SCATTER, SKY, TRIP = "scatter (lambertian, light)", "sky", "trip gate, record fetch, pool exit"


def _rows(text):
    """{phase label: {total, VALU, SALU, v_mov, v_cndmask, s_nop}} of a tools/isa_budget.py table"""
    out = {}
    for line in text.splitlines():
        m = re.match(r"(.{50})" + r"\s*(\d+)" * len(COLS) + r"\s", line)
        if m:
            out[m.group(1).strip()] = dict(zip(COLS, (int(v) for v in m.groups()[1:])))
    assert {WHOLE, HEAD, CAMERA, CONTEXT, WALK, SCATTER, SKY, TRIP} <= set(out), sorted(out)
    return out


def _sums(rows):
    """the figures this change is held to"""
    return {"total": rows[WHOLE]["total"], "v_mov": rows[WHOLE]["v_mov"],
            "glue SALU": sum(rows[p]["SALU"] for p in (HEAD, CAMERA, CONTEXT, WALK)),
            "camera + context VALU": sum(rows[p]["VALU"] for p in (CAMERA, CONTEXT)),
            "hot s_nop": sum(rows[p]["s_nop"] for p in (SCATTER, SKY, TRIP))}


def _committed(which):
    return _rows((ROOT / "profiles" / f"headline_flags_isa_budget_{which}.txt").read_text())


@pytest.fixture(scope="module")
def budget(tmp_path_factory):
    out = tmp_path_factory.mktemp("flags_isa") / "pt_render.s"
    cmd = ["/opt/rocm/bin/hipcc", *_flags(), "-gline-tables-only", "--cuda-device-only", "-S", "-o", str(out), str(CSRC / "pt_render.hip")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_budget.py"), "--asm", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return _rows(p.stdout)


def test_before_table_is_the_parents():
    before = _committed("before")
    runwalk_after = _rows((ROOT / "profiles" / "headline_runwalk_isa_budget_after.txt").read_text())
    assert before[WHOLE] == runwalk_after[WHOLE], (before[WHOLE], runwalk_after[WHOLE])
    assert (before[WHOLE]["total"], before[WHOLE]["v_mov"]) == (2595, 124), before[WHOLE]  # the parent commit's figures


def test_committed_budget_is_below_the_parents():
    before, after = _sums(_committed("before")), _sums(_committed("after"))
    print(f"before {before}\nafter  {after}")
    assert after["total"] < before["total"], (after, before)
    assert after["v_mov"] <= before["v_mov"], (after, before)
    assert after["glue SALU"] < before["glue SALU"], (after, before)
    assert after["camera + context VALU"] < before["camera + context VALU"], (after, before)
    assert after["hot s_nop"] < before["hot s_nop"], (after, before)


def test_headline_kernel_within_the_committed_budget(budget):
    now, after = _sums(budget), _sums(_committed("after"))
    print(f"cross-compiled {now}\ncommitted      {after}")
    for what in after:
        assert now[what] <= after[what], (what, now, after)
