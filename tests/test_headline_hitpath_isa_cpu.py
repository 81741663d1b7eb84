"""From the hit to the next sample in the headline kernel's gfx950 assembly (cross-compiled, no GPU): a hit shaded from its one shade
record (pt_device.hpp: shade_record) instead of two records of the hittable and two of the material, the cold lane state in two 16-byte
LDS records per thread (pt_render.hip: Cold<true>) and the trip gate without the sphere-holder test.  Every figure is READ from the two
committed tables of tools/isa_budget.py, profiles/headline_hitpath_isa_budget_{before,after}.txt — the parent commit's and this tree's —
and the cross-compiled tree is held to the committed after-table.
When it trips: `make -C path_tracer_amd/csrc asm && python tools/isa_budget.py` shows where the instructions went (docs/EXPERIMENTS.md,
"One shade record per hit, cold lane state in two records", has the ISA of the shade head as it should come out)."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

from test_kernel_resources_cpu import _flags  # the Makefile's FLAGS, parsed once

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "path_tracer_amd" / "csrc"
COLS = ("total", "VALU", "SALU", "v_mov", "v_cndmask", "s_nop", "SMEM", "LDS", "VMEM", "branch", "wait")
WHOLE, HEAD, QUEUE, SCATTER, TRIP = ("whole kernel", "shade head + resolve_hit", "pixel queue, cold state, store", "scatter (lambertian, light)",
                                     "trip gate, record fetch, pool exit")


def _rows(text):
    """{phase label: {column: count}} of a tools/isa_budget.py table"""
    out = {}
    for line in text.splitlines():
        m = re.match(r"(.{50})" + r"\s*(\d+)" * len(COLS) + r"(\s|$)", line)
        if m:
            out[m.group(1).strip()] = dict(zip(COLS, (int(v) for v in m.groups()[1:len(COLS) + 1])))
    assert {WHOLE, HEAD, QUEUE, SCATTER, TRIP} <= set(out), sorted(out)
    return out


def _sums(rows):
    """the figures this change is held to"""
    return {"total": rows[WHOLE]["total"], "v_mov": rows[WHOLE]["v_mov"], "LDS": rows[WHOLE]["LDS"], "wait": rows[WHOLE]["wait"],
            "shade head total": rows[HEAD]["total"], "shade head LDS": rows[HEAD]["LDS"], "shade head + scatter LDS": rows[HEAD]["LDS"] + rows[SCATTER]["LDS"],
            "cold state LDS": rows[QUEUE]["LDS"], "trip total": rows[TRIP]["total"]}


def _committed(which):
    return _rows((ROOT / "profiles" / f"headline_hitpath_isa_budget_{which}.txt").read_text())


@pytest.fixture(scope="module")
def budget(tmp_path_factory):
    out = tmp_path_factory.mktemp("hitpath_isa") / "pt_render.s"
    cmd = ["/opt/rocm/bin/hipcc", *_flags(), "-gline-tables-only", "--cuda-device-only", "-S", "-o", str(out), str(CSRC / "pt_render.hip")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_budget.py"), "--asm", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return _rows(p.stdout)


def test_before_table_is_the_parents():
    before = _committed("before")
    flags_after = _rows((ROOT / "profiles" / "headline_flags_isa_budget_after.txt").read_text())
    assert before[WHOLE] == flags_after[WHOLE], (before[WHOLE], flags_after[WHOLE])
    assert (before[WHOLE]["total"], before[WHOLE]["v_mov"]) == (2581, 124), before[WHOLE]  # the parent commit's figures


def test_committed_budget_is_below_the_parents():
    before, after = _sums(_committed("before")), _sums(_committed("after"))
    print(f"before {before}\nafter  {after}")
    assert after["shade head LDS"] < before["shade head LDS"] and after["shade head total"] < before["shade head total"], (after, before)
    assert after["shade head + scatter LDS"] < before["shade head + scatter LDS"], (after, before)  # (the material's two words were read in `shade`)
    assert after["cold state LDS"] < before["cold state LDS"], (after, before)
    assert after["trip total"] < before["trip total"], (after, before)
    assert after["total"] <= before["total"] and after["v_mov"] <= before["v_mov"], (after, before)
    assert after["LDS"] < before["LDS"] and after["wait"] <= before["wait"], (after, before)


def test_headline_kernel_within_the_committed_budget(budget):
    now, after = _sums(budget), _sums(_committed("after"))
    print(f"cross-compiled {now}\ncommitted      {after}")
    for what in after:
        assert now[what] <= after[what], (what, now, after)
