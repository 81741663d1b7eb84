#!/usr/bin/env python3
"""Instruction budget of the headline kernel's bounce loop, phase by phase (CPU only: reads gfx950 assembly).

    make -C path_tracer_amd/csrc asm && python tools/isa_budget.py            # path_tracer_amd/csrc/build/*.s
    python tools/isa_budget.py --asm some.s [--src DIR] [--kernel REGEX] [--totals]

The assembly must carry line tables (`make asm` compiles with -gline-tables-only; they do not change the code).  Every
instruction of the kernel is attributed to the source function its `.loc` names — inlined code keeps the innermost function's
line, and the comment behind it the call sites it was inlined through — and functions are grouped into the phases of one loop iteration.
A helper that several phases share (vector math, div_exact, the generator, wave builtins of the HIP headers) counts towards the phase
it was inlined into; instructions without a location of their own (the register allocator's copies at a block's edge) towards the
phase of the instruction stream they sit in — except the kernel's set-up ahead of the loop, behind render_kernel's own statements there (the
staging, the depth check): the loop's hoisted constants and lane_reset's initial values, which count towards lane_reset's phase whether or
not one of lane_reset's own instructions happens to stand in front of them.  Counts are STATIC: what the loop's text
holds, not what a wave executes.  Beside each phase: what the reference's arithmetic needs there.
"""
import argparse
import collections
import glob
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "path_tracer_amd" / "csrc"
HEADLINE = r"render_kernelILi0ELb1ELb1ELb0ELb1ELb0ELb0ELi0ELb0ELi65545E"  # cfg2: UV_NONE, LDS, MLDS, !COOP, CL, GRID = 0, lambertian + light, rect / box only

# phase -> (functions, algorithmic operations of SURVEY §8d for that phase)
PHASES = [
    ("loop head, back-edge, priority poll", ["render_kernel"], "-"),
    ("pixel queue, cold state, store", ["lane_acquire", "lane_store", "lane_reset", "store_rgb", "fast_seed", "begin", "resume", "add_sample", "count_ray",
                                         "get_acc", "get_s", "get_pix", "get_x", "get_y", "get_xy", "get_iters", "init", "a_word", "b_word"], "12 B per pixel; mean: 3 div per pixel"),
    ("camera ray (lane_regenerate)", ["lane_regenerate", "lane_prepare", "camera_ray"], "91 per sample (5 draws x 8)"),
    ("ray context (make_ctx, wave_all_regular)", ["make_ctx", "wave_all_regular"], "0 (the reference divides per side; 3 reciprocals here)"),
    ("run loop + slab_pool set-up", ["hit_world_range", "hit_world", "hit_begin", "slab_pool"], "0 (list walk)"),
    ("run scans (irregular rays, runs without a pool)", ["hit_records", "hit_records_rectbox"], "rect 4 / 12 / 33; box = 6 x rect"),
    ("slab pass (per 2 entries)", ["slab_chunk_pass:pass"], "0 (culling; replaces 43 rect tests x 4..33 per ray)"),
    ("leaving-ray proof (inside gate)", ["slab_chunk_pass:proof"], "0 (culling)"),
    ("trip gate, record fetch, pool exit", ["slab_chunk_pass:trip"], "0"),
    ("exact sides (6 x rect_side_cmpx)", ["rect_side_cmpx", "box_cmpx"], "6 x (4 / 12 / 33) per candidate box"),
    ("shade head + resolve_hit", ["lane_shade", "resolve_hit", "shade_record", "set_face_normal"], "hit point 6, face normal 6 + 3"),
    ("scatter (lambertian, light)", ["shade", "shade_with", "texture_value", "rng_unit_vec"], "lambertian 46 (2 draws); light 0"),
    ("sky", ["sky_color", "sky_unit_y"], "24"),
]
COLS = ["total", "VALU", "SALU", "v_mov", "v_cndmask", "s_nop", "SMEM", "LDS", "VMEM", "branch", "wait"]


def function_ranges(src):
    """{file name: [(first line, last line, phase index)]} for the functions PHASES names; slab_chunk_pass in three parts."""
    where = {f: i for i, (_, fs, _) in enumerate(PHASES) for f in fs}
    names = {f.split(":")[0] for f in where}
    out = collections.defaultdict(list)
    for path in [Path(src) / "pt_render.hip", Path(src) / "pt_device.hpp"]:
        lines = path.read_text().splitlines()
        for i, line in enumerate(lines):
            m = re.match(r"\s*(?:__host__ )?(?:__device__|void)\s[^;=]*?\b(\w+)\s*\([^;]*$", line)
            if not m or m.group(1) not in names or line.lstrip().startswith("//"):
                continue
            name, depth, j, opened = m.group(1), 0, i, False
            while j < len(lines):  # the definition ends where its braces balance (comments hold none unbalanced here)
                code = lines[j].split("//")[0]
                depth += code.count("{") - code.count("}")
                opened = opened or "{" in code
                if opened and depth <= 0:
                    break
                j += 1
            first, last = i + 1, j + 1
            if name == "slab_chunk_pass":
                # the candidate loop starts where `had3` is taken; the trip's part at the gate's comparison (`vote`; `active` in older trees)
                a = next(k for k in range(i, j) if re.search(r"\bhad3 =", lines[k])) + 1
                b = next(k for k in range(a, j) if re.search(r"\((vote|active)\) :|const bool active", lines[k])) + 1
                out[path.name] += [(first, a - 1, where["slab_chunk_pass:pass"]), (a, b - 1, where["slab_chunk_pass:proof"]), (b, last, where["slab_chunk_pass:trip"])]
            else:
                out[path.name].append((first, last, where[name]))
    return out


def setup_lines(src):
    """(first, last) line of render_kernel's statements ahead of its loop: the kernel's set-up"""
    lines = (Path(src) / "pt_render.hip").read_text().splitlines()
    first = next(i for i, line in enumerate(lines) if re.match(r"void render_kernel\(", line)) + 1
    last = next(i for i in range(first, len(lines)) if re.match(r"\s*for \(;;\) \{", lines[i]))
    return first, last


def kind_of(op):
    if op == "s_nop":
        return "s_nop"
    if op.startswith(("s_waitcnt", "s_wait")):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_barrier", "s_setprio", "s_sleep", "s_sethalt")):
        return "branch"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "SMEM"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    return "VALU" if op.startswith("v_") else "other"


def budget(asm_path, kernel_re, src):
    ranges = function_ranges(src)
    scans = next(i for i, (_, fs, _) in enumerate(PHASES) if "hit_records" in fs)
    reset = next(i for i, (_, fs, _) in enumerate(PHASES) if "lane_reset" in fs)
    setup_first, setup_last = setup_lines(src)
    files, rows = {}, [collections.Counter() for _ in PHASES]
    inside, phase, name, in_setup = False, 0, None, False
    for line in open(asm_path):
        m = re.match(r"\s*\.file\s+(\d+)\s+(?:\"[^\"]*\"\s+)?\"([^\"]*)\"", line)
        if m:
            files[int(m.group(1))] = Path(m.group(2)).name
        if not inside:
            m = re.match(r"(\S+):\s", line)
            if m and re.search(kernel_re, m.group(1)) and not m.group(1).startswith("."):
                inside, name, phase = True, m.group(1), 0
            continue
        if line.startswith(".Lfunc_end"):
            break
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            # the location, then (in the comment the compiler leaves) the chain of call sites it was inlined through, innermost first:
            # the first of them that lies in a function PHASES names decides; none (a helper reached from a line 0, say): the phase stays
            chain = [(files.get(int(m.group(1)), ""), int(m.group(2)))]
            chain += [(Path(f).name, int(ln)) for f, ln in re.findall(r"@\[ (\S+?):(\d+):\d+", line)]
            if chain[0][1] == 0 and in_setup:  # no location, behind the kernel's own set-up statements: lane_reset's (see above)
                phase = reset
                continue
            in_setup = len(chain) == 1 and chain[0][0].endswith(".hip") and setup_first <= chain[0][1] <= setup_last
            hits = []
            for fname, ln in chain:
                hits += [ph for first, last, ph in ranges.get("pt_render.hip" if fname.endswith(".hip") else fname, []) if first <= ln <= last][:1]
            if hits:  # (a run scan contains the same side tests as a pool's exact trip: the scan it was inlined into decides)
                phase = scans if scans in hits else hits[0]
            continue
        m = re.match(r"\t([a-z][a-z_0-9]*)", line)
        if not m:
            continue
        op, row = m.group(1), rows[phase]
        row["total"] += 1
        row[kind_of(op)] += 1
        if op.startswith("v_mov_b32"):
            row["v_mov"] += 1
        if op.startswith("v_cndmask"):
            row["v_cndmask"] += 1
    if name is None:
        sys.exit(f"no kernel matching {kernel_re} in {asm_path}")
    return name, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="gfx950 assembly with line tables (default: the .s of `make asm`)")
    ap.add_argument("--kernel", default=HEADLINE, help="regex on the kernel's mangled name (default: the cfg2 kernel)")
    ap.add_argument("--src", default=str(CSRC), help="the directory of the sources the assembly was compiled from (default: this tree's csrc)")
    ap.add_argument("--totals", action="store_true", help="print only `total v_mov` (what tests/test_headline_isa_cpu.py bounds)")
    args = ap.parse_args()
    asm = args.asm or next(iter(sorted(glob.glob(str(CSRC / "build" / "*gfx950*.s")))), None)
    if not asm:
        sys.exit("no assembly: run `make -C path_tracer_amd/csrc asm` first, or pass --asm")
    name, rows = budget(asm, args.kernel, args.src)
    total = collections.Counter()
    for r in rows:
        total.update(r)
    if args.totals:
        print(total["total"], total["v_mov"])
        return
    print(f"kernel {name}\nstatic instructions per phase of the loop (v_mov, v_cndmask and s_nop are also counted in VALU / their kind)\n")
    head = f"{'phase':50s}" + "".join(f"{c:>10s}" for c in COLS) + "  algorithmic operations (SURVEY 8d)"
    print(head)
    for (label, _, alg), r in zip(PHASES, rows):
        print(f"{label:50s}" + "".join(f"{r[c]:10d}" for c in COLS) + f"  {alg}")
    print(f"{'whole kernel':50s}" + "".join(f"{total[c]:10d}" for c in COLS))
    print(f"\nscalar share: {(total['SALU'] + total['s_nop'] + total['SMEM'] + total['branch'] + total['wait']) / total['total']:.3f} of the instructions;  "
          f"v_mov_b32: {total['v_mov']} ({total['v_mov'] / total['VALU']:.3f} of VALU)")


if __name__ == "__main__":
    main()
