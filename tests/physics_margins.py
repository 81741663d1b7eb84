"""Writes profiles/physics_model_margins.txt (for information only): per case and field the largest observed
error/bound ratio on decided rays, the borderline and skipped shares, and which cases reject which wrong oracle.

    python tests/physics_margins.py cpu  cpu.json      # the oracle, both math modes, and every mutant over every case
    python tests/physics_margins.py gpu  gpu.json      # the device (needs an MI355X)
    python tests/physics_margins.py text cpu.json gpu.json profiles/physics_model_margins.txt
"""
import json
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE)]

import physics_cases as PC  # noqa: E402
from physics_compare import compare  # noqa: E402


def _merge(a, b):
    out = dict(a)
    out["ratios"] = {k: max(a["ratios"].get(k, 0.0), b["ratios"].get(k, 0.0)) for k in set(a["ratios"]) | set(b["ratios"])}
    return out


def cpu(path):
    import test_physics_model_cpu as T
    from oracle import binding
    binding.load()
    stats = {}
    for name in PC.BOUNCE_NAMES:
        stats[name] = _merge(T.run_bounce_case(binding, name, True), T.run_bounce_case(binding, name, False))
    for name in PC.CAMERA_NAMES:
        f1, s1 = T.run_camera_case(binding, name, True)
        f2, s2 = T.run_camera_case(binding, name, False)
        stats["camera_" + name] = _merge(s1, s2)
        stats["camera_fields_" + name] = _merge(f1, f2)
    binding.set_math(False)
    kills = {}
    text = (T.ORACLE_DIR / "pt_oracle.c").read_text()
    with tempfile.TemporaryDirectory() as tmp:
        for k, (mutant, (old, new, targets)) in enumerate(T.MUTANTS.items()):
            o = binding.bind(T.compile_oracle(text.replace(old, new), Path(tmp), f"m{k}"))
            kills[mutant] = []
            for name in (PC.CAMERA_NAMES if targets == "camera" else PC.BOUNCE_NAMES):
                try:
                    (T.run_camera_case if targets == "camera" else T.run_bounce_case)(o, name, True)
                except AssertionError:
                    kills[mutant].append(name)
    Path(path).write_text(json.dumps(dict(stats=stats, kills=kills), indent=1))


def gpu(path):
    import test_gpu_physics_model as G
    from path_tracer_amd import abi
    lib = abi.load_library()
    stats = {}
    for name in PC.BOUNCE_NAMES:
        case = PC.bounce_case(name)
        stats[name] = compare(G.device_bounce(lib, case), case, name)
        if name in PC.POOLED:
            with G.forced_pools():
                out = G.device_bounce(lib, case)
            stats[name] = _merge(stats[name], compare(out, case, name + " pooled"))
    for name in PC.CAMERA_NAMES:
        case = PC.camera_case(name)
        stats["camera_" + name] = compare(G.device_camera_rays(lib, case), case, name)
    Path(path).write_text(json.dumps(dict(stats=stats), indent=1))


def text(cpu_json, gpu_json, out):
    c = json.loads(Path(cpu_json).read_text())
    g = json.loads(Path(gpu_json).read_text())["stats"] if Path(gpu_json).exists() else {}
    lines = ["Physics model margins: largest |record - model| / bound over the decided rays of each case, per field.",
             "oracle = oracle/pt_oracle.c in both math modes (CPU); device = pt_debug_bounce / pt_debug_camera_rays on an MI355X,",
             "pools forced as well where the case is in physics_cases.POOLED.  For information only: the tests assert <= 1.", ""]
    for name, s in c["stats"].items():
        lines.append(f"{name}: rays {s.get('n', '-')}, borderline {s.get('borderline', 0):.1%}, skipped {s.get('skipped', 0):.1%}"
                     + (f", decided hits {s['decided_hits']}, misses {s['decided_misses']}" if "decided_hits" in s else ""))
        for f in sorted(s["ratios"]):
            dev = g.get(name, {}).get("ratios", {}).get(f)
            lines.append(f"    {f:18s} oracle {s['ratios'][f]:.3f}   device " + (f"{dev:.3f}" if dev is not None else "-"))
    lines += ["", "Wrong oracles (tests/test_physics_model_cpu.py::MUTANTS) and the cases whose comparison rejects them:"]
    for m, cases in c["kills"].items():
        lines.append(f"  {m}: " + (", ".join(cases) if cases else "NOT REJECTED"))
    Path(out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    dict(cpu=cpu, gpu=gpu, text=text)[sys.argv[1]](*sys.argv[2:])
