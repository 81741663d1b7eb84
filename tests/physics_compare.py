"""compare(): hold recorded bounces or camera rays (from the oracle or from the device) to tests/physics_model.py.

A decided ray (every decision margin >= 2) must agree in every integer field and lie within the model's bound in every
float field.  A ray with ONE borderline decision must agree with the model as evaluated, or with the model re-evaluated
with that decision taken the other way (which must not itself raise a second borderline decision).  Rays with two or
more borderline decisions are counted as skipped.  The caps on those shares and the floors on what each case must
exercise are conditions of the comparison, asserted here."""
import math

import physics_model as M
from path_tracer_amd import abi

CAP_SKIPPED = 0.02
CAP_BORDERLINE = 0.10
CAP_BORDERLINE_EDGE = 0.50
MIN_DECIDED_HITS = 30
MIN_DECIDED_MISSES = 20
MIN_BRANCH = 20


class BounceCase:
    """A scene, its recorded inputs and (lazily, once) the model's evaluation of every ray."""

    def __init__(self, name, ps, recs, edge=False, can_miss=True, dielectric=False, medium=False):
        self.name, self.ps, self.recs, self.edge, self.can_miss = name, ps, recs, edge, can_miss
        self.dielectric, self.medium = dielectric, medium
        self.scene = M.Scene(ps)
        self._rows = None

    def rows(self):
        if self._rows is None:
            self._rows = [M.bounce_record(self.scene, self.recs[k]) for k in range(len(self.recs))]
            self._check_boxes()
        return self._rows

    def flipped(self, k, decision):
        return M.bounce_record(self.scene, self.recs[k], flip=decision)

    def _check_boxes(self):
        """The model's own cross-check: a decided box hit lies where the three slabs say the line enters or leaves."""
        for k, (val, _, T) in enumerate(self._rows):
            i = val["hittable"]
            if i < 0 or self.scene.h[i][0] != abi.PT_HIT_BOX or T.borderline() or val["t"] != val["t"]:
                continue
            r = self.recs[k]
            slabs = M.box_slabs(self.scene.h[i][4], [float(x) for x in r.origin], [float(x) for x in r.dir])
            assert slabs is not None and min(abs(val["t"] - s) for s in slabs) <= 1e-9 * max(1.0, abs(val["t"])), \
                f"{self.name}[{k}]: box hit at t={val['t']} but the slabs give {slabs}"


class CameraCase:
    def __init__(self, name, ctor_args, cam, width, height, xy, states):
        self.name, self.ctor_args, self.cam, self.width, self.height, self.xy, self.states = name, ctor_args, cam, width, height, xy, states
        self._rows = None

    def rows(self):
        if self._rows is None:
            self._rows = [M.camera_ray(self.cam, int(self.xy[k][0]), int(self.xy[k][1]), self.width, self.height, int(self.states[k]))
                          for k in range(len(self.states))]
        return self._rows


def _vec(x):
    return [float(a) for a in x] if hasattr(x, "__len__") else [float(x)]


def _field_errors(got, val, bnd, fields, ratios=None):
    """[(field, got, want, bound)] of the float fields outside their bound; NaN agrees with NaN, inf with the same inf."""
    bad = []
    for name in fields:
        g, w, b = _vec(getattr(got, name)), _vec(val[name]), _vec(bnd[name])
        for gi, wi, bi in zip(g, w, b):
            if (gi != gi and wi != wi) or gi == wi:
                ratio = 0.0
            elif gi != gi or wi != wi or abs(gi) == math.inf or abs(wi) == math.inf:
                ratio = 0.0 if bi == math.inf else math.inf
            else:
                err = abs(gi - wi)
                ratio = 0.0 if bi == math.inf else (err / bi if bi > 0 else math.inf)
            if ratios is not None:
                ratios[name] = max(ratios.get(name, 0.0), ratio)
            if ratio > 1.0:
                bad.append((name, g, w, b))
                break
    return bad


def _bounce_errors(got, val, bnd, with_uv, ratios=None):
    bad = [(name, getattr(got, name), val[name], 0) for name in M.BOUNCE_INT_FIELDS if int(getattr(got, name)) != int(val[name])]
    fields = [f for f in M.BOUNCE_FLOAT_FIELDS if with_uv or f not in ("u", "v")]
    if bad:
        return bad      # the float fields of another path say nothing
    return _field_errors(got, val, bnd, fields, ratios)


def _describe(case, k, bad, T):
    r = case.recs[k]
    lines = [f"ray {k}: origin {list(r.origin)} dir {list(r.dir)} time {r.time} state {r.rng_state}"]
    for name, g, w, b in bad:
        lines.append(f"  {name}: got {g!r}, model {w!r}, bound {b!r}")
    low = sorted(zip(T.margins, T.names))[:6]
    lines.append("  smallest margins: " + ", ".join(f"{n}={m:.3g}" for m, n in low))
    return "\n".join(lines)


def compare(records, model, what):
    """-> statistics (dict) of the comparison; raises AssertionError naming ray, field, both values, bound and margins."""
    if isinstance(model, CameraCase):
        return _compare_camera(records, model, what)
    case = model
    rows = case.rows()
    n = len(rows)
    assert len(records) >= n
    with_uv = case.scene.has_image
    ratios, failures = {}, []
    borderline = skipped = hits = misses = 0
    branches = {}
    for k in range(n):
        val, bnd, T = rows[k]
        low = T.borderline()
        if not low:
            bad = _bounce_errors(records[k], val, bnd, with_uv, ratios)
            if bad:
                failures.append(_describe(case, k, bad, T))
            if val["status"] == abi.PT_BOUNCE_MISS:
                misses += 1
            else:
                hits += 1
            for b in T.info:
                branches[b] = branches.get(b, 0) + 1
            continue
        if len(low) >= 2:
            skipped += 1
            continue
        borderline += 1
        bad = _bounce_errors(records[k], val, bnd, with_uv)
        if not bad:
            continue
        val2, bnd2, T2 = case.flipped(k, low[0])
        if [j for j in T2.borderline() if j != low[0]]:
            skipped += 1
            borderline -= 1
            continue
        bad2 = _bounce_errors(records[k], val2, bnd2, with_uv)
        if bad2:
            failures.append(_describe(case, k, bad, T) + f"\n  and with '{T.names[low[0]]}' taken the other way:\n" + _describe(case, k, bad2, T2))
    stats = dict(n=n, borderline=borderline / n, skipped=skipped / n, decided_hits=hits, decided_misses=misses,
                 ratios=ratios, branches=branches)
    assert not failures, f"{what}: {len(failures)} of {n} rays disagree with the model\n" + "\n".join(failures[:5])
    assert skipped <= CAP_SKIPPED * n, f"{what}: {skipped} of {n} rays skipped (two borderline decisions)"
    cap = CAP_BORDERLINE_EDGE if case.edge else CAP_BORDERLINE
    assert borderline <= cap * n, f"{what}: {borderline} of {n} rays borderline (cap {cap:.0%})"
    assert hits >= MIN_DECIDED_HITS, f"{what}: only {hits} decided hits"
    if case.can_miss:
        assert misses >= MIN_DECIDED_MISSES, f"{what}: only {misses} decided misses"
    if case.dielectric:
        for b in ("reflect", "refract"):
            assert branches.get(b, 0) >= MIN_BRANCH, f"{what}: only {branches.get(b, 0)} decided rays on the {b} branch"
    if case.medium:
        for b in ("medium scatters", "medium passes"):
            assert branches.get(b, 0) >= MIN_BRANCH, f"{what}: only {branches.get(b, 0)} decided rays where the {b}"
    return stats


def _compare_camera(records, case, what):
    rows = case.rows()
    ratios, failures = {}, []
    for k, (val, bnd) in enumerate(rows):
        got = records[k]
        if int(got.rng_state) != val["rng_state"]:
            failures.append(f"ray {k}: rng_state got {got.rng_state}, model {val['rng_state']}")
            continue
        bad = _field_errors(got, val, bnd, ("origin", "dir", "time"), ratios)
        for name, g, w, b in bad:
            failures.append(f"ray {k} (pixel {list(case.xy[k])}, state {case.states[k]}): {name}: got {g!r}, model {w!r}, bound {b!r}")
    assert not failures, f"{what}: {len(failures)} camera rays disagree with the model\n" + "\n".join(failures[:5])
    return dict(n=len(rows), ratios=ratios, borderline=0.0, skipped=0.0)


def compare_camera_fields(cam, ctor_args, what):
    """The constructor: every field of a PtCamera against model.camera(*ctor_args)."""
    val, bnd = M.camera(*ctor_args)
    ratios = {}
    bad = _field_errors(cam, val, bnd, M.CAMERA_FIELDS, ratios)
    assert not bad, f"{what}: " + "; ".join(f"{n}: got {g!r}, model {w!r}, bound {b!r}" for n, g, w, b in bad)
    return dict(ratios=ratios)


def field_ratio_line(name, stats):
    r = stats["ratios"]
    return (f"{name:34s} borderline {stats.get('borderline', 0):6.1%} skipped {stats.get('skipped', 0):5.1%}  "
            + " ".join(f"{k}={v:.3f}" for k, v in sorted(r.items())))
