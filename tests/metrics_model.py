"""The image error restated from its header (include/pt_metrics.h: pt_image_error), for the tests that hold the kernel to it
(tests/test_gpu_metrics.py) and the definition to its own promises (tests/test_metrics_cpu.py).

The differences are numpy float32 (one rounding each).  Every term is a Python float — binary64, each operation rounded once —, every sum
is a sum of `fractions.Fraction`s, which is exact, and `float(Fraction)` rounds it once, correctly (round-to-nearest-even).  Nothing
here knows how the kernel accumulates.  The per-pixel plane is numpy float32, one operation at a time."""
import math
from fractions import Fraction

import numpy as np

F = np.float32
DEFAULT_EPS = 1e-4
NO_LDS = 1
WORDS, SUMS = 68, 9


def _round(total: Fraction) -> float:
    try:
        return float(total)  # correctly rounded
    except OverflowError:    # at or above 2^1024 - 2^970: what round-to-nearest gives
        return math.inf


def image_error(a, ref, rect=None, eps=DEFAULT_EPS, plane=False):
    """-> dict(sum_sq, sum_abs, sum_rel: 3 floats each; max_abs: 3 float32; pixels, skipped: int[; plane: [H][W] float32]).
    a, ref: [H][W][3] float32.  rect: (x0, y0, x1, y1) or None for the whole frame."""
    a = np.ascontiguousarray(a, F)
    ref = np.ascontiguousarray(ref, F)
    assert a.shape == ref.shape and a.ndim == 3 and a.shape[2] == 3
    h, w, _ = a.shape
    x0, y0, x1, y1 = (0, 0, w, h) if rect is None else rect
    assert 0 <= x0 <= x1 <= w and 0 <= y0 <= y1 <= h
    with np.errstate(all="ignore"):
        d = (a - ref).astype(F)  # binary32, rounded once; numpy keeps subnormals
        inside = np.zeros((h, w), bool)
        inside[y0:y1, x0:x1] = True
        part = inside & np.isfinite(a).all(axis=2) & np.isfinite(ref).all(axis=2) & np.isfinite(d).all(axis=2)
        skipped = int((inside & ~part).sum())
        sums = {k: [Fraction(0)] * 3 for k in ("sum_sq", "sum_abs", "sum_rel")}
        eps = float(eps)
        dp, rp = d[part], ref[part]
        for ch in range(3):
            sq_sum, ab_sum, rel_sum = Fraction(0), Fraction(0), Fraction(0)
            for dv, rv in zip(dp[:, ch].tolist(), rp[:, ch].tolist()):  # tolist(): float32 -> Python float, exactly
                sq = dv * dv          # exact in binary64: 24 x 24 bits
                ab = abs(dv)          # -0 -> +0
                rel = sq / (rv * rv + eps)  # the product exact, the sum and the quotient rounded once
                sq_sum += Fraction(sq)
                ab_sum += Fraction(ab)
                rel_sum += Fraction(rel)
            sums["sum_sq"][ch], sums["sum_abs"][ch], sums["sum_rel"][ch] = sq_sum, ab_sum, rel_sum
        out = {k: [_round(v) for v in vs] for k, vs in sums.items()}
        out["max_abs"] = [F(np.abs(dp[:, ch]).max()) if dp.shape[0] else F(0) for ch in range(3)]
        out["pixels"], out["skipped"] = int(part.sum()), skipped
        if plane:
            e = (((d[..., 0] * d[..., 0]).astype(F) + (d[..., 1] * d[..., 1]).astype(F)).astype(F) + (d[..., 2] * d[..., 2]).astype(F)).astype(F)
            e = (e / F(3)).astype(F)
            out["plane"] = np.where(part, e, F(np.inf)).astype(F)
    return out


def mean(v, pixels):
    """The hosts' derived figure: ordinary binary64, in the header's order."""
    return ((v[0] + v[1]) + v[2]) / (3.0 * pixels) if pixels else math.nan


def mse(res):
    return mean(res["sum_sq"], res["pixels"])


def mae(res):
    return mean(res["sum_abs"], res["pixels"])


def rel_mse(res):
    return mean(res["sum_rel"], res["pixels"])


def psnr(res, peak=1.0):
    m = mse(res)
    if math.isnan(m):
        return math.nan
    return math.inf if m == 0.0 else 10.0 * math.log10(peak * peak / m)


def bits(res):
    """The result as the integers the GPU tests compare: the sums as uint64 views, max_abs as uint32 views, the counts."""
    return {"sum_sq": [int(np.float64(v).view(np.uint64)) for v in res["sum_sq"]],
            "sum_abs": [int(np.float64(v).view(np.uint64)) for v in res["sum_abs"]],
            "sum_rel": [int(np.float64(v).view(np.uint64)) for v in res["sum_rel"]],
            "max_abs": [int(F(v).view(np.uint32)) for v in res["max_abs"]],
            "pixels": int(res["pixels"]), "skipped": int(res["skipped"])}
