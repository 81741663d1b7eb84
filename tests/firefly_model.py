"""include/pt_post.h's firefly stage restated in numpy binary32, operation by operation, from the header's text: every array is float32,
every operation is one numpy operation on float32 arrays (rounded once, nothing fused) and the order is the header's.  The neighbour
loop runs over the eight offsets in the header's order, each step on whole frames.  Not a test file: tests/test_firefly_cpu.py holds
its properties and its quality record, tests/test_gpu_firefly.py holds the kernel's bits to it."""
import numpy as np

F = np.float32
REPAIR, NO_LDS = 1, 2
DEFAULTS = dict(rank=1, k=1.0, repair=True)
INF = F(np.inf)


def luminance(c):
    """Y(c) = (0.2126f * R + 0.7152f * G) + 0.0722f * B."""
    c = np.asarray(c, F)
    with np.errstate(all="ignore"):
        return ((F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]).astype(F) + F(0.0722) * c[..., 2]).astype(F)


def finite(c):
    """fabsf(ch) < +inf for each of the three channels (NaN fails)."""
    with np.errstate(all="ignore"):
        return (np.abs(np.asarray(c, F)) < INF).all(axis=-1)


def shifted(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx] where that lies inside the frame, else `fill`."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    b[yd, xd] = a[ys, xs]
    return b


def firefly(color, variance=None, rank=1, k=1.0, repair=True):
    """-> (out, variance_out or None, (clamped, repaired)).  color, variance: [H][W][3] float32."""
    c = np.ascontiguousarray(color, dtype=F)
    assert c.ndim == 3 and c.shape[2] == 3 and rank in (1, 2) and np.isfinite(k) and k > 0
    h, w, _ = c.shape
    k = F(k)
    fin, Y = finite(c), luminance(c)
    m1, m2 = np.full((h, w), -INF, F), np.full((h, w), -INF, F)
    n = np.zeros((h, w), np.int32)
    total = np.zeros((h, w, 3), F)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                ok = shifted(fin, dx, dy, False)  # inside the frame and finite(q)
                cq, Yq = shifted(c, dx, dy, F(0)), shifted(Y, dx, dy, F(0))
                n = n + ok.astype(np.int32)
                total = np.where(ok[..., None], (total + cq).astype(F), total)
                first = ok & (Yq > m1)
                second = ok & ~first & (Yq > m2)
                m2 = np.where(first, m1, np.where(second, Yq, m2)).astype(F)
                m1 = np.where(first, Yq, m1).astype(F)
        m = m1 if rank == 1 else m2
        L = (k * m).astype(F)
        clamp = fin & (n >= rank) & (Y > L) & (Y > F(0))
        s = (np.where(L > F(0), L, F(0)).astype(F) / Y).astype(F)
        s2 = (s * s).astype(F)
        fix = ~fin & bool(repair) & (n > 0)
        mean = (total / n.astype(F)[..., None]).astype(F)
        out = np.where(clamp[..., None], (c * s[..., None]).astype(F), np.where(fix[..., None], mean, c)).astype(F)
        vout = None
        if variance is not None:
            v = np.ascontiguousarray(variance, dtype=F)
            assert v.shape == c.shape
            vout = np.where(clamp[..., None], (v * s2[..., None]).astype(F), np.where(fix[..., None], INF, v)).astype(F)
    # an untouched pixel is a copy: the bits of its NaNs are the input's (np.where keeps them)
    return out, vout, (int(clamp.sum()), int(fix.sum()))
