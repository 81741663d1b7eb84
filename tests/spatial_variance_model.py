"""include/pt_spatial_variance.h's spatial variance estimate restated in numpy binary32, operation by operation, from the header's text:
every array is float32, every operation is one numpy operation on float32 arrays (rounded once, nothing fused) and the order is the
header's.  The window loops run over the offsets in the header's order (dy outer, dx inner; the horizontal pair before the vertical one),
each step on whole frames.  Not a test file: tests/test_spatial_variance_cpu.py holds its properties and its quality record,
tests/test_gpu_spatial_variance.py holds the kernel's bits to it."""
import numpy as np

F = np.float32
DEMODULATE, NO_LDS = 1, 2
MAX_RADIUS = 3
DEFAULTS = dict(radius=2, min_pairs=4, tol_depth=0.1, tol_normal=0.5, demodulate=True)
INF = F(np.inf)


def shifted(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx] where that lies inside the frame, else `fill`."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    if abs(dx) >= w or abs(dy) >= h:
        return b
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    b[yd, xd] = a[ys, xs]
    return b


def keep(variance_in):
    """pt_variance_denoise's sanitising test: every channel is (>= 0 && < +inf); -0 passes."""
    v = np.asarray(variance_in, F)
    with np.errstate(all="ignore"):
        return ((v >= F(0)) & (v < INF)).all(axis=-1)


def spatial_variance(color, variance_in=None, *, albedo=None, normal=None, depth=None, id=None, radius=DEFAULTS["radius"],
                     min_pairs=DEFAULTS["min_pairs"], tol_depth=DEFAULTS["tol_depth"], tol_normal=DEFAULTS["tol_normal"], demodulate=None):
    """-> (variance_out, (estimated, holes)).  color, albedo, normal, variance_in: [H][W][3] float32; depth: [H][W] float32; id: [H][W]
    int32.  demodulate: None = where an albedo plane is given (the hosts' rule)."""
    c = np.ascontiguousarray(color, dtype=F)
    demodulate = albedo is not None if demodulate is None else bool(demodulate)
    assert c.ndim == 3 and c.shape[2] == 3 and 1 <= radius <= MAX_RADIUS and min_pairs >= 1
    assert not demodulate or albedo is not None
    h, w, _ = c.shape
    r = int(radius)
    with np.errstate(all="ignore"):
        if demodulate:
            m = (np.asarray(albedo, F) + F(1e-3)).astype(F)
            e = (c / m).astype(F)
        else:
            m = np.ones_like(c)
            e = c
        usable = (np.abs(e) < INF).all(axis=-1)
        z = None if depth is None else np.asarray(depth, F)
        k = None if id is None else np.asarray(id, np.int32)
        n = None if normal is None else np.asarray(normal, F)
        tn2 = F(tol_normal) * F(tol_normal)
        cons = {}
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ok = shifted(usable, dx, dy, False)
                if z is not None:
                    zq = shifted(z, dx, dy, F(0))
                    near = (zq > F(0)) & (np.abs((zq - z).astype(F)) <= (F(tol_depth) * z).astype(F))
                    ok = ok & np.where(z > F(0), near, ~(zq > F(0)))
                if k is not None:
                    ok = ok & (shifted(k, dx, dy, 0) == k)
                if n is not None:
                    dn = (n - shifted(n, dx, dy, F(0))).astype(F)
                    dd = (((dn[..., 0] * dn[..., 0]).astype(F) + (dn[..., 1] * dn[..., 1]).astype(F)).astype(F)
                          + (dn[..., 2] * dn[..., 2]).astype(F)).astype(F)
                    ok = ok & (dd <= tn2)
                cons[dx, dy] = ok
        ssd = np.zeros((h, w, 3), F)
        pairs = np.zeros((h, w), np.int32)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                eq = shifted(e, dx, dy, F(0))
                for ox, oy in ((1, 0), (0, 1)):
                    if (dx < r) if ox else (dy < r):
                        take = cons[dx, dy] & cons[dx + ox, dy + oy]
                        d = (eq - shifted(e, dx + ox, dy + oy, F(0))).astype(F)
                        ssd = np.where(take[..., None], (ssd + (d * d).astype(F)).astype(F), ssd)
                        pairs = pairs + take.astype(np.int32)
        kept = keep(variance_in) if variance_in is not None else np.zeros((h, w), bool)
        est = ~kept & usable & (pairs >= int(min_pairs))
        hole = ~kept & ~est
        value = ((ssd / (F(2.0) * pairs.astype(F))[..., None]).astype(F) * (m * m).astype(F)).astype(F)
        out = np.where(est[..., None], value, INF).astype(F)
        if variance_in is not None:
            out = np.where(kept[..., None], np.ascontiguousarray(variance_in, dtype=F), out)  # a copy: the bits are the input's
    return out, (int(est.sum()), int(hole.sum()))
