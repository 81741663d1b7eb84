"""The a-trous denoiser as include/pt_render.h defines it (pt_denoise), restated in numpy binary32: written from the header's text, not
from the kernel.  Vectorised over the pixels, a loop over the 25 taps in the defined order (dy outer, dx inner); every array is float32
and every numpy operation on float32 arrays is one correctly rounded IEEE operation, so the model computes exactly what the header
says — the kernel is held to it bit for bit (tests/test_gpu_denoise.py).  Imports nothing of the product."""
import numpy as np

F = np.float32
DEMODULATE = 1
KERNEL = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]
DEFAULTS = dict(iterations=5, sigma_color=32.0, sigma_normal=0.5, sigma_depth=0.2, sigma_albedo=0.0, demodulate=True)

LOG2E = F(float.fromhex("0x1.715476p+0"))
LN2_HI = F(float.fromhex("0x1.62e4p-1"))
LN2_LO = F(float.fromhex("0x1.7f7d1cp-20"))
POLY = [F(float.fromhex(c)) for c in ("0x1.6c16c2p-10", "0x1.111112p-7", "0x1.555556p-5", "0x1.555556p-3", "0x1p-1", "0x1p+0", "0x1p+0")]


def exp_neg(x):
    """pt_exp_neg: e^-x for 0 <= x < 80, the header's operations one by one."""
    x = np.asarray(x, dtype=F)
    k = np.rint(x * LOG2E)  # round half to even
    t = -((x - k * LN2_HI) - k * LN2_LO)
    q = np.full_like(x, POLY[0])
    for c in POLY[1:]:
        q = q * t + c  # two operations, each rounded: numpy does not fuse
    out = np.ldexp(q, -k.astype(np.int32))
    assert x.dtype == k.dtype == t.dtype == q.dtype == out.dtype == F
    return out


def _k(sigma):
    s = F(sigma)
    return F(1.0) / (s * s)


def denoise(color, albedo=None, normal=None, depth=None, *, iterations=5, sigma_color=32.0, sigma_normal=0.5, sigma_depth=0.2,
            sigma_albedo=0.0, demodulate=True):
    """color, albedo, normal: [h][w][3]; depth: [h][w]; returns [h][w][3] float32."""
    with np.errstate(all="ignore"):
        return _denoise(color, albedo, normal, depth, iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo, demodulate)


def _denoise(color, albedo, normal, depth, iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo, demodulate):
    c = np.array(color, dtype=F)
    h, w, _ = c.shape
    assert 1 <= iterations <= 8
    albedo = None if albedo is None else np.asarray(albedo, dtype=F)
    normal = None if normal is None else np.asarray(normal, dtype=F)
    depth = None if depth is None else np.asarray(depth, dtype=F)
    if demodulate:
        assert albedo is not None, "PT_DENOISE_DEMODULATE needs the albedo plane"
        c = c / (albedo + F(1e-3))
    on_c = sigma_color > 0
    on_n = sigma_normal > 0 and normal is not None
    on_d = sigma_depth > 0 and depth is not None
    on_a = sigma_albedo > 0 and albedo is not None
    k_n = _k(sigma_normal) if on_n else None
    k_a = _k(sigma_albedo) if on_a else None
    if on_d:
        sd = F(sigma_depth)
        den = (sd * sd) * (depth * depth) + F(1e-12)

    def sq3(d):
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    for i in range(iterations):
        s = 1 << i
        k_c = _k(np.ldexp(F(sigma_color), -i)) if on_c else None
        total = np.zeros((h, w, 3), F)
        wsum = np.zeros((h, w), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                # pixels p whose tap q = p + (ox, oy) is inside the frame
                y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                x = np.zeros((y1 - y0, x1 - x0), F)
                x = (sq3(c[P] - c[Q]) * k_c) if on_c else x
                x = x + ((sq3(normal[P] - normal[Q]) * k_n) if on_n else F(0))
                if on_d:
                    dz = depth[P] - depth[Q]
                    x = x + (dz * dz) / den[P]
                else:
                    x = x + F(0)
                x = x + ((sq3(albedo[P] - albedo[Q]) * k_a) if on_a else F(0))
                ok = x < F(80.0)  # False for NaN
                wgt = (KERNEL[dy + 2] * KERNEL[dx + 2]) * exp_neg(np.where(ok, x, F(0)))
                cq = c[Q]
                total[P] = np.where(ok[..., None], total[P] + wgt[..., None] * cq, total[P])
                wsum[P] = np.where(ok, wsum[P] + wgt, wsum[P])
                assert x.dtype == wgt.dtype == F
        nxt = np.where((wsum != 0)[..., None], total / wsum[..., None], c)
        assert nxt.dtype == F
        c = nxt
    if demodulate:
        c = c * (albedo + F(1e-3))
    assert c.dtype == F
    return c
