"""The variance estimate and the variance-guided denoiser as include/pt_render.h defines them (pt_variance_estimate,
pt_variance_denoise), restated in numpy binary32: written from the header's text, not from the kernels.  Vectorised over the pixels, loops
over the 9 prefilter taps and the 25 filter taps in the defined order (dy outer, dx inner); every array is float32 and every numpy
operation on float32 arrays is one correctly rounded IEEE operation, so the model computes exactly what the header says — the kernels are
held to it bit for bit (tests/test_gpu_variance_denoise.py).  Imports nothing of the product; pt_exp_neg and K are pt_denoise's."""
import numpy as np

from denoise_model import KERNEL, exp_neg

F = np.float32
DEMODULATE = 1
GAUSS = [F(1 / 4), F(1 / 2), F(1 / 4)]
DEFAULTS = dict(iterations=5, sigma_variance=2.0, sigma_normal=0.5, sigma_depth=0.2, sigma_albedo=0.0, demodulate=True)


def estimate(S, H, n, a):
    """S, H: [..., 3] float32 sums and half sums; n, a: [...] int32 counts.  Returns the [..., 3] variance of the resolved pixel:
    +inf where a == 0 or a == n, else (A - B)^2 * (a b / n^2) with A = H / a, B = (S - H) / b, b = n - a."""
    S, H = np.asarray(S, dtype=F), np.asarray(H, dtype=F)
    n, a = np.asarray(n, dtype=np.int64), np.asarray(a, dtype=np.int64)
    none = (a == 0) | (a == n)
    with np.errstate(all="ignore"):
        fa, fb, fn = a.astype(F), (n - a).astype(F), n.astype(F)
        f = (fa * fb) / (fn * fn)
        A = H / fa[..., None]
        B = (S - H) / fb[..., None]
        d = A - B
        var = (d * d) * f[..., None]
    assert var.dtype == F
    return np.where(none[..., None], F(np.inf), var).astype(F)


def _k(sigma):
    s = F(sigma)
    return F(1.0) / (s * s)


def sanitise(v):
    v = np.asarray(v, dtype=F)
    with np.errstate(all="ignore"):
        return np.where((v >= F(0)) & (v < F(np.inf)), v, F(0)).astype(F)


def denoise(color, variance, albedo=None, normal=None, depth=None, *, iterations=5, sigma_variance=2.0, sigma_normal=0.5, sigma_depth=0.2,
            sigma_albedo=0.0, demodulate=True):
    """color, variance, albedo, normal: [h][w][3]; depth: [h][w]; returns (out, variance_out), both [h][w][3] float32."""
    with np.errstate(all="ignore"):
        return _denoise(color, variance, albedo, normal, depth, iterations, sigma_variance, sigma_normal, sigma_depth, sigma_albedo, demodulate)


def _windows(h, w, oy, ox):
    """The pixels P whose neighbour Q = P + (ox, oy) is inside the frame, as slices; None if there is none."""
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def prefilter(v):
    """vbar: the 3 x 3 Gaussian over the in-frame neighbours at a distance of one pixel, normalised by the weights taken."""
    h, w, _ = v.shape
    vs = np.zeros((h, w, 3), F)
    gs = np.zeros((h, w), F)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            pq = _windows(h, w, dy, dx)
            if pq is None:
                continue
            P, Q = pq
            g = GAUSS[dy + 1] * GAUSS[dx + 1]
            vs[P] = vs[P] + g * v[Q]
            gs[P] = gs[P] + g
    out = vs / gs[..., None]
    assert out.dtype == F
    return out


def _denoise(color, variance, albedo, normal, depth, iterations, sigma_variance, sigma_normal, sigma_depth, sigma_albedo, demodulate):
    c = np.array(color, dtype=F)
    v = sanitise(variance)
    h, w, _ = c.shape
    assert v.shape == c.shape and 1 <= iterations <= 8
    albedo = None if albedo is None else np.asarray(albedo, dtype=F)
    normal = None if normal is None else np.asarray(normal, dtype=F)
    depth = None if depth is None else np.asarray(depth, dtype=F)
    if demodulate:
        assert albedo is not None, "PT_VDENOISE_DEMODULATE needs the albedo plane"
        m = albedo + F(1e-3)
    else:
        m = np.ones((h, w, 3), F)
    c = c / m
    v = v / (m * m)
    on_c = sigma_variance > 0
    on_n = sigma_normal > 0 and normal is not None
    on_d = sigma_depth > 0 and depth is not None
    on_a = sigma_albedo > 0 and albedo is not None
    k_n = _k(sigma_normal) if on_n else None
    k_a = _k(sigma_albedo) if on_a else None
    if on_c:
        sv = F(sigma_variance)
        sv2 = sv * sv
    if on_d:
        sd = F(sigma_depth)
        den = (sd * sd) * (depth * depth) + F(1e-12)

    def sq3(d):
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    for i in range(iterations):
        s = 1 << i
        if on_c:
            iv = F(1.0) / (sv2 * prefilter(v) + F(1e-8))
        total = np.zeros((h, w, 3), F)
        vtotal = np.zeros((h, w, 3), F)
        wsum = np.zeros((h, w), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                pq = _windows(h, w, dy * s, dx * s)
                if pq is None:
                    continue
                P, Q = pq
                if on_c:
                    d = c[P] - c[Q]
                    ivp = iv[P]
                    x = ((d[..., 0] * d[..., 0]) * ivp[..., 0] + (d[..., 1] * d[..., 1]) * ivp[..., 1]) + (d[..., 2] * d[..., 2]) * ivp[..., 2]
                else:
                    x = np.zeros(c[P].shape[:2], F)
                x = x + ((sq3(normal[P] - normal[Q]) * k_n) if on_n else F(0))
                if on_d:
                    dz = depth[P] - depth[Q]
                    x = x + (dz * dz) / den[P]
                else:
                    x = x + F(0)
                x = x + ((sq3(albedo[P] - albedo[Q]) * k_a) if on_a else F(0))
                ok = x < F(80.0)  # False for NaN
                wgt = (KERNEL[dy + 2] * KERNEL[dx + 2]) * exp_neg(np.where(ok, x, F(0)))
                total[P] = np.where(ok[..., None], total[P] + wgt[..., None] * c[Q], total[P])
                vtotal[P] = np.where(ok[..., None], vtotal[P] + (wgt * wgt)[..., None] * v[Q], vtotal[P])
                wsum[P] = np.where(ok, wsum[P] + wgt, wsum[P])
                assert x.dtype == wgt.dtype == F
        took = (wsum != 0)[..., None]
        c_next = np.where(took, total / wsum[..., None], c)
        v_next = np.where(took, vtotal / (wsum * wsum)[..., None], v)
        assert c_next.dtype == v_next.dtype == F
        c, v = c_next, v_next
    out, vout = c * m, v * (m * m)
    assert out.dtype == vout.dtype == F
    return out, vout
