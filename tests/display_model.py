"""The display stage as include/pt_render.h defines it (pt_display_meter, pt_display_apply), restated in numpy: written from the header's
text, not from the kernels.  Every float array is float32 and every numpy operation on float32 arrays is one correctly rounded IEEE
operation; the solve is Python integers and one binary64 division.  The kernels are held to it bit for bit (tests/test_gpu_display.py).
Imports nothing of the product; pt_exp_neg is tests/denoise_model.py's."""
import numpy as np

from denoise_model import exp_neg

F = np.float32
REFERENCE, REINHARD, ACES = 0, 1, 2
TONES = {"reference": REFERENCE, "reinhard": REINHARD, "aces": ACES}
LOGC = [5732, 16248, 25711, 34312, 42196, 49472, 56229, 62534]
LOG2_KEY = F(float.fromhex("-0x1.3ca9c6p+1"))
LN2 = F(float.fromhex("0x1.62e430p-1"))
X_MAX = F(2.0 ** 20)
DEFAULTS = dict(tone=ACES, ev_bias=0.0, ev_min=-16.0, ev_max=16.0, lo_permille=400, hi_permille=950, adapt_up=1.0, adapt_down=1.0, white=4.0)


def luminance(color):
    c = np.asarray(color, dtype=F)
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def bins_of(y):
    """Bin of each luminance: 0 ... 255, or 256 = rejected (NaN, +-inf, negative, +-0)."""
    y = np.asarray(y, dtype=F)
    bits = y.view(np.uint32)
    k = np.clip((bits >> 20).astype(np.int64) - ((127 - 16) << 3), 0, 255)
    with np.errstate(invalid="ignore"):
        ok = (y > 0) & np.isfinite(y)
    return np.where(ok, k, 256)


def histogram(color, rect=None):
    """The 256 bins followed by `rejected` (uint32[257]) of the frame [h][w][3], or of its rectangle (x0, y0, x1, y1), y = 0 the bottom row
    (the frame buffer's row 0)."""
    c = np.asarray(color, dtype=F)
    if rect is not None:
        x0, y0, x1, y1 = rect
        c = c[y0:y1, x0:x1]
    with np.errstate(all="ignore"):
        b = bins_of(luminance(c))
    return np.bincount(b.ravel(), minlength=257).astype(np.uint32)


def bin_value(b):
    return 65536 * ((b >> 3) - 16) + LOGC[b & 7]


def solve(hist, lo_permille=400, hi_permille=950):
    """(S, C) of the band [lo_n, hi_n) of ranks: Python integers."""
    n = int(sum(int(v) for v in hist[:256]))
    lo_n, hi_n = n * lo_permille // 1000, n * hi_permille // 1000
    rank, s, c = 0, 0, 0
    for b in range(256):
        end = rank + int(hist[b])
        cb = max(0, min(end, hi_n) - max(rank, lo_n))
        s += cb * bin_value(b)
        c += cb
        rank = end
    return s, c


def target(hist, *, ev_bias=0.0, ev_min=-16.0, ev_max=16.0, lo_permille=400, hi_permille=950, **_):
    """e_t, or None where C == 0."""
    s, c = solve(hist, lo_permille, hi_permille)
    if c == 0:
        return None
    t = F((float(s) / float(c)) * 2.0 ** -16)  # |s|, c < 2^53: the conversions are exact, the division is binary64's
    return F(min(max((LOG2_KEY - t) + F(ev_bias), F(ev_min)), F(ev_max)))


class State:
    """e and whether a metering has set it (the PtDisplay's device words)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.e, self.primed, self.last = F(0.0), False, np.zeros(257, np.uint32)

    def set_exposure(self, ev):
        self.e, self.primed = F(min(max(F(ev), F(-32.0)), F(32.0))), True

    def meter(self, color, rect=None, *, adapt_up=1.0, adapt_down=1.0, **params):
        self.last = histogram(color, rect)
        et = target(self.last, **params)
        if et is None:
            return self.e
        if self.primed:
            a = F(adapt_up) if et > self.e else F(adapt_down)
            self.e = F(self.e + F(F(et - self.e) * a))
        else:
            self.e = et
        self.primed = True
        return self.e


def scale_of(e):
    e = F(e)
    k = np.ceil(e)
    return F(np.ldexp(exp_neg(F(F(k - e) * LN2)), int(k)))


def curve(x, tone, white=4.0):
    x = np.asarray(x, dtype=F)
    if tone == REFERENCE:
        return x
    if tone == REINHARD:
        iw2 = F(1.0) / (F(white) * F(white))
        return (x * (F(1.0) + x * iw2)) / (F(1.0) + x)
    assert tone == ACES
    return (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))


def quantise(y):
    """pt_tonemap_rgb8's quantiser for one plane of values: sqrt, clamp to [0, 0.999], * 256, truncate; int(NaN) = 0."""
    with np.errstate(all="ignore"):
        s = np.sqrt(np.asarray(y, dtype=F))
        cl = np.where(s < 0, F(0.0), np.where(F(0.999) < s, F(0.999), s)).astype(F)
        sc = F(256.0) * cl
        return np.where(sc == sc, sc, F(0.0)).astype(np.int32).astype(np.uint8)


def apply(color, e, tone=ACES, white=4.0):
    """(rgb8 [h][w][3] with row 0 = top, linear [h][w][3] in the frame's layout) of the frame at exposure e."""
    c = np.asarray(color, dtype=F)
    with np.errstate(all="ignore"):
        x = c * scale_of(e)
        x = np.where(x >= 0, x, F(0.0)).astype(F)
        x = np.where(x > X_MAX, X_MAX, x).astype(F)
        y = curve(x, tone, white).astype(F)
    assert y.dtype == F
    return quantise(y)[::-1].copy(), y
