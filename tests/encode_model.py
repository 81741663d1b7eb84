"""The encode stage restated from its header (include/pt_encode.h: pt_encode), for the tests that hold the kernel to it
(tests/test_gpu_encode.py) and the definition to its properties (tests/test_encode_cpu.py).  numpy only: the two tables are read from the
header's macros, a code is np.searchsorted over them, the dither's f is binary32 arithmetic rounded once per operation, the threshold is
the Bayer formula.  Nothing here shares code with the kernel, which finds its codes another way."""
import re
from pathlib import Path

import numpy as np

HEADER = Path(__file__).resolve().parent.parent / "include" / "pt_encode.h"
F = np.float32
REFERENCE, SRGB = 0, 1
DITHER, NO_VEC = 1, 2


def header_table(name):
    """The binary32 values of the macro `name` of the header, in its order."""
    body = re.search(r"#define %s \{(.*?)\}" % name, HEADER.read_text(), re.S).group(1).replace("\\\n", " ")
    return np.array([float.fromhex(v.strip().rstrip("f")) for v in body.split(",")], dtype=np.float64).astype(F)


M = header_table("PT_SRGB8_THRESHOLDS")  # M[j - 1] is the header's M[j]
L = header_table("PT_SRGB8_LEVELS")      # L[c]


def bayer(u, v):
    """B(u, v) of the header, for integer arrays 0 ... 7."""
    u, v = np.asarray(u), np.asarray(v)
    b = np.zeros(np.broadcast(u, v).shape, dtype=np.int64)
    for i in range(3):
        b += ((((u ^ v) >> i) & 1) << (2 * (2 - i) + 1)) | (((v >> i) & 1) << (2 * (2 - i)))
    return b


def thresholds(width, height, phase=(0, 0)):
    """t for every pixel of the frame, [height][width] with row 0 the BOTTOM row (py), binary32: exact."""
    px = (np.arange(width, dtype=np.int64) + int(phase[0])) & 7
    py = (np.arange(height, dtype=np.int64) + int(phase[1])) & 7
    return ((bayer(px[None, :], py[:, None]).astype(F) + F(0.5)) * F(2.0 ** -6)).astype(F)


def quantise(x):
    """The reference's quantiser: sqrt, clamp to [0, 0.999], * 256, truncate; NaN gives 0."""
    x = np.asarray(x, dtype=F)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(x)                                                    # correctly rounded; NaN for negatives, -0 for -0
        cl = np.where(s < 0, F(0), np.where(F(0.999) < s, F(0.999), s)).astype(F)  # std::clamp: NaN stays NaN
        sc = (F(256.0) * cl).astype(F)
    return np.where(np.isnan(sc), 0, np.nan_to_num(sc, nan=0.0)).astype(np.int64).astype(np.uint8)


def srgb_codes(x):
    """The number of j in 1 ... 255 with M[j] <= x; NaN compares false with everything."""
    x = np.asarray(x, dtype=F)
    return np.where(np.isnan(x), 0, np.searchsorted(M, np.nan_to_num(x, nan=0.0), side="right")).astype(np.uint8)


def dither_codes(x, t):
    """The dithered code of the values x against the thresholds t (same shape or broadcastable)."""
    x = np.asarray(x, dtype=F)
    inside = (x > 0) & (x < 1)                                            # NaN: False
    xs = np.where(inside, x, F(0.5)).astype(F)
    c = np.searchsorted(L[1:255], xs, side="right")                       # the number of j in 1 ... 254 with L[j] <= x
    f = ((xs - L[c]).astype(F) / (L[c + 1] - L[c]).astype(F)).astype(F)
    code = c + (f >= np.asarray(t, dtype=F))
    with np.errstate(invalid="ignore"):
        return np.where(inside, code, np.where(x >= 1, 255, 0)).astype(np.uint8)


def encode(linear, transfer=SRGB, dither=False, phase=(0, 0)):
    """pt_encode: linear [height][width][3] float32 with row 0 the bottom -> uint8 [height][width][3] with row 0 the top."""
    linear = np.asarray(linear, dtype=F)
    h, w, _ = linear.shape
    if transfer == REFERENCE:
        assert not dither
        codes = quantise(linear)
    elif dither:
        codes = dither_codes(linear, thresholds(w, h, phase)[:, :, None])  # one t for the three channels
    else:
        codes = srgb_codes(linear)
    return np.ascontiguousarray(codes[::-1])
