"""Derive the two tables of include/pt_encode.h (PT_SRGB8_THRESHOLDS, PT_SRGB8_LEVELS) with integer arithmetic alone and print them as
the header's macros.  No GPU, no libm: the sRGB exponent is 2.4 = 12/5, so "x >= ((v + 0.055) / 1.055)^2.4" is the rational inequality
x^5 >= ((v + 0.055) / 1.055)^12, which fractions.Fraction decides exactly.

    python tools/encode_tables.py            the two macros, as they stand in the header
    python tools/encode_tables.py --check    compare with the header; exit 1 on a difference
"""
import hashlib
import struct
import sys
from fractions import Fraction
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "include" / "pt_encode.h"


def at_least_eotf(x: Fraction, v: Fraction) -> bool:
    """x >= EOTF(v), IEC 61966-2-1's decoding function; the branch is chosen by v."""
    if v <= Fraction(4045, 100000):
        return x >= v / Fraction(1292, 100)
    return x ** 5 >= ((v + Fraction(55, 1000)) / Fraction(1055, 1000)) ** 12


def f32(bits: int) -> Fraction:
    return Fraction(struct.unpack("<f", struct.pack("<I", bits))[0])


def smallest_binary32_at_least_eotf(v: Fraction) -> int:
    """The bits of the smallest positive binary32 x with x >= EOTF(v), by bisection over the (ordered) bit patterns of [+0, 1.0f]."""
    lo, hi = 0, 0x3F800000  # f32(lo) fails for v > 0, f32(hi) = 1 holds for v <= 1
    assert not at_least_eotf(f32(lo), v) and at_least_eotf(f32(hi), v)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if at_least_eotf(f32(mid), v):
            hi = mid
        else:
            lo = mid
    return hi


def tables():
    m = [smallest_binary32_at_least_eotf(Fraction(2 * c - 1, 510)) for c in range(1, 256)]
    l = [0] + [smallest_binary32_at_least_eotf(Fraction(c, 255)) for c in range(1, 256)]
    return m, l


def hexfloat(bits: int) -> str:
    if bits == 0:
        return "0x0p+0f"
    e, frac = (bits >> 23) - 127, bits & 0x7FFFFF
    assert bits >> 23 > 0, "no entry is subnormal"
    return "0x1.%06xp%+df" % (frac << 1, e) if frac else "0x1p%+df" % e


def macro(name: str, bits) -> str:
    rows = [", ".join(hexfloat(b) for b in bits[i:i + 8]) for i in range(0, len(bits), 8)]
    return "#define %s { \\\n  %s }" % (name, ", \\\n  ".join(rows))


def digest(bits) -> str:
    return hashlib.sha256(b"".join(struct.pack("<I", b) for b in bits)).hexdigest()


def main():
    m, l = tables()
    text = macro("PT_SRGB8_THRESHOLDS", m) + "\n" + macro("PT_SRGB8_LEVELS", l)
    if "--check" in sys.argv:
        have = HEADER.read_text()
        ok = all(part in have for part in text.split("\n#define"))
        print("pt_encode.h holds the derived tables" if ok else "pt_encode.h DIFFERS from the derived tables")
        sys.exit(0 if ok else 1)
    print(text)
    print("/* sha256: M %s, L %s */" % (digest(m)[:16], digest(l)[:16]), file=sys.stderr)


if __name__ == "__main__":
    main()
