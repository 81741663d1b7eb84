"""A binary64 model of one bounce (hit_world + emitted + scatter) and of the camera, written from the geometry and the
optics, with a worst-case rounding bound beside every continuous output and the margin of every decision on the way.

It is the yardstick the CPU oracle and the device are held to (tests/test_physics_model_cpu.py,
tests/test_gpu_physics_model.py); it shares no code with either.  Values are plain Python floats (binary64).  Wherever a
second formula exists the model uses it: the sphere's roots in the cancellation-free form q = -(b + sgn(b) sqrt(D)),
t = q/a, c/q; the triangle by plane intersection and barycentrics from the Gram matrix (one model for the Moller-Trumbore
and the Badouel strategy); the box cross-checked as three slabs (`box_slabs`); the medium as entry and exit of its solid;
Schlick's r0 from the two indices; Snell's law as "the tangential part scales by eta, the normal part restores length 1".

Error bounds.  U = 2^-24 is the unit roundoff of binary32.  Every bound has the form n * U * S (+ propagated input
bounds): S is the sum of the magnitudes of the terms that meet in the formula, so cancellation widens the bound, and n
counts the binary32 operations of the straightforward evaluation that touch those terms.  The rules, used everywhere:
    x + y, x - y      E = Ex + Ey + U |x +- y|                    (one rounding of the result; the cancellation widens the
                      bound through Ex + Ey, which stay absolute while the result shrinks: never more than n U S)
    x * y             E = |y| Ex + |x| Ey + U |x y|
    x / y             E = Ex / |y| + |x / y| Ey / |y| + U |x / y|
    dot(x, y)         E = sum(|y_i| Ex_i + |x_i| Ey_i) + 3 U sum |x_i y_i|     (a product and at most two sums per term)
    sqrt(x)           E = max deviation of sqrt over [x - Ex, x + Ex] + U sqrt(x + Ex)     (exact, not first order)
    sin, cos, log, pow5, atan2, asin, tan:  first order in the argument + 4 U |result|: the pinned set is within 1 ulp of
                      the platform's, which is within 1 ulp (= 2 U) of the true value (tests/test_math_cpu.py).
Each function states its own count next to the formula.  No constant was tuned against the code under test.

Decisions.  `Trace.decide` records, for every comparison on the path, the distance from the threshold in units of that
quantity's own bound.  A ray is decided when every margin is >= 2 (the bounds are worst case, so 1 would do; 2 is
headroom).  `bounce(..., flip=k)` re-evaluates with the k-th decision taken the other way.  A comparison of exact
quantities (bound 0) or with inf/NaN on a side has margin inf and the outcome the comparison itself gives.

Random numbers.  `xorshift32` is the model's own generator (held to tests/golden/xorshift32_kat.json).  The four samplers
are restated in binary64 from the reference's text, include/rtweekend.hpp: float_t :39-42 (the 32-bit state converted to
binary32, times 2^-32), float_t(min,max) :45-48, unit_vec :60-67, in_unit_ball :70-80, in_unit_disk :83-88.

Semantics taken from the reference's text rather than from geometry or optics (paths under include/; "README row n" is the
n-th row of "Behaviour the reference leaves undefined" in oracle/README.md, "-" where that table has no row):

    | what the model does                                                   | reference line               | README row |
    |-----------------------------------------------------------------------|------------------------------|------------|
    | the triangle's normal is cross(edge1, edge2), not normalised          | triangle.hpp:96 (:52 Badouel)| -          |
    | the medium's normal is (1,0,0) and its front_face is 1                | constant_medium.hpp:75-76    | -          |
    | a medium or triangle hit leaves u,v as the previous accepted          | triangle.hpp:96-98,          | 1          |
    |   candidate of the same hit_world left them (zero at first)           | constant_medium.hpp:72-76    |            |
    | emission is returned without the attenuation                          | render.hpp:73                | -          |
    | an image texel is scaled by the binary32 constant 1.0f/255            | texture.hpp:146              | -          |
    | the texel index truncates and clamps (NaN/negative 0, overflow last)  | texture.hpp:139-143          | 2          |
    | the sphere's u,v are the Mercator coordinates of the face-flipped     | sphere.hpp:88,100            | -          |
    |   normal, not of the outward one                                      |                              |            |
    | the medium's exit is searched from entry + 0.0001                     | constant_medium.hpp:45       | -          |
    | the medium draws its random number only when clamped entry < exit     | constant_medium.hpp:56,65    | -          |
    | a ray lying in a rectangle's plane (t = 0/0) is accepted with t = NaN | rectangle.hpp:36,40          | -          |
    | triangle parallel test: |det| < 1e-7 (Moller-Trumbore), 1e-6 (Badouel)| triangle.hpp:71, :28         | -          |
    | rectangles, triangles and media accept t == max, spheres need t < max | rectangle.hpp:36,sphere.hpp:77| -         |
    | refract(): cos clamped to 1, |1 - |perp|^2| under the root            | vec.hpp:30,33                | -          |
    | a miss returns attenuation * ((1-h) white + h (0.5,0.7,1)), h from y  | render.hpp:83-87             | -          |
    | pi is the binary32 constant of rtweekend.hpp                          | rtweekend.hpp:22             | -          |
    | a dielectric draws its random number only when it can refract         | material.hpp:80              | -          |
"""
import math

import numpy as np

from path_tracer_amd import abi

U = 2.0 ** -24
INF = math.inf
NAN = math.nan
TMIN = float(np.float32(0.001))       # render.hpp:60, a binary32 literal
MED_OFFSET = float(np.float32(0.0001))
PI32 = float(np.float32(math.pi))     # rtweekend.hpp:22
DECIDED = 2.0
TRANS = 4.0 * U                       # relative bound of a pinned transcendental's result (see above)

BOUNCE_FLOAT_FIELDS = ("t", "p", "normal", "u", "v", "color", "sc_origin", "sc_dir", "sc_time")
BOUNCE_INT_FIELDS = ("status", "hittable", "material", "front_face", "rng_state")


# ---- random numbers ---------------------------------------------------------------------------------------------------

def xorshift32(x: int) -> int:
    """Marsaglia's 32-bit xorshift with the triple (7, 1, 9) in the order right, left, right."""
    x ^= x >> 7
    x ^= (x << 1) & 0xFFFFFFFF
    x ^= x >> 9
    return x


def xorshift32_inverse(y: int) -> int:
    """The state before `y`: each of the three steps is undone by repeating its shift until it has left the word."""
    def undo_right(v, s):
        r = v
        for _ in range(32 // s + 1):
            r = v ^ (r >> s)
        return r

    def undo_left(v, s):
        r = v
        for _ in range(32 // s + 1):
            r = v ^ ((r << s) & 0xFFFFFFFF)
        return r
    return undo_right(undo_left(undo_right(y, 9), 1), 7)


class Rng:
    def __init__(self, state):
        self.s = int(state) & 0xFFFFFFFF

    def float_t(self):
        """rtweekend.hpp:39-42: exact once the state is rounded to binary32 (round to nearest even)."""
        self.s = xorshift32(self.s)
        return float(np.float32(self.s)) * 2.0 ** -32

    def range(self, lo, hi, Elo=0.0, Ehi=0.0):
        """rtweekend.hpp:45-48: lo + (hi - lo) f.  A difference, a product, a sum: E = Elo + (Elo + Ehi) f + 3 U S."""
        f = self.float_t()
        return lo + (hi - lo) * f, Elo + (Elo + Ehi) * f + 3 * U * (abs(lo) + abs(hi - lo) * f)


def sqrt_bound(x, Ex):
    """(sqrt(x), bound): the largest change of the root over [x - Ex, x + Ex], plus the root's own rounding."""
    if not (x >= 0) or not (Ex < INF):
        return (math.sqrt(x) if x >= 0 else NAN), INF
    r = math.sqrt(x)
    return r, max(math.sqrt(x + Ex) - r, r - math.sqrt(max(x - Ex, 0.0))) + U * math.sqrt(x + Ex)


def unit_vec(rng, T):
    """rtweekend.hpp:60-67."""
    x, Ex = rng.range(-1.0, 1.0)
    maxy, Em = sqrt_bound(1 - x * x, 2 * abs(x) * Ex + 2 * U)          # x*x and 1 - .: 2 U on S <= 1 + x^2 <= 2
    y, Ey = rng.range(-maxy, maxy, Em, Em)
    absz, Ez = sqrt_bound(maxy * maxy - y * y, 2 * maxy * Em + 2 * abs(y) * Ey + 2 * U * (maxy * maxy + y * y))
    up = T.decide("unit_vec > 0.5", rng.float_t(), 0.5, 0.0, "gt")
    return (x, y, absz if up else -absz), (Ex, Ey, Ez)


def in_unit_ball(rng):
    """rtweekend.hpp:70-80.  theta = 2 pi f, phi = pi f: the constant (U), the product (U), 0 + . exact."""
    r = rng.float_t()
    theta = 2 * PI32 * rng.float_t()
    phi = PI32 * rng.float_t()
    Eth, Eph = 2 * U * theta, 2 * U * phi
    sp, cp, st, ct = math.sin(phi), math.cos(phi), math.sin(theta), math.cos(theta)
    Esp, Ecp = abs(cp) * Eph + TRANS * abs(sp), abs(sp) * Eph + TRANS * abs(cp)
    Est, Ect = abs(ct) * Eth + TRANS * abs(st), abs(st) * Eth + TRANS * abs(ct)
    plan, Eplan = r * sp, r * Esp + U * abs(r * sp)
    z, Ez = r * cp, r * Ecp + U * abs(r * cp)
    x, y = plan * ct, plan * st
    return (x, y, z), (abs(ct) * Eplan + abs(plan) * Ect + U * abs(x), abs(st) * Eplan + abs(plan) * Est + U * abs(y), Ez)


def in_unit_disk(rng):
    """rtweekend.hpp:83-88."""
    x, Ex = rng.range(-1.0, 1.0)
    maxy, Em = sqrt_bound(1 - x * x, 2 * abs(x) * Ex + 2 * U)
    y, Ey = rng.range(-maxy, maxy, Em, Em)
    return (x, y), (Ex, Ey)


# ---- decisions --------------------------------------------------------------------------------------------------------

class Trace:
    """The decisions of one evaluation, in order: names and margins.  `flip` inverts the decision with that index."""

    def __init__(self, flip=None):
        self.names, self.margins, self.flip = [], [], flip
        self.info = []      # branches taken, for the comparison's floors: reflect / refract, medium scatters / passes

    def decide(self, name, x, thr, bound, op):
        if op == "gt":
            out = x > thr
        elif op == "lt":
            out = x < thr
        elif op == "ge":
            out = x >= thr
        else:
            out = x <= thr
        if x != x or thr != thr or abs(x) == INF or abs(thr) == INF:
            m = INF          # NaN compares false, inf is beyond any bound: the comparison itself decides
        elif bound == 0.0:
            m = INF          # exact quantities: the comparison itself decides, equality included
        elif bound != bound or bound == INF:
            m = 0.0
        else:
            m = abs(x - thr) / bound
        if self.flip == len(self.margins):
            out = not out
        self.names.append(name)
        self.margins.append(m)
        return out

    def borderline(self):
        return [k for k, m in enumerate(self.margins) if m < DECIDED]


# ---- small vector helpers ---------------------------------------------------------------------------------------------

def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _adot(a, b):
    return abs(a[0] * b[0]) + abs(a[1] * b[1]) + abs(a[2] * b[2])


def _dot_bound(a, Ea, b, Eb):
    return _adot(Ea, b) + _adot(a, Eb) + 3 * U * _adot(a, b)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _perm(a, b, c):
    """Sum of |a_i b_j c_k| over the six permutations: the S of a triple product, whatever its association."""
    a, b, c = [abs(x) for x in a], [abs(x) for x in b], [abs(x) for x in c]
    return (a[0] * (b[1] * c[2] + b[2] * c[1]) + a[1] * (b[0] * c[2] + b[2] * c[0]) + a[2] * (b[0] * c[1] + b[1] * c[0]))


def _triple_bound(a, Ea, b, Eb, c, Ec):
    """A triple product a . (b x c) in any association: per term two products, a difference (cross) and at most two sums
    (dot): 5 U on the six-term S, plus the three inputs' bounds to first order."""
    return 5 * U * _perm(a, b, c) + _perm(Ea, b, c) + _perm(a, Eb, c) + _perm(a, b, Ec)


def _at(o, d, t, Et):
    """o + t d per component: a product (U |t d|) and a sum (U |p|)."""
    p = (o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2])
    return p, (abs(d[0]) * Et + U * abs(t * d[0]) + U * abs(p[0]), abs(d[1]) * Et + U * abs(t * d[1]) + U * abs(p[1]),
               abs(d[2]) * Et + U * abs(t * d[2]) + U * abs(p[2]))


def _unit(d):
    """d / |d|: dot (3 U relative, all terms positive), root (half of it, + U), quotient (U): under 4 U relative."""
    ln = math.sqrt(_dot(d, d))
    ud = tuple(x / ln for x in d)
    return ud, tuple(4 * U * abs(x) for x in ud), ln


# ---- the scene as Python numbers --------------------------------------------------------------------------------------

class Scene:
    def __init__(self, ps):
        self.h = [(h.kind, h.material, h.boundary_kind, h.strategy, tuple(float(x) for x in h.f))
                  for h in (ps.hittables[i] for i in range(ps.n_hittables))]
        self.m = [(m.kind, m.texture, tuple(float(x) for x in m.color), float(m.param))
                  for m in (ps.materials[i] for i in range(ps.n_materials))]
        self.t = [(t.kind, tuple(float(x) for x in t.color0), tuple(float(x) for x in t.color1), int(t.width), int(t.height),
                   int(t.offset), float(t.freq)) for t in (ps.textures[i] for i in range(ps.n_textures))]
        self.atlas = bytes(ps.atlas)
        self.has_image = any(t[0] == abi.PT_TEX_IMAGE for t in self.t)


class Hit:
    """`key` names the binary32 computation that produced t: two hits with the same key on the same ray are the same
    operations on the same inputs, so their t are equal bit for bit and a comparison between them is exact."""
    __slots__ = ("t", "Et", "p", "Ep", "n", "En", "ff", "u", "v", "Eu", "Ev", "uv", "key")

    def __init__(self):
        self.uv = False
        self.key = None


# ---- hittables --------------------------------------------------------------------------------------------------------

def _face(T, name, d, n, En):
    """front_face = the ray meets the surface against its outward normal; the record's normal faces the ray."""
    ff = T.decide(name, _dot(d, n), 0.0, _adot(d, En) + 3 * U * _adot(d, n), "lt")
    return ff, (n if ff else tuple(-x for x in n))


def sphere_centre(f, tm):
    """The centre at the ray's time, linear between the two key times, outside them too.  s = (tm - t0)/(t1 - t0): 3 U;
    s * delta with delta's own U: 5 U; the sum: U on S.  E_i = 6 U (|c0_i| + |s delta_i|)."""
    c0, c1, t0, t1 = f[0:3], f[3:6], f[7], f[8]
    if t0 == t1:
        return c0, (0.0, 0.0, 0.0)
    s = (tm - t0) / (t1 - t0)
    return (tuple(c0[i] + s * (c1[i] - c0[i]) for i in range(3)),
            tuple(6 * U * (abs(c0[i]) + abs(s * (c1[i] - c0[i]))) for i in range(3)))


def sphere_roots(T, f, o, d, tm, tag):
    """Both roots of |o + t d - c|^2 = r^2, near first, or None.  With oc = o - c: a = d.d, b = oc.d, c = oc.oc - r^2,
    D = b^2 - a c, roots (-b -+ sqrt D)/a; evaluated here as q = -(b + sgn(b) sqrt D), {q/a, c/q}.
    Bounds of the straightforward form: oc: Ec + U |oc|; a: 3 U a; b: dot rule; c: dot rule (3 U |oc|^2), the square
    (U r^2) and the difference (U |c|); D: 2|b|Eb + |c|Ea + a Ec, two products and a difference; numerator N = -b -+ sqrt D:
    Eb + Esqrt + U |N|; root: quotient rule."""
    r = f[6]
    c, Ec = sphere_centre(f, tm)
    oc = tuple(o[i] - c[i] for i in range(3))
    Eoc = tuple(Ec[i] + U * abs(oc[i]) for i in range(3))
    a = _dot(d, d)
    Ea = 3 * U * a
    b = _dot(oc, d)
    Eb = _adot(Eoc, d) + 3 * U * _adot(oc, d)
    oc2 = _dot(oc, oc)
    cc = oc2 - r * r
    Ecc = 2 * _adot(oc, Eoc) + 3 * U * oc2 + U * r * r + U * abs(cc)
    D = b * b - a * cc
    ED = 2 * abs(b) * Eb + abs(cc) * Ea + a * Ecc + U * (b * b + abs(a * cc) + abs(D))
    if not T.decide(tag + "discriminant > 0", D, 0.0, ED, "gt"):
        return None
    sq, Esq = sqrt_bound(max(D, 0.0), ED)
    q = -(b + math.copysign(sq, b))
    if q != 0.0:
        t1, t2 = q / a, cc / q
    else:
        t1 = t2 = 0.0
    near, far = min(t1, t2), max(t1, t2)
    En_ = Eb + Esq
    return (near, En_ / a + abs(near) * (Ea / a + 2 * U), far, En_ / a + abs(far) * (Ea / a + 2 * U), c, Ec, a)


def _in_range(T, tag, t, Et, mn, mx, Emx, same):
    lo = T.decide(tag + "t > min", t, mn, Et, "gt")
    hi = T.decide(tag + "t < closest", t, mx, 0.0 if same else Et + Emx, "lt")
    return lo and hi


def sphere_hit(T, f, o, d, tm, mn, mx, Emx, mxkey, tag, want_uv=True):
    roots = sphere_roots(T, f, o, d, tm, tag)
    if roots is None:
        return None
    near, Enear, far, Efar, c, Ec, _ = roots
    knear, kfar = ("sphere near", f[0:9], tm), ("sphere far", f[0:9], tm)
    if _in_range(T, tag + "near ", near, Enear, mn, mx, Emx, mxkey == knear):
        t, Et, key = near, Enear, knear
    elif _in_range(T, tag + "far ", far, Efar, mn, mx, Emx, mxkey == kfar):
        t, Et, key = far, Efar, kfar
    else:
        return None
    h = Hit()
    h.key = key
    h.t, h.Et = t, Et
    h.p, h.Ep = _at(o, d, t, Et)
    r = f[6]
    # outward normal (p - c)/r, a negative radius turning it inwards: difference, quotient
    n = tuple((h.p[i] - c[i]) / r for i in range(3))
    En = tuple((h.Ep[i] + Ec[i]) / abs(r) + 2 * U * abs(n[i]) for i in range(3))
    h.ff, h.n = _face(T, tag + "front_face", d, n, En)
    h.En = En
    if want_uv:
        x, y, z = h.n
        # u = 1 - (phi + pi)/(2 pi), phi = atan2(z, x); v = (theta + pi/2)/pi, theta = asin(y).  phi to first order in x, z;
        # the sum, the quotient and 1 - . on values <= 1 with pi's own U: under 6 U.  theta by evaluating asin at both ends.
        if x < 0:   # behind the -x axis atan2 jumps from pi to -pi with the sign of z: a decision
            z = abs(z) if T.decide(tag + "atan2 branch z >= 0", z, 0.0, En[2], "ge") else -abs(z)
        phi = math.atan2(z, x)
        Ephi =(abs(x) * En[2] + abs(z) * En[0]) / max(x * x + z * z, 1e-300) + TRANS * abs(phi)
        h.u, h.Eu = 1 - (phi + math.pi) / (2 * math.pi), Ephi / (2 * math.pi) + 6 * U
        if T.decide(tag + "|normal.y| <= 1", abs(y), 1.0, En[1], "le"):
            yc = min(max(y, -1.0), 1.0)
            th = math.asin(yc)
            Eth = max(abs(math.asin(min(yc + En[1], 1.0)) - th), abs(th - math.asin(max(yc - En[1], -1.0)))) + TRANS * abs(th)
            h.v, h.Ev = (th + math.pi / 2) / math.pi, Eth / math.pi + 4 * U
        else:
            h.v, h.Ev = NAN, 0.0   # asin of a rounded |y| > 1
        h.uv = True
    return h


_RECT_AXES = {0: (2, 0, 1), 1: (1, 0, 2), 2: (0, 1, 2)}   # plane axis, first and second in-plane axis of xy, xz, yz


def rect_hit(T, axis, a0, a1, b0, b1, k, o, d, mn, mx, Emx, mxkey, tag, Emn=0.0):
    """The plane's t = (k - o_k)/d_k: a difference and a quotient of exact inputs, Et = 2 U |t|.  In-plane
    coordinates o + t d by `_at`'s rule; u = (a - a0)/(a1 - a0): difference, difference, quotient."""
    ik, ia, ib = _RECT_AXES[axis]
    if d[ik] == 0.0:
        t = NAN if k == o[ik] else math.copysign(INF, k - o[ik])
        Et = 0.0
    else:
        t = (k - o[ik]) / d[ik]
        Et = 2 * U * abs(t)
    key = ("plane", ik, k)
    if T.decide(tag + "t < min", t, mn, Et + Emn, "lt") or T.decide(tag + "t > closest", t, mx, 0.0 if key == mxkey else Et + Emx, "gt"):
        return None
    a, b = o[ia] + t * d[ia], o[ib] + t * d[ib]
    Ea = abs(d[ia]) * Et + U * abs(t * d[ia]) + U * abs(a)
    Eb = abs(d[ib]) * Et + U * abs(t * d[ib]) + U * abs(b)
    if (T.decide(tag + "a < a0", a, a0, Ea, "lt") or T.decide(tag + "a > a1", a, a1, Ea, "gt")
            or T.decide(tag + "b < b0", b, b0, Eb, "lt") or T.decide(tag + "b > b1", b, b1, Eb, "gt")):
        return None
    h = Hit()
    h.key = key
    h.t, h.Et = t, Et
    h.p, h.Ep = _at(o, d, t, Et)
    n = [0.0, 0.0, 0.0]
    n[ik] = 1.0
    h.ff = d[ik] < 0          # d . n is d_k exactly: no margin
    h.n, h.En = (tuple(n) if h.ff else tuple(-x for x in n)), (0.0, 0.0, 0.0)
    h.u, h.Eu = (a - a0) / (a1 - a0), Ea / abs(a1 - a0) + 3 * U * abs((a - a0) / (a1 - a0))
    h.v, h.Ev = (b - b0) / (b1 - b0), Eb / abs(b1 - b0) + 3 * U * abs((b - b0) / (b1 - b0))
    h.uv = True
    return h


def box_hit(T, f, o, d, mn, mx, Emx, mxkey, tag, Emn=0.0):
    """The nearest of the six faces the ray meets within the range: each face is its plane cut to the other two extents."""
    lo, hi = f[0:3], f[3:6]
    best = None
    for axis, ik in ((0, 2), (1, 1), (2, 0)):
        _, ia, ib = _RECT_AXES[axis]
        for k in (hi[ik], lo[ik]):
            h = rect_hit(T, axis, lo[ia], hi[ia], lo[ib], hi[ib], k, o, d, mn, mx, Emx, mxkey, f"{tag}face{axis}{'+' if k == hi[ik] else '-'} ", Emn)
            if h is not None:
                best, mx, Emx, mxkey = h, h.t, h.Et, h.key
    return best


def box_slabs(f, o, d):
    """(t_enter, t_exit) of the line through the box as the intersection of three slabs, or None: the cross-check of
    `box_hit` (compare() asserts that a decided box hit lies at one of the two)."""
    t0, t1 = -INF, INF
    for i in range(3):
        if d[i] == 0.0:
            if not (f[i] <= o[i] <= f[3 + i]):
                return None
            continue
        a, b = (f[i] - o[i]) / d[i], (f[3 + i] - o[i]) / d[i]
        t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
    return (t0, t1) if t0 <= t1 else None


def triangle_hit(T, f, strategy, o, d, mn, mx, Emx, mxkey, tag):
    """The ray meets the plane through v0 with normal n = e1 x e2 at t = n.(v0 - o) / n.d; the point w = o + t d - v0 has
    barycentrics (beta, gamma) solving the Gram system [e1.e1 e1.e2; e1.e2 e2.e2] (beta, gamma) = (w.e1, w.e2); inside is
    beta >= 0, gamma >= 0, beta + gamma <= 1.
    Bounds.  Moller-Trumbore evaluates t, beta, gamma as quotients of triple products of (o - v0, d, e1, e2) by
    det = -n.d: `_triple_bound` for each, then the quotient rule.  Badouel evaluates t the same way and the barycentrics
    through the hit point: w = p - v0 (`_at`, a difference), the five dots (dot rule), the 2x2 determinants (two products
    and a difference: 2 U S + inputs) and a quotient."""
    v0, e1, e2, n, C12, g11, g12, g22, G, En, E11, E12, E22, EG = _triangle_constants(f)
    det = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
    ad = (abs(d[0]), abs(d[1]), abs(d[2]))
    # d exact, the edges with their own U: (5 + 1 + 1) U on the permanent |d| . C12
    Edet = 7 * U * (ad[0] * C12[0] + ad[1] * C12[1] + ad[2] * C12[2])
    eps = 1e-6 if strategy == abi.PT_TRI_BADOUEL else 1e-7
    if T.decide(tag + "|det| < epsilon", abs(det), eps, Edet + U * eps, "lt"):
        return None
    s = (o[0] - v0[0], o[1] - v0[1], o[2] - v0[2])
    as_ = (abs(s[0]), abs(s[1]), abs(s[2]))
    adet = abs(det)
    t = -(n[0] * s[0] + n[1] * s[1] + n[2] * s[2]) / det
    # o - v0 with its own U as well: 8 U on the permanent |s| . C12
    Et = 8 * U * (as_[0] * C12[0] + as_[1] * C12[1] + as_[2] * C12[2]) / adet + abs(t) * Edet / adet + U * abs(t)
    key = ("triangle", f[0:9], strategy)
    Ecl = 0.0 if key == mxkey else Et + Emx
    p = (o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2])
    w = (p[0] - v0[0], p[1] - v0[1], p[2] - v0[2])
    w1, w2 = _dot(w, e1), _dot(w, e2)
    beta, gamma = (g22 * w1 - g12 * w2) / G, (g11 * w2 - g12 * w1) / G
    if strategy == abi.PT_TRI_BADOUEL:
        Ee1, Ee2 = tuple(U * abs(x) for x in e1), tuple(U * abs(x) for x in e2)
        Ep = _at(o, d, t, Et)[1]
        Ew = tuple(Ep[i] + U * abs(w[i]) for i in range(3))
        Ew1, Ew2 = _dot_bound(w, Ew, e1, Ee1), _dot_bound(w, Ew, e2, Ee2)
        Ebn = g22 * Ew1 + abs(w1) * E22 + abs(g12) * Ew2 + abs(w2) * E12 + 2 * U * (abs(g22 * w1) + abs(g12 * w2))
        Egn = g11 * Ew2 + abs(w2) * E11 + abs(g12) * Ew1 + abs(w1) * E12 + 2 * U * (abs(g11 * w2) + abs(g12 * w1))
        Ebeta = Ebn / G + abs(beta) * EG / G + U * abs(beta)
        Egamma = Egn / G + abs(gamma) * EG / G + U * abs(gamma)
        # order of the reference's tests: plane range first (negative t, then the range), then the barycentrics
        if T.decide(tag + "t < 0", t, 0.0, Et, "lt"):
            return None
        if T.decide(tag + "t < min", t, mn, Et, "lt") or T.decide(tag + "t > closest", t, mx, Ecl, "gt"):
            return None
        range_first = True
    else:
        # triple products of (s, d, e): 7 U on the permanent, whose |s| x |d| part is shared
        SD = (as_[1] * ad[2] + as_[2] * ad[1], as_[2] * ad[0] + as_[0] * ad[2], as_[0] * ad[1] + as_[1] * ad[0])
        Ebeta = 7 * U * _adot(SD, e2) / adet + abs(beta) * Edet / adet + U * abs(beta)
        Egamma = 7 * U * _adot(SD, e1) / adet + abs(gamma) * Edet / adet + U * abs(gamma)
        range_first = False
    if (T.decide(tag + "beta < 0", beta, 0.0, Ebeta, "lt") or T.decide(tag + "beta > 1", beta, 1.0, Ebeta, "gt")
            or T.decide(tag + "gamma < 0", gamma, 0.0, Egamma, "lt")
            or T.decide(tag + "beta + gamma > 1", beta + gamma, 1.0, Ebeta + Egamma + U * abs(beta + gamma), "gt")):
        return None
    if not range_first:
        if T.decide(tag + "t < min", t, mn, Et, "lt") or T.decide(tag + "t > closest", t, mx, Ecl, "gt"):
            return None
    h = Hit()
    h.key = key
    h.t, h.Et = t, Et
    h.p, h.Ep = _at(o, d, t, Et)
    h.ff, h.n = _face(T, tag + "front_face", d, n, En)
    h.En = En
    return h


_TRIANGLES = {}


def _triangle_constants(f):
    """What depends on the triangle alone: edges (a difference each: U |e|), normal, C12_i = |e1_j e2_k| + |e1_k e2_j| (the
    edge part of every permanent), the Gram matrix and, for Badouel, its bounds; the normal's bound per component: two
    products and a difference (2 U S) + the edges' own U (another 2 U S)."""
    c = _TRIANGLES.get(f)
    if c is None:
        v0, v1, v2 = f[0:3], f[3:6], f[6:9]
        e1 = tuple(v1[i] - v0[i] for i in range(3))
        e2 = tuple(v2[i] - v0[i] for i in range(3))
        Ee1, Ee2 = tuple(U * abs(x) for x in e1), tuple(U * abs(x) for x in e2)
        C12 = tuple(abs(e1[j] * e2[k]) + abs(e1[k] * e2[j]) for j, k in ((1, 2), (2, 0), (0, 1)))
        g11, g12, g22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
        E11, E12, E22 = _dot_bound(e1, Ee1, e1, Ee1), _dot_bound(e1, Ee1, e2, Ee2), _dot_bound(e2, Ee2, e2, Ee2)
        EG = g22 * E11 + g11 * E22 + 2 * abs(g12) * E12 + 2 * U * (g11 * g22 + g12 * g12)
        c = _TRIANGLES[f] = (v0, e1, e2, _cross(e1, e2), C12, g11, g12, g22, g11 * g22 - g12 * g12, tuple(4 * U * x for x in C12),
                             E11, E12, E22, EG)
    return c


def medium_hit(T, h, o, d, tm, mn, mx, Emx, rng, tag):  # noqa: C901
    """A homogeneous medium filling a convex solid: the ray is inside between entry and exit; the free path is
    -ln(xi)/density along the ray; it scatters if that is no longer than the stretch inside (clamped to the range).
    t = entry + path/|d|.  |d|: 3 U relative (dot, root); stretch * |d|: the two clamped ends' bounds, a difference, a
    product; path = (-1/density) ln xi: the logarithm's 4 U and a product; t: quotient and sum."""
    _, _, bkind, _, f = h
    if bkind == abi.PT_HIT_SPHERE:
        roots = sphere_roots(T, f, o, d, tm, tag + "boundary ")
        if roots is None:
            return None
        t1, E1, t2, E2 = roots[0:4]
    else:
        first = box_hit(T, f, o, d, -INF, INF, 0.0, None, tag + "entry ")
        if first is None:
            return None
        t1, E1 = first.t, first.Et
        second = box_hit(T, f, o, d, t1 + MED_OFFSET, INF, 0.0, None, tag + "exit ", E1 + U * abs(t1 + MED_OFFSET))
        if second is None:
            return None
        t2, E2 = second.t, second.Et
    if bkind == abi.PT_HIT_SPHERE and not T.decide(tag + "exit > entry + offset", t2, t1 + MED_OFFSET, E1 + E2 + U * abs(t1), "gt"):
        return None
    if T.decide(tag + "entry < min", t1, mn, E1, "lt"):
        t1, E1 = mn, 0.0
    if T.decide(tag + "exit > closest", t2, mx, E2 + Emx, "gt"):
        t2, E2 = mx, Emx
    if T.decide(tag + "entry >= exit", t1, t2, E1 + E2, "ge"):
        return None
    t1 = max(t1, 0.0)
    ln = math.sqrt(_dot(d, d))
    inside = (t2 - t1) * ln
    Einside = (E1 + E2 + U * abs(t2 - t1)) * ln + 4 * U * abs(inside)
    xi = rng.float_t()
    lg = math.log(xi) if xi > 0 else -INF
    path = f[9] * lg                    # f[9] is -1/density as the scene table carries it
    Epath = TRANS * abs(path) + U * abs(path)
    if T.decide(tag + "path > inside", path, inside, Epath + Einside, "gt"):
        T.info.append("medium passes")
        return None
    T.info.append("medium scatters")
    r = Hit()
    r.t = t1 + path / ln
    r.Et = E1 + (Epath + 4 * U * abs(path)) / ln + U * abs(r.t)
    r.p, r.Ep = _at(o, d, r.t, r.Et)
    r.n, r.En, r.ff = (1.0, 0.0, 0.0), (0.0, 0.0, 0.0), True
    return r


# ---- textures and materials -------------------------------------------------------------------------------------------

def _texel(T, tag, coord, Ecoord, freq, size, flipv):
    """Index along one axis: frac(coord * freq) * (size - 1), truncated.  Two decisions: coord * freq against the nearest
    integer (where frac wraps) and the scaled coordinate against the nearest integer (where the index steps)."""
    if coord != coord:
        return 0
    x = coord * freq
    Ex = abs(freq) * Ecoord + U * abs(x)
    near = round(x)
    below = T.decide(tag + "coord*freq < integer", x, float(near), Ex, "lt")
    fr = x - (near - 1 if below else near)          # frac on the decided side of the integer
    fr = min(max(fr, 0.0), 1.0)
    if flipv:
        c, Ec = (1 - fr) * (size - 1), (Ex + U) * (size - 1) + U * (1 - fr) * (size - 1)
    else:
        c, Ec = fr * (size - 1), Ex * (size - 1) + U * fr * (size - 1)
    near = round(c)
    idx = near - 1 if T.decide(tag + "texel < integer", c, float(near), Ec, "lt") else near
    return min(max(idx, 0), size - 1)


def texture_value(T, sc, tex, h, tag):
    """(colour, bound per channel)"""
    kind, c0, c1, w, hh, off, freq = sc.t[tex]
    if kind == abi.PT_TEX_SOLID:
        return c0, (0.0, 0.0, 0.0)
    if kind == abi.PT_TEX_CHECKER:
        # sin(10 x) sin(10 y) sin(10 z) < 0 picks the odd colour.  10 p: a product; sin to first order + 4 U; two products.
        s, Es = [], []
        for i in range(3):
            a = 10.0 * h.p[i]
            Ea = 10.0 * h.Ep[i] + U * abs(a)
            s.append(math.sin(a) if abs(a) < INF else NAN)
            Es.append(abs(math.cos(a)) * Ea + TRANS * abs(s[-1]) if abs(a) < INF else INF)
        prod = s[0] * s[1] * s[2]
        Eprod = Es[0] * abs(s[1] * s[2]) + Es[1] * abs(s[0] * s[2]) + Es[2] * abs(s[0] * s[1]) + 2 * U * abs(prod)
        return (c0 if T.decide(tag + "checker < 0", prod, 0.0, Eprod, "lt") else c1), (0.0, 0.0, 0.0)
    i = _texel(T, tag + "u ", h.u, h.Eu, freq, w, False)
    j = _texel(T, tag + "v ", h.v, h.Ev, freq, hh, True)
    k = (j * w + i + off) * 3
    col = tuple(sc.atlas[k + c] / 255.0 for c in range(3))
    return col, tuple(2 * U * x for x in col)       # the constant's rounding and the product


def reflect(ud, Eud, n, En):
    """Mirror: v - 2 (v.n) n.  The dot by its rule, doubled exactly; the product and the difference."""
    dn = _dot(ud, n)
    Edn = _dot_bound(ud, Eud, n, En)
    out = tuple(ud[i] - 2 * dn * n[i] for i in range(3))
    E = tuple(Eud[i] + 2 * Edn * abs(n[i]) + 2 * abs(dn) * En[i] + U * abs(2 * dn * n[i]) + U * abs(out[i]) for i in range(3))
    return out, E, dn, Edn


def scatter(T, sc, mat, d, h, att, rng):
    """-> (status, colour, Ecolour, sc_dir or None, Esc_dir)"""
    kind, tex, mcol, param = sc.m[mat]
    if kind == abi.PT_MAT_LIGHTSOURCE:
        col, Ecol = texture_value(T, sc, tex, h, "emit ")
        return abi.PT_BOUNCE_ABSORBED, col, Ecol, None, None
    if kind == abi.PT_MAT_LAMBERTIAN:
        uv, Euv = unit_vec(rng, T)
        sd = tuple(h.n[i] + uv[i] for i in range(3))
        Esd = tuple(h.En[i] + Euv[i] + U * abs(sd[i]) for i in range(3))
        col, Ecol = texture_value(T, sc, tex, h, "albedo ")
        return (abi.PT_BOUNCE_SCATTERED, tuple(att[i] * col[i] for i in range(3)),
                tuple(att[i] * Ecol[i] + U * att[i] * col[i] for i in range(3)), sd, Esd)
    if kind == abi.PT_MAT_ISOTROPIC:
        ball, Eball = in_unit_ball(rng)
        col, Ecol = texture_value(T, sc, tex, h, "albedo ")
        return (abi.PT_BOUNCE_SCATTERED, tuple(att[i] * col[i] for i in range(3)),
                tuple(att[i] * Ecol[i] + U * att[i] * col[i] for i in range(3)), ball, Eball)
    ud, Eud, _ = _unit(d)
    col = tuple(att[i] * mcol[i] for i in range(3))
    Ecol = tuple(U * abs(x) for x in col)
    if kind == abi.PT_MAT_METAL:
        refl, Erefl, _, _ = reflect(ud, Eud, h.n, h.En)
        ball, Eball = in_unit_ball(rng)
        if param == 0.0:
            sd, Esd = refl, Erefl
        else:
            sd = tuple(refl[i] + param * ball[i] for i in range(3))
            Esd = tuple(Erefl[i] + param * Eball[i] + U * abs(param * ball[i]) + U * abs(sd[i]) for i in range(3))
        if T.decide("metal dot > 0", _dot(sd, h.n), 0.0, _dot_bound(sd, Esd, h.n, h.En), "gt"):
            return abi.PT_BOUNCE_SCATTERED, col, Ecol, sd, Esd
        return abi.PT_BOUNCE_ABSORBED, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), sd, Esd
    # dielectric: Snell's law with eta = n_incident / n_transmitted, total internal reflection, Schlick's reflectance
    n1, n2 = (1.0, param) if h.ff else (param, 1.0)
    eta = n1 / n2
    Eeta = U * eta if h.ff else 0.0
    refl, Erefl, dn, Edn = reflect(ud, Eud, h.n, h.En)
    cos_i = min(-dn, 1.0)
    sin2 = 1 - cos_i * cos_i
    sin_i, Esin = sqrt_bound(max(sin2, 0.0), 2 * abs(cos_i) * Edn + 2 * U * (1 + cos_i * cos_i))
    tir = T.decide("cannot_refract", eta * sin_i, 1.0, eta * Esin + sin_i * Eeta + U * eta * sin_i, "gt")
    take_reflect = tir
    if not tir:
        # Schlick: R = r0 + (1 - r0)(1 - cos)^5, r0 = ((n1 - n2)/(n1 + n2))^2.  r0: three roundings, squared: 7 U;
        # 1 - cos: Ecos + U S; the fifth power to first order + 4 U; then a difference, a product, a sum: 3 U S.
        r0 = ((n1 - n2) / (n1 + n2)) ** 2
        Er0 = 8 * U * r0
        x = 1 - cos_i
        Ex = Edn + U * (1 + abs(cos_i))
        p5 = x ** 5
        Ep5 = 5 * x ** 4 * Ex + TRANS * p5
        R = r0 + (1 - r0) * p5
        ER = Er0 * (1 + p5) + (1 - r0) * Ep5 + 3 * U * (r0 + (1 - r0) * p5)
        take_reflect = T.decide("reflectance > xi", R, rng.float_t(), ER, "gt")
    T.info.append("reflect" if take_reflect else "refract")
    if take_reflect:
        return abi.PT_BOUNCE_SCATTERED, col, Ecol, refl, Erefl
    # the tangential part scales by eta; the normal part restores unit length (on the far side of the surface)
    inner = tuple(ud[i] + cos_i * h.n[i] for i in range(3))
    Einner = tuple(Eud[i] + abs(h.n[i]) * Edn + abs(cos_i) * h.En[i] + U * abs(cos_i * h.n[i]) + U * abs(inner[i]) for i in range(3))
    perp = tuple(eta * inner[i] for i in range(3))
    Eperp = tuple(eta * Einner[i] + abs(inner[i]) * Eeta + U * abs(perp[i]) for i in range(3))
    l2 = _dot(perp, perp)
    El2 = 2 * _adot(perp, Eperp) + 3 * U * l2
    root, Eroot = sqrt_bound(abs(1 - l2), El2 + U * (1 + l2))
    sd = tuple(perp[i] - root * h.n[i] for i in range(3))
    Esd = tuple(Eperp[i] + abs(h.n[i]) * Eroot + root * h.En[i] + U * abs(root * h.n[i]) + U * abs(sd[i]) for i in range(3))
    return abi.PT_BOUNCE_SCATTERED, col, Ecol, sd, Esd


# ---- one bounce -------------------------------------------------------------------------------------------------------

def bounce(sc: Scene, o, d, tm, state, att, flip=None):
    """-> (values, bounds, trace): dicts over the fields of PtBounceOut (vectors as tuples); a field the record leaves
    at zero is 0 with bound 0."""
    T = Trace(flip)
    rng = Rng(state)
    best, best_i = None, -1
    mx, Emx, mxkey = INF, 0.0, None
    u = v = Eu = Ev = 0.0
    for i, hh in enumerate(sc.h):
        kind, _, _, strategy, f = hh
        tag = f"h{i} "
        if kind == abi.PT_HIT_SPHERE:
            h = sphere_hit(T, f, o, d, tm, TMIN, mx, Emx, mxkey, tag, sc.has_image)
        elif kind == abi.PT_HIT_XY_RECT:
            h = rect_hit(T, 0, f[0], f[1], f[2], f[3], f[4], o, d, TMIN, mx, Emx, mxkey, tag)
        elif kind == abi.PT_HIT_XZ_RECT:
            h = rect_hit(T, 1, f[0], f[1], f[2], f[3], f[4], o, d, TMIN, mx, Emx, mxkey, tag)
        elif kind == abi.PT_HIT_YZ_RECT:
            h = rect_hit(T, 2, f[0], f[1], f[2], f[3], f[4], o, d, TMIN, mx, Emx, mxkey, tag)
        elif kind == abi.PT_HIT_TRIANGLE:
            h = triangle_hit(T, f, strategy, o, d, TMIN, mx, Emx, mxkey, tag)
        elif kind == abi.PT_HIT_BOX:
            h = box_hit(T, f, o, d, TMIN, mx, Emx, mxkey, tag)
        else:
            h = medium_hit(T, hh, o, d, tm, TMIN, mx, Emx, rng, tag)
        if h is None:
            continue
        if h.uv:
            u, v, Eu, Ev = h.u, h.v, h.Eu, h.Ev
        best, best_i, mx, Emx, mxkey = h, i, h.t, h.Et, h.key
    Z = (0.0, 0.0, 0.0)
    val = dict(status=abi.PT_BOUNCE_MISS, hittable=-1, material=-1, front_face=0, t=0.0, p=Z, normal=Z, u=0.0, v=0.0,
               color=Z, sc_origin=Z, sc_dir=Z, sc_time=0.0)
    bnd = dict(t=0.0, p=Z, normal=Z, u=0.0, v=0.0, color=Z, sc_origin=Z, sc_dir=Z, sc_time=0.0)
    if best is None:
        # the sky: h = (y/|d| + 1)/2 blends white into (0.5, 0.7, 1): Eh < 3 U; the blend: two products and a sum on
        # values <= 1 with the constants' own U; the attenuation's product
        ud, Eud, _ = _unit(d)
        hgt = 0.5 * (ud[1] + 1.0)
        Eh = 0.5 * (Eud[1] + U * (abs(ud[1]) + 1))
        sky = tuple((1 - hgt) + hgt * k for k in (0.5, float(np.float32(0.7)), 1.0))
        val["color"] = tuple(att[i] * sky[i] for i in range(3))
        bnd["color"] = tuple(att[i] * (2 * Eh + 5 * U) + U * att[i] * sky[i] for i in range(3))
    else:
        best.u, best.v, best.Eu, best.Ev = u, v, Eu, Ev
        mat = sc.h[best_i][1]
        status, col, Ecol, sd, Esd = scatter(T, sc, mat, d, best, att, rng)
        val.update(status=status, hittable=best_i, material=mat, front_face=int(best.ff), t=best.t, p=best.p, normal=best.n,
                   u=u, v=v, color=col)
        bnd.update(t=best.Et, p=best.Ep, normal=best.En, u=Eu, v=Ev, color=Ecol)
        if status == abi.PT_BOUNCE_SCATTERED:
            val.update(sc_origin=best.p, sc_dir=sd, sc_time=tm)
            bnd.update(sc_origin=best.Ep, sc_dir=Esd)
    val["rng_state"] = rng.s
    return val, bnd, T


def bounce_record(sc: Scene, rec, flip=None):
    return bounce(sc, tuple(float(x) for x in rec.origin), tuple(float(x) for x in rec.dir), float(rec.time), int(rec.rng_state),
                  tuple(float(x) for x in rec.attenuation), flip)


# ---- camera -----------------------------------------------------------------------------------------------------------

CAMERA_FIELDS = ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w", "lens_radius", "time0", "time1")


def camera(look_from, look_at, vup, vfov_deg, aspect, aperture, focus_dist, time0, time1):
    """A thin-lens camera: w points from the target to the eye, u = vup x w normalised, v = w x u; the focal plane at
    focus_dist spans 2 tan(vfov/2) focus_dist vertically and aspect times that horizontally; lower_left_corner is its
    corner.  -> (values, bounds) over the fields of PtCamera.
    Bounds: theta = vfov * pi / 180: 3 U; tan to first order + 4 U; w: a difference (U S) then `_unit` on a rounded vector;
    u likewise after a cross product (2 U S); v: a cross product of two rounded vectors; the spans: products; the corner:
    three differences of halved vectors."""
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    frm, at, up = [tuple(f32(x) for x in a) for a in (look_from, look_at, vup)]
    vfov_deg, aspect, aperture, focus_dist = f32(vfov_deg), f32(aspect), f32(aperture), f32(focus_dist)
    half = math.radians(vfov_deg) / 2
    hh = math.tan(half)
    Ehh = (1 + hh * hh) * 3 * U * half + TRANS * hh
    vh, Evh = 2 * hh, 2 * Ehh
    vw, Evw = aspect * vh, aspect * Evh + U * aspect * vh

    def unit_of(a, Ea):
        ln = math.sqrt(_dot(a, a))
        Eln = _adot(a, Ea) / ln + 3 * U * ln
        return tuple(x / ln for x in a), tuple(Ea[i] / ln + abs(a[i]) / ln * Eln / ln + U * abs(a[i]) / ln for i in range(3))

    def cross_of(a, Ea, b, Eb):
        c = _cross(a, b)
        E = tuple(2 * U * (abs(a[j] * b[k]) + abs(a[k] * b[j])) + abs(b[k]) * Ea[j] + abs(a[j]) * Eb[k] + abs(b[j]) * Ea[k]
                  + abs(a[k]) * Eb[j] for j, k in ((1, 2), (2, 0), (0, 1)))
        return c, E
    Z = (0.0, 0.0, 0.0)
    dw = tuple(frm[i] - at[i] for i in range(3))
    w, Ew = unit_of(dw, tuple(U * (abs(frm[i]) + abs(at[i])) for i in range(3)))
    cu, Ecu = cross_of(up, Z, w, Ew)
    u, Eu = unit_of(cu, Ecu)
    v, Ev = cross_of(w, Ew, u, Eu)
    kh, Ekh = focus_dist * vw, focus_dist * Evw + U * focus_dist * vw
    kv, Ekv = focus_dist * vh, focus_dist * Evh + U * focus_dist * vh
    hor = tuple(kh * x for x in u)
    Ehor = tuple(abs(u[i]) * Ekh + kh * Eu[i] + U * abs(hor[i]) for i in range(3))
    ver = tuple(kv * x for x in v)
    Ever = tuple(abs(v[i]) * Ekv + kv * Ev[i] + U * abs(ver[i]) for i in range(3))
    fw = tuple(focus_dist * x for x in w)
    llc = tuple(frm[i] - hor[i] / 2 - ver[i] / 2 - fw[i] for i in range(3))
    Ellc = tuple(Ehor[i] / 2 + Ever[i] / 2 + focus_dist * Ew[i] + U * abs(fw[i])
                 + 3 * U * (abs(frm[i]) + abs(hor[i] / 2) + abs(ver[i] / 2) + abs(fw[i])) for i in range(3))
    val = dict(origin=frm, lower_left_corner=llc, horizontal=hor, vertical=ver, u=u, v=v, w=w, lens_radius=aperture / 2,
               time0=f32(time0), time1=f32(time1))
    bnd = dict(origin=Z, lower_left_corner=Ellc, horizontal=Ehor, vertical=Ever, u=Eu, v=Ev, w=Ew, lens_radius=0.0,
               time0=0.0, time1=0.0)
    return val, bnd


def camera_ray(cam, x, y, width, height, state):
    """One primary ray of pixel (x, y) from the fields of a PtCamera: the sample lies at ((x + xi1)/W, (y + xi2)/H) of the
    focal plane, the origin is displaced over the lens disk, the time is uniform over the shutter interval.
    s, t: a sum and a quotient, 2 U; the lens offset: `in_unit_disk`, the radius' product, two products and a sum; the
    direction: five terms meet, two of them products of a rounded factor (3 U), four sums: 7 U S + the offset's bound."""
    rng = Rng(state)
    s = (x + rng.float_t()) / width
    t = (y + rng.float_t()) / height
    (dx, dy), (Edx, Edy) = in_unit_disk(rng)
    lens = float(cam.lens_radius)
    rx, ry = lens * dx, lens * dy
    Erx, Ery = lens * Edx + U * abs(rx), lens * Edy + U * abs(ry)
    cu, cv, org = [tuple(float(a) for a in q) for q in (cam.u, cam.v, cam.origin)]
    llc, hor, ver = [tuple(float(a) for a in q) for q in (cam.lower_left_corner, cam.horizontal, cam.vertical)]
    off = tuple(cu[i] * rx + cv[i] * ry for i in range(3))
    Eoff = tuple(abs(cu[i]) * Erx + abs(cv[i]) * Ery + 2 * U * (abs(cu[i] * rx) + abs(cv[i] * ry)) for i in range(3))
    origin = tuple(org[i] + off[i] for i in range(3))
    Eorigin = tuple(Eoff[i] + U * (abs(org[i]) + abs(off[i])) for i in range(3))
    dirn = tuple(llc[i] + s * hor[i] + t * ver[i] - org[i] - off[i] for i in range(3))
    Edir = tuple(Eoff[i] + 7 * U * (abs(llc[i]) + abs(s * hor[i]) + abs(t * ver[i]) + abs(org[i]) + abs(off[i])) for i in range(3))
    tm, Etm = rng.range(float(cam.time0), float(cam.time1))
    return (dict(origin=origin, dir=dirn, time=tm, rng_state=rng.s), dict(origin=Eorigin, dir=Edir, time=Etm))
