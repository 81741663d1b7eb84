/* The two forms of the slab pool's per-entry test (path_tracer_amd/csrc/pt_device.hpp: slab_chunk_pass), stated side by side in portable C and
 * compared bit for bit: L (the entry bound the key is made of), the candidate decision `L <= exit`, and the key.
 *
 *   scalar form          a = fma(lo, y, om), b = fma(hi, y, op), om = (0 - (o + S)) y, op = (0 - (o - S)) y;
 *                        entry = max over the axes of min(a, b), exit = min over the axes of max(a, b)
 *   sign-resolved form   (near, far) = y < 0 ? (hi, lo) : (lo, hi) — what the octant table holds for the lane's direction octant;
 *                        An = (o + copysign(S, y)) (-y), Af = (o - copysign(S, y)) (-y);
 *                        entry = max over the axes of fma(near, y, An), exit = min over the axes of fma(far, y, Af)
 *   both                 S = fma(|o|, 9u, 7u B), y = RN(1 / d), L = max(entry, PT_TMIN), candidate iff L <= exit, key = (L & ~15) | j
 *
 * The signs of zeros in a, b, entry and exit may differ between the forms (the comment above the pass says where); L, the decision and the
 * key may not.  Inputs: regular rays (2^-40 <= |d_c| <= 2^40, |o_c| <= 2^60), lo <= hi, B >= every |coordinate|:
 *   - argv[1] random cases (default 10^8), half of them on a small lattice with the origin often ON a bound (the renderer's bounce rays),
 *     half with exponents spread over the guarded range;
 *   - an enumerated set: lo == hi (a rect), bounds equal to the origin, |d| at 2^-40 and 2^40 and next to them, origins and bounds of +0
 *     and -0, huge and tiny coordinates, every one of the eight direction octants for each; and the all-NaN pad entry.
 * Prints the counts and "ok", or the first counter-example.   gcc -O2 -ffp-contract=off [-fopenmp] slab_forms_main.c -lm
 * (stand-alone: it may also be built with -fsanitize=address,undefined) */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define PT_TMIN 0.001f

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

typedef struct { float lo[3], hi[3], o[3], d[3], B; int j; } Case;
typedef struct { uint32_t L, key; int cand; } Out;

static Out finish(float entry, float exit_, int j) {
  Out r;
  const float L = fmaxf(entry, PT_TMIN);
  r.L = bits(L);
  r.cand = L <= exit_;
  r.key = (bits(L) & ~15u) | ((uint32_t)j & 15u);
  return r;
}

static float shift(float o, float B) { return fmaf(fabsf(o), 0x1.2p-21f, 0x1.cp-22f * B); }

static Out scalar_form(const Case* c) {
  float a[3], b[3];
  for (int k = 0; k < 3; k++) {
    const float y = 1.0f / c->d[k], S = shift(c->o[k], c->B);
    const float om = (0.0f - (c->o[k] + S)) * y, op = (0.0f - (c->o[k] - S)) * y;
    a[k] = fmaf(c->lo[k], y, om);
    b[k] = fmaf(c->hi[k], y, op);
  }
  const float tn = fmaxf(fmaxf(fminf(a[0], b[0]), fminf(a[1], b[1])), fminf(a[2], b[2]));
  const float tf = fminf(fminf(fmaxf(a[0], b[0]), fmaxf(a[1], b[1])), fmaxf(a[2], b[2]));
  return finish(tn, tf, c->j);
}

static Out sign_form(const Case* c) {
  float n[3], f[3];
  for (int k = 0; k < 3; k++) {
    const float y = 1.0f / c->d[k], S = copysignf(shift(c->o[k], c->B), y);
    const int s = (int)(bits(y) >> 31); /* the octant's bit of this axis */
    const float near = s ? c->hi[k] : c->lo[k], far = s ? c->lo[k] : c->hi[k];
    const float An = (c->o[k] + S) * -y, Af = (c->o[k] - S) * -y;
    n[k] = fmaf(near, y, An);
    f[k] = fmaf(far, y, Af);
  }
  return finish(fmaxf(fmaxf(n[0], n[1]), n[2]), fminf(fminf(f[0], f[1]), f[2]), c->j);
}

static int check(const Case* c) {
  const Out a = scalar_form(c), b = sign_form(c);
  return a.L == b.L && a.cand == b.cand && a.key == b.key;
}

static void report(const Case* c) {
  const Out a = scalar_form(c), b = sign_form(c);
  printf("FAILED: lo (%a %a %a) hi (%a %a %a) o (%a %a %a) d (%a %a %a) B %a: scalar L %08x cand %d key %08x, sign-resolved L %08x cand %d key %08x\n",
         c->lo[0], c->lo[1], c->lo[2], c->hi[0], c->hi[1], c->hi[2], c->o[0], c->o[1], c->o[2], c->d[0], c->d[1], c->d[2], c->B,
         a.L, a.cand, a.key, b.L, b.cand, b.key);
}

static uint64_t mix(uint64_t x) { /* splitmix64: case i's stream depends on i alone */
  x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31);
}

static void set_B(Case* c) {
  float B = 0.0f;
  for (int k = 0; k < 3; k++) { B = fmaxf(B, fabsf(c->lo[k])); B = fmaxf(B, fabsf(c->hi[k])); }
  c->B = B;
}

static void random_case(uint64_t i, Case* c) {
  uint64_t s = mix(i);
  const int lattice = (int)(s & 1);
  c->j = (int)((s >> 1) & 15);
  for (int k = 0; k < 3; k++) {
    s = mix(s);
    float lo, hi, o, d;
    if (lattice) {
      lo = (float)((int)(s & 15) - 8);
      hi = lo + (float)((s >> 4) & 3); /* 0: a rect's axis */
      const int w = (int)((s >> 6) & 7);
      o = w == 0 ? lo : w == 1 ? hi : w == 2 ? (lo + hi) * 0.5f : w == 3 ? nextafterf(lo, -INFINITY) : w == 4 ? nextafterf(hi, INFINITY)
                     : (float)((int)((s >> 9) & 31) - 16) + (float)((s >> 14) & 0xffff) * 0x1p-16f;
      d = from_bits((uint32_t)(((s >> 31) & 1) << 31) | (uint32_t)((127 - 12 + ((s >> 32) % 13)) << 23) | (uint32_t)((s >> 40) & 0x7fffff)); /* 2^-12 .. 2 */
    } else {
      const float v0 = from_bits((uint32_t)(((s >> 0) & 1) << 31) | (uint32_t)((127 - 20 + ((s >> 1) % 50)) << 23) | (uint32_t)(mix(s + 1) & 0x7fffff));
      const float v1 = from_bits((uint32_t)(((s >> 8) & 1) << 31) | (uint32_t)((127 - 20 + ((s >> 9) % 50)) << 23) | (uint32_t)(mix(s + 2) & 0x7fffff));
      lo = fminf(v0, v1); hi = fmaxf(v0, v1);
      o = from_bits((uint32_t)(((s >> 16) & 1) << 31) | (uint32_t)((127 - 20 + ((s >> 17) % 50)) << 23) | (uint32_t)(mix(s + 3) & 0x7fffff));
      d = from_bits((uint32_t)(((s >> 24) & 1) << 31) | (uint32_t)((127 - 40 + ((s >> 25) % 80)) << 23) | (uint32_t)(mix(s + 4) & 0x7fffff)); /* [2^-40, 2^40) */
    }
    c->lo[k] = lo; c->hi[k] = hi; c->o[k] = o; c->d[k] = d;
  }
  set_B(c);
}

int main(int argc, char** argv) {
  const long long n_random = argc > 1 ? atoll(argv[1]) : 100000000ll;
  long long bad = 0, cands = 0;
  long long first_bad = -1;
#pragma omp parallel for schedule(static) reduction(+ : bad, cands)
  for (long long i = 0; i < n_random; i++) {
    Case c;
    random_case((uint64_t)i, &c);
    cands += scalar_form(&c).cand;
    if (!check(&c)) {
      bad++;
#pragma omp critical
      if (first_bad < 0 || i < first_bad) first_bad = i;
    }
  }
  if (bad) { Case c; random_case((uint64_t)first_bad, &c); report(&c); printf("%lld of %lld random cases differ\n", bad, n_random); return 1; }
  printf("checked %lld random cases (%lld of them candidates)\n", n_random, cands);

  /* the enumerated corners: every (lo, hi) pair with lo <= hi from V, origins from V and ON both bounds and next to them, |d| at and next to
   * the ends of the guarded range and in between, all eight octants; the three axes walk the lists at different phases */
  const float V[] = {-0.0f, 0.0f, -1.0f, 1.0f, -0.5f, 0.5f, 3.0f, -3.0f, 555.0f, -555.0f, 0x1p27f, -0x1p27f, 0x1p27f + 16.0f, 0x1p60f, -0x1p60f,
                     0x1p-126f, -0x1p-126f, 0x1p-149f, 0x1.fffffep-1f, 0x1.000002p0f};
  const float D[] = {0x1p-40f, 0x1.000002p-40f, 0x1p40f, 0x1.fffffep39f, 1.0f, 0x1.333334p-2f, 0x1.fffffep-1f, 3.0f};
  const int nv = (int)(sizeof V / sizeof V[0]), nd = (int)(sizeof D / sizeof D[0]);
  long long n_enum = 0;
  int seen[8] = {0};
  for (int i0 = 0; i0 < nv; i0++)
    for (int i1 = 0; i1 < nv; i1++) {
      if (!(V[i0] <= V[i1])) continue; /* (-0 <= +0 and +0 <= -0: both orders of the zeros are cases) */
      for (int io = 0; io < nv + 6; io++)
        for (int id = 0; id < nd; id++)
          for (int q = 0; q < 8; q++) {
            Case c;
            c.j = (i0 + io + q) & 15;
            for (int k = 0; k < 3; k++) {
              const int a = (i0 + 3 * k) % nv, b = (i1 + 3 * k) % nv;
              const float lo = V[a] <= V[b] ? V[a] : V[b], hi = V[a] <= V[b] ? V[b] : V[a];
              const int w = (io + k) % (nv + 6);
              c.lo[k] = lo; c.hi[k] = hi;
              c.o[k] = w < nv ? V[w] : w == nv ? lo : w == nv + 1 ? hi : w == nv + 2 ? nextafterf(lo, -INFINITY) : w == nv + 3 ? nextafterf(lo, INFINITY)
                       : w == nv + 4 ? nextafterf(hi, -INFINITY) : nextafterf(hi, INFINITY);
              c.d[k] = ((q >> k) & 1) ? -D[(id + k) % nd] : D[(id + k) % nd];
            }
            set_B(&c);
            int oct = 0;
            for (int k = 0; k < 3; k++) oct |= (int)(bits(1.0f / c.d[k]) >> 31) << k;
            seen[oct]++;
            n_enum++;
            if (!check(&c)) { report(&c); return 1; }
          }
    }
  for (int q = 0; q < 8; q++) if (!seen[q]) { printf("FAILED: octant %d never enumerated\n", q); return 1; }
  { /* the pad entry: NaN bounds, whatever the ray: entry = PT_TMIN, never a candidate, in both forms */
    Case c;
    random_case(12345, &c);
    for (int k = 0; k < 3; k++) { c.lo[k] = NAN; c.hi[k] = NAN; }
    const Out a = scalar_form(&c), b = sign_form(&c);
    if (!check(&c) || a.cand || b.cand || a.L != bits(PT_TMIN)) { report(&c); return 1; }
    n_enum++;
  }
  printf("checked %lld enumerated cases, all eight octants\nok\n", n_enum);
  return 0;
}
