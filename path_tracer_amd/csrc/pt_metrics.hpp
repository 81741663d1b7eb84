// pt_metrics.hpp — the image error's kernels (include/pt_metrics.h: pt_image_error).  Included by pt_render.hip inside its anonymous
// namespace, after pt_spatial_variance.hpp.
//
// imgerr_accumulate_kernel<LDS>: one thread per pixel and trip, 256 threads, a grid-stride walk over the rectangle (over the whole frame
// where an error plane is written).  A pixel that takes part makes nine binary64 terms — sq, ab, rel per channel — and adds each to its
// accumulator: PT_IMAGE_ERROR_WORDS 64-bit words, word j weighing 2^(32 j - 1074).  A term's significand m (53 bits, the hidden one
// included) stands at bit s = max(e, 1) - 1 of that number (e the biased exponent), so m << (s mod 32) is at most 84 bits: three chunks
// < 2^32 for the words s / 32, s / 32 + 1 and s / 32 + 2, each added with ONE integer atomic; a chunk of zero adds nothing.  Integer adds
// commute: the words hold the same bits whatever the order, the grid or the path.  No word can overflow (the header has the bound).
//
// LDS: a workgroup keeps IMGERR_COPIES copies of the nine accumulators in LDS, a lane adding to copy (lane mod IMGERR_COPIES) with
// ds_add_u64.  The terms of an image lie within a few binades, so nearly every lane of a wave adds to the SAME two or three words: one
// copy would serialise 64 lanes on one address, eight copies — consecutive 8-byte slots, sixteen different banks — leave eight.  At the
// end the workgroup sums the copies and adds the words that are not zero (a handful) to `scratch` with 64-bit global atomics.
// !LDS (PT_IMAGE_ERROR_NO_LDS): every chunk goes to `scratch` with a global atomic — the same words.
// The largest |d| is kept per lane in a register across the trips and the counts per wave in scalar registers (ballots), as svar_kernel
// keeps its counts; both reach `scratch` with integer max / add atomics once per workgroup (!LDS: per lane / wave).
//
// imgerr_finish_kernel: one wave.  Lane s < 9 owns accumulator s, staged in LDS: it propagates the carries (every word then holds 32
// bits), finds the leading bit, takes the 53 bits from there, rounds to nearest even on the guard bit and the OR of everything below,
// and stores the binary64 bits; lanes 9 and 10 store the counts and the maxima.
#ifndef PT_IMGERR_MAX_BLOCKS
#define PT_IMGERR_MAX_BLOCKS 1024 /* 4 workgroups per CU: what a CU's 160 KiB of LDS hold of the accumulating kernel's 39 KiB */
#endif
enum { IMGERR_WORDS = PT_IMAGE_ERROR_WORDS, IMGERR_SUMS = PT_IMAGE_ERROR_SUMS, IMGERR_ACC_WORDS = IMGERR_SUMS * IMGERR_WORDS,
       IMGERR_COPIES = 8,
       IMGERR_MAX_AT = IMGERR_ACC_WORDS,        // scratch words: the accumulators, then max_abs bits x 3, pixels, skipped
       IMGERR_PIXELS_AT = IMGERR_MAX_AT + 3, IMGERR_SKIPPED_AT = IMGERR_PIXELS_AT + 1, IMGERR_SCRATCH_WORDS = IMGERR_SKIPPED_AT + 1 };
static_assert(IMGERR_WORDS == 68 && IMGERR_SUMS == 9, "imgerr_finish_kernel gives lane s < 9 the 68 words of accumulator s");
static_assert(sizeof(PtImageErrorResult) == 104 && offsetof(PtImageErrorResult, pixels) == 72 && offsetof(PtImageErrorResult, max_abs) == 88,
              "imgerr_finish_kernel stores the result as 64-bit words 0 ... 8 (the sums), 9, 10 (the counts) and 32-bit words 22 ... 25");

struct ImgErrArgs {
  const float* a;              // [height][width][3]
  const float* ref;            // may be a
  float* plane;                // or NULL: [height][width]
  unsigned long long* scratch; // IMGERR_SCRATCH_WORDS words, zeroed on the stream before the launch
  int width;
  int x0, y0, x1, y1;          // the rectangle (never the four zeros: resolved by the host)
  int wx0, wy0, ww;            // the walk: the rectangle, or the whole frame where a plane is written; ww its width
  unsigned n;                  // the walk's pixels, <= 2^30
  double eps;
};

// Adds the term t >= 0 (finite) to the accumulator whose word j is acc[j * STRIDE].
template <bool LDS>
__device__ __forceinline__ void imgerr_add(unsigned long long* acc, double t) {
  constexpr int STRIDE = LDS ? IMGERR_COPIES : 1;
  const unsigned long long b = (unsigned long long)__double_as_longlong(t);
  const unsigned e = (unsigned)(b >> 52); // (the sign is 0)
  unsigned long long m = b & ((1ull << 52) - 1);
  if (e) m |= 1ull << 52;
  const unsigned s = e ? e - 1u : 0u, r = s & 31u;
  unsigned long long* w = acc + (s >> 5) * STRIDE;
  const unsigned long long lo = m << r, hi = r ? m >> (64u - r) : 0ull; // m << r as 64 + 21 bits
  const unsigned long long c0 = lo & 0xffffffffull, c1 = lo >> 32;
  if (c0) atomicAdd(w, c0);
  if (c1) atomicAdd(w + STRIDE, c1);
  if (hi) atomicAdd(w + 2 * STRIDE, hi); // (s / 32 <= 63: word 65 at most)
}

template <bool LDS>
__global__ __launch_bounds__(256) void imgerr_accumulate_kernel(ImgErrArgs a) {
  __shared__ unsigned long long s_acc[LDS ? IMGERR_ACC_WORDS * IMGERR_COPIES : 1];
  __shared__ unsigned s_max[LDS ? 3 : 1];
  __shared__ unsigned s_count[LDS ? 2 : 1];
  if constexpr (LDS) {
    for (int i = threadIdx.x; i < IMGERR_ACC_WORDS * IMGERR_COPIES; i += 256) s_acc[i] = 0ull;
    if (threadIdx.x < 3) s_max[threadIdx.x] = 0u;
    if (threadIdx.x < 2) s_count[threadIdx.x] = 0u;
    __syncthreads();
  }
  unsigned long long* const acc = LDS ? s_acc + (threadIdx.x & (IMGERR_COPIES - 1)) : a.scratch;
  constexpr int ACC = IMGERR_WORDS * (LDS ? IMGERR_COPIES : 1); // from one accumulator to the next
  unsigned mr = 0u, mg = 0u, mb = 0u;         // the lane's largest fabsf(d), as bits (ordered like the values: they are >= +0)
  unsigned wave_pixels = 0u, wave_skipped = 0u; // wave-uniform
  const unsigned stride = gridDim.x * 256u;
  for (unsigned base = blockIdx.x * 256u; base < a.n; base += stride) { // (base < 2^30 + 2^18: no wrap; the trip count is the workgroup's)
    const unsigned i = base + threadIdx.x;
    bool part = false, skip = false;
    if (i < a.n) {
      const int x = a.wx0 + (int)(i % (unsigned)a.ww), y = a.wy0 + (int)(i / (unsigned)a.ww);
      const long long p = (long long)y * a.width + x;
      float e = __builtin_inff();
      if (x >= a.x0 && x < a.x1 && y >= a.y0 && y < a.y1) {
        const float rr = a.ref[p * 3], rg = a.ref[p * 3 + 1], rb = a.ref[p * 3 + 2];
        const float dr = a.a[p * 3] - rr, dg = a.a[p * 3 + 1] - rg, db = a.a[p * 3 + 2] - rb;
        // a finite difference has finite operands (inf - x is inf or NaN, NaN - x is NaN): the three tests are the header's nine
        part = fabsf(dr) < __builtin_inff() && fabsf(dg) < __builtin_inff() && fabsf(db) < __builtin_inff();
        skip = !part;
        if (part) {
          e = ((dr * dr + dg * dg) + db * db) / 3.0f;
          const float d[3] = {dr, dg, db}, r[3] = {rr, rg, rb};
#pragma unroll
          for (int ch = 0; ch < 3; ch++) {
            const double dd = (double)d[ch], rd = (double)r[ch];
            const double sq = dd * dd, ab = fabs(dd);
            const double rel = sq / (rd * rd + a.eps);
            imgerr_add<LDS>(acc + ch * ACC, sq);
            imgerr_add<LDS>(acc + (3 + ch) * ACC, ab);
            imgerr_add<LDS>(acc + (6 + ch) * ACC, rel);
          }
          mr = max(mr, __float_as_uint(fabsf(dr))); mg = max(mg, __float_as_uint(fabsf(dg))); mb = max(mb, __float_as_uint(fabsf(db)));
        }
      }
      if (a.plane) a.plane[p] = e;
    }
    wave_pixels += (unsigned)__popcll(__ballot(part)); // (no early exit above: every lane of a wave reaches the ballots)
    wave_skipped += (unsigned)__popcll(__ballot(skip));
  }
  unsigned long long* const g = a.scratch;
  if constexpr (LDS) {
    if (mr) atomicMax(&s_max[0], mr);
    if (mg) atomicMax(&s_max[1], mg);
    if (mb) atomicMax(&s_max[2], mb);
    if ((threadIdx.x & 63) == 0) {
      if (wave_pixels) atomicAdd(&s_count[0], wave_pixels);
      if (wave_skipped) atomicAdd(&s_count[1], wave_skipped);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < IMGERR_ACC_WORDS; i += 256) {
      unsigned long long v = 0ull; // (the copies of a word add up to at most what the frame's bound allows the word itself)
#pragma unroll
      for (int c = 0; c < IMGERR_COPIES; c++) v += s_acc[i * IMGERR_COPIES + c];
      if (v) atomicAdd(g + i, v);
    }
    if (threadIdx.x < 3 && s_max[threadIdx.x]) atomicMax(g + IMGERR_MAX_AT + threadIdx.x, (unsigned long long)s_max[threadIdx.x]);
    if (threadIdx.x < 2 && s_count[threadIdx.x]) atomicAdd(g + IMGERR_PIXELS_AT + threadIdx.x, (unsigned long long)s_count[threadIdx.x]);
  } else {
    if (mr) atomicMax(g + IMGERR_MAX_AT, (unsigned long long)mr);
    if (mg) atomicMax(g + IMGERR_MAX_AT + 1, (unsigned long long)mg);
    if (mb) atomicMax(g + IMGERR_MAX_AT + 2, (unsigned long long)mb);
    if ((threadIdx.x & 63) == 0) {
      if (wave_pixels) atomicAdd(g + IMGERR_PIXELS_AT, (unsigned long long)wave_pixels);
      if (wave_skipped) atomicAdd(g + IMGERR_SKIPPED_AT, (unsigned long long)wave_skipped);
    }
  }
}

// The words w[0 ... 67] of one accumulator (each below 2^62) as ONE number of units 2^-1074, rounded once to binary64, nearest-even: its bits.
__device__ unsigned long long imgerr_round(unsigned long long* w) {
  unsigned long long carry = 0ull;
  int top = -1;
  for (int j = 0; j < IMGERR_WORDS; j++) {
    const unsigned long long v = w[j] + carry;
    w[j] = v & 0xffffffffull;
    carry = v >> 32;
    if (w[j]) top = j;
  } // (carry is 0 here: the last word a carry can reach is 66)
  if (top < 0) return 0ull; // +0
  const int lead = 32 * top + (31 - __clz((int)(unsigned)w[top])); // the leading bit
  if (lead <= 52) return w[0] | (w[1] << 32); // a subnormal, or a normal of the first binade: the number IS its bits, exactly
  const int sh = lead - 52;                   // the 53 bits from `lead` down start at bit sh; the biased exponent is sh + 1
  if (sh >= 2046) return 0x7ff0000000000000ull; // at or above 2^1024: +inf
  const int j0 = sh >> 5, r = sh & 31;          // (j0 <= 63: j0 + 2 is a word)
  const unsigned long long lo = w[j0] | (w[j0 + 1] << 32), hi = w[j0 + 2];
  const unsigned long long q = (r ? (lo >> r) | (hi << (64 - r)) : lo) & ((1ull << 53) - 1); // bit 52 is the leading bit
  const int gj = (sh - 1) >> 5, gr = (sh - 1) & 31; // the guard bit
  const bool guard = (w[gj] >> gr) & 1ull;
  bool sticky = (w[gj] & ((1ull << gr) - 1)) != 0ull;
  for (int j = 0; j < gj; j++) sticky = sticky || w[j] != 0ull;
  unsigned long long bits = ((unsigned long long)sh << 52) + q; // q's bit 52 makes the exponent field sh + 1
  if (guard && (sticky || (q & 1ull))) bits += 1ull;            // (a carry out of the significand is the next binade, or +inf, as it should be)
  return bits;
}

__global__ __launch_bounds__(64) void imgerr_finish_kernel(const unsigned long long* scratch, PtImageErrorResult* result) {
  __shared__ unsigned long long s_w[IMGERR_ACC_WORDS];
  for (int i = threadIdx.x; i < IMGERR_ACC_WORDS; i += 64) s_w[i] = scratch[i];
  __syncthreads();
  unsigned long long* const out64 = reinterpret_cast<unsigned long long*>(result);
  unsigned* const out32 = reinterpret_cast<unsigned*>(result);
  const int t = threadIdx.x;
  if (t < IMGERR_SUMS) out64[t] = imgerr_round(s_w + t * IMGERR_WORDS);
  else if (t == 9) out64[9] = scratch[IMGERR_PIXELS_AT];
  else if (t == 10) out64[10] = scratch[IMGERR_SKIPPED_AT];
  else if (t < 14) out32[22 + (t - 11)] = (unsigned)scratch[IMGERR_MAX_AT + (t - 11)];
  else if (t == 14) out32[25] = 0u;
}
