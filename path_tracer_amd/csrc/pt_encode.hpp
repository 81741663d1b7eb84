// pt_encode.hpp — the encode stage's kernel (include/pt_encode.h: pt_encode, pt_display_encode).  Included by pt_render.hip inside its
// anonymous namespace, after pt_metrics.hpp: behind display_curve / display_clamp / display_scale and quantise, which the fused
// instantiations reuse unchanged.
//
// encode_kernel<TONE, MODE, VEC>: display_apply_kernel's shape — a row is 3 * width independent values; blockIdx.x walks a row's values, 256
// lanes a workgroup; blockIdx.y walks the rows, gridDim.y apart, so no frame needs a grid dimension above the limit; the flip is in the
// store index (row 0 of rgb8 is the top).  VEC: four values per lane, one 16-byte load and one packed 4-byte store, where 3 * width is a
// multiple of 4 and the planes are aligned; !VEC: one value per lane.  12 bytes in and 3 bytes out per pixel, nothing else: memory-bound.
//   TONE  ENCODE_PLAIN: the values are encoded as they are (pt_encode); a PT_TONE_*: pt_display_apply's exposure, clamp and curve first
//         (pt_display_encode) — the very expressions of display_apply_kernel, so the same bits as its linear_out
//   MODE  ENC_REFERENCE: quantise(); ENC_SRGB: the thresholds M; ENC_DITHER: the levels L and the Bayer threshold
//
// How a lane finds its code.  The header's count "the number of j with M[j] <= x" over a sorted table is a search.  A binary search of
// 255 entries is eight DEPENDENT loads.  Here the exponent and the top ENC_KEY_BITS = 5 mantissa bits of x (clamped to [2^-13, 1), below
// which no threshold lies) index a byte table: the number of entries below that bin's lower edge.  A bin of 1/32 octave holds at most
// ENC_CMP = 3 entries of either table (static_assert below; the top octave holds 67 thresholds over 32 bins), so the code is that start
// plus ENC_CMP INDEPENDENT comparisons against the entries that follow it, the table padded with NaN (never <= x, not even for x = +inf):
// one byte load and three loads, all from LDS.  The comparisons are made with x itself, not the clamped value, so NaN (every comparison
// false, and the clamp sends it to bin 0) and negatives give 0 and values >= 1 give 255 without a branch.  A workgroup copies the one
// table its MODE needs (259 floats), the 416 start bytes and, for the dither, the 64 thresholds t to LDS once — 1.7 KiB — and then
// walks its rows.
// Counts per value: ENC_SRGB 1 + 3 LDS loads, 3 compares; ENC_DITHER 1 + 3 + 2 LDS loads (L[c], L[c + 1]) + 1 (t), two subtractions, one
// division.  4 key bits would need 5 compares, 6 bits 2 with a table of 832 bytes.  Both tables, the start bytes and their bounds are
// built from the header's macros at compile time; nothing is restated.
#ifndef PT_ENCODE_MAX_BLOCKS
#define PT_ENCODE_MAX_BLOCKS 2048 /* 8 workgroups of 256 lanes per CU: every wave slot of 256 CUs once; more rows are walked */
#endif
enum { ENCODE_PLAIN = -1 };
enum { ENC_REFERENCE = 0, ENC_SRGB = 1, ENC_DITHER = 2 };
enum { ENC_KEY_BITS = 5, ENC_KEY_SHIFT = 23 - ENC_KEY_BITS, ENC_KEY0 = (127 - 13) << ENC_KEY_BITS, // the bin of 2^-13
       ENC_KEYS = ((126 << ENC_KEY_BITS) + (1 << ENC_KEY_BITS) - 1) - ENC_KEY0 + 1,              // ... to the bin below 1.0f: 13 octaves
       ENC_CMP = 3, ENC_ROWS = 256 + ENC_CMP };

// A table as the kernel searches it: at[j] = the j-th entry that counts (M[j + 1]; L[j + 1]), then NaN (which is <= no x, +inf
// included); start[k] = the number of entries
// below the lower edge of bin k, of the first `searched` entries: the dither's table keeps L[255] as a level and never searches it.  The
// dither's levels L[0 ... 255] are at[] shifted by one with L[0] = 0 in front: L[c] = c ? at[c - 1] : 0.
struct EncTable {
  float at[ENC_ROWS];
  unsigned char start[ENC_KEYS];
  int widest; // the most entries in one bin
};
constexpr float enc_bin_edge(int k) { return __builtin_bit_cast(float, (unsigned)(ENC_KEY0 + k) << ENC_KEY_SHIFT); }
template <int N>
constexpr EncTable enc_table(const float (&entries)[N], int first, int count, int searched) {
  EncTable t{};
  for (int j = 0; j < ENC_ROWS; j++) t.at[j] = j < count ? entries[first + j] : __builtin_nanf("");
  int below = 0; // the entries are sorted: one walk
  for (int k = 0; k < ENC_KEYS; k++) {
    while (below < searched && t.at[below] < enc_bin_edge(k)) below++;
    t.start[k] = (unsigned char)below;
    if (k > 0 && below - t.start[k - 1] > t.widest) t.widest = below - t.start[k - 1];
  }
  if (searched - below > t.widest) t.widest = searched - below; // the last bin: everything below 1.0f
  return t;
}
constexpr float kEncM[255] = PT_SRGB8_THRESHOLDS;
constexpr float kEncL[256] = PT_SRGB8_LEVELS;
constexpr EncTable kEncTableM = enc_table(kEncM, 0, 255, 255); // M[1 ... 255]
constexpr EncTable kEncTableL = enc_table(kEncL, 1, 255, 254); // L[1 ... 255], searched to L[254]: L[255] = 1.0f is never <= an x below 1
__device__ const EncTable g_enc_m = kEncTableM, g_enc_l = kEncTableL;
static_assert(kEncTableM.widest == ENC_CMP && kEncTableL.widest == ENC_CMP, "ENC_CMP comparisons reach every entry of a bin");
static_assert(kEncM[0] >= enc_bin_edge(0) && kEncL[1] >= enc_bin_edge(0) && kEncL[0] == 0.0f && kEncL[255] == 1.0f && kEncM[254] < 1.0f,
              "no entry lies below 2^-13 or at or above 1.0f but L[255]");
static_assert(ENC_KEYS == 416 && ENC_KEYS + ENC_ROWS <= 3 * 256, "the prologue's three strides of 256 lanes");

// the 8 x 8 Bayer matrix of the header
constexpr int enc_bayer(int u, int v) {
  int b = 0;
  for (int i = 0; i < 3; i++) b += ((((u ^ v) >> i) & 1) << (2 * (2 - i) + 1)) | (((v >> i) & 1) << (2 * (2 - i)));
  return b;
}
static_assert(enc_bayer(0, 0) == 0 && enc_bayer(1, 0) == 32 && enc_bayer(2, 0) == 8 && enc_bayer(7, 0) == 42 && enc_bayer(0, 1) == 48 &&
              enc_bayer(7, 7) == 21, "row 0 is 0 32 8 40 2 34 10 42");

struct EncLds {
  float at[ENC_ROWS];
  float t[64]; // ENC_DITHER: the thresholds, [v][u]
  unsigned char start[ENC_KEYS];
};

// the number of entries of the table that are <= x (S: the staged table, or — PT_ENCODE_TABLES_GLOBAL — the code object's)
template <class S>
__device__ __forceinline__ int enc_count(const S& s, float x) {
  const float y = fminf(fmaxf(x, 0x1p-13f), 0x1.fffffep-1f); // NaN -> 2^-13
  const int k = (int)(__float_as_uint(y) >> ENC_KEY_SHIFT) - ENC_KEY0;
  const int c = s.start[k];
  int n = c;
#pragma unroll
  for (int i = 0; i < ENC_CMP; i++) n += s.at[c + i] <= x;
  return n;
}

// the code of value x, number `v` of its row (pixel v / 3), whose dither row is ty = (py + phase_y) & 7
template <int MODE, class S>
__device__ __forceinline__ uint8_t enc_code(const S& s, const float* bayer_t, float x, unsigned v, unsigned phase_x, unsigned ty) {
  if (MODE == ENC_REFERENCE) return quantise(x);
  if (MODE == ENC_SRGB) return (uint8_t)enc_count(s, x);
  const int c = min(enc_count(s, x), 254); // (x >= 1: any level pair, the result is replaced below)
  const float lo = c ? s.at[c - 1] : 0.0f, hi = s.at[c];
  const float f = (x - lo) / (hi - lo);
  const float t = bayer_t[ty * 8 + ((v / 3 + phase_x) & 7)];
  const int code = c + (f >= t);
  return (uint8_t)(!(x > 0.0f) ? 0 : x >= 1.0f ? 255 : code);
}

struct EncodeArgs {
  const float* src;      // [height][width][3], row 0 = bottom
  uint8_t* rgb8;         // [height][width][3], row 0 = top
  const unsigned* state; // fused: the display state's words, or NULL (then 2^ev)
  float ev, iw2;         // fused: the stateless exposure, 1 / white^2
  int width, height;
  unsigned phase_x, phase_y; // & 7
};

template <int TONE, int MODE, bool VEC>
__global__ __launch_bounds__(256) void encode_kernel(EncodeArgs a) {
  __shared__ EncLds s;
  const EncTable& g = MODE == ENC_SRGB ? g_enc_m : g_enc_l;
#ifdef PT_ENCODE_TABLES_GLOBAL // A/B builds only (make variant EXTRA=-DPT_ENCODE_TABLES_GLOBAL): every lane reads the code object's tables through the
  const EncTable& tab = g;     // vector cache, nothing but the dither's thresholds is staged; profiles/encode_bench.txt has the outcome
#else
  const EncLds& tab = s;
#endif
  if (MODE != ENC_REFERENCE) {
#ifndef PT_ENCODE_TABLES_GLOBAL
    for (int i = threadIdx.x; i < ENC_ROWS + ENC_KEYS; i += 256) {
      if (i < ENC_ROWS) s.at[i] = g.at[i];
      else s.start[i - ENC_ROWS] = g.start[i - ENC_ROWS];
    }
#endif
    if (MODE == ENC_DITHER && threadIdx.x < 64) {
      const int u = threadIdx.x & 7, w = threadIdx.x >> 3;
      s.t[threadIdx.x] = ((float)enc_bayer(u, w) + 0.5f) * 0x1p-6f;
    }
    __syncthreads();
  }
  const long long row_items = VEC ? 3ll * a.width / 4 : 3ll * a.width;
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= row_items) return;
  float scale = 1.0f;
  if (TONE != ENCODE_PLAIN) scale = a.state ? __uint_as_float(a.state[DISP_SCALE]) : display_scale(a.ev);
  const unsigned v0 = (unsigned)(VEC ? f * 4 : f); // < 3 * 2^30
  for (int row = blockIdx.y; row < a.height; row += gridDim.y) { // row 0 = top
    const int py = a.height - 1 - row;
    const unsigned ty = ((unsigned)py + a.phase_y) & 7;
    const long long src = (long long)py * row_items + f, dst = (long long)row * row_items + f;
    if (VEC) {
      f4 y = reinterpret_cast<const f4*>(a.src)[src];
      if (TONE != ENCODE_PLAIN) {
        constexpr int T = TONE == ENCODE_PLAIN ? 0 : TONE;
        y.x = display_curve<T>(display_clamp(y.x * scale), a.iw2); y.y = display_curve<T>(display_clamp(y.y * scale), a.iw2);
        y.z = display_curve<T>(display_clamp(y.z * scale), a.iw2); y.w = display_curve<T>(display_clamp(y.w * scale), a.iw2);
      }
      uchar4 o;
      o.x = enc_code<MODE>(tab, s.t, y.x, v0, a.phase_x, ty); o.y = enc_code<MODE>(tab, s.t, y.y, v0 + 1, a.phase_x, ty);
      o.z = enc_code<MODE>(tab, s.t, y.z, v0 + 2, a.phase_x, ty); o.w = enc_code<MODE>(tab, s.t, y.w, v0 + 3, a.phase_x, ty);
      reinterpret_cast<uchar4*>(a.rgb8)[dst] = o;
    } else {
      float y = a.src[src];
      if (TONE != ENCODE_PLAIN) {
        constexpr int T = TONE == ENCODE_PLAIN ? 0 : TONE;
        y = display_curve<T>(display_clamp(y * scale), a.iw2);
      }
      a.rgb8[dst] = enc_code<MODE>(tab, s.t, y, v0, a.phase_x, ty);
    }
  }
}
