// pt_spatial_variance.hpp — the spatial variance estimate's kernel (include/pt_spatial_variance.h: pt_spatial_variance).  Included by
// pt_render.hip inside its anonymous namespace, after pt_device.hpp (f4).
//
// One thread per pixel in a PT_SVAR_TILE_W x PT_SVAR_TILE_H pixel workgroup, pt_firefly's shape: a wave is two rows of 32.  LDS: the
// workgroup first stages its tile with a halo of PT_SVAR_MAX_RADIUS pixels as TWO 16-byte records per slot, (e.rgb, z) and (n.xyz, bits
// of k), each kind in an array of its own: the 16 lanes one ds_read_b128 serves together (lanes 0-3, 12-15, 20-27 of a row, and so on)
// then read 16 different slots of one row of one array, whose bank (byte address / 4 mod 64) is 4 x (slot mod 16) — one bank set each.
// Interleaved, at a stride of 32 bytes, the same read would be two-way conflicted.  The demodulation division and the usable test are
// made once per slot: the record's e.r is NaN for a slot that is outside the frame or not usable (a usable e is finite), so `e.r == e.r`
// is the header's usable(q).  A lane that has to estimate first builds consistent(q|p) for its window as a bit mask — bit
// (dy + 3) * 8 + (dx + 3), so that q' is the next bit and q'' the bit 8 further — and then walks the pairs in the header's order on mask
// bits, reading e from LDS only for the pairs it takes.  !LDS (PT_SVAR_NO_LDS): the same operations on the same values in the same order,
// every record made from global memory where it is wanted — the bits do not depend on the path.
//
// The grid is at most PT_SVAR_MAX_BLOCKS workgroups, each of which walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ...; the counts are
// kept per wave in scalar registers across the tiles, added up in LDS at the end and added to `counts` with ONE 64-bit atomic per
// workgroup (!LDS: one per wave, the path uses no LDS at all), as firefly_kernel does and for its reason (profiles/firefly_bench.txt).
#ifndef PT_SVAR_MAX_BLOCKS
#define PT_SVAR_MAX_BLOCKS 2048 /* 8 workgroups = 32 waves per CU: all resident at the kernel's occupancy of 8 waves per SIMD */
#endif
struct SvarArgs {
  const float* color;       // [height][width][3]
  const float* albedo;      // or NULL (never NULL with demodulate)
  const float* normal;      // or NULL
  const float* depth;       // or NULL: [height][width]
  const int* id;            // or NULL: [height][width]
  const float* variance_in; // or NULL
  float* variance_out;      // may be variance_in
  unsigned long long* counts; // or NULL: uint32 {estimated, holes} as one 64-bit word, zeroed on the stream before the launch
  int width, height, tiles_x, tiles;
  int radius, min_pairs;
  unsigned demodulate;
  float tol_depth, tol_normal;
};

enum { SVAR_TW = PT_SVAR_TILE_W + 2 * PT_SVAR_MAX_RADIUS, SVAR_TH = PT_SVAR_TILE_H + 2 * PT_SVAR_MAX_RADIUS, SVAR_SLOTS = SVAR_TW * SVAR_TH,
       SVAR_LDS_BYTES = SVAR_SLOTS * 32 + 8 /* the tile's two records per slot and the workgroup's two counts */ };
static_assert(PT_SVAR_TILE_W == 32 && PT_SVAR_TILE_H == 8, "svar_kernel maps a 256-thread workgroup as 8 rows of 32 lanes");
static_assert(PT_SVAR_MAX_RADIUS == 3, "svar_kernel's window mask has rows of 8 bits: 7 offsets and one spare");

// The first record of pixel (qx, qy): (e.rgb, z); e.r is NaN where the pixel is outside the frame or not usable.
__device__ __forceinline__ f4 svar_record_e(const SvarArgs& a, int qx, int qy) {
  f4 v = {__builtin_nanf(""), 0.0f, 0.0f, 0.0f};
  if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
    const long long q = (long long)qy * a.width + qx;
    float r = a.color[q * 3], g = a.color[q * 3 + 1], b = a.color[q * 3 + 2];
    if (a.demodulate) {
      r = r / (a.albedo[q * 3] + 1e-3f); g = g / (a.albedo[q * 3 + 1] + 1e-3f); b = b / (a.albedo[q * 3 + 2] + 1e-3f);
    }
    const bool usable = fabsf(r) < __builtin_inff() && fabsf(g) < __builtin_inff() && fabsf(b) < __builtin_inff();
    v.x = usable ? r : __builtin_nanf(""); v.y = g; v.z = b;
    if (a.depth) v.w = a.depth[q];
  }
  return v;
}

// The second record: (n.xyz, bits of k); zeros for a NULL plane and outside the frame (where the first record already says "not usable").
__device__ __forceinline__ f4 svar_record_n(const SvarArgs& a, int qx, int qy) {
  f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
    const long long q = (long long)qy * a.width + qx;
    if (a.normal) { v.x = a.normal[q * 3]; v.y = a.normal[q * 3 + 1]; v.z = a.normal[q * 3 + 2]; }
    if (a.id) v.w = __int_as_float(a.id[q]);
  }
  return v;
}

template <bool LDS>
__global__ __launch_bounds__(256) void svar_kernel(SvarArgs a) {
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int r = a.radius;
  const float tn2 = a.tol_normal * a.tol_normal;
  __shared__ f4 s_e[LDS ? SVAR_SLOTS : 1];
  __shared__ f4 s_n[LDS ? SVAR_SLOTS : 1];
  __shared__ unsigned s_count[LDS ? 2 : 1];
  if constexpr (LDS) {
    if (threadIdx.x < 2) s_count[threadIdx.x] = 0u; // (ordered before the adds below by the barriers of the first tile)
  }
  unsigned wave_estimated = 0u, wave_holes = 0u; // wave-uniform
  for (unsigned t = blockIdx.x; t < (unsigned)a.tiles; t += gridDim.x) { // (the trip count is the workgroup's: the barriers are uniform)
    const int bx = (int)(t % (unsigned)a.tiles_x), by = (int)(t / (unsigned)a.tiles_x);
    const int x = bx * PT_SVAR_TILE_W + lx, y = by * PT_SVAR_TILE_H + ly;
    if constexpr (LDS) {
      if (t != blockIdx.x) __syncthreads(); // the previous tile has been read by every wave
      const int x0 = bx * PT_SVAR_TILE_W - PT_SVAR_MAX_RADIUS, y0 = by * PT_SVAR_TILE_H - PT_SVAR_MAX_RADIUS;
      for (int i = threadIdx.x; i < SVAR_SLOTS; i += 256) {
        const int gx = x0 + i % SVAR_TW, gy = y0 + i / SVAR_TW;
        s_e[i] = svar_record_e(a, gx, gy);
        s_n[i] = svar_record_n(a, gx, gy);
      }
      __syncthreads();
    }
    bool estimated = false, hole = false;
    if (x < a.width && y < a.height) {
      const long long p = ((long long)y * a.width + x) * 3;
      float vr = 0.0f, vg = 0.0f, vb = 0.0f;
      bool keep = false;
      if (a.variance_in) {
        vr = a.variance_in[p]; vg = a.variance_in[p + 1]; vb = a.variance_in[p + 2];
        keep = vr >= 0.0f && vr < __builtin_inff() && vg >= 0.0f && vg < __builtin_inff() && vb >= 0.0f && vb < __builtin_inff();
      }
      if (!keep) {
        const int lp = (ly + PT_SVAR_MAX_RADIUS) * SVAR_TW + lx + PT_SVAR_MAX_RADIUS; // the pixel's slot in the tile (LDS)
        auto rec_e = [&](int dx, int dy) -> f4 {
          if constexpr (LDS) return s_e[lp + dy * SVAR_TW + dx]; // inside the tile: |dx|, |dy| <= the halo
          else return svar_record_e(a, x + dx, y + dy);
        };
        auto rec_n = [&](int dx, int dy) -> f4 {
          if constexpr (LDS) return s_n[lp + dy * SVAR_TW + dx];
          else return svar_record_n(a, x + dx, y + dy);
        };
        const f4 pe = rec_e(0, 0), pn = rec_n(0, 0);
        const float zp = pe.w;
        const int kp = __float_as_int(pn.w);
        const bool hit = zp > 0.0f;
        const float zlim = a.tol_depth * zp;
        unsigned long long mask = 0ull;
        for (int dy = -r; dy <= r; dy++) {
          for (int dx = -r; dx <= r; dx++) {
            const f4 qe = rec_e(dx, dy);
            bool ok = qe.x == qe.x; // usable(q)
            if (a.depth) ok = ok && (hit ? (qe.w > 0.0f && fabsf(qe.w - zp) <= zlim) : !(qe.w > 0.0f));
            if (a.id || a.normal) {
              const f4 qn = rec_n(dx, dy);
              if (a.id) ok = ok && __float_as_int(qn.w) == kp;
              if (a.normal) {
                const float nx = pn.x - qn.x, ny = pn.y - qn.y, nz = pn.z - qn.z;
                ok = ok && ((nx * nx + ny * ny) + nz * nz) <= tn2;
              }
            }
            if (ok) mask |= 1ull << ((dy + 3) * 8 + (dx + 3));
          }
        }
        float sr = 0.0f, sg = 0.0f, sb = 0.0f;
        int pairs = 0;
        for (int dy = -r; dy <= r; dy++) {
          for (int dx = -r; dx <= r; dx++) {
            const int bit = (dy + 3) * 8 + (dx + 3);
            if (!((mask >> bit) & 1ull)) continue;
            const bool right = dx < r && ((mask >> (bit + 1)) & 1ull), up = dy < r && ((mask >> (bit + 8)) & 1ull);
            if (!(right || up)) continue;
            const f4 e = rec_e(dx, dy);
            if (right) {
              const f4 e1 = rec_e(dx + 1, dy);
              const float dr = e.x - e1.x, dg = e.y - e1.y, db = e.z - e1.z;
              sr = sr + dr * dr; sg = sg + dg * dg; sb = sb + db * db;
              pairs = pairs + 1;
            }
            if (up) {
              const f4 e1 = rec_e(dx, dy + 1);
              const float dr = e.x - e1.x, dg = e.y - e1.y, db = e.z - e1.z;
              sr = sr + dr * dr; sg = sg + dg * dg; sb = sb + db * db;
              pairs = pairs + 1;
            }
          }
        }
        if (pe.x == pe.x && pairs >= a.min_pairs) {
          const float fn = 2.0f * (float)pairs;
          float mr = 1.0f, mg = 1.0f, mb = 1.0f;
          if (a.demodulate) { mr = a.albedo[p] + 1e-3f; mg = a.albedo[p + 1] + 1e-3f; mb = a.albedo[p + 2] + 1e-3f; }
          vr = (sr / fn) * (mr * mr); vg = (sg / fn) * (mg * mg); vb = (sb / fn) * (mb * mb);
          estimated = true;
        } else {
          vr = vg = vb = __builtin_inff();
          hole = true;
        }
      }
      a.variance_out[p] = vr; a.variance_out[p + 1] = vg; a.variance_out[p + 2] = vb; // (kept: the bits it read)
    }
    if (a.counts) { // (no early return above: every lane of a wave reaches the ballots)
      wave_estimated += (unsigned)__popcll(__ballot(estimated));
      wave_holes += (unsigned)__popcll(__ballot(hole));
    }
  }
  if (a.counts) { // integer atomics: the order of the adds does not matter
    const unsigned long long both = (unsigned long long)wave_estimated | ((unsigned long long)wave_holes << 32); // (each half stays below 2^30 + 1: no carry)
    if constexpr (LDS) {
      if ((threadIdx.x & 63) == 0) {
        if (wave_estimated) atomicAdd(&s_count[0], wave_estimated);
        if (wave_holes) atomicAdd(&s_count[1], wave_holes);
      }
      __syncthreads();
      if (threadIdx.x == 0 && (s_count[0] | s_count[1])) atomicAdd(a.counts, (unsigned long long)s_count[0] | ((unsigned long long)s_count[1] << 32));
    } else {
      if ((threadIdx.x & 63) == 0 && both) atomicAdd(a.counts, both);
    }
  }
}
