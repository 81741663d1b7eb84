// pt_firefly.hpp — the firefly stage's kernel (include/pt_post.h: pt_firefly).  Included by pt_render.hip inside its anonymous namespace,
// after pt_device.hpp (f4).
//
// One thread per pixel in a PT_FIREFLY_TILE_W x PT_FIREFLY_TILE_H pixel workgroup, the a-trous filters' shape: a wave is two rows of 32, so a
// neighbour's 64 reads are two runs of contiguous pixels.  LDS: the workgroup first stages its tile with a halo of one pixel as one 16-byte
// record (R, G, B, Y) per slot, and every lane reads its eight neighbours and itself with one ds_read_b128 each — the 16 lanes such a read
// serves together lie in one row at consecutive slots, 256 contiguous bytes, one per bank.  The record's Y is the header's Y(c) for a
// finite pixel and NaN for a slot that is outside the frame or holds a pixel that is not finite: Y of a finite pixel is never NaN
// (pt_post.h), so `Y == Y` is the header's "inside the frame and finite(q)" and the three channel tests are made once per slot instead of
// once per tap.  !LDS (PT_FIREFLY_NO_LDS): the same operations on the same values in the same order, every neighbour read from global
// memory — the bits do not depend on the path.
//
// The grid is at most PT_FIREFLY_MAX_BLOCKS workgroups, each of which walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ...: what the
// counts cost is the number of atomics on their one address.  A wave keeps its two counts in scalar registers across its tiles (a ballot
// per tile); at the end the waves of a workgroup add them up in LDS and one lane adds both to `counts` with ONE 64-bit atomic (!LDS: one
// per wave, the path uses no LDS at all).  One atomic per wave and tile took 0.20 ms at 1920 x 1080 against 0.017 ms for the kernel without
// counts (profiles/firefly_bench.txt).
#ifndef PT_FIREFLY_MAX_BLOCKS
#define PT_FIREFLY_MAX_BLOCKS 2048 /* 8 workgroups = 32 waves per CU: all resident at the kernel's occupancy of 8 waves per SIMD */
#endif
struct FireflyArgs {
  const float* color;    // [height][width][3]
  const float* variance; // or NULL
  float* out;
  float* variance_out;   // or NULL; may be variance
  unsigned long long* counts; // or NULL: uint32 {clamped, repaired} as one 64-bit word, zeroed on the stream before the launch
  int width, height, tiles_x, tiles;
  int rank;              // 1 or 2
  unsigned repair;
  float k;
};

enum { FIREFLY_TW = PT_FIREFLY_TILE_W + 2, FIREFLY_TH = PT_FIREFLY_TILE_H + 2, FIREFLY_SLOTS = FIREFLY_TW * FIREFLY_TH,
       FIREFLY_LDS_BYTES = FIREFLY_SLOTS * 16 + 8 /* the tile and the workgroup's two counts */ };
static_assert(PT_FIREFLY_TILE_W == 32 && PT_FIREFLY_TILE_H == 8, "firefly_kernel maps a 256-thread workgroup as 8 rows of 32 lanes");

__device__ __forceinline__ float firefly_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ bool firefly_finite(float r, float g, float b) {
  return fabsf(r) < __builtin_inff() && fabsf(g) < __builtin_inff() && fabsf(b) < __builtin_inff();
}

template <bool LDS>
__global__ __launch_bounds__(256) void firefly_kernel(FireflyArgs a) {
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const float nan = __builtin_nanf("");
  __shared__ f4 s_c[LDS ? FIREFLY_SLOTS : 1];
  __shared__ unsigned s_n[LDS ? 2 : 1];
  if constexpr (LDS) {
    if (threadIdx.x < 2) s_n[threadIdx.x] = 0u; // (ordered before the adds below by the barriers of the first tile)
  }
  unsigned wave_clamped = 0u, wave_repaired = 0u;    // wave-uniform
  for (unsigned t = blockIdx.x; t < (unsigned)a.tiles; t += gridDim.x) { // (the trip count is the workgroup's: the barriers are uniform)
    const int bx = (int)(t % (unsigned)a.tiles_x), by = (int)(t / (unsigned)a.tiles_x);
    const int x = bx * PT_FIREFLY_TILE_W + lx, y = by * PT_FIREFLY_TILE_H + ly;
    if constexpr (LDS) {
      if (t != blockIdx.x) __syncthreads(); // the previous tile has been read by every wave
      const int x0 = bx * PT_FIREFLY_TILE_W - 1, y0 = by * PT_FIREFLY_TILE_H - 1;
      for (int i = threadIdx.x; i < FIREFLY_SLOTS; i += 256) {
        const int gx = x0 + i % FIREFLY_TW, gy = y0 + i / FIREFLY_TW;
        f4 v = {0.0f, 0.0f, 0.0f, nan};
        if (gx >= 0 && gx < a.width && gy >= 0 && gy < a.height) {
          const long long q = ((long long)gy * a.width + gx) * 3;
          v.x = a.color[q]; v.y = a.color[q + 1]; v.z = a.color[q + 2];
          if (firefly_finite(v.x, v.y, v.z)) v.w = firefly_luma(v.x, v.y, v.z);
        }
        s_c[i] = v;
      }
      __syncthreads();
    }
    bool clamped = false, repaired = false;
    if (x < a.width && y < a.height) {
      const long long p = ((long long)y * a.width + x) * 3;
      const int lp = (ly + 1) * FIREFLY_TW + lx + 1; // the pixel's slot in the tile (LDS)
      float pr, pg, pb, Yp;
      bool p_finite;
      if constexpr (LDS) {
        const f4 v = s_c[lp];
        pr = v.x; pg = v.y; pb = v.z; Yp = v.w;
        p_finite = Yp == Yp;
      } else {
        pr = a.color[p]; pg = a.color[p + 1]; pb = a.color[p + 2];
        p_finite = firefly_finite(pr, pg, pb);
        Yp = firefly_luma(pr, pg, pb);
      }
      float m1 = -__builtin_inff(), m2 = -__builtin_inff(), sr = 0.0f, sg = 0.0f, sb = 0.0f;
      int n = 0;
#pragma unroll
      for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
          if (dx == 0 && dy == 0) continue;
          float qr = 0.0f, qg = 0.0f, qb = 0.0f, Yq = nan;
          bool ok;
          if constexpr (LDS) {
            const f4 v = s_c[lp + dy * FIREFLY_TW + dx]; // inside the tile: the halo is one pixel
            qr = v.x; qg = v.y; qb = v.z; Yq = v.w;
            ok = Yq == Yq;
          } else {
            const int qx = x + dx, qy = y + dy;
            ok = qx >= 0 && qx < a.width && qy >= 0 && qy < a.height;
            if (ok) {
              const long long q = ((long long)qy * a.width + qx) * 3;
              qr = a.color[q]; qg = a.color[q + 1]; qb = a.color[q + 2];
              ok = firefly_finite(qr, qg, qb);
              Yq = firefly_luma(qr, qg, qb);
            }
          }
          if (ok) {
            n = n + 1;
            sr = sr + qr; sg = sg + qg; sb = sb + qb;
            if (Yq > m1) { m2 = m1; m1 = Yq; }
            else if (Yq > m2) m2 = Yq;
          }
        }
      }
      float vr = 0.0f, vg = 0.0f, vb = 0.0f;
      if (a.variance_out) { vr = a.variance[p]; vg = a.variance[p + 1]; vb = a.variance[p + 2]; }
      float o_r = pr, o_g = pg, o_b = pb;
      if (p_finite) {
        const float L = a.k * (a.rank == 1 ? m1 : m2);
        if (n >= a.rank && Yp > L && Yp > 0.0f) {
          const float s = (L > 0.0f ? L : 0.0f) / Yp;
          const float s2 = s * s;
          o_r = pr * s; o_g = pg * s; o_b = pb * s;
          vr = vr * s2; vg = vg * s2; vb = vb * s2;
          clamped = true;
        }
      } else if (a.repair && n > 0) {
        const float fn = (float)n;
        o_r = sr / fn; o_g = sg / fn; o_b = sb / fn;
        vr = vg = vb = __builtin_inff();
        repaired = true;
      }
      a.out[p] = o_r; a.out[p + 1] = o_g; a.out[p + 2] = o_b;
      if (a.variance_out) { a.variance_out[p] = vr; a.variance_out[p + 1] = vg; a.variance_out[p + 2] = vb; }
    }
    if (a.counts) { // (no early return above: every lane of a wave reaches the ballots)
      wave_clamped += (unsigned)__popcll(__ballot(clamped));
      wave_repaired += (unsigned)__popcll(__ballot(repaired));
    }
  }
  if (a.counts) { // integer atomics: the order of the adds does not matter
    const unsigned long long both = (unsigned long long)wave_clamped | ((unsigned long long)wave_repaired << 32); // (each half stays below 2^30: no carry)
    if constexpr (LDS) {
      if ((threadIdx.x & 63) == 0) {
        if (wave_clamped) atomicAdd(&s_n[0], wave_clamped);
        if (wave_repaired) atomicAdd(&s_n[1], wave_repaired);
      }
      __syncthreads();
      if (threadIdx.x == 0 && (s_n[0] | s_n[1])) atomicAdd(a.counts, (unsigned long long)s_n[0] | ((unsigned long long)s_n[1] << 32));
    } else {
      if ((threadIdx.x & 63) == 0 && both) atomicAdd(a.counts, both);
    }
  }
}
