// The display stage's two streaming kernels in the forms that were tried (profiles/display_bench.txt records what was kept), 1920 x 1080,
// on a constant frame, a smooth frame and exp2(uniform(-20, 20)); HIP events around 50 back-to-back launches after a warm-up.
//   meter:  M<U, VEC, PEEL> — U pixels per thread and trip with their loads issued before the first atomic; VEC: the thread's pixels are
//           consecutive and come in as three 16-byte loads (U = 4); PEEL: the lanes that share the first lane's bin are added once.
//   apply:  A0 one thread per float, A1 one per pixel (the form of tonemap_kernel), A4 four floats per thread (16-byte load, 4-byte store).
// Every meter form must give the first form's histogram; every apply form the first form's bytes.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -o display_stage display_stage.hip
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

constexpr int W = 1920, H = 1080, BINS = 257, T = 256;

__device__ __forceinline__ int bin_of(float r, float g, float b) {
  const float y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
  const unsigned bits = __float_as_uint(y);
  if (!(y > 0.0f) || bits >= 0x7f800000u) return 256;
  const int k = (int)(bits >> 20) - ((127 - 16) << 3);
  return k < 0 ? 0 : k > 255 ? 255 : k;
}

template <bool PEEL>
__device__ __forceinline__ void add(unsigned* lds, int bin) {
  if (PEEL) {
    const int lead = __builtin_amdgcn_readfirstlane(bin);
    const bool same = bin >= 0 && bin == lead;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(same);
    if (same) {
      if ((int)(threadIdx.x & 63) == __builtin_ctzll(m)) atomicAdd(&lds[lead], (unsigned)__builtin_popcountll(m));
    } else if (bin >= 0) {
      atomicAdd(&lds[bin], 1u);
    }
  } else if (bin >= 0) {
    atomicAdd(&lds[bin], 1u);
  }
}

template <int U, bool VEC, bool PEEL>
__global__ __launch_bounds__(T) void meter(const float* __restrict__ color, unsigned* __restrict__ hist, unsigned n) {
  __shared__ unsigned lds[BINS];
  for (int i = threadIdx.x; i < BINS; i += T) lds[i] = 0u;
  __syncthreads();
  const unsigned stride = gridDim.x * T;
  if (VEC) { // n % 4 == 0: groups of four consecutive pixels
    const unsigned groups = n / 4;
    for (unsigned base = blockIdx.x * T; base < groups; base += stride) {
      const unsigned g = base + threadIdx.x;
      int bin[4] = {-1, -1, -1, -1};
      if (g < groups) {
        const float4* p = reinterpret_cast<const float4*>(color) + (size_t)g * 3;
        const float4 a = p[0], b = p[1], c = p[2];
        bin[0] = bin_of(a.x, a.y, a.z); bin[1] = bin_of(a.w, b.x, b.y); bin[2] = bin_of(b.z, b.w, c.x); bin[3] = bin_of(c.y, c.z, c.w);
      }
#pragma unroll
      for (int u = 0; u < 4; u++) add<PEEL>(lds, bin[u]);
    }
  } else {
    for (unsigned base = blockIdx.x * T; base < n; base += stride * U) {
      float v[U][3];
      bool on[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const unsigned i = base + u * stride + threadIdx.x;
        on[u] = i < n;
        if (on[u]) { v[u][0] = color[(size_t)i * 3]; v[u][1] = color[(size_t)i * 3 + 1]; v[u][2] = color[(size_t)i * 3 + 2]; }
      }
#pragma unroll
      for (int u = 0; u < U; u++) add<PEEL>(lds, on[u] ? bin_of(v[u][0], v[u][1], v[u][2]) : -1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BINS; i += T)
    if (lds[i]) atomicAdd(&hist[i], lds[i]);
}

__device__ __forceinline__ uint8_t quantise(float y) {
  float s = __fsqrt_rn(y);
  float cl = (s < 0.0f) ? 0.0f : (0.999f < s) ? 0.999f : s;
  float sc = 256.0f * cl;
  return (uint8_t)((sc == sc) ? (int)sc : 0);
}
__device__ __forceinline__ float aces(float c, float scale) {
  float x = c * scale;
  if (!(x >= 0.0f)) x = 0.0f;
  if (x > 0x1p20f) x = 0x1p20f;
  return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
}

__global__ __launch_bounds__(256) void apply0(const float* color, const float* scale_p, uint8_t* rgb8) {
  const long long rf = 3ll * W, f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= rf) return;
  const float scale = *scale_p;
  const int row = blockIdx.y;
  rgb8[(long long)row * rf + f] = quantise(aces(color[(long long)(H - 1 - row) * rf + f], scale));
}
__global__ __launch_bounds__(256) void apply1(const float* color, const float* scale_p, uint8_t* rgb8) {
  const int x = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
  if (x >= W) return;
  const float scale = *scale_p;
  const long long pix = (long long)(H - 1 - row) * W + x;
  for (int ch = 0; ch < 3; ch++) rgb8[((long long)row * W + x) * 3 + ch] = quantise(aces(color[pix * 3 + ch], scale));
}
__global__ __launch_bounds__(256) void apply4(const float* color, const float* scale_p, uint8_t* rgb8) {
  const long long rq = 3ll * W / 4, q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= rq) return;
  const float scale = *scale_p;
  const int row = blockIdx.y;
  const float4 v = reinterpret_cast<const float4*>(color)[(long long)(H - 1 - row) * rq + q];
  uchar4 o;
  o.x = quantise(aces(v.x, scale)); o.y = quantise(aces(v.y, scale)); o.z = quantise(aces(v.z, scale)); o.w = quantise(aces(v.w, scale));
  reinterpret_cast<uchar4*>(rgb8)[(long long)row * rq + q] = o;
}

#define CK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
  const size_t n = (size_t)W * H;
  std::vector<std::vector<float>> frames(3, std::vector<float>(n * 3));
  std::mt19937 rng(1);
  std::uniform_real_distribution<float> uni(-20.0f, 20.0f), jitter(0.9f, 1.1f);
  for (size_t i = 0; i < n * 3; i++) {
    frames[0][i] = 0.7f;
    frames[1][i] = (0.05f + 2.0f * (float)((i / 3) % W) / W * (float)((i / 3) / W) / H) * jitter(rng);
    frames[2][i] = std::exp2(uni(rng));
  }
  const char* names[3] = {"constant", "smooth", "random"};
  float *color, *scale;
  unsigned* hist;
  uint8_t* rgb8;
  CK(hipMalloc((void**)&color, n * 12)); CK(hipMalloc((void**)&scale, 4)); CK(hipMalloc((void**)&hist, BINS * 4)); CK(hipMalloc((void**)&rgb8, n * 3));
  const float one = 0.5f;
  CK(hipMemcpy(scale, &one, 4, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int f = 0; f < 3; f++) {
    CK(hipMemcpy(color, frames[f].data(), n * 12, hipMemcpyHostToDevice));
    std::vector<unsigned> want;
    auto run_meter = [&](const char* name, auto kernel, unsigned blocks) -> int {
      CK(hipMemset(hist, 0, BINS * 4));
      hipLaunchKernelGGL(kernel, dim3(blocks), dim3(T), 0, 0, color, hist, (unsigned)n);
      std::vector<unsigned> got(BINS);
      CK(hipMemcpy(got.data(), hist, BINS * 4, hipMemcpyDeviceToHost));
      if (want.empty()) want = got;
      const bool same = got == want;
      for (int i = 0; i < 5; i++) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(T), 0, 0, color, hist, (unsigned)n);
      CK(hipEventRecord(e0));
      for (int i = 0; i < 50; i++) hipLaunchKernelGGL(kernel, dim3(blocks), dim3(T), 0, 0, color, hist, (unsigned)n);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, e0, e1));
      std::printf("%-9s meter %-14s blocks %4u  %7.2f us  %s\n", names[f], name, blocks, ms * 20.0f, same ? "same histogram" : "DIFFERENT HISTOGRAM");
      return 0;
    };
    for (unsigned blocks : {2048u, 1024u, 512u, 256u, 128u}) {
      if (run_meter("U1", meter<1, false, false>, blocks)) return 1;
      if (run_meter("U1 peel", meter<1, false, true>, blocks)) return 1;
      if (run_meter("U4", meter<4, false, false>, blocks)) return 1;
      if (run_meter("U4 peel", meter<4, false, true>, blocks)) return 1;
      if (run_meter("U8 peel", meter<8, false, true>, blocks)) return 1;
      if (run_meter("VEC", meter<4, true, false>, blocks)) return 1;
      if (run_meter("VEC peel", meter<4, true, true>, blocks)) return 1;
    }
    std::vector<uint8_t> want8;
    auto run_apply = [&](const char* name, auto kernel, dim3 grid) -> int {
      CK(hipMemset(rgb8, 0, n * 3));
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, 0, color, scale, rgb8);
      std::vector<uint8_t> got(n * 3);
      CK(hipMemcpy(got.data(), rgb8, n * 3, hipMemcpyDeviceToHost));
      if (want8.empty()) want8 = got;
      const bool same = got == want8;
      for (int i = 0; i < 5; i++) hipLaunchKernelGGL(kernel, grid, dim3(256), 0, 0, color, scale, rgb8);
      CK(hipEventRecord(e0));
      for (int i = 0; i < 50; i++) hipLaunchKernelGGL(kernel, grid, dim3(256), 0, 0, color, scale, rgb8);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, e0, e1));
      std::printf("%-9s apply %-14s grid %5u x %4u  %7.2f us  %s\n", names[f], name, grid.x, grid.y, ms * 20.0f, same ? "same bytes" : "DIFFERENT BYTES");
      return 0;
    };
    if (run_apply("per float", apply0, dim3((3 * W + 255) / 256, H))) return 1;
    if (run_apply("per pixel", apply1, dim3((W + 255) / 256, H))) return 1;
    if (run_apply("four floats", apply4, dim3((3 * W / 4 + 255) / 256, H))) return 1;
  }
  CK(hipFree(color)); CK(hipFree(scale)); CK(hipFree(hist)); CK(hipFree(rgb8));
  return 0;
}
