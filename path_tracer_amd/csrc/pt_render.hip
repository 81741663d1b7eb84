// pt_render.hip — kernels + C ABI (include/pt_render.h) of the MI355X-native render() hot path.
//
// Replaces render<W,H,S>() / executor() / render_pixel()  (reference include/render.hpp:25-160).
//
// Mapping: one lane owns one pixel for ALL of its samples — the reference's single xorshift32
// stream per pixel, consumed sequentially across samples (render.hpp:95-101,130-133), leaves no other bit-exact
// choice.  Lanes are persistent: they pull pixels (8x8 tiles by default) from a per-launch queue, heaviest tiles
// first (cost-probe pass + lpt_order_kernel), and run a "regenerate in place" loop — a lane whose path ended starts
// its next sample in the same iteration, so the wave-uniform primitive loop always runs with all live lanes (what
// ballot/prefix compaction would buy, without moving state between lanes).  Three kernel families:
//   render_kernel<IMG, LDS, MLDS, COOP>   scene resident in LDS (or the scalar cache); COOP adds the cooperative
//                                         traversal (a ray's list split over idle lanes) and the split queue
//   render_kernel_stream<IMG>             scene larger than LDS: workgroup-synchronous LDS-tile streaming
//   bounce / camera_rays / math kernels   function-level probes for the parity tests
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <type_traits>
#include <string>
#include <vector>

#include "../../include/pt_render.h"
#include "../../include/pt_post.h"
#include "../../include/pt_spatial_variance.h"
#include "../../include/pt_metrics.h"
#include "../../include/pt_encode.h"
#include "pt_device.hpp"
#include "pt_flatten.hpp"

#ifdef PT_STAMPS
__device__ unsigned long long g_stamps[8];
#endif
#ifdef PT_STAMPS_WALK
__device__ unsigned long long g_walk[8];
#endif
#ifdef PT_STAMPS_RUNS
__device__ unsigned long long g_runs[16];
#endif
#ifdef PT_STAMPS_TRI
__device__ unsigned long long g_tri[16];
#endif
#ifdef PT_STAMPS_BLOCKS /* diagnostic build (make variant NAME=libpt_blocks.so EXTRA=-DPT_STAMPS_BLOCKS; tools/block_residency.py): per workgroup of the
                           frame launch where it ran (XCC_ID << 32 | HW_ID) and when it started / ended (s_memrealtime, 100 MHz) */
__device__ unsigned long long g_blocks[3 * 8192];
#endif

using namespace ptd;

static_assert(sizeof(PtHittable) == 64 && sizeof(PtMaterial) == 32 && sizeof(PtTexture) == 48 && sizeof(PtCamera) == 96);
static_assert(sizeof(Cam) == sizeof(PtCamera));

namespace {

#ifndef PT_MIN_WAVES
#define PT_MIN_WAVES 7 /* non-IMG resident kernel: 71 VGPRs, no scratch; +6.5 % on the headline scene (A/B, one process) */
#endif
#ifndef PT_MIN_WAVES_IMG
#define PT_MIN_WAVES_IMG 5 /* image-texture kernels: 96 VGPRs; +10 % on the 496-hittable scene (A/B, one process) */
#endif
#ifndef PT_MIN_WAVES_CL
#define PT_MIN_WAVES_CL 7 /* cold lane state in LDS: 68 VGPRs; measured 8 waves (64 VGPRs, no spill) -5 %, 7 waves +2 %, 6 waves -3 % */
#endif
#ifndef PT_MIN_WAVES_COOP
#define PT_MIN_WAVES_COOP 5 /* cooperative kernels: 93 VGPRs, no scratch (7 waves: 72 VGPRs + 76 B/lane of spills in the loop) */
#endif
#ifndef PT_MIN_WAVES_TRIPOOL
#define PT_MIN_WAVES_TRIPOOL 5 /* triangle-pool kernels: 96 VGPRs.  Round 6, with the camera rays' candidate cache and two pair batches / two expansion trips in flight in the grid walk: 1080p x 32 spp 1 116 ms at 7 waves (72 VGPRs + 228 B of scratch), 986 at 6 (80 VGPRs), 978 at 5; with the pipelined walk 1 116 at 6, 979 at 5 — profiles/r06_ab_tri_cache.txt, r06_ab_tri_pipe.txt; rounds 3-5 (no cache, no pipelining) measured 7 best */
#endif
#ifndef PT_MIN_WAVES_BINSTEP
#define PT_MIN_WAVES_BINSTEP 4 /* bin_step_kernel (pt_binned.hpp): 128 VGPRs, no scratch (6 waves: 80 VGPRs + 236 B of scratch with the pipelined trips) */
#endif
#ifndef PT_MIN_WAVES_COOP_IMG
#define PT_MIN_WAVES_COOP_IMG 5 /* 96 VGPRs + 60 B/lane of spills; spill-free needs 116 VGPRs = 4 waves: 496-hittable scene -9 % (A/B) */
#endif
#ifndef PT_MIN_WAVES_AOV
#define PT_MIN_WAVES_AOV 4 /* aov_kernel (pt_render_aov): 128 VGPRs + 92 - 116 B/lane of scratch (spills around the traversal, inside the per-sample loop), 20 KB of static LDS per workgroup.  Left to itself the compiler takes 168 - 173 VGPRs, no scratch, 2 waves; measured at 1080p x 16 samples with 2 / 3 / 4 waves: Cornell-style scene 0.68 / 0.55 / 0.50 ms, 496-hittable scene 2.93 / 2.11 / 1.93, 100 k triangles 324 / 242 / 210 — the spills cost less than the occupancy buys (profiles/aov_bench.txt: the A/B and the resource table) */
#endif
// How a kernel obtains the u,v an image texture looks up (DESIGN.md §3 "u,v of the final hit")
enum { UV_NONE = 0, UV_WINNER = 1, UV_TRACKED = 2 };
constexpr int kBlock = 256;                 // 4 wavefronts = 4 tiles per workgroup
constexpr int kWavesPerBlock = kBlock / 64;
#ifndef PT_GRID_BLOCK
#define PT_GRID_BLOCK 256
#endif
constexpr int kGridBlock = PT_GRID_BLOCK;   // workgroup size of the LDS-resident kernels that walk a sphere grid (render_kernel: BLOCK)
constexpr size_t kMaxLdsBlob = ptf::kLdsImageBytes;   // blob staged in LDS when it fits (64 KB; the flattener budgets the slab pools' octant tables by it)
constexpr size_t kMaxLdsWithMaterials = 16 * 1024; // stage the material table too when records + materials are this small
constexpr size_t kMaxLdsColdScene = 10 * 1024;    // records + materials this small: the 8-wave kernel with LDS-resident cold lane state
constexpr float kCoopMinTraversal = 2500.0f;        // estimated VALU instructions of one list scan (~110 spheres)
constexpr int kGridMinTiles = 0;                    // since the grid's retuning it wins at every frame size: see choose_variant
constexpr unsigned kQueueRing = 256;        // launches in flight on one scene may not exceed this

// The kernels' only argument.  Every member starts "off": a launcher writes only what its launch uses.
struct KArgs {
  Cam cam = {};
  // Behind the camera, and read like it — from the kernarg segment, once per bounce, where the bounce has latency to hide (render_kernel):
  // the one slab pool of a rect / box-only scene as launch constants (pt_device.hpp: PoolPlan; scene_pool_plan, pass_pool_plan).  one = 0: no such scene; 2: a pool of one chunk.
  PoolPlan plan = {};
  const f4* blob = nullptr;
  const f4* mats = nullptr;
  const f4* pool = nullptr;    // tables of the triangle pools (pt_flatten.hpp: put_tri_pool); NULL when the scene has none
  const uint8_t* atlas = nullptr;
  float* fb = nullptr;
  int n_runs = 0, blob_f4 = 0, mats_f4 = 0; // (mats_f4: the materials AND the shade table behind them — what an LDS image stages behind the blob)
  // the shade table of a small rect / box-only scene (pt_flatten.hpp: Flat::shade; pt_device.hpp: shade_record): the hittable at record offset `off` has
  // record shade_k + (off >> 1) of the image [blob][materials][shade table].  0: the scene has none (no kernel that reads it is chosen then)
  int shade_k = 0;
  int width = 0, height = 0, samples = 0, depth = 0;
  float inv_w = 0.0f, inv_h = 0.0f; // RN(1 / (float)width), RN(1 / (float)height): camera_ray
  int pinhole = 0;    // cam_is_pinhole(cam): camera_ray skips the lens arithmetic
  int shard_index = 0, shard_count = 0;
  int tiles_x = 0, n_tiles = 0;
  int n_local_pixels = 0;  // 64 x the tiles this shard owns (incl. padding pixels of edge tiles)
  unsigned int* queue = nullptr; // per-launch dequeue counter, zeroed on the stream before the kernel
  unsigned int* cost = nullptr;  // non-NULL: cost-probe pass, per local tile ray counts
  // The probe's samples are the frame's FIRST samples: with resume_rng the probe leaves every pixel's plain radiance sum in fb and its
  // generator's state in resume_rng[local pixel]; the frame launch (resume_spp = what the probe rendered) starts every pixel from both, at
  // sample resume_spp — the same stream, the same order of additions (render.hpp:95-101), and no sample is rendered twice.
  unsigned int* resume_rng = nullptr;
  int resume_spp = 0;
  // Sample windows of a PtAccum (pt_render_accumulate): `samples` is the window's END, resume_spp its start, and a finished pixel leaves
  // its plain radiance sum in fb and its generator's state in resume_rng — the probe's branch of lane_store — instead of the mean.
  int keep_state = 0;
  // Masked windows of an adaptive PtAccum (pt_adaptive_window): one byte per pixel in the frame buffer's layout without the channel
  // ([y][x], or [local tile][64] for shards); lane_acquire skips a pixel whose byte is 0 like a padding pixel.  NULL: every pixel.
  const uint8_t* mask = nullptr;
  // Headline-family launches (launch_render): once prio_onset queue positions are taken, a wave sets its issue priority — every 64
  // iterations — by the samples its slowest pixel still has to render: >= prio_t3 -> 3, >= prio_t2 -> 2, >= prio_t1 -> 1, else 0 (render_kernel).
  // prio_t1 = 0: never.
  int prio_onset = 0, prio_t1 = 0, prio_t2 = 0, prio_t3 = 0;
  int cost_max = 0;    // probe: 1 = keep the tile's HEAVIEST pixel (x 64) instead of the sum over its pixels
  const int* order = nullptr;  // non-NULL: queue position -> local tile, heaviest first
  const int* n_split = nullptr; // non-NULL (COOP kernels): [0] how many leading tiles of `order` go through the wide phase, [1] log2 G
  int tile_granular = 0; // PT_FLAG_TILE_GRANULAR
  int tile_group = 64;   // tile-granular launches: lanes of a wave that take pixels together (64: the whole wave = a tile; 32 / 16: half / quarter tiles)
  int heavy_pixels = 0;  // > 0 (tile-granular grid kernels, chain-bound launches): the first heavy_pixels queue positions — the heaviest tiles of the
  int heavy_lanes = 64;  //   cost-sorted order — are taken heavy_lanes pixels at a time, by the first heavy_lanes lanes of a wave (lane_acquire)
  int scatter_p = 0;     // > 0 (triangle-pool kernels): queue positions are dealt to tiles in runs of 2^scatter_log pixels with this stride (lane_acquire)
  int scatter_log = 0;
  int lanes_cap = 64;    // < 64 (triangle-pool kernels, fewer pixels than lanes): only the first lanes_cap lanes of a wave take pixels (lane_acquire)
  int n_hittables = 0;
  int coop_prefix = -1;  // >= 0: cooperative traversal allowed, list splittable up to this hittable; -1: disabled
  int fast_ok = 0; // every rect/box coordinate finite and <= 2^60: rays may use the shared-reciprocal division
  // PT_FLAG_FAST_RNG (opt-in, not the reference's image): a work unit is one CHUNK of a tile's pixels; `samples` above is
  // then the chunk length, fast_chunks the chunks per pixel, samples_total the caller's spp, fb the partial-sum workspace
  // [chunk][framebuffer layout] (fast_reduce_kernel adds the chunks in order and divides).  0 = the reference's single stream.
  int fast_chunks = 0, samples_total = 0;
  int fast_chunk0 = 0;      // global index of the launch's first chunk (sample windows start at 64 x fast_chunk0; pt_render: 0)
  long long fast_stride = 0; // floats per chunk plane of the workspace
  // the camera rays' candidate cache of the triangle-pool kernels (pt_device.hpp: TriPrimCtx): one line per resident lane; NULL: none
  unsigned int* tri_cache = nullptr;
  float foot[11] = {};      // (llc - origin) xyz, hor / W xyz, ver / H xyz, the bound dd on |d - d_centre| over a pixel's camera rays, dd's rounding term
  float width_f = 0.0f, height_f = 0.0f; // (float)width, (float)height: the divisors of render.hpp:96-97, converted once (lane_regenerate)
};
static_assert(std::is_trivially_copyable<KArgs>::value, "KArgs is copied into the kernarg segment as it is");

// Per-lane state of the persistent loop.  A lane owns ONE pixel at a time, for all of its samples (the
// reference's single RNG stream per pixel, render.hpp:130-133, forbids splitting a pixel), but lanes are not
// tied to a tile: a lane that has finished its pixel pulls the next one from a per-launch queue, so every lane
// of the chip stays busy until the frame's pixels run out.
// The part of a lane's state that is touched only when a sample or a pixel ends — the radiance sum, the sample count,
// which pixel it is — lives either in registers or, for small scenes, in per-thread LDS slots (three LDS instructions per
// finished sample: Cold<true>): 8 registers less pressure inside the traversal.  It would even fit 8 waves per SIMD (64 VGPRs, no
// spill), but that is slower than 7 (-5 % vs +2 % on the headline scene; PT_MIN_WAVES_CL).
typedef __attribute__((address_space(3))) float* lds_fp;
constexpr int kColdSlots = 8; // dwords per thread
template <bool IN_LDS> struct Cold;
template <> struct Cold<false> {
  V3 acc;
  int s, pix, x, y;
  unsigned int iters;
  __device__ __forceinline__ void init(lds_fp) { acc = mk(0.0f, 0.0f, 0.0f); s = 0; pix = -1; x = 0; y = 0; iters = 0; }
  __device__ __forceinline__ void begin(int pix_, int x_, int y_, int s0 = 0) { acc = mk(0.0f, 0.0f, 0.0f); s = s0; iters = 0; pix = pix_; x = x_; y = y_; }
  __device__ __forceinline__ void resume(V3 acc_, int s0) { acc = acc_; s = s0; }
  __device__ __forceinline__ int add_sample(V3 o) { acc = acc + o; return ++s; }
  __device__ __forceinline__ void count_ray() { iters++; }
  __device__ __forceinline__ V3 get_acc() const { return acc; }
  __device__ __forceinline__ int get_s() const { return s; }
  __device__ __forceinline__ int get_pix() const { return pix; }
  __device__ __forceinline__ int get_x() const { return x; }
  __device__ __forceinline__ int get_y() const { return y; }
  __device__ __forceinline__ void get_xy(int& x_, int& y_) const { x_ = x; y_ = y; }
  __device__ __forceinline__ unsigned int get_iters() const { return iters; }
};
// Two 16-byte records per thread: A = (acc.x, acc.y, acc.z, s) at p[0], B = (x, y, pix, iters) at p[kBlock].  A finished sample is ONE
// ds_read_b128, three adds and an increment, ONE ds_write_b128 (field by field, strided kBlock dwords apart, it was four dword reads and four
// dword writes); a new sample reads (x, y) with one ds_read_b64 — they lead B so that the pair is 8-byte aligned.  Thread t's records lie at
// 16 t: each 16-lane group of a b128 access covers 256 contiguous bytes, every bank once.
typedef __attribute__((address_space(3))) f4* lds_rec_p;
typedef int i2v __attribute__((ext_vector_type(2)));
template <> struct Cold<true> {
  lds_rec_p p; // this thread's records: A at p[0], B at p[kBlock]
  __device__ __forceinline__ lds_fp a_word(int k) const { return (lds_fp)p + k; }
  __device__ __forceinline__ lds_fp b_word(int k) const { return (lds_fp)(p + kBlock) + k; }
  __device__ __forceinline__ void init(lds_fp base) { p = (lds_rec_p)base + threadIdx.x; }
  // (the zeros as one opaque 64-bit pair: a constant quad is hoisted out of the loop and held across the traversal — four of its 72 registers —,
  // and a pair is one v_mov_b64 to make and one to copy where four dwords are four moves)
  __device__ __forceinline__ void begin(int pix_, int x_, int y_) {
    unsigned long long z = 0;
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+v"(z));
#endif
    const float zl = __int_as_float((int)(unsigned int)z), zh = __int_as_float((int)(unsigned int)(z >> 32));
    p[0] = f4{zl, zh, zl, zh};
    p[kBlock] = f4{__int_as_float(x_), __int_as_float(y_), __int_as_float(pix_), zh};
  }
  __device__ __forceinline__ void begin(int pix_, int x_, int y_, int s0) {
    p[0] = f4{0.0f, 0.0f, 0.0f, __int_as_float(s0)};
    p[kBlock] = f4{__int_as_float(x_), __int_as_float(y_), __int_as_float(pix_), __int_as_float(0)};
  }
  __device__ __forceinline__ void resume(V3 acc_, int s0) { p[0] = f4{acc_.x, acc_.y, acc_.z, __int_as_float(s0)}; }
  __device__ __forceinline__ int add_sample(V3 o) {
    f4 r = p[0];
    const int s = __float_as_int(r.w) + 1;
    p[0] = f4{r.x + o.x, r.y + o.y, r.z + o.z, __int_as_float(s)};
    return s;
  }
  __device__ __forceinline__ void count_ray() { *b_word(3) = __int_as_float(__float_as_int(*b_word(3)) + 1); }
  __device__ __forceinline__ V3 get_acc() const { const f4 r = p[0]; return mk(r.x, r.y, r.z); }
  __device__ __forceinline__ int get_s() const { return __float_as_int(*a_word(3)); }
  __device__ __forceinline__ int get_pix() const { return __float_as_int(*b_word(2)); }
  __device__ __forceinline__ int get_x() const { return __float_as_int(*b_word(0)); }
  __device__ __forceinline__ int get_y() const { return __float_as_int(*b_word(1)); }
  __device__ __forceinline__ void get_xy(int& x, int& y) const { const i2v v = *(const __attribute__((address_space(3))) i2v*)(p + kBlock); x = v.x; y = v.y; }
  __device__ __forceinline__ unsigned int get_iters() const { return (unsigned int)__float_as_int(*b_word(3)); }
};

template <bool CL>
struct LaneT {
  uint32_t rng;
  V3 att;
  Ray ray;
  int b;
  Cold<CL> cold; // radiance sum, sample count, pixel identity, ray count (cost probe)
  bool live;     // owns a pixel with samples left
  bool retired;  // the queue is empty for this lane
  bool need_new; // next iteration starts a new sample
  bool split_done; // (wave-uniform) the split queue is exhausted
  int wide;        // (wave-uniform) log2 lanes per pixel while this wave serves the split queue; 0 = one lane per pixel
  unsigned int split_pixels; // (wave-uniform) 64 x the tiles handed out through the split queue
};

template <typename Lane>
__device__ __forceinline__ void lane_reset(Lane& L, lds_fp cold_base) {
  L.rng = 0;
  L.att = mk(1.0f, 1.0f, 1.0f);
  L.ray.o = mk(0.0f, 0.0f, 0.0f); L.ray.d = mk(0.0f, 0.0f, 1.0f); L.ray.tm = 0.0f;
  L.b = 0;
  L.cold.init(cold_base);
  L.live = false; L.retired = false; L.need_new = true; L.split_done = false; L.wide = 0; L.split_pixels = 0;
}

// pt_fast_seed (include/pt_render.h), device and host
__host__ __device__ __forceinline__ uint32_t fast_seed(uint32_t pixel, uint32_t chunk) {
  uint32_t h = pixel * 0x9E3779B1u + chunk * 0x85EBCA77u + 0x165667B1u;
  h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
  return h ? h : 1u;
}

// Kernel arguments that only the rare paths read (queue, order, frame geometry, framebuffer ...): read through `a` they are
// SGPR-resident for the whole loop and push other values out into VGPR lanes (v_readlane + hazard nops in the hot path).  The
// rare paths therefore read them from the kernarg segment on the spot, through a pointer the optimiser cannot see through
// (so that the loads stay where they are).  The kernels take KArgs as their only argument: the segment IS a KArgs.
#ifdef __HIP_DEVICE_COMPILE__
#define PT_COLD_ARGS(name, a)                                                            \
  unsigned long long name##_p = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr(); \
  asm volatile("" : "+s"(name##_p));                                                      \
  const __attribute__((address_space(4))) KArgs& name = *(const __attribute__((address_space(4))) KArgs*)name##_p
#else
#define PT_COLD_ARGS(name, a) const KArgs& name = a
#endif

struct __attribute__((packed, aligned(4))) Rgb12 { float r, g, b; }; // a pixel of the framebuffer: global_{load,store}_dwordx3 need dword alignment only

// Wave-aggregated dequeue: one atomicAdd per wave for all lanes that need a pixel (ballot + prefix count),
// pixels handed out in tile order so a fresh wave starts on one coherent 8x8 tile.
//
// Wide phase (COOP kernels, L.wide = log2 G > 0): the heaviest tiles (the first *a.n_split positions of the cost-sorted
// order) come from a queue of their own, one PIXEL per aligned group of G lanes.  All G lanes of a group hold the same
// pixel and compute everything redundantly — same seed, same RNG draws, same shading — except the traversal, where each
// tests 1/G of the list (hit_world_lds) — so a pixel's sequential chain gets shorter without any state ever moving
// between lanes.  A wave leaves the phase when that queue is empty and its last wide pixel is done.
template <bool FAST = false, typename Lane>
__device__ __forceinline__ void lane_acquire(Lane& L, const KArgs& a) {
  // (triangle-pool kernels: a wave's time is the sum over its lanes — when a launch has fewer pixels than lanes, every wave takes
  // its share, lanes_cap pixels, instead of the first waves taking 64 each and the rest none)
  if (a.lanes_cap < 64 && (int)(threadIdx.x & 63) >= a.lanes_cap) L.retired = true;
  const bool want = !L.live && !L.retired;
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(want);
  if (mask == 0) return;
  PT_COLD_ARGS(k, a);
  const int lane = threadIdx.x & 63;
  const int leader = __builtin_ctzll(mask);
  const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
  const unsigned int split_pixels = L.split_pixels; // read once per wave (render_kernel): constant during the launch
  unsigned int i = 0;
  if (L.wide && L.split_done) {                           // nothing left to hand out in this phase:
    if (__builtin_amdgcn_ballot_w64(L.live) != 0) return; //   idle groups wait for the wave's last wide pixels (no memory op)
    L.wide = 0;                                           //   all done: carry on with the ordinary queue below
  }
  if (L.wide) {
    const unsigned int groups = (unsigned int)__builtin_popcountll(mask) >> L.wide; // idle groups (all-or-none per group)
    unsigned int b = 0;
    if (lane == leader) b = atomicAdd(k.queue + 1, groups);
    b = __builtin_amdgcn_readlane(b, leader);
    if (b + groups >= split_pixels) L.split_done = true;
    i = b + (rank >> L.wide);
    const bool got = want && i < split_pixels;
    // wave-uniform decisions first (no ballot under a divergent branch)
    const bool any_got = __builtin_amdgcn_ballot_w64(got) != 0, any_live = __builtin_amdgcn_ballot_w64(L.live) != 0;
    if (!any_got && !any_live) L.wide = 0; // queue was already empty and nothing in flight: ordinary queue below
    else if (!got) return;                 // (groups that got a pixel go on to set it up)
  }
  if (!L.wide) {
    // tile-granular mode: a wave takes its next 64 pixels only when all of its lanes are idle — or (round 6, tile_group = 32 / 16) an aligned
    // GROUP of its lanes takes the next half / quarter tile as soon as that group is idle: a wave's iteration costs the same whether 64 or 40
    // of its lanes are live, and a tile's lanes idle from their own last sample to the tile's (lane utilisation 0.78 on the headline frame)
    unsigned long long mask2 = mask;
    if (k.tile_granular) {
      const unsigned long long live_m = __builtin_amdgcn_ballot_w64(L.live);
      if (k.tile_group >= 64) { if (live_m != 0) return; }
      else {
        const int g0 = lane & ~(k.tile_group - 1);
        const unsigned long long gm = ((k.tile_group == 32 ? 0xffffffffull : 0xffffull) << g0);
        const bool group_idle = (live_m & gm) == 0;
        mask2 = __builtin_amdgcn_ballot_w64(want && group_idle);
        if (mask2 == 0) return;
      }
    }
    // The heaviest tiles in narrower waves.  A tile's time is its heaviest pixel's sequential chain times the wave's iteration, and an
    // iteration of a wave that steps 16 pixels together is shorter than one that steps 64 (the longest grid walk, the largest candidate
    // count, every material among them): the 4K frame's heaviest tiles alone take 55 / 48 / 43 ms at 64 / 32 / 16 lanes.  A launch that is
    // bound by those chains (launch_render: heavy_pixels) hands the head of the cost-sorted queue out heavy_lanes pixels at a time — a
    // quarter of a tile per wave, the other lanes idle until it is done — and everything behind it as whole tiles.  (The peek races with
    // other waves' takes: a wave may take a narrow piece just behind the head, or a whole tile just inside it; both are merely other
    // partitions of the same pixels.  At launch every resident wave peeks an untouched queue, so the head is never shorter than one piece per
    // wave — a quarter of the resident waves in tiles, which is the rule's own length; shorter forced heads measure the same.)
    const bool want2 = want && ((mask2 >> lane) & 1ull);
    const int leader2 = __builtin_ctzll(mask2);
    const unsigned int rank2 = __builtin_amdgcn_mbcnt_hi((unsigned int)(mask2 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask2, 0u));
    unsigned int take = (unsigned int)__builtin_popcountll(mask2);
    if (k.heavy_pixels > 0 && k.tile_granular) {
      unsigned int cur = 0;
      if (lane == leader2) cur = __hip_atomic_load(k.queue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      cur = __builtin_amdgcn_readlane(cur, leader2);
      if (cur < (unsigned int)k.heavy_pixels) take = min(take, (unsigned int)k.heavy_lanes);
    }
    unsigned int base = 0;
    if (lane == leader2) base = atomicAdd(k.queue, take);
    base = __builtin_amdgcn_readlane(base, leader2);
    if (!want2 || rank2 >= take) return;
    i = split_pixels + base + rank2;
  }
  if (i >= (unsigned int)k.n_local_pixels) { L.retired = true; return; }
  // fast mode: the queue hands out (tile, chunk) units, a tile's chunks back to back
  unsigned int unit = i >> 6;
  int in_tile = (int)(i & 63);
  {
    // Triangle-pool kernels: a wave takes its live rays ONE AT A TIME, so its time is the SUM over its lanes' pixels, and 64 pixels of
    // one heavy tile in one wave are a chain 64 times as long as the heaviest pixel's (a shard of 1/8 of the 100 k-triangle frame took
    // 3.3 s of the whole frame's 3.8 s).  So consecutive queue positions are dealt in runs of 2^scatter_log pixels (default: single
    // pixels) to tiles that lie scatter_p apart in the (cost-sorted) order: a wave's 64 pixels come from 64 tiles spread evenly over the
    // cost distribution — every wave gets a stratified sample of the frame's work — and a tile's pixels go to 64 different waves.
    // 1080p x 32 spp: whole frame 3.78 -> 3.12 s, shard 0/8 3.29 -> 0.53 s (runs of 2 / 4 / 8 / 16 pixels: 0.59 / 0.65 / 0.82 / 1.22 s).
    // A bijection of [0, 64 nt): run c = i >> g -> (position c mod nt, run-in-tile (c / nt) mod (64 >> g)), position -> position *
    // scatter_p mod nt with gcd(scatter_p, nt) = 1.  Which pixel a lane renders changes nothing in the image: a pixel's seed is its id.
    if (k.scatter_p > 0) {
      const unsigned int g = (unsigned int)k.scatter_log, nt = (unsigned int)k.n_local_pixels >> 6, c = i >> g;
      const unsigned int pos = c % nt, row = (c / nt) & ((64u >> g) - 1u);
      unit = (unsigned int)(((unsigned long long)pos * (unsigned int)k.scatter_p) % nt);
      in_tile = (int)((row << g) + (i & ((1u << g) - 1u)));
    }
  }
  int chunk = 0;
  if constexpr (FAST) { chunk = (int)(unit % (unsigned int)k.fast_chunks); unit /= (unsigned int)k.fast_chunks; } // (fast mode: nt counts (tile, chunk) units)
  // queue position -> local tile: identity, or the cost-sorted order of the probe pass (heaviest tiles first)
  const int l = k.order ? k.order[unit] : (int)unit;
  const long long g = (long long)l * k.shard_count + k.shard_index; // global tile (pt_render.h: round-robin shards)
  const int tx = (int)(g % k.tiles_x), ty = (int)(g / k.tiles_x);
  const int x = tx * PT_TILE + (in_tile & 7), y = ty * PT_TILE + (in_tile >> 3);
  // padding pixel, or a pixel outside a masked window's mask: stays as it is, ask again next iteration
  if (g >= k.n_tiles || x >= k.width || y >= k.height ||
      (k.mask && !k.mask[k.shard_count == 1 ? (long long)y * k.width + x : (long long)l * PT_TILE_PIXELS + in_tile])) return;
  // render.hpp:130-132: seed = linear id of the pixel in the WHOLE frame, truncated to 32 bits
  const uint32_t id = (uint32_t)((unsigned long long)y * (unsigned long long)k.width + (unsigned long long)x);
  if constexpr (FAST) {
    // the last chunk of a pixel may be shorter: its sample counter starts ahead so that every chunk ends at k.samples
    const int n_here = min(k.samples, k.samples_total - chunk * k.samples);
    L.cold.begin((l * PT_TILE_PIXELS + in_tile) | (chunk << 24), x, y, k.samples - n_here);
    L.rng = fast_seed(id, (uint32_t)(chunk + k.fast_chunk0));
  } else {
    L.cold.begin(l * PT_TILE_PIXELS + in_tile, x, y);
    L.rng = id;
    if (k.resume_spp > 0) { // the probe pass rendered this pixel's first samples (KArgs.resume_rng): carry on where it stopped
      const int pix = l * PT_TILE_PIXELS + in_tile;
      const long long at = k.shard_count == 1 ? ((long long)y * k.width + x) * 3 : (long long)pix * 3;
      const Rgb12 part = *(const Rgb12*)(k.fb + at);
      L.cold.resume(mk(part.r, part.g, part.b), k.resume_spp);
      L.rng = k.resume_rng[pix];
    }
  }
  L.live = true;
  L.need_new = true;
}

// One 12-byte store per finished pixel (render.hpp:105): global_store_dwordx3 needs dword alignment only.
// (HBM write traffic of a frame launch: 26.3 MB against the algorithmic 24.9 MB — profiles/r03_cornell_pmc_write.csv, the
// 148 ms dispatch.  The "68 MB" of the round-2 summaries was the cost-probe launch's per-pixel atomics, picked up because the
// summary took each counter's maximum over the two launches: tools/pmc_summary.py now reads the frame launch only.  Deferring
// the stores until a wave's whole tile is done — eight lanes writing 96 contiguous bytes — was tried and changes nothing:
// 26.26 MB.)
__device__ __forceinline__ void store_rgb(float* p, V3 c) { *(Rgb12*)p = Rgb12{c.x, c.y, c.z}; }

template <bool FAST = false, typename Lane>
__device__ __forceinline__ void lane_store(Lane& L, const KArgs& a) {
  L.live = false;
  PT_COLD_ARGS(k, a);
  if (L.wide && ((threadIdx.x & 63) & ((1 << L.wide) - 1))) return; // wide phase: one lane of the group writes
  if (k.cost || k.keep_state) {
    if (k.cost) { // cost-probe pass: only the tile's ray count is kept
      // a wave holds a tile until its last pixel is done, so a tile's duration follows its heaviest pixel; the cooperative
      // kernels' model also needs the lane time, i.e. the sum
      if (k.cost_max) atomicMax(&k.cost[L.cold.get_pix() >> 6], L.cold.get_iters() * PT_TILE_PIXELS);
      else atomicAdd(&k.cost[L.cold.get_pix() >> 6], L.cold.get_iters());
    }
    // ... and, where a later launch resumes from it (the frame launch after the probe, the next sample window of a PtAccum), the
    // pixel's state after these samples (KArgs.resume_rng)
    if (k.resume_rng) {
      const long long at = k.shard_count == 1 ? ((long long)L.cold.get_y() * k.width + L.cold.get_x()) * 3 : (long long)L.cold.get_pix() * 3;
      store_rgb(k.fb + at, L.cold.get_acc());
      k.resume_rng[L.cold.get_pix()] = L.rng;
    }
    return;
  }
  long long idx;
  if constexpr (FAST) { // fast mode: this chunk's plain sum into its plane of the workspace
    const int packed = L.cold.get_pix(), pix = packed & 0xffffff;
    if (k.shard_count == 1) idx = ((long long)L.cold.get_y() * k.width + L.cold.get_x()) * 3;
    else idx = (long long)pix * 3;
    idx += (long long)(packed >> 24) * k.fast_stride;
    store_rgb(k.fb + idx, L.cold.get_acc());
    return;
  }
  V3 acc = L.cold.get_acc() / (float)k.samples; // render.hpp:102
  if (k.shard_count == 1) idx = ((long long)L.cold.get_y() * k.width + L.cold.get_x()) * 3;
  else idx = (long long)L.cold.get_pix() * 3;
  store_rgb(k.fb + idx, acc);
}

// Start the next sample of a lane whose path ended (render.hpp:95-99); the pixel itself is finished where its last
// sample ends (lane_shade), so this — and the camera code — appears once in the loop.
template <typename Lane>
__device__ __forceinline__ void lane_regenerate(Lane& L, const KArgs& a) {
  if (L.live && L.need_new) {
    // The camera is 30 floats of kernel argument.  Read through `a.cam` they sit in SGPRs for the whole loop, and the
    // register allocator, out of SGPRs, parks others in VGPR lanes (v_writelane / v_readlane + hazard s_nops all over the
    // loop).  KArgs starts with the camera, so here it is read from the kernarg segment where it is needed: four scalar
    // loads per regeneration instead.  (The pointer is made opaque so that the loads are not hoisted out of the loop.)
    static_assert(offsetof(KArgs, cam) == 0, "the camera leads the kernel arguments");
#ifdef __HIP_DEVICE_COMPILE__
    typedef const __attribute__((address_space(4))) Cam* kcam_p;
    unsigned long long kp = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    const Cam cam = *(kcam_p)kp;
    const __attribute__((address_space(4))) KArgs& k = *(const __attribute__((address_space(4))) KArgs*)kp; // frame geometry: same reasoning
#else
    const Cam cam = a.cam; // (host pass of the single-source compile: never run)
    const KArgs& k = a;
#endif
    // (the frame's size as floats, converted once on the host: set_frame.  The pixel's x and y stay integers in the cold state: its eight
    // slots are taken, and lane_store needs the integers for frames wider than 2^24, where the float does not give them back)
    int px, py;
    L.cold.get_xy(px, py);
    L.ray = camera_ray(cam, (float)px, (float)py, k.width_f, k.height_f, k.inv_w, k.inv_h, L.rng, k.pinhole != 0);
    L.att = mk(1.0f, 1.0f, 1.0f);
    L.b = 0;
    L.need_new = false;
  }
}

// The texture coordinates of a lane's hit, asked for by image textures only (pt_device.hpp: texture_value): (u, v) as the reference
// defines them, and — for kernels that derive them from the final hit — the sphere's normal itself, from which the texel follows
// without the mercator pair wherever that is unambiguous (pt_device.hpp: sphere_texel_fast).
template <int UV, typename PB>
struct HitUv {
  PB recs;
  const HitState& h;
  const Ray& ray;
  const Rec& rec;
  __device__ __forceinline__ void operator()(float& u, float& v) const {
    if (UV == UV_TRACKED) { u = h.u; v = h.v; }
    else if (UV == UV_WINNER) winner_uv(recs, h.hit, ray, h.closest, rec, u, v);
    else { u = 0.0f; v = 0.0f; }
  }
  __device__ __forceinline__ bool sphere_normal(V3& n) const {
    if constexpr (UV == UV_WINNER) {
      if (hit_kind(h.hit) == DK_SPHERE) { n = rec.normal; return true; } // winner_uv: mercator(rec.normal)
    }
    return false;
  }
};

// emitted / scatter / sky for the nearest hit (render.hpp:60-88) and the sample bookkeeping (:100).
// SKY_FIRST (the headline family: kernels without a grid walk, a cooperative phase or a pool): the sky's colour is computed ahead of the hit
// branch, for every lane.  Everything that reads the ray and the attenuation this iteration came in with is then computed BEFORE any
// branch writes the next ones, so the branches write the lane state in place, under their own EXEC mask (some lane of 64 nearly always
// misses everything, so a wave walks through the sky's code anyway; lanes with a hit drop the value) — computed inside the miss branch,
// behind the hit branch in program order, it kept the old ray and attenuation alive across the hit branch and the whole lane state was
// built in a second register set and moved back at the loop's back-edge (45 v_mov per iteration).  The price: where NO lane of a wave
// misses — a closed scene — the sky's code ran for nothing: ~17 issue slots of an iteration's ~900 when every live ray is regular, ~30 on
// the general path.  The other kernel families keep the sky inside the miss branch: their iterations are several
// times as long, and the cooperative kernels and irregular waves would pay the general path.
// SHADE_REC (kernels of rect / box-only scenes with lambertian + light materials whose records AND materials are in LDS — the headline kernel):
// the hit is shaded from its ONE shade record (pt_device.hpp: shade_record) — every scene these kernels are chosen for has the table (choose_variant)
// — instead of two records of the hittable and two of the material in two dependent round trips.
template <int UV, bool FAST = false, int MATS = MATS_ALL, bool SKY_FIRST = false, typename Lane, typename PB, typename PM>
__device__ __forceinline__ void lane_shade(Lane& L, const KArgs& a, const HitState& h, PB recs, PM mats, bool regular = false) {
  constexpr bool SHADE_REC = !FAST && MATS == (MATS_LAMB_LIGHT_SOLID | MATS_RECTBOX_ONLY) && __is_same(PB, lds_f4p) && __is_same(PM, lds_f4p);
  if (!L.live) return;
  if (a.cost) L.cold.count_ray(); // cost-probe pass (wave-uniform)
  V3 out = mk(0.0f, 0.0f, 0.0f);
  bool cont = false;
  auto hit_branch = [&]() {
    if constexpr (SHADE_REC) {
      f4 M0, M1;
      const Rec rec = shade_record(recs, a.shade_k, h.hit, L.ray, h.closest, M0, M1); // per-lane gather of the one shade record of what was hit
      const HitUv<UV, PB> uv{recs, h, L.ray, rec};
      cont = shade_with<(MATS & 0x1ff)>(M0, M1, mats, a.atlas, rec, uv, L.ray, L.att, L.rng, out, regular);
    } else {
    Rec rec = resolve_hit<(MATS & MATS_RECTBOX_ONLY) != 0>(recs, h.hit, L.ray, h.closest); // per-lane gather of the one record that was hit
    // UV_TRACKED kernels carried u,v through the scan (stale values included); UV_WINNER derives them from the final hit
    // when an image texture asks; UV_NONE: the scene has no image texture, nothing reads them
    const HitUv<UV, PB> uv{recs, h, L.ray, rec};
    cont = shade<(MATS & 0x1ff)>(mats, a.atlas, rec, uv, L.ray, L.att, L.rng, out, regular);
    }
    if (cont && ++L.b >= a.depth) { // bounce loop exhausted: black (render.hpp:91)
      out = mk(0.0f, 0.0f, 0.0f);
      cont = false;
    }
  };
  if constexpr (SKY_FIRST) {
    out = sky_color(L.ray, L.att, regular);
    if (h.hit >= 0) hit_branch();
  } else {
    if (h.hit < 0) out = sky_color(L.ray, L.att, regular);
    else hit_branch();
  }
  if (!cont) {
    L.need_new = true;
    // final_color += get_color(r)  render.hpp:100; pixel done: the lane is idle from here on
    if (L.cold.add_sample(out) == a.samples) lane_store<FAST>(L, a);
  }
}

// One turn of the crank before tracing: finish/advance pixels, pull new ones, start new samples.
// Returns false when this lane has nothing to trace this iteration.
template <bool FAST = false, typename Lane>
__device__ __forceinline__ void lane_prepare(Lane& L, const KArgs& a) {
  lane_acquire<FAST>(L, a); // idle lanes pull their next pixel ...
  lane_regenerate(L, a); // ... and every lane whose path ended (or that is new) starts a sample
}

#ifdef PT_STAMPS
// Diagnostic build only (`make stamps` -> libpt_stamps.so; never shipped, never timed): s_memtime shares of one loop
// iteration of the resident kernels, summed over waves; read with pt_debug_stamps / tools/stamps.py.
#define PT_STAMP(var) unsigned long long var = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0)
#endif

// Scene blob resident for the whole kernel: staged once into LDS (LDS=true) or read through the scalar cache.
// MLDS: the material table is staged too (small tables only: it rides behind the records in the same buffer), so
// the whole bounce — traversal, hit record, material, texture constants — runs out of LDS without a global load.
// COOP: the traversal can split a ray's list over idle lanes (hit_world_lds); costs ~10 VGPRs and ~7 % of the
// ordinary-mode throughput, so the launcher picks it only where the makespan floor matters (choose_variant).
// CL: the cold part of the lane state lives in LDS (Cold<true>); small scenes only (8 KB per workgroup).
// FAST: PT_FLAG_FAST_RNG (opt-in decorrelated mode; its own instantiations, so the parity kernels carry none of it)
// BADOUEL: the scene has Badouel-strategy triangles (their loop is compiled only into these instantiations)
// GRID: the kernel carries the sphere-grid walk (pt_device.hpp: sphere_grid_walk).  Scenes without a culling grid and without
// an image texture — the headline Cornell-style scene — run instantiations without it (less code in the hot kernel, and
// nothing the walk needs can weigh on its 72-register budget).
// TRIPOOL: the kernel carries the exact culling of long triangle runs (pt_device.hpp: tri_pool_scan); scalar-cache variant only
// (such scenes are far beyond LDS), its own register budget.
// MATS: the material / texture kinds the scene can contain (pt_device.hpp: MATS_*): the headline family has instantiations for
// "lambertian + lightsource over solid textures" that carry no metal / glass / isotropic / checker / image code.
// BLOCK: threads per workgroup.  The loop has no barrier, so the workgroup size only decides how many waves share one LDS image of the scene:
// the 496-hittable scene's 31 KB image + the queued walk's per-wave LDS (1 KB) fit four workgroups per CU, i.e. four waves per SIMD at 256
// threads and five at 320 (kGridBlock).
template <int UV, bool LDS, bool MLDS, bool COOP, bool CL = false, bool FAST = false, bool BADOUEL = false, int GRID = 1, bool TRIPOOL = false,
          int MATS = MATS_ALL, int BLOCK = kBlock>
__global__ __launch_bounds__(BLOCK, TRIPOOL ? PT_MIN_WAVES_TRIPOOL : CL ? PT_MIN_WAVES_CL : COOP ? (UV ? PT_MIN_WAVES_COOP_IMG : PT_MIN_WAVES_COOP) : (UV ? PT_MIN_WAVES_IMG : PT_MIN_WAVES))
void render_kernel(KArgs a) {
  constexpr bool IMG = UV == UV_TRACKED;
  constexpr bool kSkyFirst = GRID == 0 && !COOP && !FAST && !TRIPOOL; // the headline family (lane_shade)
  typedef LaneT<CL> Lane;
  static_assert(!CL || BLOCK == kBlock, "the LDS-resident cold lane state is laid out for kBlock threads");
  static_assert(BLOCK % 64 == 0 && BLOCK / 64 <= PT_MAX_WAVES_PER_BLOCK, "per-wave LDS arrays are sized for PT_MAX_WAVES_PER_BLOCK waves");
  static_assert(!TRIPOOL || BLOCK == kBlock, "the triangle pool's per-wave LDS arrays are sized for kBlock threads");
  __shared__ __attribute__((aligned(16))) float cold_slots[CL ? kColdSlots * kBlock : 1];
  extern __shared__ f4 smem[];
  if (LDS) {
    const int n = a.blob_f4 + (MLDS ? a.mats_f4 : 0); // a.mats == a.blob + a.blob_f4 (one device buffer)
    for (int i = threadIdx.x; i < n; i += BLOCK) smem[i] = a.blob[i];
    __syncthreads();
  }
#ifdef PT_STAMPS_WALK
  if (threadIdx.x < 8) walk_ctr()[threadIdx.x] = 0;
  __syncthreads();
#endif
#ifdef PT_STAMPS_BLOCKS
  if (threadIdx.x == 0 && !a.cost && blockIdx.x < 8192) {
    const unsigned long long where = ((unsigned long long)__builtin_amdgcn_s_getreg(0x1814) << 32) | (unsigned int)__builtin_amdgcn_s_getreg(0xF804); // XCC_ID, HW_ID
    g_blocks[3 * blockIdx.x] = where;
    g_blocks[3 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
  }
  struct BlockEnd { bool on; unsigned int b; __device__ ~BlockEnd() { if (on) g_blocks[3 * b + 2] = __builtin_amdgcn_s_memrealtime(); } } block_end{threadIdx.x == 0 && !a.cost && blockIdx.x < 8192, blockIdx.x};
#endif
  Lane L;
  lane_reset(L, (lds_fp)cold_slots);
  if (COOP && a.n_split) {
    L.split_pixels = (unsigned int)a.n_split[0] * PT_TILE_PIXELS;
    L.wide = a.n_split[1];
  }
  if (a.depth <= 0) return; // depth 0: every sample returns black (render.hpp:58,91); the frame is pre-zeroed
#ifdef PT_STAMPS
  unsigned long long s_prep = 0, s_trav = 0, s_shade = 0, s_iters = 0;
#endif
  unsigned int prio_it = 0; // (headline family) iterations of this wave, for the priority poll below
  for (;;) {
#ifdef PT_STAMPS
    PT_STAMP(t0);
#endif
    // LONGEST REMAINING CHAIN FIRST, from mid-frame on (headline family only: kernels without a grid walk, a cooperative phase or a pool).
    // All resident waves take the heaviest tiles at t = 0, and a third of them never take another: their tile runs for the whole frame,
    // at 3.5 x a lone wave's iteration because six other waves share the SIMD's issue slots — and the frame ends with the longest of those
    // chains, ~10 ms after its work would be done if it could be spread (profiles/r05_wave_tail_cornell.txt).  A pixel's chain cannot be
    // cut, but its wave can be given the slots: once half the queue is taken, every wave tells the SIMD's arbiter how much its slowest
    // pixel still has to do — more than 1/2, 1/4, 1/8 of the samples: priority 3, 2, 1 (s_setprio; polled every 64 iterations: one scalar
    // compare per iteration, ~25 instructions per poll).  Waves on light tiles lose slots they had to spare; the long chains end earlier:
    // Cornell-style 1080p x 1024 spp 139.5 -> 128.2 ms, x 256 spp 37.8 -> 34.9, shard 0 of 4 / 8: 51.9 / 41.6 -> 45.6 / 40.3
    // (profiles/r05_ab_chain_priority.txt; ladders 2.5-5-10, 3-6-12, 2-4-16 and onsets 7/16 ... 9/16 within 1 %; from the start of the
    // frame, or by the PROBE's estimate of a tile's heaviest pixel: worse than none — what a wave knows about its own progress is exact, what the
    // probe guessed is not).  The grid kernels lose 5 % with it (latency-bound at four waves per SIMD) and do not carry it.
    if constexpr (GRID == 0 && !COOP && !FAST && !TRIPOOL && LDS) {
      if (a.prio_t1 > 0 && ((++prio_it) & 63u) == 0u) {
        PT_COLD_ARGS(k, a);
        unsigned int head = 0;
        if ((threadIdx.x & 63) == 0) head = __hip_atomic_load(k.queue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        head = __builtin_amdgcn_readfirstlane(head);
        if (head >= (unsigned int)k.prio_onset) {
          int rem = L.live ? k.samples - L.cold.get_s() : 0;
#pragma unroll
          for (int st = 32; st >= 1; st >>= 1) rem = max(rem, __shfl_xor(rem, st, 64));
          if (rem >= k.prio_t3) __builtin_amdgcn_s_setprio(3);
          else if (rem >= k.prio_t2) __builtin_amdgcn_s_setprio(2);
          else if (rem >= k.prio_t1) __builtin_amdgcn_s_setprio(1);
          else __builtin_amdgcn_s_setprio(0);
        }
      }
    }
    // Pull until some lane has a ray to trace.  (A loop of its own around lane_prepare, not a `continue` of the outer one: on a path that
    // skips the traversal and the shading, the compiler's structured control flow leaves the lane state that the shading writes undefined,
    // which kept it from being written in place — the whole lane state went through a second register set on every iteration.  A pull that
    // brings only padding pixels used to pass the priority poll above again and count as an iteration of prio_it; now it does neither, so
    // the poll's 64-iteration cadence counts traced iterations only: a shift of a few iterations for the waves that meet edge tiles.)
    bool drained = false;
    do {
      lane_prepare<FAST>(L, a);
      if (__builtin_amdgcn_ballot_w64(L.live) != 0) break;
      drained = __builtin_amdgcn_ballot_w64(!L.retired) == 0; // queue drained for the whole wave; else only padding pixels this time: pull again
    } while (!drained);
    if (drained) break;
#ifdef PT_STAMPS
    PT_STAMP(t1);
#endif
    HitState h;
    bool regular = false; // (wave-uniform) every live ray is regular: the sky's shortcut (sky_unit_y)
    if constexpr (LDS) {
      if constexpr (COOP) {
        // ordinary and cooperative traversal (few live lanes: each live ray's list split over the idle lanes)
        const CoopScene cs{a.n_runs, a.coop_prefix};
        hit_world_lds<IMG>((lds_f4p)smem, (cst_f4p)a.blob, cs, L.ray, L.rng, L.live, true, a.fast_ok != 0, L.wide, h);
      } else {
        // (rect / box-only scenes) the pool plan: ONE load from the kernarg segment per bounce, requested ahead of the ray context's
        // reciprocals, which hide it; through an opaque pointer, like the camera in lane_regenerate and for its reason — eight more
        // SGPRs held across the whole loop are what the allocator parks in VGPR lanes
        PoolPlan plan;
        if constexpr ((MATS & MATS_RECTBOX_ONLY) != 0) {
          static_assert(offsetof(KArgs, plan) == sizeof(Cam), "the pool plan rides behind the camera");
#ifdef __HIP_DEVICE_COMPILE__
          unsigned long long kp = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
          asm volatile("" : "+s"(kp));
          // (as ONE vector of the four words the pool needs: member by member it is three loads; all eight, and the allocator reuses the
          // registers of the words nobody reads while the load is in flight — a full wait a few instructions behind it)
          typedef int i4v __attribute__((ext_vector_type(4)));
          const i4v w = *(const __attribute__((address_space(4))) i4v*)(kp + offsetof(KArgs, plan));
          plan.one = w[0]; plan.n = w[1]; plan.bmax = __int_as_float(w[2]); plan.x_off = w[3];
#else
          plan = a.plan;
#endif
        }
        // (the headline family votes on masks: the irregular lanes' from the context's own comparisons, the live lanes' the one the pull loop
        // above has just tested — two scalar instructions where the vote on the per-lane flags materialised them first)
        unsigned long long irregular = 0;
        RayCtx c = kSkyFirst ? make_ctx<true>(L.ray, a.fast_ok != 0, &irregular) : make_ctx(L.ray, a.fast_ok != 0);
        c.live = L.live;
        const bool fast = kSkyFirst ? (irregular & __builtin_amdgcn_ballot_w64(L.live)) == 0 : wave_all_regular(c, L.live);
        regular = fast;
        hit_world<IMG, BADOUEL, GRID, false, (MATS & MATS_RECTBOX_ONLY) != 0>((lds_f4p)smem, (cst_f4p)a.blob, a.n_runs, c, fast, L.rng, h, nullptr, nullptr, &plan);
      }
#ifdef PT_STAMPS
      asm volatile("" ::"v"(h.closest), "v"(h.hit));
      PT_STAMP(t2);
#endif
      if constexpr (MLDS) lane_shade<UV, FAST, MATS, kSkyFirst>(L, a, h, (lds_f4p)smem, (lds_f4p)smem + a.blob_f4, regular);
      else lane_shade<UV, FAST, MATS, kSkyFirst>(L, a, h, (lds_f4p)smem, a.mats, regular);
#ifdef PT_STAMPS
      asm volatile("" ::"v"(L.att.x), "v"(L.ray.d.x));
      PT_STAMP(t3);
      s_prep += t1 - t0; s_trav += t2 - t1; s_shade += t3 - t2; s_iters++;
#endif
    } else {
      RayCtx c = make_ctx(L.ray, a.fast_ok != 0);
      c.live = L.live;
      const bool fast = wave_all_regular(c, L.live);
      if constexpr (TRIPOOL) {
        TriPrimCtx pc;
        pc.cache = a.tri_cache;
        pc.prim = L.live && L.b == 0;
        pc.xy = L.cold.get_x() | (L.cold.get_y() << 16);
        pc.pix = L.cold.get_pix();
#ifdef __HIP_DEVICE_COMPILE__
        pc.foot = (const __attribute__((address_space(4))) float*)((unsigned long long)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(KArgs, foot));
#else
        pc.foot = nullptr;
#endif
        hit_world<IMG, BADOUEL, GRID, TRIPOOL, (MATS & MATS_RECTBOX_ONLY) != 0>((cst_f4p)a.blob, (cst_f4p)a.blob, a.n_runs, c, fast, L.rng, h, a.pool, &pc);
      } else
      hit_world<IMG, BADOUEL, GRID, TRIPOOL, (MATS & MATS_RECTBOX_ONLY) != 0>((cst_f4p)a.blob, (cst_f4p)a.blob, a.n_runs, c, fast, L.rng, h, a.pool);
      lane_shade<UV, FAST, MATS, kSkyFirst>(L, a, h, a.blob, a.mats, fast);
    }
  }
#ifdef PT_STAMPS_WALK
  __syncthreads();
  if (threadIdx.x < 8) atomicAdd(&g_walk[threadIdx.x], walk_ctr()[threadIdx.x]);
#endif
#ifdef PT_STAMPS
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&g_stamps[0], s_prep); atomicAdd(&g_stamps[1], s_trav); atomicAdd(&g_stamps[2], s_shade);
    atomicAdd(&g_stamps[3], s_iters);
  }
#endif
}

// Scene blob larger than LDS (100 k triangles = 4.8 MB): the workgroup walks the list in lock-step and streams
// each run through one LDS tile — cooperative 16 B/lane copy, barrier, every wave tests its 64 rays against the
// tile's records by LDS broadcast, barrier.  Arithmetic intensity is ~200 lane-ops per streamed byte
// (256 rays x ~40 ops per 48-byte triangle), so the stream needs < 0.4 TB/s chip-wide: compute-bound by design.
constexpr int kTileF4 = 2016;      // 32,256 B; a multiple of every record size (2, 3, 4 f4); five workgroups per CU
constexpr int kSmallRunF4 = 48;    // runs this short are read through the scalar cache instead (no barriers)

// Tail of such a frame: a pixel is one sequential chain and a full scan of the list is long (100 k triangles: ~15 ms per
// workgroup iteration), so the heaviest pixels (8-15 rays per sample against a mean of 2) keep a few lanes busy long after
// the queue is empty, while the lock-step scan costs the same whether 1 or 64 lanes of a wave are live.  So a wave that is
// down to <= 32 live rays spreads each of them over G = 64 >> ceil(log2 live) lanes for the whole scan (lane j of a group
// tests every G-th record of each tile; one butterfly merge with the reference's acceptance rule at the end: see
// hit_world_lds), and a wave with no live ray only keeps the barriers.  Scenes with a constant_medium (in-traversal RNG
// draw) or stale-u,v hazards scan the ordinary way.
template <int UV, bool FAST = false, bool BADOUEL = false>
__global__ __launch_bounds__(kBlock) void render_kernel_stream(KArgs a) {
  constexpr bool IMG = UV == UV_TRACKED;
  __shared__ f4 tile[kTileF4];
  typedef LaneT<false> Lane;
  Lane L;
  lane_reset(L, (lds_fp) nullptr);
  if (a.depth <= 0) return;
  const cst_f4p cblob = (cst_f4p)a.blob;
  const bool coop_scene = !IMG && a.coop_prefix >= a.n_hittables; // list splittable end to end (no medium)
  for (;;) {
    lane_prepare<FAST>(L, a);
    if (!__syncthreads_or(L.live)) {
      if (!__syncthreads_or(!L.retired)) break;
      continue;
    }
    RayCtx c = make_ctx(L.ray, a.fast_ok != 0);
    c.live = L.live;
    const bool fast = wave_all_regular(c, L.live);
    const unsigned long long live_mask = __builtin_amdgcn_ballot_w64(L.live);
    const int nlive = __builtin_popcountll(live_mask);
    const bool wave_idle = nlive == 0; // nothing to trace: this wave only copies tiles and keeps the barriers
    int logG = 0;
    if (coop_scene && fast && nlive >= 1 && nlive <= 32) {
      logG = coop_group_log(nlive);
      coop_handoff(c, live_mask, nlive, logG);
      c.live = ((threadIdx.x & 63) >> logG) < nlive; // lanes of a group that serves a live ray
    }
    const int j = (threadIdx.x & 63) & ((1 << logG) - 1);
    HitState h;
    hit_begin(h);
    for (int ri = 0; ri < a.n_runs; ++ri) {
      f4 runf = cblob[ri];
      const int kind = as_i(runf.x) & 7, off = as_i(runf.y), cnt = as_i(runf.z); // (& 7: this kernel scans every run where it stands, absorbed or not — pt_flatten.hpp)
      const int sz = record_size(kind);
      if (cnt * sz <= kSmallRunF4) {
        if (!wave_idle) {
          if (logG) hit_records_strided<IMG>(a.blob + off, cblob, kind, cnt, 0, off, j, logG, c, h);
          else hit_records<IMG, 4, 4, true, BADOUEL, false>(cblob + off, cblob, kind, cnt, off, c, fast, L.rng, h);
        }
        continue;
      }
      const int per_tile = kTileF4 / sz;
      for (int first = 0; first < cnt; first += per_tile) {
        const int n = min(per_tile, cnt - first);
        const int nf4 = n * sz, base = off + first * sz;
        for (int i = threadIdx.x; i < nf4; i += kBlock) tile[i] = a.blob[base + i];
        __syncthreads();
        if (!wave_idle) {
          if (logG) hit_records_strided<IMG, false>((lds_f4p)tile, cblob, kind, n, 0, base, j, logG, c, h);
          else hit_records<IMG, 4, 4, false, BADOUEL, false>((lds_f4p)tile, cblob, kind, n, base, c, fast, L.rng, h);
        }
        __syncthreads();
      }
    }
    if (logG) coop_merge_handback<IMG>(h, live_mask, L.live, logG);
    lane_shade<UV, FAST>(L, a, h, a.blob, a.mats);
  }
}

// The reference's single-task executor (render.hpp:113-122, USE_SINGLE_TASK): one default-seeded RNG for the whole frame,
// pixels x-outer / y-inner.  One sequential chain by definition, so one wave runs it (launch <<<1, 64>>>, every lane the same);
// u,v are tracked through the scan as the reference's temp_rec does (no per-scene kernel choice for a parity-only mode).
__global__ __launch_bounds__(64) void render_single_stream_kernel(KArgs a) {
  // all 64 lanes run the same chain redundantly (the traversal's wave-level exchanges need a full wave); lane 0 stores
  const bool writer = threadIdx.x == 0;
  const cst_f4p cblob = (cst_f4p)a.blob;
  uint32_t rng = 2463534242u; // xorshift.hpp:18
  for (int x = 0; x != a.width; ++x)
    for (int y = 0; y != a.height; ++y) {
      V3 acc = mk(0.0f, 0.0f, 0.0f);
      for (int s = 0; s < a.samples; ++s) {
        Ray ray = camera_ray(a.cam, x, y, a.width, a.height, a.inv_w, a.inv_h, rng, a.pinhole != 0);
        V3 att = mk(1.0f, 1.0f, 1.0f), out = mk(0.0f, 0.0f, 0.0f); // depth exhausted: black (render.hpp:91)
        for (int b = 0; b < a.depth; ++b) {
          RayCtx c = make_ctx(ray, a.fast_ok != 0);
          HitState h;
          hit_world<true, true>(a.blob, cblob, a.n_runs, c, c.reg, rng, h);
          if (h.hit < 0) { out = sky_color(ray, att); break; }
          const Rec rec = resolve_hit(a.blob, h.hit, ray, h.closest);
          auto uv = [&](float& u, float& v) { u = h.u; v = h.v; };
          if (!shade(a.mats, a.atlas, rec, uv, ray, att, rng, out)) break;
          out = mk(0.0f, 0.0f, 0.0f);
        }
        acc = acc + out;
      }
      const V3 mean = acc / (float)a.samples;
      float* px = a.fb + ((long long)y * a.width + x) * 3;
      if (writer) { px[0] = mean.x; px[1] = mean.y; px[2] = mean.z; }
    }
}

#include "pt_binned.hpp"

// ---- longest-processing-time-first tile order -------------------------------------------------------------
// A pixel cannot be split (one sequential RNG stream), so the frame's makespan is bounded below by its heaviest
// tile, and a heavy tile picked up LAST adds its whole duration to the tail (measured on the 496-hittable scene:
// mean 2.4 of 5 resident waves per SIMD over the launch).  A probe pass renders the first few samples of every
// pixel and counts rays per tile (same seeds; since round 5 the frame launch resumes from those samples — KArgs.resume_rng); this kernel buckets the tiles
// into 32 classes of ratio 2^(1/4) below the maximum and emits them heaviest class first.  The order only decides
// WHEN a pixel is rendered, never its value, so the (atomic, run-to-run varying) order inside a class is harmless.
// A tile's estimate is its heaviest pixel over a few samples — a noisy number for exactly the pixels that matter (an isolated glass or smoke
// pixel takes 3 rays or 50 per sample), and the two ways of being wrong are not alike: a tile that starts too early costs nothing, a heavy
// tile that starts late is the frame's tail.  So, for whole frames, a tile is ranked by the largest estimate among itself and its eight
// neighbours (a dilation of the cost map): heavy pixels lie along silhouettes that run through neighbouring tiles.  What it removes: one
// launch in five of the 496-hittable 1080p frame took 407 instead of 376 ms — every workgroup resident from the first microsecond, ONE of them
// 40 ms longer than the rest (tools/block_residency.py) — because a tile whose estimate had come out too light sits at a run-to-run varying
// place of its class, and sometimes that place is among the last dequeues.  1080p x 1024 spp 383 - 388 (373 ... 409) -> 375.2 +- 1.5 ms over
// 40 launches, x 256 spp 108 -> 102, 4K x 256 spp 332 (323 ... 352) -> 310 +- 1; neighbours weighted 0.25 / 0.5 / 0.75 / 1.5 or two rings of
// them bring the slow launches back in part (a neighbour ranked above the heavy tile itself, or too many tiles in the top classes);
// averaging a pixel with its neighbours instead — nine times the samples — made it WORSE (404 ms: the heavy pixels are isolated ones).
// profiles/r05_launch_spread_smoke.txt.
__global__ __launch_bounds__(256) void tile_dilate_kernel(const unsigned int* __restrict__ cost, int tiles_x, int tiles_y, unsigned int* __restrict__ out) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= tiles_x * tiles_y) return;
  const int tx = t % tiles_x, ty = t / tiles_x;
  unsigned int m = 0;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const int x = tx + dx, y = ty + dy;
      if (x >= 0 && x < tiles_x && y >= 0 && y < tiles_y) m = max(m, cost[y * tiles_x + x]);
    }
  out[t] = m;
}

constexpr int kLptClasses = 32;
__global__ __launch_bounds__(1024) void lpt_order_kernel(const unsigned int* __restrict__ cost, int n, int* __restrict__ order,
                                                        int n_waves, float trav_cost, float fixed_cost, float s_chain, int forced_logG,
                                                        int* __restrict__ n_split) {
  __shared__ float s_cost_sum[kLptClasses];
  __shared__ unsigned int s_max;
  __shared__ float s_sum;
  __shared__ unsigned int s_count[kLptClasses], s_cursor[kLptClasses];
  if (threadIdx.x == 0) { s_max = 1; s_sum = 0.0f; }
  if (threadIdx.x < kLptClasses) { s_count[threadIdx.x] = 0; s_cost_sum[threadIdx.x] = 0.0f; }
  __syncthreads();
  unsigned int m = 0;
  float sum = 0.0f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) { m = max(m, cost[i]); sum += (float)cost[i]; }
  atomicMax(&s_max, m);
  atomicAdd(&s_sum, sum);
  __syncthreads();
  const float mx = (float)s_max;
  auto cls = [&](unsigned int c) {
    if (c == 0) return kLptClasses - 1;
    int k = (int)(4.0f * __log2f(mx / (float)c)); // 0 = within 2^(1/4) of the heaviest tile
    return min(max(k, 0), kLptClasses - 1);
  };
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int k = cls(cost[i]);
    atomicAdd(&s_count[k], 1u);
    atomicAdd(&s_cost_sum[k], (float)cost[i]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // How many of the heaviest tiles to render G lanes per pixel (lane_acquire), and G itself.  A tile rendered whole is one
    // chain of length ~ its cost; wide, its pixels are chains `speedup` times shorter but cost 1/`eff` as much lane time
    // (camera and shading are computed redundantly by the G lanes, the merge is extra).  Per iteration: traversal T
    // (splittable) + S(G) (not; grows with the merge stages):  speedup = (T + S1) / (T/G + S),  eff = (T + S1) / (T + G*S).
    // With the tiles handed out heaviest first the makespan is about
    //     max( (cost kept whole + cost wide / eff) / n_waves , heaviest tile kept whole , heaviest tile / speedup )
    // evaluated for every group size and every prefix of classes; the best pair wins (often the empty prefix).  Small
    // frames and the shards of a multi-GPU job are chain-bound and get large groups; big frames get small ones or none.
    float best = 3.4e38f;
    int split = 0, best_logG = forced_logG > 0 ? forced_logG : 3;
    const float nw = (float)max(n_waves, 1);
    unsigned int acc = 0;
    for (int k = 0; k < kLptClasses; k++) { s_cursor[k] = acc; acc += s_count[k]; }
    for (int logG = (forced_logG > 0 ? forced_logG : 1); logG <= (forced_logG > 0 ? forced_logG : 6); logG++) {
      // Per iteration ~2 400 instruction slots are not split (camera, shading, run headers, merge stages — every lane of a
      // group runs them redundantly) against the list scan's T: lane time of a wide tile grows as (T + G*2400) / (T + 2400),
      // its chain shortens as (T + 2400) / (T/G + 2400).  Refit in round 2 on the 496-hittable scene after the scan got
      // cheaper (tools/model_sweep.py; the round-1 fit charged only 420 slots for the lane time and over-split shards:
      // shard 0/8 of the 1080p frame 113 -> 102 ms, 4K x 512 spp 365 -> 348 ms, whole frames unchanged).
      const float G = (float)(1 << logG);
      const float eff = (trav_cost + fixed_cost) / (trav_cost + G * fixed_cost);
      const float speedup = (trav_cost + s_chain) / (trav_cost / G + s_chain);
      float split_cost = 0.0f;
      unsigned int tiles = 0;
      for (int k = 0; k <= kLptClasses; k++) { // k = number of leading classes that are wide
        const float next_whole = k < kLptClasses ? mx * exp2f(-0.25f * (float)k) : 0.0f; // upper bound of class k
        const float balanced = ((s_sum - split_cost) + split_cost / eff) / nw;
        const float span = fmaxf(balanced, fmaxf(next_whole, k > 0 ? mx / speedup : 0.0f));
        if (span < best * 0.98f) { best = span; split = (int)tiles; best_logG = logG; } // needs a clear win to change
        if (k < kLptClasses) { tiles += s_count[k]; split_cost += s_cost_sum[k]; }
      }
    }
    if (n_split) n_split[1] = best_logG;
    if (n_split) *n_split = split;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) order[atomicAdd(&s_cursor[cls(cost[i])], 1u)] = i;
}

// ---- first-hit feature buffers (include/pt_render.h: pt_render_aov) ---------------------------------------------
// The AOV pass of n samples is the reference's render at depth 1 with the first bounce's record kept: pixel p owns one xorshift32 stream
// seeded with its linear id (render.hpp:130-132); sample s draws its camera ray from it (render.hpp:96-99), runs ONE iteration of the
// bounce loop (render.hpp:58-89: traversal, emitted, scatter — bounce_kernel's body, with every culling structure the scene has) and
// leaves the stream where that bounce left it.  A pass of its own: it shares no code path, no register budget and no workspace with
// render_kernel (DESIGN.md §1 "First-hit feature buffers", §3 "The AOV pass").  One wave per 8x8 tile, lane ly * 8 + lx; every plane's term is added in sample order
// from +0 and divided once by (float)samples (render.hpp:102).
struct AovArgs {
  Cam cam = {};
  const f4* blob = nullptr;
  const f4* mats = nullptr;
  const f4* pool = nullptr;
  const uint8_t* atlas = nullptr;
  float* albedo = nullptr;   // [pixel][3]; every plane: NULL = not wanted
  float* normal = nullptr;   // [pixel][3]
  float* direct = nullptr;   // [pixel][3]
  float* depth = nullptr;    // [pixel]
  float* coverage = nullptr; // [pixel]
  int* id = nullptr;         // [pixel]
  int n_runs = 0;
  int width = 0, height = 0, samples = 0;
  float inv_w = 0.0f, inv_h = 0.0f;
  int pinhole = 0, fast_ok = 0;
  int shard_index = 0, shard_count = 1;
  int tiles_x = 0, n_tiles = 0;
  int local_tiles = 0; // tiles of the planes: every tile of a whole frame; pt_shard_tiles() for a shard (its last one may be padding)
};
static_assert(std::is_trivially_copyable<AovArgs>::value, "AovArgs is copied into the kernarg segment as it is");

template <bool IMG, int WALK>
__global__ __launch_bounds__(kBlock, PT_MIN_WAVES_AOV) void aov_kernel(AovArgs a) {
  const int l = (int)blockIdx.x * kWavesPerBlock + (int)(threadIdx.x >> 6); // local tile: one per wave
  if (l >= a.local_tiles) return;                                           // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const long long g = (long long)l * a.shard_count + a.shard_index; // global tile (pt_render.h: round-robin shards)
  const bool sharded = a.shard_count != 1;
  const bool tile_in_frame = g < a.n_tiles;
  V3 alb = mk(0.0f, 0.0f, 0.0f), nrm = mk(0.0f, 0.0f, 0.0f), dir = mk(0.0f, 0.0f, 0.0f);
  float dep = 0.0f, cov = 0.0f;
  int first_id = -1;
  bool in_frame = false;
  long long at = (long long)l * PT_TILE_PIXELS + lane; // the pixel's element in the per-pixel layout: [local tile][64], or [y][x]
  if (tile_in_frame) { // (wave-uniform: a shard's padding tile traces nothing)
    const int tx = (int)(g % a.tiles_x), ty = (int)(g / a.tiles_x);
    const int px = tx * PT_TILE + (lane & 7), py = ty * PT_TILE + (lane >> 3);
    in_frame = px < a.width && py < a.height;
    // every lane of the wave stays active through the traversal, which exchanges data between lanes (grid walk, triangle pool: see
    // bounce_kernel): a padding lane repeats an in-frame pixel of its tile — same seed, same work — and stores nothing of it
    const int x = min(px, a.width - 1), y = min(py, a.height - 1);
    if (!sharded) at = (long long)y * a.width + x;
    uint32_t rng = (uint32_t)((unsigned long long)y * (unsigned long long)a.width + (unsigned long long)x); // render.hpp:130-132
    for (int s = 0; s < a.samples; ++s) {
      Ray ray = camera_ray(a.cam, x, y, a.width, a.height, a.inv_w, a.inv_h, rng, a.pinhole != 0);
      V3 att = mk(1.0f, 1.0f, 1.0f);
      RayCtx c = make_ctx(ray, a.fast_ok != 0);
      HitState h;
      hit_world<IMG, true, WALK, true>(a.blob, (cst_f4p)a.blob, a.n_runs, c, wave_all_regular(c, true), rng, h, a.pool);
      const float closest = h.closest, hu = h.u, hv = h.v;
      const int hit = h.hit;
      V3 color, n_term = mk(0.0f, 0.0f, 0.0f), d_term;
      float t_term = 0.0f, c_term = 0.0f;
      int hittable = -1;
      if (hit < 0) {
        color = sky_color(ray, att);
        d_term = color;
      } else {
        const Rec rec = resolve_hit(a.blob, hit, ray, closest);
        hittable = rec.hittable;
        n_term = rec.normal; t_term = closest; c_term = 1.0f;
        float pu = hu, pv = hv;
        if (!IMG) winner_uv(a.blob, hit, ray, closest, rec, pu, pv);
        V3 out = mk(0.0f, 0.0f, 0.0f);
        auto uv = [&](float& u, float& v) { u = pu; v = pv; };
        if (shade(a.mats, a.atlas, rec, uv, ray, att, rng, out)) { color = att; d_term = mk(0.0f, 0.0f, 0.0f); } // scattered: the new attenuation
        else { color = out; d_term = out; }                                                                       // absorbed: the emitted colour
      }
      alb = alb + color; nrm = nrm + n_term; dir = dir + d_term;
      dep = dep + t_term; cov = cov + c_term;
      if (s == 0) first_id = hittable;
    }
    const float n = (float)a.samples;
    alb = alb / n; nrm = nrm / n; dir = dir / n; dep = dep / n; cov = cov / n; // render.hpp:102
  }
  // whole frames: pixels outside the frame have no element; shards: padding pixels get 0, and -1 in `id`
  if (!in_frame) {
    if (!sharded) return;
    alb = nrm = dir = mk(0.0f, 0.0f, 0.0f); dep = cov = 0.0f; first_id = -1;
  }
  if (a.albedo) store_rgb(a.albedo + at * 3, alb);
  if (a.normal) store_rgb(a.normal + at * 3, nrm);
  if (a.direct) store_rgb(a.direct + at * 3, dir);
  if (a.depth) a.depth[at] = dep;
  if (a.coverage) a.coverage[at] = cov;
  if (a.id) a.id[at] = first_id;
}

// ---- probes ---------------------------------------------------------------------------------
template <bool IMG, int WALK = 1>
__global__ void bounce_kernel(const f4* __restrict__ blob, int n_runs, const f4* __restrict__ mats, const f4* __restrict__ pool,
                              const uint8_t* __restrict__ atlas, const PtBounceIn* __restrict__ in,
                              PtBounceOut* __restrict__ outp, int n, int fast_ok) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  // every lane of the wave stays active (the tail repeats the last record and does not store): the traversal exchanges data
  // between lanes (grid walk split phase: ds_bpermute, DPP), and a lane that has exited reads as zero there
  const bool valid_lane = k < n;
  if (!valid_lane) k = n - 1;
  PtBounceIn I = in[k];
  Ray ray;
  ray.o = mk(I.origin[0], I.origin[1], I.origin[2]);
  ray.d = mk(I.dir[0], I.dir[1], I.dir[2]);
  ray.tm = I.time;
  uint32_t rng = I.rng_state;
  V3 att = mk(I.attenuation[0], I.attenuation[1], I.attenuation[2]);
  PtBounceOut O;
  memset(&O, 0, sizeof O);
  RayCtx c = make_ctx(ray, fast_ok != 0);
  HitState h;
  hit_world<IMG, true, WALK, true>(blob, (cst_f4p)blob, n_runs, c, wave_all_regular(c, true), rng, h, pool); // every culling structure the scene has (WALK: which sphere-grid walk)
  const float closest = h.closest, hu = h.u, hv = h.v;
  const int hit = h.hit;
  if (hit < 0) {
    V3 c = sky_color(ray, att);
    O.status = PT_BOUNCE_MISS; O.hittable = -1; O.material = -1;
    O.color[0] = c.x; O.color[1] = c.y; O.color[2] = c.z;
  } else {
    Rec rec = resolve_hit(blob, hit, ray, closest);
    O.hittable = rec.hittable; O.material = rec.mat; O.front_face = rec.front_face ? 1 : 0;
    O.t = closest;
    O.p[0] = rec.p.x; O.p[1] = rec.p.y; O.p[2] = rec.p.z;
    O.normal[0] = rec.normal.x; O.normal[1] = rec.normal.y; O.normal[2] = rec.normal.z;
    float pu = hu, pv = hv;
    if (!IMG) winner_uv(blob, hit, ray, closest, rec, pu, pv);
    O.u = pu; O.v = pv;
    V3 out = mk(0.0f, 0.0f, 0.0f);
    auto uv = [&](float& u, float& v) { u = pu; v = pv; };
    if (shade(mats, atlas, rec, uv, ray, att, rng, out)) {
      O.status = PT_BOUNCE_SCATTERED;
      O.color[0] = att.x; O.color[1] = att.y; O.color[2] = att.z;
      O.sc_origin[0] = ray.o.x; O.sc_origin[1] = ray.o.y; O.sc_origin[2] = ray.o.z;
      O.sc_dir[0] = ray.d.x; O.sc_dir[1] = ray.d.y; O.sc_dir[2] = ray.d.z;
      O.sc_time = ray.tm;
    } else {
      O.status = PT_BOUNCE_ABSORBED;
      O.color[0] = out.x; O.color[1] = out.y; O.color[2] = out.z;
    }
  }
  O.rng_state = rng;
  if (valid_lane) outp[k] = O;
}

__global__ void camera_rays_kernel(Cam cam, int width, int height, const int* __restrict__ xy,
                                   const uint32_t* __restrict__ rng_in, PtCameraRay* __restrict__ out, int n) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  uint32_t rng = rng_in[k];
  Ray r = camera_ray(cam, xy[2 * k], xy[2 * k + 1], width, height, 1.0f / (float)width, 1.0f / (float)height, rng, cam_is_pinhole(cam));
  PtCameraRay o;
  o.origin[0] = r.o.x; o.origin[1] = r.o.y; o.origin[2] = r.o.z;
  o.dir[0] = r.d.x; o.dir[1] = r.d.y; o.dir[2] = r.d.z;
  o.time = r.tm; o.rng_state = rng;
  out[k] = o;
}

__global__ void math_kernel(int op, const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                            long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x = a[i], y = b ? b[i] : 0.0f, r;
  switch (op) {
    case 0: r = ptm::sinf_(x); break;
    case 1: r = ptm::cosf_(x); break;
    case 2: r = ptm::logf_(x); break;
    case 3: r = ptm::pow5f_(x); break;
    case 4: r = ptm::atan2f_(x, y); break;
    case 5: r = ptm::asinf_(x); break;
    case 6: r = ptm::fmod1f_(x); break;
    case 7: r = sqrt_rn(x); break;
    case 9: { float yy = 1.0f / y; r = div_exact(x, y, yy, x * yy); break; } // the shared-reciprocal quotient (|q| >= 2^-60)
    case 10: r = rcp_rn_guarded(x); break; // RN(1/a) for 2^-40 <= |a| <= 2^40 (pt_device.hpp: make_ctx)
    case 11: r = sqrt_rn_unit(x); break;   // correctly rounded sqrt for x = 0 or 2^-60 <= x <= 4
    case 12: r = sky_unit_y(x, y, true); break; // unit_vector(d).y = x / sqrt(y) for a regular ray (y = d.d): the sky's shortcut
    case 13: r = checker_sines_negative(x, y, 1.0f) ? 1.0f : 0.0f; break; // texture.hpp:43-45 on (a, b, 1): the checker's sign-only form
    case 14: { float c_; ptm::sincosf_(x, r, c_); break; }  // sin through the fused form
    case 15: { float s_; ptm::sincosf_(x, s_, r); break; }  // cos through the fused form
    default: r = x / y; break;
  }
  out[i] = r;
}

// pt_debug_sphere_texel: the texel an image texture on a sphere selects for the unit normal n — what texture_value takes (the fast
// path where it is unambiguous, the reference's chain otherwise: out_ij), the reference's chain alone (exact_ij), and which one it was.
__global__ void sphere_texel_kernel(const float* __restrict__ nxyz, long long n, float freq, uint32_t w, uint32_t h, int32_t* __restrict__ out_ij,
                                    int32_t* __restrict__ exact_ij, uint8_t* __restrict__ fast, float* __restrict__ uv4) {
  long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const V3 nn = mk(nxyz[3 * k], nxyz[3 * k + 1], nxyz[3 * k + 2]);
  float u, v;
  mercator(nn, u, v);
  const uint32_t ei = texel_index(ptm::fmod1f_(u * freq) * (float)(w - 1), w - 1);
  const uint32_t ej = texel_index((1.0f - ptm::fmod1f_(v * freq)) * (float)(h - 1), h - 1);
  uint32_t i = 0, j = 0;
  const bool took = sphere_texel_fast(nn, freq, w, h, i, j);
  out_ij[2 * k] = (int32_t)(took ? i : ei); out_ij[2 * k + 1] = (int32_t)(took ? j : ej);
  exact_ij[2 * k] = (int32_t)ei; exact_ij[2 * k + 1] = (int32_t)ej;
  fast[k] = took ? 1 : 0;
  if (uv4) { // (u, v) of the reference's chain and of the binary32 approximations: the deviation the short form's margin E_uv covers
    float uf, vf;
    sphere_uv_fast(nn, uf, vf);
    uv4[4 * k] = u; uv4[4 * k + 1] = v; uv4[4 * k + 2] = uf; uv4[4 * k + 3] = vf;
  }
}

// PT_FLAG_FAST_RNG: framebuffer = (chunk plane 0 + plane 1 + ... in order) / samples — a fixed order, so the mode is
// deterministic run to run (and bit-comparable with the oracle's restatement of it).
__global__ void fast_reduce_kernel(const float* __restrict__ partial, float* __restrict__ fb, long long n, long long stride,
                                   int chunks, float samples) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float sum = 0.0f;
  for (int c = 0; c < chunks; c++) sum = sum + partial[(long long)c * stride + i];
  fb[i] = sum / samples;
}

// Root-side un-interleave of the gathered shard tiles -> [y][x][rgb].
__global__ void unshard_kernel(const float* __restrict__ gathered, float* __restrict__ fb, int width, int height,
                               int tiles_x, int shard_count, int tiles_per_shard) {
  int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= width) return;
  int g = (y / PT_TILE) * tiles_x + (x / PT_TILE);
  long long src = (((long long)(g % shard_count) * tiles_per_shard + g / shard_count) * PT_TILE_PIXELS +
                   (y % PT_TILE) * PT_TILE + (x % PT_TILE)) * 3;
  long long dst = ((long long)y * width + x) * 3;
  fb[dst] = gathered[src]; fb[dst + 1] = gathered[src + 1]; fb[dst + 2] = gathered[src + 2];
}

// main.cpp:33-59 for one channel — sqrt gamma, clamp [0,0.999], *256, truncate: THE output stage, every 8-bit image goes through it
__device__ __forceinline__ uint8_t quantise(float radiance) {
  float s = sqrt_rn(radiance);
  float cl = (s < 0.0f) ? 0.0f : (0.999f < s) ? 0.999f : s; // std::clamp
  float sc = 256.0f * cl;
  int v = (sc == sc) ? (int)sc : 0; // int(NaN) is UB in the reference; defined as 0
  return (uint8_t)v;
}

// THE mean of n samples: lane_store's correctly rounded IEEE division (render.hpp:102; -fhip-fp32-correctly-rounded-divide-sqrt, no
// reciprocal), 0 where nothing was sampled
__device__ __forceinline__ float mean_of(float sum, int n) { return n > 0 ? sum / (float)n : 0.0f; }

// the sample count of pixel `pix` of an accumulator: its own (adaptive: cnt) or the one every pixel has (plain: cnt NULL, `done` > 0)
__device__ __forceinline__ int count_of(const int* __restrict__ cnt, int done, long long pix) { return cnt ? cnt[pix] : done; }

// The output stage with the vertical flip (row 0 = top).  MEAN = false: `src` is a finished frame buffer (pt_tonemap_rgb8: nothing is
// divided); MEAN = true: resolve + output stage in one pass over an accumulator's sums (whole frames), the same mean as accum_resolve_kernel
template <bool MEAN>
__global__ void tonemap_kernel(const float* __restrict__ src, const int* __restrict__ cnt, int done, uint8_t* __restrict__ rgb8, int width, int height) {
  int x = blockIdx.x * blockDim.x + threadIdx.x, row = blockIdx.y; // row 0 = top
  if (x >= width) return;
  int j = height - 1 - row;
  const long long pix = (long long)j * width + x;
  const int n = MEAN ? count_of(cnt, done, pix) : 0;
  for (int ch = 0; ch < 3; ch++) {
    const float v = src[pix * 3 + ch];
    rgb8[((long long)row * width + x) * 3 + ch] = quantise(MEAN ? mean_of(v, n) : v);
  }
}

// ---- sample windows (PtAccum) ---------------------------------------------------------------------------------------------------
// fast mode: the window's chunk planes added to the running sum in chunk order, NOT divided — fast_reduce_kernel's order of additions
// continued across windows (its first addition is 0 + plane 0, as the accumulator's sum starts at 0)
__global__ void fast_accum_kernel(const float* __restrict__ partial, float* __restrict__ sum, long long n, long long stride, int chunks) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = sum[i];
  for (int c = 0; c < chunks; c++) s = s + partial[(long long)c * stride + i];
  sum[i] = s;
}

// fb = sum / n, per pixel for an adaptive accumulator (cnt) and by `done` for a plain one (cnt NULL)
__global__ void accum_resolve_kernel(const float* __restrict__ sum, const int* __restrict__ cnt, int done, float* __restrict__ fb, long long floats) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= floats) return;
  fb[i] = mean_of(sum[i], count_of(cnt, done, i / 3));
}

// ---- adaptive sampling (pt_adaptive_*): per-pixel counts, the two-half-buffer error estimate and masked windows ---------------------
// The frame of an adaptive PtAccum as its small kernels see it.  Per-pixel arrays use the frame buffer's layout without the channel:
// pixel i is (i % width, i / width) for whole frames and (local tile i / 64, ly * 8 + lx = i % 64) for shards, whose padding pixels
// (edge tiles, the padded last tile) are no pixels of the frame.
struct AFrame {
  int width, height, shard_index, shard_count, tiles_x, n_tiles;
  long long pixels; // P = pt_framebuffer_floats / 3
};

// pixel `in` (ly * 8 + lx) of local tile l: its place in the frame; false for padding (edge tiles, the padded last tile)
__host__ __device__ __forceinline__ bool atile_xy(const AFrame& f, long long l, int in, int& x, int& y) {
  const long long g = l * f.shard_count + f.shard_index;
  x = (int)(g % f.tiles_x) * PT_TILE + (in & 7); y = (int)(g / f.tiles_x) * PT_TILE + (in >> 3);
  return g < f.n_tiles && x < f.width && y < f.height;
}
// pixel i of a per-pixel array: row-major for whole frames, (local tile, index in tile) for shards
__host__ __device__ __forceinline__ bool aframe_xy(const AFrame& f, long long i, int& x, int& y) {
  if (f.shard_count == 1) { x = (int)(i % f.width); y = (int)(i / f.width); return true; }
  return atile_xy(f, i >> 6, (int)(i & 63), x, y);
}

// every pixel's generator state at 0 samples: its linear id in the whole frame (render.hpp:130-132), indexed like KArgs.resume_rng —
// by padded tile for whole frames too (atile_xy), NOT by the row-major pixel of the per-pixel arrays (aframe_xy)
__global__ void adaptive_seed_kernel(AFrame f, unsigned int* __restrict__ rng, long long words) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= words) return;
  int x, y;
  rng[j] = atile_xy(f, j >> 6, (int)(j & 63), x, y) ? (uint32_t)((unsigned long long)y * (unsigned long long)f.width + (unsigned long long)x) : 0u;
}

// masked window, step 1: which local tiles hold at least one pixel of the mask
__global__ void adaptive_tiles_kernel(AFrame f, const uint8_t* __restrict__ mask, int local_tiles, uint8_t* __restrict__ active) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= local_tiles) return;
  uint8_t any = 0;
  for (int in = 0; in < PT_TILE_PIXELS && !any; in++) {
    const long long pix = (long long)l * PT_TILE_PIXELS + in;
    int x, y;
    if (!atile_xy(f, l, in, x, y)) continue;
    any = mask[f.shard_count == 1 ? (long long)y * f.width + x : pix];
  }
  active[l] = any ? 1 : 0;
}

// masked window, step 2 (one workgroup): the active tiles in dequeue order — the kept heaviest-first order, or raster order — by a
// stable scan; count[0] = how many
__global__ __launch_bounds__(1024) void adaptive_compact_kernel(const uint8_t* __restrict__ active, const int* __restrict__ order, int n,
                                                                int* __restrict__ list, int* __restrict__ count) {
  __shared__ int wave_sum[16];
  __shared__ int base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int start = 0; start < n; start += 1024) {
    const int i = start + tid;
    const int t = i < n ? (order ? order[i] : i) : 0;
    const bool on = i < n && active[t];
    const unsigned long long b = __builtin_amdgcn_ballot_w64(on);
    if (lane == 0) wave_sum[wave] = __builtin_popcountll(b);
    __syncthreads();
    int at = base;
    for (int v = 0; v < wave; v++) at += wave_sum[v];
    if (on) list[at + __builtin_popcountll(b & ((1ull << lane) - 1ull))] = t;
    __syncthreads();
    if (tid == 0) for (int v = 0; v < 16; v++) base += wave_sum[v];
    __syncthreads();
  }
  if (tid == 0) *count = base;
}

// after a window of w samples, over the pixels it rendered: its contribution D = S after - S before goes to half A while A has fewer
// samples than B (ties to B), then n += w; and S before := S after, for the next window (PtAccum.prev)
__global__ void adaptive_book_kernel(AFrame f, const uint8_t* __restrict__ mask, const float* __restrict__ sum, float* __restrict__ prev,
                                     float* __restrict__ half, int* __restrict__ cnt, int* __restrict__ cnt_a, int w) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= f.pixels) return;
  int x, y;
  if (!aframe_xy(f, i, x, y) || (mask && !mask[i])) return;
  const int n = cnt[i], a = cnt_a[i];
  const float s0 = sum[3 * i], s1 = sum[3 * i + 1], s2 = sum[3 * i + 2];
  if (a < n - a) {
    half[3 * i] = half[3 * i] + (s0 - prev[3 * i]);
    half[3 * i + 1] = half[3 * i + 1] + (s1 - prev[3 * i + 1]);
    half[3 * i + 2] = half[3 * i + 2] + (s2 - prev[3 * i + 2]);
    cnt_a[i] = a + w;
  }
  cnt[i] = n + w;
  prev[3 * i] = s0; prev[3 * i + 1] = s1; prev[3 * i + 2] = s2;
}

// the two-half-buffer error (include/pt_render.h): correctly rounded binary32 throughout, no contraction (-ffp-contract=off)
__device__ __forceinline__ float adaptive_err(const float* __restrict__ sum, const float* __restrict__ half, int n, int a, long long i) {
  if (a == 0 || a == n) return __builtin_inff();
  const float ix = mean_of(sum[3 * i], n), iy = mean_of(sum[3 * i + 1], n), iz = mean_of(sum[3 * i + 2], n); // (0 < a < n here)
  const float ax = mean_of(half[3 * i], a), ay = mean_of(half[3 * i + 1], a), az = mean_of(half[3 * i + 2], a);
  const float num = (fabsf(ix - ax) + fabsf(iy - ay)) + fabsf(iz - az);
  return num / (1e-4f + sqrt_rn((ix + iy) + iz));
}

__global__ void adaptive_error_kernel(AFrame f, const float* __restrict__ sum, const float* __restrict__ half, const int* __restrict__ cnt,
                                      const int* __restrict__ cnt_a, float* __restrict__ err) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= f.pixels) return;
  err[i] = adaptive_err(sum, half, cnt[i], cnt_a[i], i);
}

// the next window's mask: active = n < max_spp && (n < min_spp || noisy(p) || (dilate && a neighbour in the frame is noisy)),
// noisy(q) = n_q < max_spp && !(err_q <= threshold); n_active += the active pixels (one atomic per wave)
__global__ void adaptive_select_kernel(AFrame f, const float* __restrict__ sum, const float* __restrict__ half, const int* __restrict__ cnt,
                                       const int* __restrict__ cnt_a, float threshold, int min_spp, int max_spp, int dilate,
                                       uint8_t* __restrict__ mask, unsigned long long* __restrict__ n_active) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool on = false;
  if (i < f.pixels) {
    int x, y;
    if (aframe_xy(f, i, x, y)) {
      auto noisy = [&](long long q) { const int n = cnt[q]; return n < max_spp && !(adaptive_err(sum, half, n, cnt_a[q], q) <= threshold); };
      const int n = cnt[i];
      if (n < max_spp) {
        on = n < min_spp || noisy(i);
        if (!on && dilate) // (whole frames only: pt_adaptive_select)
          for (int dy = -1; dy <= 1 && !on; dy++)
            for (int dx = -1; dx <= 1 && !on; dx++) {
              const int qx = x + dx, qy = y + dy;
              if ((dx || dy) && qx >= 0 && qx < f.width && qy >= 0 && qy < f.height) on = noisy((long long)qy * f.width + qx);
            }
      }
    }
    mask[i] = on ? 1 : 0;
  }
  const unsigned long long b = __builtin_amdgcn_ballot_w64(on);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_active, (unsigned long long)__builtin_popcountll(b));
}

// ---- denoiser: the edge-avoiding a-trous filter (include/pt_render.h: pt_denoise) ----------------------------------------------------
// Image space only: nothing of the render kernels is involved.  The header states every operation; this is that text in HIP, with
// -ffp-contract=off (no product is fused into a sum) and the correctly rounded division of the build's flags.
__device__ __forceinline__ float exp_neg(float x) { // pt_exp_neg: 0 <= x < 80
  const float k = __builtin_rintf(x * 0x1.715476p+0f);
  const float t = -((x - k * 0x1.62e4p-1f) - k * 0x1.7f7d1cp-20f);
  float q = 0x1.6c16c2p-10f;
  q = q * t + 0x1.111112p-7f;
  q = q * t + 0x1.555556p-5f;
  q = q * t + 0x1.555556p-3f;
  q = q * t + 0.5f;
  q = q * t + 1.0f;
  q = q * t + 1.0f;
  return ldexpf(q, -(int)k);
}

enum { DN_COLOR = 1, DN_NORMAL = 2, DN_DEPTH = 4, DN_ALBEDO = 8, DN_DEMOD_IN = 16, DN_REMOD_OUT = 32 };

// The filter core: what atrous_kernel and vdn_kernel (below) share.  One iteration of either is one thread per pixel in a 32 x 8 pixel
// workgroup (a wave is two rows of 32, so a tap's 64 reads from global memory are two runs of contiguous records).  ND / AL: the launch
// reads the (normal, depth) / (albedo) records at all.  STEP = 0: every tap is read from global memory, at the step of the arguments.
// STEP = 1, 2: the step is STEP and the workgroup first stages its tile with the halo of 2 STEP pixels in LDS, and the taps read LDS.  Same
// operations on the same values in the same order either way: the bits do not depend on the path.  The core is the tile's geometry, the
// arguments both launches carry, the guide records fetched from either place and a tap's exponent from the guide terms; each kernel adds
// its payload: its colour records and their staging, its colour term, its sums and its write-out.  (The staging loop and the 5 x 5 walk
// stay written out in both kernels: behind shared functions they compile to other registers and instructions —
// profiles/atrous_core_refactor.txt.)
struct FilterArgs { // the tail of both kernels' arguments
  const f4* g_nd;   // per pixel (normal, depth); read when ND
  const f4* g_al;   // per pixel (albedo, 0); read when AL
  int width, height, step;
  unsigned terms;   // DN_* (and VDN_LAST): which terms are on, and what this launch does to what it reads and writes
  float k_color;    // the filter's colour scale: atrous_kernel's k_c, vdn_kernel's sv2
  float k_n, sd2, k_a;
};

template <int STEP>
struct FilterTile {
  static constexpr int R = 2 * STEP, TW = 32 + 2 * R, TH = 8 + 2 * R, N = TW * TH;
};

struct Guides { f4 nd, al; }; // a pixel's guide records
constexpr Guides kNoGuides = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};

// the records at index i of the packed planes (i: a pixel) or of the staged tile (i: a slot); one the launch does not read stays as in g
template <bool ND, bool AL, class I>
__device__ __forceinline__ Guides guides_at(const f4* nd, const f4* al, I i, Guides g) {
  if (ND) g.nd = nd[i];
  if (AL) g.al = al[i];
  return g;
}

// a tap's exponent: the payload's colour term xc and the three guide terms between the centre p and the tap q, summed in the header's order
template <bool ND, bool AL>
__device__ __forceinline__ float filter_exponent(const FilterArgs& f, float xc, const Guides& p, const Guides& q, float den) {
  const bool t_n = ND && (f.terms & DN_NORMAL), t_d = ND && (f.terms & DN_DEPTH), t_a = AL && (f.terms & DN_ALBEDO);
  float xn = 0.0f, xd = 0.0f, xa = 0.0f;
  if (t_n) { const float dnx = p.nd.x - q.nd.x, dny = p.nd.y - q.nd.y, dnz = p.nd.z - q.nd.z; xn = ((dnx * dnx + dny * dny) + dnz * dnz) * f.k_n; }
  if (t_d) { const float dz = p.nd.w - q.nd.w; xd = (dz * dz) / den; }
  if (t_a) { const float dar = p.al.x - q.al.x, dag = p.al.y - q.al.y, dab = p.al.z - q.al.z; xa = ((dar * dar + dag * dag) + dab * dab) * f.k_a; }
  return ((xc + xn) + xd) + xa;
}

// ---- the a-trous filter's kernels ----
struct ATrousArgs {
  const float* in;  // c_i: [height][width][3] (iteration 0: the caller's colour, or its copy in scratch)
  float* out;       // c_(i+1)
  FilterArgs f;     // k_color: k_c of this iteration; terms: DN_DEMOD_IN / DN_REMOD_OUT say whether this launch de- / remodulates
};

// The prepass: the guide planes the caller handed over, packed into one or two 16-byte records per pixel, so that a tap reads its guides
// with one or two global_load_dwordx4 instead of up to seven scalar-sized loads from three planes.  A NULL plane packs as 0.
// (vdn_pack_kernel ends with the same text: behind a shared function it compiles to other registers — profiles/atrous_core_refactor.txt.)
__global__ __launch_bounds__(256) void atrous_pack_kernel(const float* __restrict__ normal, const float* __restrict__ depth,
                                                          const float* __restrict__ albedo, f4* __restrict__ g_nd, f4* __restrict__ g_al, long long pixels) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pixels) return;
  if (g_nd) {
    f4 r = {0.0f, 0.0f, 0.0f, 0.0f};
    if (normal) { r.x = normal[p * 3]; r.y = normal[p * 3 + 1]; r.z = normal[p * 3 + 2]; }
    if (depth) r.w = depth[p];
    g_nd[p] = r;
  }
  if (g_al) {
    const f4 r = {albedo[p * 3], albedo[p * 3 + 1], albedo[p * 3 + 2], 0.0f};
    g_al[p] = r;
  }
}

// The payload: three floats of colour per pixel, demodulated as they are read — in the staged tile once per slot instead of once per tap —
// a colour term with one scale k_c, and the weighted colour sum.
template <bool ND, bool AL, int STEP>
__global__ __launch_bounds__(256) void atrous_kernel(ATrousArgs a) {
  using T = FilterTile<STEP>;
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int x = blockIdx.x * 32 + lx, y = blockIdx.y * 8 + ly;
  const bool demod = AL && (a.f.terms & DN_DEMOD_IN);
  const int step = STEP ? STEP : a.f.step;
  __shared__ float s_r[STEP ? T::N : 1], s_g[STEP ? T::N : 1], s_b[STEP ? T::N : 1];
  __shared__ f4 s_nd[STEP && ND ? T::N : 1], s_al[STEP && AL ? T::N : 1];
  if constexpr (STEP > 0) {
    const int x0 = blockIdx.x * 32 - T::R, y0 = blockIdx.y * 8 - T::R;
    for (int i = threadIdx.x; i < T::N; i += 256) {
      const int gx = x0 + i % T::TW, gy = y0 + i / T::TW;
      float cr = 0.0f, cg = 0.0f, cb = 0.0f;
      Guides g = kNoGuides;
      if (gx >= 0 && gx < a.f.width && gy >= 0 && gy < a.f.height) { // (a slot outside the frame is never read: its tap is skipped)
        const long long q = (long long)gy * a.f.width + gx;
        cr = a.in[q * 3]; cg = a.in[q * 3 + 1]; cb = a.in[q * 3 + 2];
        g = guides_at<ND, AL>(a.f.g_nd, a.f.g_al, q, g);
        if (demod) { cr = cr / (g.al.x + 1e-3f); cg = cg / (g.al.y + 1e-3f); cb = cb / (g.al.z + 1e-3f); }
      }
      s_r[i] = cr; s_g[i] = cg; s_b[i] = cb;
      if (ND) s_nd[i] = g.nd;
      if (AL) s_al[i] = g.al;
    }
    __syncthreads();
  }
  if (x >= a.f.width || y >= a.f.height) return;
  const long long p = (long long)y * a.f.width + x;
  const int lp = (ly + T::R) * T::TW + lx + T::R; // the pixel's slot in the tile (STEP > 0)
  const bool t_c = a.f.terms & DN_COLOR;
  Guides gp = kNoGuides;
  float pr, pg, pb;
  if constexpr (STEP > 0) {
    gp = guides_at<ND, AL>(s_nd, s_al, lp, gp);
    pr = s_r[lp]; pg = s_g[lp]; pb = s_b[lp];
  } else {
    gp = guides_at<ND, AL>(a.f.g_nd, a.f.g_al, p, gp);
    pr = a.in[p * 3]; pg = a.in[p * 3 + 1]; pb = a.in[p * 3 + 2];
    if (demod) { pr = pr / (gp.al.x + 1e-3f); pg = pg / (gp.al.y + 1e-3f); pb = pb / (gp.al.z + 1e-3f); }
  }
  const float den = a.f.sd2 * (gp.nd.w * gp.nd.w) + 1e-12f;
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, ws = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + dy * step;
    if (qy < 0 || qy >= a.f.height) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + dx * step;
      if (qx < 0 || qx >= a.f.width) continue;
      constexpr float K[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
      const float h = K[dy + 2] * K[dx + 2];
      float cr, cg, cb;
      Guides gq;
      if constexpr (STEP > 0) {
        const int lq = lp + dy * STEP * T::TW + dx * STEP; // inside the tile: |dy STEP|, |dx STEP| <= R
        cr = s_r[lq]; cg = s_g[lq]; cb = s_b[lq];
        gq = guides_at<ND, AL>(s_nd, s_al, lq, gp);
      } else {
        const long long q = (long long)qy * a.f.width + qx;
        cr = a.in[q * 3]; cg = a.in[q * 3 + 1]; cb = a.in[q * 3 + 2];
        gq = guides_at<ND, AL>(a.f.g_nd, a.f.g_al, q, gp);
        if (demod) { cr = cr / (gq.al.x + 1e-3f); cg = cg / (gq.al.y + 1e-3f); cb = cb / (gq.al.z + 1e-3f); }
      }
      float xc = 0.0f;
      if (t_c) { const float dr = pr - cr, dg = pg - cg, db = pb - cb; xc = ((dr * dr + dg * dg) + db * db) * a.f.k_color; }
      const float xs = filter_exponent<ND, AL>(a.f, xc, gp, gq, den);
      if (!(xs < 80.0f)) continue;
      const float w = h * exp_neg(xs);
      sr = sr + w * cr; sg = sg + w * cg; sb = sb + w * cb;
      ws = ws + w;
    }
  }
  float orr = pr, og = pg, ob = pb;
  if (ws != 0.0f) { orr = sr / ws; og = sg / ws; ob = sb / ws; }
  if (AL && (a.f.terms & DN_REMOD_OUT)) { orr = orr * (gp.al.x + 1e-3f); og = og * (gp.al.y + 1e-3f); ob = ob * (gp.al.z + 1e-3f); }
  a.out[p * 3] = orr; a.out[p * 3 + 1] = og; a.out[p * 3 + 2] = ob;
}

// ---- variance-guided denoiser (include/pt_render.h: pt_variance_estimate, pt_variance_denoise) ----------------------------------------
// The a-trous filter above with the colour tolerance taken per pixel from a variance plane, and the variance carried through the levels.
// Same rules: the header states every operation, this is that text in HIP; -ffp-contract=off, correctly rounded division.

// the variance of each resolved pixel from the two half buffers: (A - B)^2 a b / n^2 (the header says why); padding pixels of a shard: 0
__global__ void variance_estimate_kernel(AFrame f, const float* __restrict__ sum, const float* __restrict__ half, const int* __restrict__ cnt,
                                         const int* __restrict__ cnt_a, float* __restrict__ var) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= f.pixels) return;
  int x, y;
  float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
  if (aframe_xy(f, i, x, y)) {
    const int n = cnt[i], a = cnt_a[i];
    if (a == 0 || a == n) {
      v0 = v1 = v2 = __builtin_inff();
    } else {
      const float fa = (float)a, fb = (float)(n - a), fn = (float)n;
      const float fr = (fa * fb) / (fn * fn);
      const float h0 = half[3 * i], h1 = half[3 * i + 1], h2 = half[3 * i + 2];
      const float d0 = h0 / fa - (sum[3 * i] - h0) / fb, d1 = h1 / fa - (sum[3 * i + 1] - h1) / fb, d2 = h2 / fa - (sum[3 * i + 2] - h2) / fb;
      v0 = (d0 * d0) * fr; v1 = (d1 * d1) * fr; v2 = (d2 * d2) * fr;
    }
  }
  var[3 * i] = v0; var[3 * i + 1] = v1; var[3 * i + 2] = v2;
}

typedef float f2v __attribute__((ext_vector_type(2)));
enum { VDN_LAST = 64 }; // beside DN_*: this launch is the last iteration and writes the caller's planes

struct VdnArgs {
  const f4* in_a;   // per pixel (c_i.r, c_i.g, c_i.b, v_i.r)
  const f2v* in_b;  // per pixel (v_i.g, v_i.b)
  f4* out_a;        // c_(i+1), v_(i+1) in the same records (every iteration but the last)
  f2v* out_b;
  float* out_color; // the last iteration: the caller's planes, [height][width][3]; out_var may be NULL
  float* out_var;
  FilterArgs f;     // k_color: sv2; terms: DN_COLOR ... DN_ALBEDO, DN_REMOD_OUT, VDN_LAST
};

// The prepass: c_0 and v_0 — the colour demodulated, the variance sanitised and demodulated — into the working records, and the guide
// planes into atrous_pack_kernel's records.  It reads every plane of the caller's completely before the filter writes any: `out` may be
// `color`, `variance_out` may be `variance`.
__global__ __launch_bounds__(256) void vdn_pack_kernel(const float* __restrict__ color, const float* __restrict__ variance,
                                                       const float* __restrict__ normal, const float* __restrict__ depth,
                                                       const float* __restrict__ albedo, f4* __restrict__ rec_a, f2v* __restrict__ rec_b,
                                                       f4* __restrict__ g_nd, f4* __restrict__ g_al, long long pixels, int demod) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pixels) return;
  float cr = color[p * 3], cg = color[p * 3 + 1], cb = color[p * 3 + 2];
  float vr = variance[p * 3], vg = variance[p * 3 + 1], vb = variance[p * 3 + 2];
  vr = (vr >= 0.0f && vr < __builtin_inff()) ? vr : 0.0f;
  vg = (vg >= 0.0f && vg < __builtin_inff()) ? vg : 0.0f;
  vb = (vb >= 0.0f && vb < __builtin_inff()) ? vb : 0.0f;
  if (demod) {
    const float mr = albedo[p * 3] + 1e-3f, mg = albedo[p * 3 + 1] + 1e-3f, mb = albedo[p * 3 + 2] + 1e-3f;
    cr = cr / mr; cg = cg / mg; cb = cb / mb;
    vr = vr / (mr * mr); vg = vg / (mg * mg); vb = vb / (mb * mb);
  }
  const f4 ra = {cr, cg, cb, vr};
  const f2v rb = {vg, vb};
  rec_a[p] = ra;
  rec_b[p] = rb;
  if (g_nd) {
    f4 r = {0.0f, 0.0f, 0.0f, 0.0f};
    if (normal) { r.x = normal[p * 3]; r.y = normal[p * 3 + 1]; r.z = normal[p * 3 + 2]; }
    if (depth) r.w = depth[p];
    g_nd[p] = r;
  }
  if (g_al) {
    const f4 r = {albedo[p * 3], albedo[p * 3 + 1], albedo[p * 3 + 2], 0.0f};
    g_al[p] = r;
  }
}

// The payload: per pixel a 16-byte record (colour, variance.r) and an 8-byte record (variance.g, variance.b), staged as they are; the
// tile's halo is >= 1, so it also serves the 3 x 3 prefilter of the variance, whose nine reads are global at STEP = 0 like the 25 taps'; a
// colour term scaled per channel by the prefiltered variance; the weighted colour sum and the variance sum weighted by w^2.
template <bool ND, bool AL, int STEP>
__global__ __launch_bounds__(256) void vdn_kernel(VdnArgs a) {
  using T = FilterTile<STEP>;
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int x = blockIdx.x * 32 + lx, y = blockIdx.y * 8 + ly;
  const int step = STEP ? STEP : a.f.step;
  __shared__ f4 s_a[STEP ? T::N : 1];
  __shared__ f2v s_b[STEP ? T::N : 1];
  __shared__ f4 s_nd[STEP && ND ? T::N : 1], s_al[STEP && AL ? T::N : 1];
  if constexpr (STEP > 0) {
    const int x0 = blockIdx.x * 32 - T::R, y0 = blockIdx.y * 8 - T::R;
    for (int i = threadIdx.x; i < T::N; i += 256) {
      const int gx = x0 + i % T::TW, gy = y0 + i / T::TW;
      f4 ra = {0.0f, 0.0f, 0.0f, 0.0f};
      f2v rb = {0.0f, 0.0f};
      Guides g = kNoGuides;
      if (gx >= 0 && gx < a.f.width && gy >= 0 && gy < a.f.height) { // (a slot outside the frame is never read: its tap is skipped)
        const long long q = (long long)gy * a.f.width + gx;
        ra = a.in_a[q]; rb = a.in_b[q];
        g = guides_at<ND, AL>(a.f.g_nd, a.f.g_al, q, g);
      }
      s_a[i] = ra; s_b[i] = rb;
      if (ND) s_nd[i] = g.nd;
      if (AL) s_al[i] = g.al;
    }
    __syncthreads();
  }
  if (x >= a.f.width || y >= a.f.height) return;
  const long long p = (long long)y * a.f.width + x;
  const int lp = (ly + T::R) * T::TW + lx + T::R; // the pixel's slot in the tile (STEP > 0)
  const bool t_c = a.f.terms & DN_COLOR;
  Guides gp = kNoGuides;
  f4 pa;
  f2v pb;
  if constexpr (STEP > 0) {
    gp = guides_at<ND, AL>(s_nd, s_al, lp, gp);
    pa = s_a[lp]; pb = s_b[lp];
  } else {
    gp = guides_at<ND, AL>(a.f.g_nd, a.f.g_al, p, gp);
    pa = a.in_a[p]; pb = a.in_b[p];
  }
  // the 3 x 3 prefilter of the variance, at a distance of one pixel whatever the step, and the colour scale it gives
  float ivr = 0.0f, ivg = 0.0f, ivb = 0.0f;
  if (t_c) {
    float vr = 0.0f, vg = 0.0f, vb = 0.0f, gs = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
      const int qy = y + dy;
      if (qy < 0 || qy >= a.f.height) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; dx++) {
        const int qx = x + dx;
        if (qx < 0 || qx >= a.f.width) continue;
        constexpr float G[3] = {0.25f, 0.5f, 0.25f};
        const float g = G[dy + 1] * G[dx + 1];
        float qr;
        f2v qb;
        if constexpr (STEP > 0) {
          const int lq = lp + dy * T::TW + dx; // inside the tile: R >= 1
          qr = s_a[lq].w; qb = s_b[lq];
        } else {
          const long long q = (long long)qy * a.f.width + qx;
          qr = a.in_a[q].w; qb = a.in_b[q];
        }
        vr = vr + g * qr; vg = vg + g * qb.x; vb = vb + g * qb.y;
        gs = gs + g;
      }
    }
    vr = vr / gs; vg = vg / gs; vb = vb / gs;
    ivr = 1.0f / (a.f.k_color * vr + 1e-8f); ivg = 1.0f / (a.f.k_color * vg + 1e-8f); ivb = 1.0f / (a.f.k_color * vb + 1e-8f);
  }
  const float den = a.f.sd2 * (gp.nd.w * gp.nd.w) + 1e-12f;
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, tr = 0.0f, tg = 0.0f, tb = 0.0f, ws = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + dy * step;
    if (qy < 0 || qy >= a.f.height) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + dx * step;
      if (qx < 0 || qx >= a.f.width) continue;
      constexpr float K[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
      const float h = K[dy + 2] * K[dx + 2];
      f4 qa;
      Guides gq;
      f2v qb;
      if constexpr (STEP > 0) {
        const int lq = lp + dy * STEP * T::TW + dx * STEP; // inside the tile: |dy STEP|, |dx STEP| <= R
        qa = s_a[lq]; qb = s_b[lq];
        gq = guides_at<ND, AL>(s_nd, s_al, lq, gp);
      } else {
        const long long q = (long long)qy * a.f.width + qx;
        qa = a.in_a[q]; qb = a.in_b[q];
        gq = guides_at<ND, AL>(a.f.g_nd, a.f.g_al, q, gp);
      }
      float xc = 0.0f;
      if (t_c) { const float dr = pa.x - qa.x, dg = pa.y - qa.y, db = pa.z - qa.z; xc = ((dr * dr) * ivr + (dg * dg) * ivg) + (db * db) * ivb; }
      const float xs = filter_exponent<ND, AL>(a.f, xc, gp, gq, den);
      if (!(xs < 80.0f)) continue;
      const float w = h * exp_neg(xs);
      const float w2 = w * w;
      sr = sr + w * qa.x; sg = sg + w * qa.y; sb = sb + w * qa.z;
      tr = tr + w2 * qa.w; tg = tg + w2 * qb.x; tb = tb + w2 * qb.y;
      ws = ws + w;
    }
  }
  float orr = pa.x, og = pa.y, ob = pa.z, vr = pa.w, vg = pb.x, vb = pb.y;
  if (ws != 0.0f) {
    const float ws2 = ws * ws;
    orr = sr / ws; og = sg / ws; ob = sb / ws;
    vr = tr / ws2; vg = tg / ws2; vb = tb / ws2;
  }
  if (a.f.terms & VDN_LAST) {
    if (AL && (a.f.terms & DN_REMOD_OUT)) {
      const float mr = gp.al.x + 1e-3f, mg = gp.al.y + 1e-3f, mb = gp.al.z + 1e-3f;
      orr = orr * mr; og = og * mg; ob = ob * mb;
      vr = vr * (mr * mr); vg = vg * (mg * mg); vb = vb * (mb * mb);
    }
    a.out_color[p * 3] = orr; a.out_color[p * 3 + 1] = og; a.out_color[p * 3 + 2] = ob;
    if (a.out_var) { a.out_var[p * 3] = vr; a.out_var[p * 3 + 1] = vg; a.out_var[p * 3 + 2] = vb; }
  } else {
    const f4 ra = {orr, og, ob, vr};
    const f2v rb = {vg, vb};
    a.out_a[p] = ra;
    a.out_b[p] = rb;
  }
}

// ---- temporal reprojection (include/pt_render.h: PtTemporal, pt_temporal_push) ----------------------------------------------------------
// The temporal half of SVGF: a frame is blended into the history of the frames before it, fetched through the previous camera.  Same rules
// as the filters above: the header states every operation, this is that text in HIP; -ffp-contract=off, correctly rounded division.
struct TemporalArgs {
  const float* color;   // [height][width][3]
  const float* depth;   // [height][width]
  const float* normal;  // [height][width][3] or NULL
  const int* id;        // [height][width] or NULL
  const float* var_in;  // [height][width][3] or NULL
  float* out_color;     // may be color
  float* out_var;       // may be var_in; or NULL
  float* out_hist;      // or NULL
  const f4* prev;       // the history read: three planes of `pixels` records — (c.rgb, N), (m2.rgb, z), (n.xyz, bits of k)
  f4* next;             // the history written: the other buffer, same layout
  long long pixels;
  int width, height;
  int has_history;      // 0: the first push (or the first after a reset): `prev` is not read
  float o[3], llc[3], hor[3], ver[3];  // the camera of this frame
  float po[3], pw[3], ph[3], pv[3];    // the previous push's: origin', w', horizontal', vertical'
  float fo, hh, vv;                    // ... and the host's constants of it
  float alpha, tol_depth, tn2;         // tn2 = tol_normal * tol_normal
};

// One thread per pixel, a 32 x 8 pixel workgroup: neighbouring pixels reproject to neighbouring history pixels, so the four taps of a
// workgroup fall into a few shared cache lines.  A tap is three 16-byte loads.  Every pixel writes its three history records.
__global__ __launch_bounds__(256) void temporal_push_kernel(TemporalArgs a) {
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int x = blockIdx.x * 32 + lx, y = blockIdx.y * 8 + ly;
  if (x >= a.width || y >= a.height) return;
  const long long p = (long long)y * a.width + x;
  const float inf = __builtin_inff();
  const float cr = a.color[p * 3], cg = a.color[p * 3 + 1], cb = a.color[p * 3 + 2];
  const float z = a.depth[p];
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (a.normal) { nx = a.normal[p * 3]; ny = a.normal[p * 3 + 1]; nz = a.normal[p * 3 + 2]; }
  const int k = a.id ? a.id[p] : 0;
  const bool fin = fabsf(cr) < inf && fabsf(cg) < inf && fabsf(cb) < inf;
  // no usable history: the frame starts one
  float N = 1.0f, ap = 1.0f;
  float c0 = cr, c1 = cg, c2 = cb, m0 = cr * cr, m1 = cg * cg, m2 = cb * cb;
  if (a.has_history && fin) {
    const float sc = ((float)x + 0.5f) / (float)a.width, tc = ((float)y + 0.5f) / (float)a.height;
    const float rx = ((a.llc[0] + sc * a.hor[0]) + tc * a.ver[0]) - a.o[0];
    const float ry = ((a.llc[1] + sc * a.hor[1]) + tc * a.ver[1]) - a.o[1];
    const float rz = ((a.llc[2] + sc * a.hor[2]) + tc * a.ver[2]) - a.o[2];
    const bool hit = z > 0.0f;
    float dx = rx, dy = ry, dz = rz; // a missed pixel reprojects as a direction
    if (hit) { dx = (a.o[0] + z * rx) - a.po[0]; dy = (a.o[1] + z * ry) - a.po[1]; dz = (a.o[2] + z * rz) - a.po[2]; }
    const float cp = -((dx * a.pw[0] + dy * a.pw[1]) + dz * a.pw[2]);
    const float r = a.fo / cp, te = cp / a.fo;
    const float s1 = (((dx * a.ph[0] + dy * a.ph[1]) + dz * a.ph[2]) * r) / a.hh + 0.5f;
    const float t1 = (((dx * a.pv[0] + dy * a.pv[1]) + dz * a.pv[2]) * r) / a.vv + 0.5f;
    const float fx = s1 * (float)a.width - 0.5f, fy = t1 * (float)a.height - 0.5f;
    if (cp > 0.0f && fx >= -1.0f && fx < (float)a.width && fy >= -1.0f && fy < (float)a.height) { // (NaN fails)
      const float fx0 = floorf(fx), fy0 = floorf(fy);
      const float ax = fx - fx0, ay = fy - fy0;
      const int x0 = (int)fx0, y0 = (int)fy0; // -1 ... width - 1, -1 ... height - 1
      const float tol_te = a.tol_depth * te;
      float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f, g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, hN = 0.0f, bs = 0.0f;
#pragma unroll
      for (int j = 0; j < 2; j++) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
          const int qx = x0 + i, qy = y0 + j;
          if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) continue;
          const float b = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
          const long long q = (long long)qy * a.width + qx;
          const f4 qa = a.prev[q], qb = a.prev[a.pixels + q], qc = a.prev[2 * a.pixels + q];
          bool ok = qa.w >= 1.0f;
          ok = ok && (hit ? (qb.w > 0.0f && fabsf(qb.w - te) <= tol_te) : !(qb.w > 0.0f));
          if (a.id) ok = ok && __float_as_int(qc.w) == k;
          if (a.normal) {
            const float ex = nx - qc.x, ey = ny - qc.y, ez = nz - qc.z;
            ok = ok && ((ex * ex + ey * ey) + ez * ez) <= a.tn2;
          }
          if (ok) {
            h0 = h0 + b * qa.x; h1 = h1 + b * qa.y; h2 = h2 + b * qa.z;
            g0 = g0 + b * qb.x; g1 = g1 + b * qb.y; g2 = g2 + b * qb.z;
            hN = hN + b * qa.w;
            bs = bs + b;
          }
        }
      }
      if (bs > 0.01f) {
        h0 = h0 / bs; h1 = h1 / bs; h2 = h2 / bs;
        g0 = g0 / bs; g1 = g1 / bs; g2 = g2 / bs;
        N = fminf(hN / bs + 1.0f, 65536.0f);
        ap = fmaxf(1.0f / N, a.alpha);
        c0 = h0 + ap * (cr - h0); c1 = h1 + ap * (cg - h1); c2 = h2 + ap * (cb - h2);
        m0 = g0 + ap * (cr * cr - g0); m1 = g1 + ap * (cg * cg - g1); m2 = g2 + ap * (cb * cb - g2);
      }
    }
  }
  float o0 = cr, o1 = cg, o2 = cb, v0 = inf, v1 = inf, v2 = inf, oh = 0.0f;
  if (fin) {
    o0 = c0; o1 = c1; o2 = c2; oh = N;
    if (N >= 4.0f) {
      v0 = fmaxf(m0 - c0 * c0, 0.0f) * ap; v1 = fmaxf(m1 - c1 * c1, 0.0f) * ap; v2 = fmaxf(m2 - c2 * c2, 0.0f) * ap;
    } else if (a.var_in) {
      v0 = a.var_in[p * 3]; v1 = a.var_in[p * 3 + 1]; v2 = a.var_in[p * 3 + 2];
    }
  } else { // a colour that is not finite stays where it is and never enters a history
    c0 = c1 = c2 = m0 = m1 = m2 = 0.0f; N = 0.0f;
  }
  a.out_color[p * 3] = o0; a.out_color[p * 3 + 1] = o1; a.out_color[p * 3 + 2] = o2;
  if (a.out_var) { a.out_var[p * 3] = v0; a.out_var[p * 3 + 1] = v1; a.out_var[p * 3 + 2] = v2; }
  if (a.out_hist) a.out_hist[p] = oh;
  const f4 ra = {c0, c1, c2, N}, rb = {m0, m1, m2, z}, rc = {nx, ny, nz, __int_as_float(k)};
  a.next[p] = ra; a.next[a.pixels + p] = rb; a.next[2 * a.pixels + p] = rc;
}

// ---- display stage (include/pt_render.h: PtDisplay, pt_display_meter, pt_display_apply) ---------------------------------------------------
// The end of the image-space chain: a luminance histogram, an exposure solved from it on the device, and exposure + tone curve + quantise()
// in one pass.  Same rules as the filters above: the header states every operation, this is that text in HIP.
//
// The state, in device memory (uint32 words): the working histogram — 256 bins, then `rejected` as a 257th — which is all zeros between
// meterings; the last metering's copy of it (pt_display_histogram); e, scale and `primed` (0: the next metering that solves is instant).
enum { DISP_BINS = 257, DISP_WORK = 0, DISP_LAST = 257, DISP_E = 514, DISP_SCALE = 515, DISP_PRIMED = 516, DISP_WORDS = 517 };
enum { DISP_METER_THREADS = 256, DISP_METER_MAX_BLOCKS = 256 }; // the fastest grid measured, one workgroup per CU (profiles/display_bench.txt): the rest of a frame is the metering loop

// bin of one pixel: 0 ... 255, or 256 = rejected (NaN, +-inf, negative, +-0)
__device__ __forceinline__ int display_bin(float r, float g, float b) {
  const float y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
  const unsigned bits = __float_as_uint(y);
  if (!(y > 0.0f) || bits >= 0x7f800000u) return 256;
  const int k = (int)(bits >> 20) - ((127 - 16) << 3);
  return k < 0 ? 0 : k > 255 ? 255 : k;
}

// 2^e for |e| <= 32 (include/pt_render.h: Scale)
__device__ __forceinline__ float display_scale(float e) {
  const float k = ceilf(e);
  return ldexpf(exp_neg((k - e) * 0x1.62e430p-1f), (int)k);
}

// One LDS histogram per workgroup, one LDS integer atomic per pixel, and the workgroup's non-zero bins to the global histogram with one
// atomic each.  What costs is the number of workgroups — each one zeroes, synchronises and flushes up to 257 atomics onto the same 257
// words — not the LDS atomics: a constant frame, whose adds all hit one address, meters no slower than a frame that spreads over every bin,
// so per-wave histograms and a ballot that adds a wave's equal bins once were measured and dropped (profiles/display_bench.txt;
// tools/ubench/display_stage.hip keeps the forms).  Hence the small grid and the grid-stride loop.
//   VEC   the pixels are ONE contiguous range (a whole frame, or a rectangle as wide as the frame) that starts on a 16-byte boundary:
//         a thread takes four consecutive pixels as three 16-byte loads; the last n % 4 pixels are taken one by one
//   !VEC  any rectangle: one pixel per thread and trip, its position from the rectangle's width
template <bool VEC>
__global__ __launch_bounds__(DISP_METER_THREADS) void display_meter_kernel(const float* __restrict__ color, unsigned* __restrict__ hist, int width,
                                                                           int x0, int y0, int rw, unsigned n) {
  __shared__ unsigned lds[DISP_BINS];
  for (int i = threadIdx.x; i < DISP_BINS; i += DISP_METER_THREADS) lds[i] = 0u;
  __syncthreads();
  const unsigned stride = gridDim.x * DISP_METER_THREADS;
  if (VEC) {
    const float* const first = color + ((long long)y0 * width + x0) * 3;
    const unsigned groups = n >> 2;
    for (unsigned g = blockIdx.x * DISP_METER_THREADS + threadIdx.x; g < groups; g += stride) {
      const f4* const q = reinterpret_cast<const f4*>(first) + (size_t)g * 3;
      const f4 a = q[0], b = q[1], c = q[2];
      atomicAdd(&lds[display_bin(a.x, a.y, a.z)], 1u);
      atomicAdd(&lds[display_bin(a.w, b.x, b.y)], 1u);
      atomicAdd(&lds[display_bin(b.z, b.w, c.x)], 1u);
      atomicAdd(&lds[display_bin(c.y, c.z, c.w)], 1u);
    }
    const unsigned i = (groups << 2) + threadIdx.x;
    if (blockIdx.x == 0 && i < n) atomicAdd(&lds[display_bin(first[(size_t)i * 3], first[(size_t)i * 3 + 1], first[(size_t)i * 3 + 2])], 1u);
  } else {
    for (unsigned i = blockIdx.x * DISP_METER_THREADS + threadIdx.x; i < n; i += stride) {
      const unsigned ry = i / (unsigned)rw, rx = i - ry * (unsigned)rw;
      const long long p = ((long long)(y0 + (int)ry) * width + (x0 + (int)rx)) * 3;
      atomicAdd(&lds[display_bin(color[p], color[p + 1], color[p + 2])], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DISP_BINS; i += DISP_METER_THREADS)
    if (lds[i]) atomicAdd(&hist[i], lds[i]);
}

struct DisplaySolveArgs {
  unsigned* state; // DISP_WORDS words
  int lo_permille, hi_permille;
  float ev_bias, ev_min, ev_max, adapt_up, adapt_down;
};

// One wave: lane l owns the bins 4 l ... 4 l + 3.  An inclusive wave scan of the lanes' counts gives every bin its first rank; the band's
// S and C are integer sums, reduced across the wave (any order: the same bits); lane 0 divides, adapts and stores e and scale.  Every lane
// copies its bins to the last-metering histogram and zeroes them for the next one.
__global__ __launch_bounds__(64) void display_solve_kernel(DisplaySolveArgs a) {
  constexpr int LOGC[8] = PT_DISPLAY_LOGC;
  const int lane = threadIdx.x;
  unsigned* const work = a.state + DISP_WORK;
  unsigned* const last = a.state + DISP_LAST;
  unsigned c[4], mine = 0u;
  for (int j = 0; j < 4; j++) { c[j] = work[4 * lane + j]; mine += c[j]; }
  unsigned incl = mine; // <= 2^31: the frame's pixels
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  const unsigned long long N = __shfl(incl, 63, 64);
  const unsigned long long lo_n = N * (unsigned long long)a.lo_permille / 1000ull, hi_n = N * (unsigned long long)a.hi_permille / 1000ull;
  unsigned long long rank = incl - mine;
  long long S = 0;
  unsigned long long C = 0;
  for (int j = 0; j < 4; j++) {
    const int b = 4 * lane + j;
    const unsigned long long end = rank + c[j];
    const unsigned long long from = rank > lo_n ? rank : lo_n, to = end < hi_n ? end : hi_n;
    if (to > from) {
      const long long value = 65536ll * ((b >> 3) - 16) + LOGC[b & 7];
      S += (long long)(to - from) * value;
      C += to - from;
    }
    rank = end;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    S += __shfl_xor(S, d, 64);
    C += __shfl_xor(C, d, 64);
  }
  for (int j = 0; j < 4; j++) { last[4 * lane + j] = c[j]; work[4 * lane + j] = 0u; }
  if (lane == 0) {
    last[256] = work[256];
    work[256] = 0u;
    if (C != 0) {
      const float t = (float)(((double)S / (double)C) * 0x1p-16);
      const float et = fminf(fmaxf((PT_DISPLAY_LOG2_KEY - t) + a.ev_bias, a.ev_min), a.ev_max);
      float e = et;
      if (a.state[DISP_PRIMED]) {
        const float e0 = __uint_as_float(a.state[DISP_E]);
        e = e0 + (et - e0) * (et > e0 ? a.adapt_up : a.adapt_down);
      }
      a.state[DISP_E] = __float_as_uint(e);
      a.state[DISP_SCALE] = __float_as_uint(display_scale(e));
      a.state[DISP_PRIMED] = 1u;
    }
  }
}

// pt_display_reset (reset != 0: the state after create) and pt_display_set_exposure (e = ev, primed)
__global__ __launch_bounds__(64) void display_set_kernel(unsigned* state, int reset, float ev) {
  if (reset)
    for (int i = threadIdx.x; i < 2 * DISP_BINS; i += 64) state[i] = 0u;
  if (threadIdx.x == 0) {
    state[DISP_E] = __float_as_uint(reset ? 0.0f : ev);
    state[DISP_SCALE] = __float_as_uint(reset ? 1.0f : display_scale(ev));
    state[DISP_PRIMED] = reset ? 0u : 1u;
  }
}

template <int TONE>
__device__ __forceinline__ float display_curve(float x, float iw2) {
  if (TONE == PT_TONE_REINHARD) return (x * (1.0f + x * iw2)) / (1.0f + x);
  if (TONE == PT_TONE_ACES) return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
  return x;
}

// One pass over the rows' values (the curve is per channel, so a row is 3 * width independent values: the loads, the byte stores and the
// float stores are all contiguous across a wave).  blockIdx.y walks the rows; row 0 of rgb8 is the top.  `scale` is read once: the state's
// (written by display_solve_kernel / display_set_kernel earlier on the stream), or 2^ev for the stateless call.  linear may be color: a
// thread reads its values before it writes them.
//   VEC   3 * width is a multiple of 4 and the planes are 16-byte aligned (rgb8: 4-byte): a thread takes four values — one 16-byte load, one
//         4-byte store of the bytes, one 16-byte store of the floats
//   !VEC  one value per thread
__device__ __forceinline__ float display_clamp(float x) {
  if (!(x >= 0.0f)) x = 0.0f;
  return x > 0x1p20f ? 0x1p20f : x;
}

template <int TONE, bool VEC>
__global__ __launch_bounds__(256) void display_apply_kernel(const float* color, const unsigned* __restrict__ state, float ev, float iw2,
                                                            uint8_t* __restrict__ rgb8, float* linear, int width, int height) {
  const long long row_items = VEC ? 3ll * width / 4 : 3ll * width;
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= row_items) return;
  const float scale = state ? __uint_as_float(state[DISP_SCALE]) : display_scale(ev);
  for (int row = blockIdx.y; row < height; row += gridDim.y) { // row 0 = top
    const long long src = (long long)(height - 1 - row) * row_items + f, dst = (long long)row * row_items + f;
    if (VEC) {
      const f4 v = reinterpret_cast<const f4*>(color)[src];
      f4 y;
      y.x = display_curve<TONE>(display_clamp(v.x * scale), iw2); y.y = display_curve<TONE>(display_clamp(v.y * scale), iw2);
      y.z = display_curve<TONE>(display_clamp(v.z * scale), iw2); y.w = display_curve<TONE>(display_clamp(v.w * scale), iw2);
      if (rgb8) {
        uchar4 o;
        o.x = quantise(y.x); o.y = quantise(y.y); o.z = quantise(y.z); o.w = quantise(y.w);
        reinterpret_cast<uchar4*>(rgb8)[dst] = o;
      }
      if (linear) reinterpret_cast<f4*>(linear)[src] = y;
    } else {
      const float y = display_curve<TONE>(display_clamp(color[src] * scale), iw2);
      if (rgb8) rgb8[dst] = quantise(y);
      if (linear) linear[src] = y;
    }
  }
}

#include "pt_firefly.hpp"
#include "pt_spatial_variance.hpp"
#include "pt_metrics.hpp"
#include "pt_encode.hpp"

thread_local std::string g_last_error;

// ---- tuning: include/pt_render.h PtTuning.  Resolved ONCE per scene (pt_scene_create / pt_debug_flatten), never on the launch path.
// A NULL PtTuning means the library's defaults with the PT_* environment variables applied on top (the override channel of tools/ and of
// A/B runs); an explicit struct is taken as it is and the environment is not consulted.
static void tuning_defaults(PtTuning& t) {
  std::memset(&t, 0, sizeof t);
  t.struct_size = (int32_t)sizeof(PtTuning);
}
static void tuning_env(PtTuning& t) {
  tuning_defaults(t);
  auto has = [](const char* n) { return std::getenv(n) != nullptr; };
  if (has("PT_NO_GRID")) t.sphere_grid = -1;
  if (const char* e = std::getenv("PT_GRID_M")) t.grid_margin = (float)std::atof(e);
  if (const char* e = std::getenv("PT_GRID_CELL")) t.grid_cell = (float)std::atof(e);
  t.slab_pools = has("PT_NO_BOXCULL") ? -1 : has("PT_POOL_ALWAYS") ? 1 : 0;
  if (has("PT_NO_TRICULL")) t.tri_pool = -1;
  if (has("PT_TRICULL")) t.tri_min_run = 256;
  if (const char* e = std::getenv("PT_TRI_M")) t.tri_M = (float)std::atof(e);
  if (has("PT_TRI_BINNED")) t.tri_binned = 1;
  if (has("PT_NO_TRI_CACHE")) t.tri_cache = -1;
  if (has("PT_NO_SPHERE_MERGE")) t.sphere_merge = -1;
  if (const char* e = std::getenv("PT_TRI_RES")) std::sscanf(e, "%d,%d,%d", &t.tri_res[0], &t.tri_res[1], &t.tri_res[2]);
  if (const char* e = std::getenv("PT_TRI_RHO")) std::sscanf(e, "%f,%f,%f", &t.tri_rho[0], &t.tri_rho[1], &t.tri_rho2);
  if (const char* e = std::getenv("PT_TRI_BUDGET_MB")) t.tri_budget_mb = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("PT_TRI_CELL")) t.tri_cell = (float)std::atof(e);
  if (const char* e = std::getenv("PT_TRI_MIN")) t.tri_min_run = std::max(1, std::atoi(e));
  if (has("PT_NO_MATSPEC")) t.generic_materials = 1;
  if (const char* e = std::getenv("PT_BLOCKS_PER_CU")) t.blocks_per_cu = std::max(1, std::atoi(e));
  if (has("PT_NO_COLD_LDS")) t.cold_state = -1;
  if (const char* e = std::getenv("PT_WIDE_LOGG")) t.wide_log2_group = std::min(6, std::max(1, std::atoi(e)));
  if (const char* e = std::getenv("PT_SPLIT_TILES")) { t.split_tiles_mode = 1; t.split_tiles = std::atoi(e); }
  if (const char* e = std::getenv("PT_LPT_MAX")) t.lpt_by_max = std::atoi(e) != 0 ? 1 : -1;
  if (const char* e = std::getenv("PT_PROBE_SPP_MAX")) t.probe_spp_max = std::max(1, std::atoi(e));
  if (has("PT_NO_PROBE_RESUME")) t.probe_resume = -1;
  if (has("PT_NO_CHAIN_PRIO")) t.chain_priority = -1;
  if (const char* e = std::getenv("PT_GRID_MIN_TILES")) t.grid_min_tiles = std::max(0, std::atoi(e));
  if (const char* e = std::getenv("PT_MODEL_FIXED")) t.model_fixed = (float)std::atof(e);
  if (const char* e = std::getenv("PT_MODEL_CHAIN")) t.model_chain = (float)std::atof(e);
  if (const char* e = std::getenv("PT_SCATTER_LOG")) t.scatter_log = std::min(5, std::max(0, std::atoi(e)));
  t.scatter_mode = has("PT_NO_SCATTER") ? -1 : has("PT_LPT_SCATTER") ? 1 : 0;
  if (const char* e = std::getenv("PT_GRID_WALK")) t.grid_walk = std::atoi(e);
  if (const char* e = std::getenv("PT_LANES_CAP")) t.lanes_cap = std::atoi(e) <= 0 ? -1 : std::min(64, std::atoi(e));
  if (const char* e = std::getenv("PT_HEAVY_TILES")) t.heavy_tiles = std::atoi(e) <= 0 ? -1 : std::atoi(e);
}
// the caller's struct (possibly from an older header: struct_size bytes are valid) or, for NULL, defaults + environment
static int resolve_tuning(const PtTuning* user, PtTuning& t, std::string& err) {
  if (!user) { tuning_env(t); return PT_OK; }
  if (user->struct_size < 8 || user->struct_size > (int32_t)sizeof(PtTuning)) { err = "PtTuning.struct_size is not a size this library knows (use pt_tuning_init)"; return PT_ERR_INVALID_ARG; }
  tuning_defaults(t);
  std::memcpy(&t, user, (size_t)user->struct_size);
  t.struct_size = (int32_t)sizeof(PtTuning);
  return PT_OK;
}

// The flattening pt_scene_create uploads (pt_debug_flatten shows the same blob).
// LDS budget: the culling grid's tables ride in the blob, and only the LDS-resident kernels walk the grid.  A scene whose
// blob exceeds kMaxLdsBlob WITH its grid but fits WITHOUT it (e.g. 1 200 small spheres: 101 KB against 62 KB) is flattened
// without the grid, so that it keeps the resident kernels instead of falling to the streaming kernel with dead tables.
static int flatten_tuned(const PtSceneDesc* desc, const PtTuning& t, ptf::Flat& flat, std::string& err) {
  const int box_cull = t.slab_pools < 0 ? 0 : t.slab_pools > 0 ? 2 : 1;
  ptf::GridTuning tune;
  if (t.grid_margin > 0.0f) tune.m = t.grid_margin;
  if (t.grid_cell > 0.0f) tune.cell = t.grid_cell;
  const bool allow_grid = t.sphere_grid >= 0;
  // Exact culling of long triangle runs (pt_tripool.hpp; pt_device.hpp: tri_pool_scan).  Default: runs of >= 4096 triangles get a
  // pool (BASELINE config 5, 100 k triangles: 68.9 -> 18.6 s per frame, bit-identical).
  bool allow_tri = t.tri_pool >= 0;
  for (int i = 0; desc && desc->hittables && i < desc->n_hittables && allow_tri; i++) // scenes with Badouel-strategy triangles render through the
    if (desc->hittables[i].kind == PT_HIT_TRIANGLE && desc->hittables[i].strategy == PT_TRI_BADOUEL) allow_tri = false; // round-2 kernels: no dead tables
  ptf::TriPoolTuning tri;
  if (t.tri_min_run > 0) tri.min_run = t.tri_min_run;
  if (t.tri_M > 0.0f) tri.M = t.tri_M;
  for (int k = 0; k < 3; k++) if (t.tri_res[k] > 0) tri.dm_res[k] = t.tri_res[k];
  if (t.tri_rho[0] != 0.0f) tri.dm_rho[0] = t.tri_rho[0]; // (< 0: no such map)
  if (t.tri_rho[1] != 0.0f) tri.dm_rho[1] = t.tri_rho[1];
  if (t.tri_rho2 != 0.0f) tri.dm_rho[2] = t.tri_rho2;
  if (t.tri_budget_mb > 0) tri.dm_budget = (long long)t.tri_budget_mb * (1 << 18); // MiB -> 4-byte entries
  if (t.tri_cell > 0.0f) tri.cell = t.tri_cell;
  if (const char* e = std::getenv("PT_TRI_GRID_BUDGET")) tri.grid_budget = (float)std::atof(e); // (experiments only: not a PtTuning field)
  const bool merge = t.sphere_merge >= 0;
  // (the octant tables of the slab pools are ptf::flatten's own decision — all pools or none, by the same LDS budget; PT_NO_POOL_OCTANTS, for
  // tests only and no PtTuning field like PT_TRI_GRID_BUDGET, lays the scene out as it was before the tables: it then renders through the
  // scalar-cache kernels)
  const bool octants = !std::getenv("PT_NO_POOL_OCTANTS");
  int rc = ptf::flatten(desc, flat, err, allow_grid, box_cull, tune, allow_tri, tri, merge, octants);
  if (rc) return rc;
  if (flat.grid_spheres > 0 && flat.blob.size() * 16 > kMaxLdsBlob) {
    ptf::Flat plain;
    std::string err2;
    if (flat.tri_pooled == 0 && ptf::flatten(desc, plain, err2, false, box_cull, tune, allow_tri, tri, merge, octants) == PT_OK && plain.blob.size() * 16 <= kMaxLdsBlob) flat = std::move(plain);
  }
  return PT_OK;
}

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define PT_HIP(expr)                                                                             \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return fail(PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// The launch-side knobs of a scene's PtTuning, resolved once in pt_scene_create — never on the launch path.
struct Knobs {
  int blocks_per_cu = 0;   // cap on resident workgroups per CU (0 = none)
  bool no_cold_lds = false;
  int wide_logG = 0;       // forced log2 group size of the wide phase (0 = the model picks)
  bool has_split_tiles = false;
  int split_tiles = 0;     // fixed number of tiles through the wide phase (< 0: all)
  int lpt_max = -1, probe_spp_max = 16; // order tiles by their heaviest pixel (-1: by kernel family); probe depth cap
  int grid_min_tiles = kGridMinTiles;    // frames (shards) of fewer tiles keep the cooperative kernels and the lists
  float model_fixed = 2400.0f, model_chain = 2400.0f; // constants of the makespan model (lpt_order_kernel)
  int scatter_log = 0;     // log2 of the pixels of one tile that a wave takes together (0: every lane a pixel of another tile)
  bool lpt_with_scatter = false; // the cost probe + heaviest-first order also for scattered (triangle-pool) renders
  bool no_scatter = false; // triangle-pool kernels hand out whole tiles' pixels to a wave again (lane_acquire)
  bool generic_materials = false;
  int grid_walk = 0;       // PtTuning.grid_walk: 0 the launcher's rule, 1 the wave-synchronous walk, 2 the queued walk
  int lanes_cap = 0;       // PtTuning.lanes_cap: grid kernels on small frames (plan_pass): 0 the rule, -1 whole tiles always, n forced
  bool no_tri_cache = false;  // PtTuning.tri_cache = -1: camera rays enumerate their direction-map list like every other ray
  bool no_chain_prio = false; // PtTuning.chain_priority = -1: no issue priorities in the headline family's frame launches
  bool no_resume = false;  // PtTuning.probe_resume = -1: the probe's samples are rendered again by the frame launch
  int heavy_tiles = 0;     // PtTuning.heavy_tiles: tiles at the head of the cost-sorted order that are handed out 16 pixels at a time: 0 the rule, -1 never, n forced
  Knobs() {}
  explicit Knobs(const PtTuning& t) {
    blocks_per_cu = std::max(0, t.blocks_per_cu);
    no_cold_lds = t.cold_state < 0;
    wide_logG = std::min(6, std::max(0, t.wide_log2_group));
    has_split_tiles = t.split_tiles_mode == 1; split_tiles = t.split_tiles;
    lpt_max = t.lpt_by_max > 0 ? 1 : t.lpt_by_max < 0 ? 0 : -1;
    if (t.probe_spp_max > 0) probe_spp_max = t.probe_spp_max;
    if (t.grid_min_tiles > 0) grid_min_tiles = t.grid_min_tiles;
    if (t.model_fixed > 0.0f) model_fixed = t.model_fixed;
    if (t.model_chain > 0.0f) model_chain = t.model_chain;
    scatter_log = std::min(5, std::max(0, t.scatter_log));
    no_scatter = t.scatter_mode < 0; lpt_with_scatter = t.scatter_mode > 0;
    generic_materials = t.generic_materials != 0;
    lanes_cap = t.lanes_cap < 0 ? -1 : std::min(64, t.lanes_cap);
    grid_walk = (t.grid_walk == 1 || t.grid_walk == 2) ? t.grid_walk : 0;
    heavy_tiles = t.heavy_tiles < 0 ? -1 : t.heavy_tiles;
    no_resume = t.probe_resume < 0;
    no_chain_prio = t.chain_priority < 0;
    no_tri_cache = t.tri_cache < 0;
  }
};

// Which kernel instantiation a pass launched (pt_debug_last_kernels): w[0] the family, then that family's template arguments in the
// template's order — render_kernel: the eleven KV members; render_kernel_stream: UV, FAST, BADOUEL; the binned pair: UV, MATS.
enum { KFAM_NONE = 0, KFAM_RENDER = 1, KFAM_STREAM = 2, KFAM_SINGLE = 3, KFAM_BINNED = 4 };
struct KTag { int w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; };

struct EventPair { // RAII: no leak on an early return
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

template <typename T>
struct DevBuf { // owned device memory (move-only): freed with the local, the PtScene or the PtAccum that holds it
  T* p = nullptr;
  size_t cap = 0; // elements asked for
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~DevBuf() { if (p) (void)hipFree(p); }
  // n elements (at least one is allocated), in place of what it held
  hipError_t alloc(size_t n) {
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const hipError_t e = hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) cap = n; else p = nullptr;
    return e;
  }
  // grow-only workspaces: nothing happens while n elements fit (hipMalloc / hipFree synchronise the device)
  hipError_t grow(size_t n) { return p && cap >= n ? hipSuccess : alloc(n); }
};

} // namespace

struct PtScene {
  DevBuf<f4> blob;      // [blob records][material table]
  f4* mats = nullptr;   // ... the material table in it (not owned)
  DevBuf<f4> pool;      // tables of the triangle pools (a buffer of their own: up to gigabytes)
  size_t pool_bytes = 0;
  DevBuf<uint8_t> atlas;
  int n_runs = 0, blob_f4 = 0, mats_f4 = 0;
  int shade_f4 = 0, shade_base = 0; // the one pool's shade table (pt_flatten.hpp: Flat::shade): its records ride behind the materials, on the device and in the LDS image
  bool has_image = false;
  bool track_uv = false; // an image texture sits on a triangle or a medium: the stale u,v such hits inherit must be tracked
  bool fast_ok = false;
  bool coop_ok = false;
  bool has_badouel = false; // Badouel-strategy triangles: the scalar-cache / streaming kernels compiled with their loop
  int coop_prefix = 0;
  int n_hittables = 0;
  mutable bool last_had_wide_phase = false;
  mutable int last_launch[4] = {0, 0, 0, 0}; // what the launcher decided for the last frame launch: workgroups, lanes_cap, heavy_pixels, queued walk (pt_debug_last_launch)
  mutable KTag last_kernels[2];     // the kernels of the last pt_render / pt_render_accumulate: [0] the probe pass, [1] the frame pass (pt_debug_last_kernels)
  mutable int last_aov[2] = {0, 0}; // the last AOV pass's kernel: sphere-grid walk (1 / 2), u,v tracked (pt_debug_last_aov)
  mutable int nsplit_override = 0; // PT_SPLIT_TILES tuning knob (host copy must outlive the async upload)
  float traversal_cost = 0.0f; // estimated VALU instructions of one ray's scan of the list (sphere runs through their lists)
  int grid_spheres = 0;        // spheres that sit in a culling grid (the resident non-cooperative kernels walk it)
  int tri_pooled = 0;          // triangles that sit in a triangle pool (the TRIPOOL kernels query it)
  bool pools_need_scalar = false; // the scene has slab pools WITHOUT octant tables (ptf::flatten): only the scalar-cache kernels scan such pools
  bool rectbox_only = false;   // every hittable is a rect or a box (kernels compiled with MATS_RECTBOX_ONLY: resolve_hit)
  bool mats_simple = false;    // every material is lambertian or lightsource over a solid texture (kernels compiled with MATS_LAMB_LIGHT_SOLID)
  PoolPlan pool_plan;          // what the flattened scene allows (scene_pool_plan); a pass's kernel gets pass_pool_plan's view of it
  mutable PoolPlan last_pool_plan; // ... and what the last frame pass was given (pt_debug_last_pool_plan)
  size_t blob_bytes = 0, atlas_bytes = 0;
  int num_cus = 256;
  size_t lds_per_block = 64 * 1024; // hipDeviceProp_t::sharedMemPerBlock (gfx950: 160 KB; the Makefile's ARCH=gfx942: 64 KB)
  mutable DevBuf<unsigned int> ws_cost; // LPT workspace: per-tile ray counts of the probe pass
  mutable DevBuf<unsigned int> ws_rank; // per local tile: the cost a tile is ranked by (tile_dilate_kernel)
  mutable DevBuf<unsigned int> ws_rng;  // per local pixel: the generator's state after the probe's samples (KArgs.resume_rng)
  mutable DevBuf<int> ws_order;         //                cost-sorted tile order
  DevBuf<int> ws_nsplit;                //                number of leading tiles to split (device scalar)
  mutable DevBuf<float> ws_partial;     // PT_FLAG_FAST_RNG: per-chunk partial sums (grow-only)
  // the binned triangle-pool renderer (pt_binned.hpp): the pooled run, the key space of its direction maps, and a grow-only workspace
  int bin_run = -1, bin_hdr = 0, bin_goff = 0, bin_keys = 0, bin_full_slices = 1, bin_base1 = 0;
  bool binned = false;          // this scene's parity-mode renders go through it
  mutable DevBuf<unsigned int> ws_tricache; // the camera rays' candidate cache: one line per resident lane of the triangle-pool kernels
  mutable DevBuf<char> ws_bin; // per-pixel state, requests and slots for the local pixels of the largest binned render so far; the sort's tables
  mutable int last_generations = 0; // generations of the last binned render (pt_debug_last_launch)
  DevBuf<unsigned int> queues; // ring of per-launch pixel-queue counters
  mutable unsigned int next_queue = 0;
  mutable hipEvent_t ring_done[kQueueRing] = {}; // recorded behind the launch that uses a slot: a wrapped ring waits for it
  int device = 0;
  // Scheduling state above marked `mutable` (queue ring cursor, LPT workspace, last-launch info) changes per launch although
  // the scene DATA is immutable: launches on one scene from several host threads serialise their ENQUEUE on this mutex.
  // The per-scene workspaces (ws_cost / ws_order / ws_rng / ws_nsplit / ws_partial) are shared by every launch on the scene, so
  // renders on ONE scene must also be stream-ordered (include/pt_render.h): callers that render one scene from several
  // streams create one PtScene per stream (path_tracer_amd/render.py keys its cache by (device, stream)).
  mutable std::mutex sched;
  mutable std::map<const void*, int> occupancy; // resident workgroups per CU, per kernel variant (queried once)
  Knobs knobs;                                  // the scene's PtTuning (launch side), as resolved when the scene was created
};

namespace {

// ---- which kernel variant a launch runs -------------------------------------------------------------------

// A render_kernel instantiation by name: one member per template parameter, with the template's defaults.
struct KV {
  int uv = UV_NONE;
  bool lds = false, mlds = false, coop = false, cl = false, fast = false, badouel = false;
  int grid = 1;
  bool tripool = false;
  int mats = MATS_ALL;
  int block = kBlock;
};
typedef void (*Kernel)(KArgs);
// (the only place that lists render_kernel's parameters by position)
template <KV V>
constexpr Kernel kernel_of = render_kernel<V.uv, V.lds, V.mlds, V.coop, V.cl, V.fast, V.badouel, V.grid, V.tripool, V.mats, V.block>;
// A kernel and the tag that names it, from ONE constant: the launcher picks kernels only through these, so the two cannot disagree.
struct Picked { Kernel kernel; KTag tag; };
template <KV V>
constexpr Picked picked_of = {kernel_of<V>, {{KFAM_RENDER, V.uv, V.lds, V.mlds, V.coop, V.cl, V.fast, V.badouel, V.grid, V.tripool, V.mats, V.block}}};
template <int UV, bool FAST = false, bool BADOUEL = false>
constexpr Picked stream_of = {render_kernel_stream<UV, FAST, BADOUEL>, {{KFAM_STREAM, UV, FAST, BADOUEL}}};

// Resident workgroups per CU of a kernel variant: queried once per scene, then from PtScene.occupancy.  < 0: the query failed (pt_last_error).
int occupancy_of(const PtScene* s, const void* kernel, int block_threads, size_t shmem) {
  auto cached = s->occupancy.find(kernel);
  if (cached != s->occupancy.end()) return cached->second;
  int per_cu = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block_threads, shmem);
  if (e != hipSuccess) { fail(PT_ERR_HIP, std::string("occupancy query of a kernel variant: ") + hipGetErrorString(e)); return -1; }
  s->occupancy[kernel] = per_cu;
  return per_cu;
}

// How a scene's kernels obtain u,v (the UV parameter of its kernel variants)
int uv_of(const PtScene* s) { return s->track_uv ? UV_TRACKED : s->has_image ? UV_WINNER : UV_NONE; }

// The triangle-pool kernel of a scene's UV mode: what choose_variant picks for such a scene, and what reserve_tricache sizes the cache for.
Picked tripool_kernel(int uv, bool fast) {
  switch (uv) {
    case UV_TRACKED: return fast ? picked_of<KV{.uv = UV_TRACKED, .fast = true, .tripool = true}> : picked_of<KV{.uv = UV_TRACKED, .tripool = true}>;
    case UV_WINNER: return fast ? picked_of<KV{.uv = UV_WINNER, .fast = true, .tripool = true}> : picked_of<KV{.uv = UV_WINNER, .tripool = true}>;
    default: return fast ? picked_of<KV{.fast = true, .tripool = true}> : picked_of<KV{.tripool = true}>;
  }
}

// The headline family's kernel — no image texture, no grid walk — for the material and hittable kinds MATS; `cold`: cold lane state in LDS
template <int MATS>
Picked headline_kernel(bool lds, bool mlds, bool cold) {
  if (!lds) return picked_of<KV{.grid = 0, .mats = MATS}>;
  if (cold) return picked_of<KV{.lds = true, .mlds = true, .cl = true, .grid = 0, .mats = MATS}>;
  return mlds ? picked_of<KV{.lds = true, .mlds = true, .grid = 0, .mats = MATS}> : picked_of<KV{.lds = true, .grid = 0, .mats = MATS}>;
}

// The binned renderer's two kernels that shade (pt_binned.hpp), compiled for a scene's UV mode and material kinds
struct BinKernels { void (*step)(BinArgs); void (*finish)(BinArgs); KTag tag; };
template <int UV, int MATS>
constexpr BinKernels bin_kernels = {bin_step_kernel<UV, MATS>, bin_finish_kernel<UV, MATS>, {{KFAM_BINNED, UV, MATS}}};

// What choose_variant decides for one pass of launch_render: the kernel, and the facts about it that the launch reads.
struct Variant {
  int rc = PT_OK;          // != PT_OK: no kernel (pt_last_error says why)
  Kernel kernel = nullptr;
  KTag tag;                // ... and its name (pt_debug_last_kernels): both set by pick() alone
  void pick(const Picked& k) { kernel = k.kernel; tag = k.tag; }
  size_t shmem = 0;        // dynamic LDS: the blob image (+ the material table) of the LDS-resident kernels
  int coop_prefix = -1;    // KArgs.coop_prefix
  bool tri_pool = false;   // the scene's triangle pools are queried (the TRIPOOL kernels)
  bool resident = false;   // render_kernel (blob in LDS or read through the scalar cache), not render_kernel_stream
  bool use_grid = false;   // the kernel walks the scene's sphere grids
  bool coop = false;       // cooperative kernel
  bool chain_bound = false; // the headline family — no sphere grid, no cooperative phase: see `plan_pass`
  bool queued_walk = false; // the kernel walks sphere grids through the pair queue (pt_debug_last_launch)
};

// The kernel variant of one pass over local_tiles tiles: `fast` — the pass is a PT_FLAG_FAST_RNG launch (the probe of such a render is not);
// n_local_pixels — the pass's KArgs.n_local_pixels.
template <int UV>
Variant choose_variant_uv(const PtScene* s, const PtRenderParams* p, int local_tiles, bool fast, int n_local_pixels) {
  Variant v;
  const bool fast_ok = s->fast_ok && !(p->flags & PT_FLAG_NO_FASTDIV);
  v.coop_prefix = (s->coop_ok && fast_ok && !(p->flags & PT_FLAG_NO_COOP)) ? s->coop_prefix : -1;
  const size_t blob_bytes = (size_t)s->blob_f4 * 16;
  // a scene with a triangle pool is queried through per-lane loads from the global blob: the scalar-cache resident kernels,
  // whatever its size (PT_FLAG_FORCE_STREAM: the streaming kernel, which scans every triangle, as the A/B)
  v.tri_pool = s->tri_pooled > 0 && !(p->flags & PT_FLAG_FORCE_STREAM);
  v.resident = (blob_bytes <= kMaxLdsBlob || (p->flags & PT_FLAG_NO_LDS) || v.tri_pool) && !(p->flags & PT_FLAG_FORCE_STREAM);
  // The LDS kernels hold only the sign-resolved slab pass, which reads a pool's octant table (pt_device.hpp: slab_chunk_pass): a scene whose pools
  // have none — the tables would have pushed its blob past the LDS image — takes the scalar-cache kernels it would take under PT_FLAG_NO_LDS.
  const bool lds = v.resident && !(p->flags & PT_FLAG_NO_LDS) && !v.tri_pool && !s->pools_need_scalar;
  // (the shade table rides behind the materials and weighs on both thresholds with them: 16 bytes per hittable of a small rect / box-only
  // scene — the 16-entry pool's 6.1 KB image holds 304 of them — so a cold-state workgroup stays within 18 KB, seven to a CU's 160 KB.
  // A rect / box-only scene of simple materials WITHOUT a table — more than ptf::kShadeMaxHittables records, which no 16 KB image holds —
  // never gets its materials staged: the kernels that would stage them read the table)
  const size_t mats_bytes = ((size_t)s->mats_f4 + (size_t)s->shade_f4) * 16;
  const bool mlds = lds && blob_bytes + mats_bytes <= kMaxLdsWithMaterials && !(s->rectbox_only && s->mats_simple && s->shade_f4 == 0);
  v.shmem = lds ? blob_bytes + (mlds ? mats_bytes : 0) : 0;
  const bool cold = mlds && v.shmem <= kMaxLdsColdScene && !s->knobs.no_cold_lds; // small scene: cold lane state in LDS (7 workgroups x (scene + 8 KB) per CU)
  // Cooperative kernels (a ray's list split over idle lanes; the heaviest tiles rendered G lanes per pixel) cost ~15 % of
  // the ordinary-mode throughput, and the part of an iteration that cannot be split (camera, shading, ray context:
  // ~4 500 cycles of a lone wave's 13 200 on the Cornell-style scene) bounds what they can win: there G = 8 shortens a
  // pixel's chain by 1.4x for 4.6x the lane time, so they pay only where the scan of the list dominates an iteration
  // (496-hittable scene, shard 0/8: 522 -> 229 ms).
  // Sphere runs with a culling grid: the ordinary resident kernels walk it (a ray then tests tens of spheres instead of
  // hundreds: 496-hittable scene 1 660 -> 3 240 Msamples/s at 1080p), the cooperative kernels scan the lists with lane
  // groups.  With the grid as first tuned (margin 1.5 r) a lone wave's walk was no shorter than a group's list scan and small
  // frames / shards kept the cooperative kernels; since the retuning (margin 0.5 r, walk after the big spheres) the walk wins
  // everywhere (tools/grid_min_tiles.py: 400x225x256 spp 99 ms against 108; shard 0/8 of the 1080p frame at 256 spp 80
  // against 102; shard 0/8 of 4K at 128 spp 61 against 102).  PT_GRID_MIN_TILES restores a threshold.
  v.use_grid = s->grid_spheres > 0 && v.resident /* the streaming kernel scans the full lists */ && local_tiles >= s->knobs.grid_min_tiles && !(p->flags & PT_FLAG_FORCE_COOP);
  v.coop = lds && v.coop_prefix >= 0 && !v.use_grid && (s->traversal_cost >= kCoopMinTraversal || (p->flags & PT_FLAG_FORCE_COOP));

  if (s->has_badouel) { // parity-completeness path: scalar-cache or streaming kernel with the Badouel loop compiled in
    if (fast) { v.rc = fail(PT_ERR_INVALID_ARG, "PT_FLAG_FAST_RNG is not offered for scenes with Badouel-strategy triangles"); return v; }
    v.pick(!v.resident ? stream_of<UV, false, true> : picked_of<KV{.uv = UV, .badouel = true}>);
    return v;
  }
  if (fast) { // opt-in decorrelated mode: its own instantiations (no cooperative kernels: a chunk is short)
    if (v.tri_pool) v.pick(tripool_kernel(UV, true));
    else if (!v.resident) v.pick(stream_of<UV, true>);
    else if (!lds) v.pick(picked_of<KV{.uv = UV, .fast = true}>);
    else v.pick(mlds ? picked_of<KV{.uv = UV, .lds = true, .mlds = true, .fast = true}> : picked_of<KV{.uv = UV, .lds = true, .fast = true}>);
    return v;
  }
  if (v.tri_pool) { v.pick(tripool_kernel(UV, false)); return v; }
  if (!v.resident) { v.pick(stream_of<UV>); return v; }
  if constexpr (UV == UV_NONE) { // no image texture and no sphere grid (the headline scene): kernels without the grid walk
    if (s->grid_spheres == 0 && !v.coop) {
      v.chain_bound = true;
      // lambertian + lightsource over solid textures: kernels without the other materials' code
      // ... and every hittable a rect or a box (the headline scene): resolve_hit without the other kinds
      v.pick(!s->mats_simple    ? headline_kernel<MATS_ALL>(lds, mlds, cold)
             : !s->rectbox_only ? headline_kernel<MATS_LAMB_LIGHT_SOLID>(lds, mlds, cold)
                                : headline_kernel<MATS_LAMB_LIGHT_SOLID | MATS_RECTBOX_ONLY>(lds, mlds, cold));
      return v;
    }
  }
  if (!lds) { v.pick(picked_of<KV{.uv = UV}>); return v; }
  // (UV_TRACKED scenes are never cooperative — track_uv is has_image && !coop_ok, and coop_prefix then stays -1 — so no such kernel is compiled)
  if constexpr (UV != UV_TRACKED) {
    if (v.coop) { v.pick(mlds ? picked_of<KV{.uv = UV, .lds = true, .mlds = true, .coop = true}> : picked_of<KV{.uv = UV, .lds = true, .coop = true}>); return v; }
  }
  if constexpr (UV == UV_NONE) {
    // (deliberately BEFORE the choice of walk: the cold-state kernel has the in-place walk only, so a scene this small keeps it even under
    // PtTuning.grid_walk = 2 — the pair queue's static LDS and extra live values would cost the occupancy CL buys)
    if (cold) { v.pick(picked_of<KV{.lds = true, .mlds = true, .cl = true}>); return v; }
  }
  if (v.use_grid) {
    // Which sphere-grid walk (pt_device.hpp: sphere_scan, GRID = 1 / 2): the pair queue where walks diverge or the launch is bound by its
    // chains — whole tiles per wave or at least 16 lanes (the rule of `plan_pass`, evaluated for the kernels' four workgroups per CU) — and
    // not on frames that are both dense (>= 4 M pixels: a tile's rays share their cells) and throughput-bound (>= 6 pixels per resident lane).
    // The rule is evaluated for the resident lanes the GRID = 2 kernels really have (their occupancy is queried like `plan_pass` does: 31 KB LDS
    // image + 4 KB of per-wave queues and slots usually allow four workgroups per CU) — round 4 assumed 16 waves per CU here and the cap of
    // `plan_pass` from the measured occupancy, and the two could disagree.  The queued walk's STATIC 4 KB of LDS (sphere_queue,
    // sphere_slots) ride on top of the dynamic blob image: where the sum exceeds what a workgroup may have, the walk stays in place.
    constexpr size_t kQueuedWalkStaticLds = (size_t)PT_MAX_WAVES_PER_BLOCK * (PT_SQ_CAP * 4 + 64 * 8);
    const Picked queued = mlds ? picked_of<KV{.uv = UV, .lds = true, .mlds = true, .grid = 2}> : picked_of<KV{.uv = UV, .lds = true, .grid = 2}>;
    int per_cu_queued = 0; // (stays 0 where the queued walk's LDS does not fit: never asked)
    if (v.shmem + kQueuedWalkStaticLds <= s->lds_per_block) {
      per_cu_queued = occupancy_of(s, (const void*)queued.kernel, kBlock, v.shmem);
      if (per_cu_queued < 0) { v.rc = PT_ERR_HIP; return v; }
    }
    if (s->knobs.blocks_per_cu) per_cu_queued = std::min(per_cu_queued, s->knobs.blocks_per_cu);
    const bool fits = per_cu_queued >= 1;
    const double lanes = (double)std::max(1, s->num_cus) * std::max(1, per_cu_queued) * kWavesPerBlock * 64.0;
    const double rho = (double)n_local_pixels / lanes;
    const bool few_lanes = rho < 0.875 && !(p->flags & (PT_FLAG_TILE_GRANULAR | PT_FLAG_PIXEL_GRANULAR | PT_FLAG_FAST_RNG)) && s->knobs.lanes_cap >= 0; // 16 rho rounds below 16
    const bool dense_and_busy = (double)p->width * p->height >= 4.0e6 && rho >= 6.0;
    v.queued_walk = fits && (s->knobs.grid_walk == 2 || (s->knobs.grid_walk == 0 && !few_lanes && !dense_and_busy && !(s->knobs.lanes_cap > 0 && s->knobs.lanes_cap < 16)));
    // the sphere-grid walk through the pair queue (pt_device.hpp: sphere_scan says where it pays)
    if (v.queued_walk) { v.pick(queued); return v; }
  }
  v.pick(mlds ? picked_of<KV{.uv = UV, .lds = true, .mlds = true}> : picked_of<KV{.uv = UV, .lds = true}>);
  return v;
}

Variant choose_variant(const PtScene* s, const PtRenderParams* p, int local_tiles, bool fast, int n_local_pixels) {
  switch (uv_of(s)) {
    case UV_TRACKED: return choose_variant_uv<UV_TRACKED>(s, p, local_tiles, fast, n_local_pixels);
    case UV_WINNER: return choose_variant_uv<UV_WINNER>(s, p, local_tiles, fast, n_local_pixels);
    default: return choose_variant_uv<UV_NONE>(s, p, local_tiles, fast, n_local_pixels);
  }
}

// ---- the pool plan (pt_device.hpp: PoolPlan; hit_world_range, PLANNED) ----------------------------------------------------
// What a flattened scene allows, read from its blob the way the kernel's walk reads it: run 0's header, the aux record in front of its
// first record, and from (pool offset, n) the tables' places as slab_pool's callers compute them.  `one` is set where run 0 heads a pool
// that spans EVERY run of the list and carries an octant table; a list with a run outside the pool, with more than one pool, or whose
// pools have no tables (the blob beyond the LDS image) leaves it clear.  Which kernel runs, and under which flags, is pass_pool_plan's.
// The kernel's word says one thing more: whether the pool is ONE chunk of the slab pass (<= 16 entries: `one` = 2), which is the only pool its
// planned path holds code for; a larger one (`one` = 1) is claimed here, reported by the read-backs like any claimed pool, and walked.
PoolPlan scene_pool_plan(const ptf::Flat& flat) {
  PoolPlan pl;
  if (flat.n_runs < 1 || flat.blob.size() <= (size_t)flat.n_runs) return pl;
  auto word = [](float f) { int32_t v; std::memcpy(&v, &f, 4); return v; };
  const ptf::F4& run = flat.blob[0];
  pl.kind = word(run.x); pl.off = word(run.y); pl.count = word(run.z);
  if ((pl.kind != DK_RECT && pl.kind != DK_BOX) || pl.off < 1 || (size_t)pl.off > flat.blob.size()) return pl;
  const ptf::F4& aux = flat.blob[(size_t)pl.off - 1]; // (largest |coordinate|, span, pool offset, entries)
  const int span = word(aux.y);
  pl.bmax = aux.x; pl.pool_off = word(aux.z); pl.n = word(aux.w);
  pool_tables(pl.pool_off, pl.n, pl.x_off, pl.oct_off);
  // (2: the pool is one chunk of the slab pass, which is all the planned path of the kernels holds — a larger pool is claimed, reported, and walked)
  pl.one = (span == flat.n_runs && pl.n > 0 && flat.pool_octants && flat.fast_ok) ? (pl.n <= 16 ? 2 : 1) : 0;
  return pl;
}

// The plan one pass's kernel is given: the scene's, claimed only for a kernel that reads it — render_kernel over the LDS image, compiled
// for rect / box-only scenes (hit_world_range: PLANNED) — and only where rays may be regular at all (PT_FLAG_NO_FASTDIV: none is, every
// wave walks the list).  Every other kernel walks as it always did and never looks at the plan.
PoolPlan pass_pool_plan(const PtScene* s, const PtRenderParams* p, const Variant& v) {
  PoolPlan pl = s->pool_plan;
  const bool reads_plan = v.tag.w[0] == KFAM_RENDER && v.tag.w[2] /* lds */ && (v.tag.w[10] & MATS_RECTBOX_ONLY) != 0;
  if (!reads_plan || !s->fast_ok || (p->flags & PT_FLAG_NO_FASTDIV)) pl.one = 0;
  return pl;
}

// What a scene's launches decide from — plain facts of the description and of its flattened form, no device: pt_scene_create_tuned
// fills the PtScene it uploads with them, pt_debug_pool_plan a PtScene that never sees a device.
void set_scene_facts(PtScene* s, const PtSceneDesc* desc, const PtTuning& tun, const ptf::Flat& flat) {
  s->knobs = Knobs(tun);
  s->n_runs = flat.n_runs;
  s->blob_f4 = (int)flat.blob.size();
  s->has_image = flat.has_image;
  s->fast_ok = flat.fast_ok;
  s->coop_ok = flat.coop_ok && !flat.has_badouel; // the cooperative scans do not carry the Badouel loop
  s->has_badouel = flat.has_badouel;
  s->track_uv = flat.has_image && !flat.coop_ok;
  s->coop_prefix = flat.coop_prefix;
  s->n_hittables = desc->n_hittables;
  for (int i = 0; i < desc->n_hittables; i++) {
    switch (desc->hittables[i].kind) {
      case PT_HIT_SPHERE: s->traversal_cost += 22.0f; break;
      case PT_HIT_TRIANGLE: s->traversal_cost += 35.0f; break;
      case PT_HIT_BOX: s->traversal_cost += 120.0f; break;
      case PT_HIT_CONSTANT_MEDIUM: s->traversal_cost += 300.0f; break;
      default: s->traversal_cost += 20.0f; break;
    }
  }
  s->grid_spheres = flat.grid_spheres;
  s->pools_need_scalar = flat.pooled > 0 && !flat.pool_octants;
  s->rectbox_only = desc->n_hittables > 0 && !s->knobs.generic_materials;
#ifdef PT_NO_RECTBOX /* A/B build */
  s->rectbox_only = false;
#endif
  for (int i = 0; i < desc->n_hittables && s->rectbox_only; i++) {
    const int k = desc->hittables[i].kind;
    if (k != PT_HIT_XY_RECT && k != PT_HIT_XZ_RECT && k != PT_HIT_YZ_RECT && k != PT_HIT_BOX) s->rectbox_only = false;
  }
  s->mats_simple = desc->n_materials > 0 && !s->knobs.generic_materials; // PtTuning.generic_materials: A/B knob (generic shading)
  for (int i = 0; i < desc->n_materials && s->mats_simple; i++) {
    const PtMaterial& m = desc->materials[i];
    if ((m.kind != PT_MAT_LAMBERTIAN && m.kind != PT_MAT_LIGHTSOURCE) || desc->textures[m.texture].kind != PT_TEX_SOLID) s->mats_simple = false;
  }
  s->tri_pooled = flat.has_badouel ? 0 : flat.tri_pooled; // (scenes with Badouel-strategy triangles keep the round-2 kernels)
  s->blob_bytes = flat.blob.size() * 16;
  s->mats_f4 = (int)flat.mats.size();
  s->shade_f4 = (int)flat.shade.size();
  s->shade_base = flat.shade_base;
  s->pool_plan = scene_pool_plan(flat);
}

} // namespace

extern "C" {

int pt_abi_version(void) { return PT_ABI_VERSION; }

const char* pt_error_string(int code) {
  switch (code) {
    case PT_OK: return "ok";
    case PT_ERR_INVALID_ARG: return "invalid argument";
    case PT_ERR_BAD_SCENE: return "malformed scene tables";
    case PT_ERR_HIP: return "HIP runtime error";
    case PT_ERR_NO_DEVICE: return "no HIP device";
    case PT_ERR_TOO_LARGE: return "scene too large";
    default: return "unknown error";
  }
}

const char* pt_last_error(void) { return g_last_error.c_str(); }

// camera.hpp:67-87 (host arithmetic, binary32, no contraction)
int pt_camera_init(PtCamera* cam, const float look_from[3], const float look_at[3], const float vup[3],
                   float vfov_deg, float aspect_ratio, float aperture, float focus_dist, float time0, float time1) {
  if (!cam || !look_from || !look_at || !vup) return fail(PT_ERR_INVALID_ARG, "pt_camera_init: NULL argument");
  struct H3 { float x, y, z; };
  auto sub = [](H3 a, H3 b) { return H3{a.x - b.x, a.y - b.y, a.z - b.z}; };
  auto scale = [](float s, H3 a) { return H3{s * a.x, s * a.y, s * a.z}; };
  auto divs = [](H3 a, float s) { return H3{a.x / s, a.y / s, a.z / s}; };
  auto dot3 = [](H3 a, H3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; };
  auto cross3 = [](H3 a, H3 b) { return H3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; };
  auto unit = [&](H3 a) { return divs(a, std::sqrt(dot3(a, a))); };
  const float pi = 3.1415926535897932385f;
  H3 origin{look_from[0], look_from[1], look_from[2]}, at{look_at[0], look_at[1], look_at[2]}, up{vup[0], vup[1], vup[2]};
  float theta = vfov_deg * pi / 180.0f; // rtweekend.hpp:31
  float h = std::tan(theta / 2.0f);
  float viewport_height = 2.0f * h;
  float viewport_width = aspect_ratio * viewport_height;
  H3 w = unit(sub(origin, at));
  H3 u = unit(cross3(up, w));
  H3 v = cross3(w, u);
  H3 horizontal = scale(focus_dist * viewport_width, u);
  H3 vertical = scale(focus_dist * viewport_height, v);
  H3 llc = sub(sub(sub(origin, divs(horizontal, 2.0f)), divs(vertical, 2.0f)), scale(focus_dist, w));
  auto st = [](float* d, H3 a) { d[0] = a.x; d[1] = a.y; d[2] = a.z; };
  st(cam->origin, origin); st(cam->lower_left_corner, llc); st(cam->horizontal, horizontal); st(cam->vertical, vertical);
  st(cam->u, u); st(cam->v, v); st(cam->w, w);
  cam->lens_radius = aperture / 2.0f;
  cam->time0 = time0;
  cam->time1 = time1;
  return PT_OK;
}

// Host-only view of the flattening (no GPU needed): blob_out/mats_out may be NULL to query sizes.
void pt_tuning_init(PtTuning* t) { if (t) tuning_defaults(*t); }
void pt_tuning_from_env(PtTuning* t) { if (t) tuning_env(*t); }

int pt_debug_flatten(const PtSceneDesc* desc, float* blob_out, int64_t blob_cap_f4, int32_t* n_blob_f4,
                     int32_t* n_runs, float* mats_out, int64_t mats_cap_f4, int32_t* flags_out) {
  return pt_debug_flatten_tuned(desc, nullptr, blob_out, blob_cap_f4, n_blob_f4, n_runs, mats_out, mats_cap_f4, flags_out);
}

int pt_debug_flatten_tuned(const PtSceneDesc* desc, const PtTuning* tuning, float* blob_out, int64_t blob_cap_f4, int32_t* n_blob_f4,
                           int32_t* n_runs, float* mats_out, int64_t mats_cap_f4, int32_t* flags_out) {
  ptf::Flat flat;
  std::string err;
  PtTuning t;
  int rc = resolve_tuning(tuning, t, err);
  if (rc) return fail(rc, err);
  rc = flatten_tuned(desc, t, flat, err); // the blob pt_scene_create would upload, knobs and LDS budget included
  if (rc) return fail(rc, err);
  if (n_blob_f4) *n_blob_f4 = (int32_t)flat.blob.size();
  if (n_runs) *n_runs = flat.n_runs;
  if (flags_out) *flags_out = (flat.has_image ? 1 : 0) | (flat.has_medium ? 2 : 0) | (flat.tri_pooled ? 4 : 0);
  if (blob_out) {
    if (blob_cap_f4 < (int64_t)flat.blob.size()) return fail(PT_ERR_INVALID_ARG, "blob buffer too small");
    if (!flat.blob.empty()) std::memcpy(blob_out, flat.blob.data(), flat.blob.size() * 16);
  }
  if (mats_out) {
    if (mats_cap_f4 < (int64_t)flat.mats.size()) return fail(PT_ERR_INVALID_ARG, "material buffer too small");
    if (!flat.mats.empty()) std::memcpy(mats_out, flat.mats.data(), flat.mats.size() * 16);
  }
  return PT_OK;
}

int pt_debug_shade_table(const PtSceneDesc* desc, const PtTuning* tuning, float* table_out, int64_t table_cap_f4, int32_t* n_f4, int32_t* base) {
  ptf::Flat flat;
  std::string err;
  PtTuning t;
  int rc = resolve_tuning(tuning, t, err);
  if (rc) return fail(rc, err);
  rc = flatten_tuned(desc, t, flat, err);
  if (rc) return fail(rc, err);
  if (n_f4) *n_f4 = (int32_t)flat.shade.size();
  if (base) *base = flat.shade_base;
  if (table_out) {
    if (table_cap_f4 < (int64_t)flat.shade.size()) return fail(PT_ERR_INVALID_ARG, "shade table buffer too small");
    if (!flat.shade.empty()) std::memcpy(table_out, flat.shade.data(), flat.shade.size() * 16);
  }
  return PT_OK;
}

int pt_debug_flatten_pool(const PtSceneDesc* desc, const PtTuning* tuning, float* pool_out, int64_t pool_cap_f4, int64_t* n_pool_f4) {
  ptf::Flat flat;
  std::string err;
  PtTuning t;
  int rc = resolve_tuning(tuning, t, err);
  if (rc) return fail(rc, err);
  rc = flatten_tuned(desc, t, flat, err);
  if (rc) return fail(rc, err);
  if (n_pool_f4) *n_pool_f4 = (int64_t)flat.pool.size_f4;
  if (pool_out) {
    if (pool_cap_f4 < (int64_t)flat.pool.size_f4) return fail(PT_ERR_INVALID_ARG, "pool buffer too small");
    flat.pool.assemble((ptf::F4*)pool_out);
  }
  return PT_OK;
}

int pt_debug_tri_pool(const PtSceneDesc* desc, int32_t out[8]) {
  if (!out) return fail(PT_ERR_INVALID_ARG, "pt_debug_tri_pool: NULL argument");
  ptf::Flat flat;
  std::string err;
  PtTuning t;
  tuning_env(t);
  int rc = flatten_tuned(desc, t, flat, err);
  if (rc) return fail(rc, err);
  out[0] = flat.tri_pooled; out[1] = flat.tri_wide;
  out[2] = (int32_t)(flat.tri_map_entries[0] >> 10); out[3] = (int32_t)((flat.tri_map_entries[1] + flat.tri_map_entries[2]) >> 10);
  out[4] = (flat.tri_map_res[0] << 20) | (flat.tri_map_res[1] << 10) | flat.tri_map_res[2];
  out[5] = (int32_t)(1000.0 * flat.tri_cells_per_triangle); out[6] = (int32_t)flat.blob.size(); out[7] = flat.grid_spheres;
  return PT_OK;
}

int pt_scene_create(const PtSceneDesc* desc, PtScene** out_scene) { return pt_scene_create_tuned(desc, nullptr, out_scene); }

int pt_scene_create_tuned(const PtSceneDesc* desc, const PtTuning* tuning, PtScene** out_scene) {
  if (!out_scene) return fail(PT_ERR_INVALID_ARG, "pt_scene_create: out_scene is NULL");
  *out_scene = nullptr;
  ptf::Flat flat;
  std::string err;
  PtTuning tun;
  int rc = resolve_tuning(tuning, tun, err);
  if (rc) return fail(rc, err);
  const bool timing = std::getenv("PT_TRI_TIMING") != nullptr; // (diagnostics: stage times on stderr, like build_tri_pool's)
  auto t_prev = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!timing) return;
    const auto t = std::chrono::steady_clock::now();
    std::fprintf(stderr, "pt_scene_create: %-27s %.3f s\n", what, std::chrono::duration<double>(t - t_prev).count());
    t_prev = t;
  };
  rc = flatten_tuned(desc, tun, flat, err);
  if (rc) return fail(rc, err);
  lap("flatten (+ culling tables)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PT_ERR_NO_DEVICE, "no HIP device visible");
  std::unique_ptr<PtScene> owner(new PtScene()); // (an early return frees what was allocated so far: every buffer is a DevBuf)
  PtScene* const s = owner.get();
  PT_HIP(hipGetDevice(&s->device));
  {
    hipDeviceProp_t prop;
    PT_HIP(hipGetDeviceProperties(&prop, s->device));
    s->num_cus = prop.multiProcessorCount;
    s->lds_per_block = prop.sharedMemPerBlock;
  }
  set_scene_facts(s, desc, tun, flat);
  // The binned renderer serves scenes with ONE pooled run whose stale u, v need no tracking (pt_binned.hpp); PtTuning.tri_binned = 1 (measured: it does not pay yet — docs/EXPERIMENTS.md — so it is opt-in).
  if (s->tri_pooled > 0 && flat.tri_pool_runs == 1 && !s->track_uv && tun.tri_binned > 0) {
    s->binned = true;
    s->bin_run = flat.tri_pool_run; s->bin_hdr = flat.tri_pool_hdr; s->bin_goff = flat.tri_pool_goff;
    s->bin_full_slices = std::min(64, std::max(1, (flat.tri_pool_count + 2047) / 2048));
    long long keys = 2; // ... + "every band record" + "every triangle, exactly" (pt_device.hpp: tri_pool_scan<true>)
    for (int k = 0; k < flat.tri_maps && k < 3; k++) keys += 3ll * flat.tri_map_res[k] * flat.tri_map_res[k];
    s->bin_keys = (int)keys;
    s->bin_base1 = flat.tri_maps > 0 ? 3 * flat.tri_map_res[0] * flat.tri_map_res[0] : 0;
  }
  // one buffer: [blob records][material table][shade table] so a kernel can stage all of it with one contiguous copy
  const size_t blob_bytes = flat.blob.size() * 16, mats_bytes = flat.mats.size() * 16;
  PT_HIP(s->blob.alloc(flat.blob.size() + flat.mats.size() + flat.shade.size()));
  s->mats = s->blob.p + flat.blob.size();
  if (blob_bytes) PT_HIP(hipMemcpy(s->blob.p, flat.blob.data(), blob_bytes, hipMemcpyHostToDevice));
  if (mats_bytes) PT_HIP(hipMemcpy(s->mats, flat.mats.data(), mats_bytes, hipMemcpyHostToDevice));
  if (!flat.shade.empty()) PT_HIP(hipMemcpy(s->mats + flat.mats.size(), flat.shade.data(), flat.shade.size() * 16, hipMemcpyHostToDevice));
  if (flat.pool.size_f4) { // the triangle pools' tables: zeroed (spare records between the tables), then table by table from where the builder left them
    s->pool_bytes = (size_t)flat.pool.size_f4 * 16;
    PT_HIP(s->pool.alloc((size_t)flat.pool.size_f4));
    PT_HIP(hipMemset(s->pool.p, 0, s->pool_bytes));
    if (timing) { (void)hipDeviceSynchronize(); lap("blob upload, pool malloc + memset"); }
    // (the big tables — hundreds of megabytes of direction-map lists — are pinned in place for their copy: a pageable hipMemcpy
    // staged them at ~3 GB/s, a third of the scene's build time in round 6)
    for (const ptf::PoolSegment& sg : flat.pool.segments) {
      if (sg.dwords.empty()) continue;
      const size_t bytes = sg.dwords.size() * 4;
      const bool pin = bytes >= (8u << 20) && hipHostRegister((void*)sg.dwords.data(), bytes, hipHostRegisterDefault) == hipSuccess;
      const hipError_t e = hipMemcpy(s->pool.p + sg.at_f4, sg.dwords.data(), bytes, hipMemcpyHostToDevice);
      if (pin) (void)hipHostUnregister((void*)sg.dwords.data());
      if (e != hipSuccess) return fail(PT_ERR_HIP, std::string("hipMemcpy of a pool table: ") + hipGetErrorString(e));
    }
  }
  lap("upload blob + pool");
  size_t atlas_bytes = flat.has_image ? (size_t)desc->atlas_bytes : 0;
  s->atlas_bytes = atlas_bytes;
  PT_HIP(s->atlas.alloc(std::max<size_t>(atlas_bytes, 16)));
  if (atlas_bytes) PT_HIP(hipMemcpy(s->atlas.p, desc->atlas, atlas_bytes, hipMemcpyHostToDevice));
  PT_HIP(s->queues.alloc(2 * kQueueRing));
  PT_HIP(s->ws_nsplit.alloc(2)); // [0] tiles through the wide phase, [1] log2 of its group size
  *out_scene = owner.release();
  return PT_OK;
}

int64_t pt_scene_device_bytes(const PtScene* s) {
  if (!s) return -1;
  return (int64_t)s->blob_bytes + ((int64_t)s->mats_f4 + s->shade_f4) * 16 + (int64_t)s->pool_bytes + (int64_t)s->atlas_bytes;
}

#ifndef PT_BUILD_ID
#define PT_BUILD_ID "unknown"
#endif
const char* pt_build_id(void) { return PT_BUILD_ID; }

void pt_scene_destroy(PtScene* s) {
  if (!s) return;
  for (hipEvent_t e : s->ring_done) if (e) (void)hipEventDestroy(e);
  delete s; // (its buffers: DevBuf members)
}

// the shard of a frame's parameters: what check_params and check_aov_params ask after their own conditions on the sizes
static int check_shard(const PtRenderParams* p) {
  if (p->shard_count < 1 || p->shard_index < 0 || p->shard_index >= p->shard_count)
    return fail(PT_ERR_INVALID_ARG, "need 0 <= shard_index < shard_count");
  return PT_OK;
}
static int check_params(const PtRenderParams* p) {
  if (!p) return fail(PT_ERR_INVALID_ARG, "render params are NULL");
  if (p->width <= 0 || p->height <= 0 || p->samples <= 0 || p->depth < 0)
    return fail(PT_ERR_INVALID_ARG, "width, height, samples must be > 0 and depth >= 0");
  return check_shard(p);
}

static int n_tiles_of(const PtRenderParams* p, int* tiles_x) {
  int tx = (p->width + PT_TILE - 1) / PT_TILE, ty = (p->height + PT_TILE - 1) / PT_TILE;
  if (tiles_x) *tiles_x = tx;
  return tx * ty;
}
// the tiles of a shard's compact buffer: the same for every shard of a frame (the last ones' final tile may be padding)
static int tiles_per_shard(int n_tiles, int shard_count) { return (n_tiles + shard_count - 1) / shard_count; }
// the tiles shard p->shard_index owns: tile t belongs to shard t % shard_count
static int local_tiles_of(const PtRenderParams* p) { return (n_tiles_of(p, nullptr) - p->shard_index + p->shard_count - 1) / p->shard_count; }
// PT_FLAG_FAST_RNG: the chunks a pixel's samples are rendered in
static int fast_chunks_of(int samples) { return (samples + PT_FAST_CHUNK_SPP - 1) / PT_FAST_CHUNK_SPP; }
// Scattered queues (lane_acquire: scatter_p) deal positions to the nt tiles with a stride: the smallest P >= max(1, nt / per_wave) coprime to nt
static unsigned int scatter_stride(unsigned int nt, unsigned int per_wave) {
  unsigned int P = nt / per_wave > 1 ? nt / per_wave : 1;
  while (std::gcd(P, nt) != 1) ++P;
  return P;
}

uint32_t pt_fast_seed(uint32_t pixel, uint32_t chunk) { return fast_seed(pixel, chunk); }

int32_t pt_shard_tiles(const PtRenderParams* p) {
  if (check_params(p)) return -1;
  return tiles_per_shard(n_tiles_of(p, nullptr), p->shard_count);
}

int64_t pt_framebuffer_floats(const PtRenderParams* p) {
  if (check_params(p)) return -1;
  if (p->shard_count == 1) return (int64_t)p->width * p->height * 3;
  return (int64_t)pt_shard_tiles(p) * PT_TILE_PIXELS * 3;
}

// grow-only per-scene workspaces (LPT cost / order arrays; fast mode's partial sums).  pt_scene_reserve() sizes them ahead of
// time so that pt_render() neither allocates nor frees (hipMalloc / hipFree synchronise the device).
static int reserve_tiles(const PtScene* s, int local_tiles) {
  const size_t t = (size_t)local_tiles;
  PT_HIP(s->ws_cost.grow(t));
  PT_HIP(s->ws_order.grow(t));
  PT_HIP(s->ws_rng.grow(t * PT_TILE_PIXELS));
  PT_HIP(s->ws_rank.grow(t));
  return PT_OK;
}
// the camera rays' candidate cache of the triangle-pool kernels: one PT_TRI_CACHE_WORDS line per lane of the launch (grow-only)
static int grow_tricache(const PtScene* s, size_t lanes) {
  PT_HIP(s->ws_tricache.grow(lanes * PT_TRI_CACHE_WORDS));
  return PT_OK;
}
static int reserve_partial(const PtScene* s, size_t floats) {
  PT_HIP(s->ws_partial.grow(floats));
  return PT_OK;
}

// The binned triangle-pool renderer (pt_binned.hpp): generations of { step, sort the requests by direction bin, band stage }, until no pixel
// is live.  How many generations a frame takes is known only on the device (the heaviest pixel's ray count), so the host reads the live
// count back every few generations: unlike the persistent kernels' launches this render has returned only when the frame is done.
static int reserve_binned(const PtScene* s, size_t n_pixels, size_t n_keys, size_t& bytes_out);
static int launch_binned(const PtScene* s, KArgs a, const PtRenderParams* p, int local_tiles, hipStream_t st) {
  if (p->depth <= 0) return PT_OK; // every sample black (render.hpp:58,91): the frame is pre-zeroed
  a.n_local_pixels = local_tiles * PT_TILE_PIXELS;
  a.tile_granular = 1; a.samples_total = p->samples; // (everything else of the persistent kernels' scheduling: off, as a KArgs starts)
  const size_t N = (size_t)a.n_local_pixels, K = (size_t)s->bin_keys;
  size_t bytes = 0;
  if (int rc = reserve_binned(s, N, K, bytes)) return rc;
  // carve the workspace (every array 256-byte aligned)
  char* base = s->ws_bin.p;
  size_t at = 0;
  auto take = [&](size_t n) { char* q = base + at; at += (n + 255) & ~(size_t)255; return q; };
  const size_t n_blocks = (K + 1023) / 1024, max_packets = (N / 64 + 1) * (size_t)s->bin_full_slices + std::min(K, N) + 1;
  BinArgs ba;
  ba.k = a;
  ba.A0 = (f4*)take(N * 16); ba.A1 = (f4*)take(N * 16); ba.A2 = (f4*)take(N * 16); ba.A3 = (f4*)take(N * 16);
  ba.A4 = (int4*)take(N * 16); ba.A5 = (f4*)take(N * 16);
  ba.slot = (unsigned long long*)take(N * 8);
  SortArgs sa;
  sa.hist = (unsigned int*)take(K * 4);
  sa.offs = (unsigned int*)take((K + 1) * 4);
  sa.block_tot = (uint2*)take(n_blocks * 8);
  sa.packets = (int2*)take(max_packets * 8);
  sa.ctl = (unsigned int*)take(64);
  unsigned int* sorted = (unsigned int*)take(N * 4);
  unsigned int* live_list[2] = {(unsigned int*)take(N * 4), (unsigned int*)take(N * 4)};
  sa.n_keys = (int)K; sa.n_blocks = (int)n_blocks; sa.full_slices = s->bin_full_slices;
  ba.hist = sa.hist; ba.ctl = sa.ctl; ba.pool_run = s->bin_run;
  ba.scatter_p = s->knobs.no_scatter ? 0 : (int)scatter_stride((unsigned int)local_tiles, 64);
  ba.dbg_base1 = s->bin_base1;
  BandArgs bd;
  bd.pool = s->pool.p; bd.blob = s->blob.p; bd.hdr = s->bin_hdr; bd.goff = s->bin_goff;
  bd.A0 = ba.A0; bd.A1 = ba.A1; bd.A5 = ba.A5; bd.slot = ba.slot; bd.offs = sa.offs; bd.packets = sa.packets; bd.ctl = sa.ctl; bd.sorted = sorted;
  bd.dense_min = 16; bd.full_slices = s->bin_full_slices;
  if (const char* e = std::getenv("PT_BAND_DENSE_MIN")) bd.dense_min = std::max(1, std::atoi(e)); // (experiments only)
  PT_HIP(hipMemsetAsync(sa.hist, 0, K * 4, st));
  PT_HIP(hipMemsetAsync(sa.ctl, 0, 64, st));
  const dim3 step_grid((unsigned int)((N + kBlock - 1) / kBlock)), step_block(kBlock);
  const int band_blocks = std::max(1, s->num_cus) * 6;
  // (a scene with an image texture has a material that is not "simple" — mats_simple wants solid textures only — so UV_WINNER comes with MATS_ALL alone)
  const BinKernels bk = s->has_image ? bin_kernels<UV_WINNER, MATS_ALL>
                                     : (s->mats_simple ? bin_kernels<UV_NONE, MATS_LAMB_LIGHT_SOLID> : bin_kernels<UV_NONE, MATS_ALL>);
  auto step = [&](int gen) -> int {
    ba.gen = gen;
    ba.live_in = live_list[gen & 1]; ba.live_out = live_list[(gen + 1) & 1];
    hipLaunchKernelGGL(bk.step, step_grid, step_block, 0, st, ba);
    PT_HIP(hipGetLastError());
    hipLaunchKernelGGL(bin_count_kernel, dim3((unsigned int)n_blocks), dim3(1024), 0, st, sa);
    hipLaunchKernelGGL(bin_prefix_kernel, dim3(1), dim3(64), 0, st, sa);
    hipLaunchKernelGGL(bin_offsets_kernel, dim3((unsigned int)n_blocks), dim3(1024), 0, st, sa);
    hipLaunchKernelGGL(bin_scatter_kernel, dim3((unsigned int)((N + 255) / 256)), dim3(256), 0, st, ba.A4, ba.A5, sa.offs, sorted, ba.live_out, sa.ctl);
    hipLaunchKernelGGL(band_kernel, dim3((unsigned int)band_blocks), dim3(64 * kBandWaves), 0, st, bd);
    PT_HIP(hipGetLastError());
    return PT_OK;
  };
  // Generations while they pay: the host reads the live count back every 8 generations (the first time after min(samples, 8)) and, once
  // fewer than `tail_frac` of the pixels are live, hands them to bin_finish_kernel.
  int gen = 0;
  unsigned int live = (unsigned int)N;
  const long long max_gen = (long long)p->samples * std::max(1, p->depth) + 2;
  double tail_frac = 0.25;
  if (const char* e = std::getenv("PT_BIN_TAIL")) tail_frac = std::atof(e); // (experiments only; 0: generations to the end)
  const unsigned int tail_at = (unsigned int)(tail_frac * (double)N);
  while (live != 0 && live >= tail_at && gen <= max_gen) {
    const int until = gen + 8;
    for (; gen < until; gen++) if (int rc = step(gen)) return rc;
    PT_HIP(hipMemcpyAsync(&live, sa.ctl + 3, sizeof live, hipMemcpyDeviceToHost, st));
    PT_HIP(hipStreamSynchronize(st));
  }
  if (live != 0 && gen <= max_gen) { // the tail: persistent waves finish what is left (ctl[3] live pixels in the list the last step wrote)
    ba.gen = gen; ba.live_in = live_list[gen & 1]; ba.live_out = live_list[(gen + 1) & 1];
    PT_HIP(hipMemsetAsync(sa.ctl + 5, 0, 4, st));
    const int per_cu = occupancy_of(s, (const void*)bk.finish, kBlock, 0);
    if (per_cu < 0) return PT_ERR_HIP;
    const unsigned int blocks = (unsigned int)std::min<long long>((long long)std::max(1, per_cu) * std::max(1, s->num_cus), ((long long)live + kBlock - 1) / kBlock * 64);
    const dim3 fgrid(std::max(1u, blocks)), fblock(kBlock);
    hipLaunchKernelGGL(bk.finish, fgrid, fblock, 0, st, ba);
    PT_HIP(hipGetLastError());
    live = 0;
  }
  s->last_generations = gen;
  s->last_kernels[1] = bk.tag;
  s->last_launch[0] = (int)step_grid.x; s->last_launch[1] = 64; s->last_launch[2] = 0; s->last_launch[3] = 0;
  if (live != 0) return fail(PT_ERR_HIP, "pt_render: the binned renderer did not finish within samples x depth generations");
  return PT_OK;
}

static int reserve_binned(const PtScene* s, size_t N, size_t K, size_t& bytes) {
  const size_t n_blocks = (K + 1023) / 1024, max_packets = (N / 64 + 1) * (size_t)s->bin_full_slices + std::min(K, N) + 1;
  auto r = [](size_t n) { return (n + 255) & ~(size_t)255; };
  bytes = 6 * r(N * 16) + r(N * 8) + r(K * 4) + r((K + 1) * 4) + r(n_blocks * 8) + r(max_packets * 8) + r(64) + 3 * r(N * 4);
  PT_HIP(s->ws_bin.grow(bytes)); // (grow-only: the bytes grow with N, the rest is the scene's)
  return PT_OK;
}

} // extern "C"

namespace {

// ---- one pass of launch_render: its launch geometry (plan_pass), its enqueue (enqueue_pass) ---------------------------------------

// What plan_pass decides from: plain values, no pointer into the scene (pt_debug_plan_pass feeds it the same way without a device).
struct PassFacts {
  int num_cus = 0;         // PtScene.num_cus
  int per_cu = 0;          // the kernel's resident workgroups per CU as queried (occupancy_of): >= 1
  int block_threads = kBlock;
  bool chain_bound = false, use_grid = false, queued_walk = false; // the pass's Variant (a fast-mode pass after a probe: or the probe's)
  uint32_t flags = 0;      // PtRenderParams.flags
  int blocks_per_cu = 0, lanes_cap = 0, heavy_tiles = 0; // Knobs of the same names
  bool no_chain_prio = false;
  long long launch_units = 0; // waves worth of work in the queue (tiles; fast mode: tiles x chunks)
  int n_local_pixels = 0;  // KArgs.n_local_pixels
  int samples = 0;         // PtRenderParams.samples (a window's length)
  bool probe = false;      // the cost-probe pass (KArgs.cost)
  bool has_order = false;  // a tile order exists (KArgs.order)
  bool has_split = false;  // a wide phase exists (KArgs.n_split)
  int tile_granular = 0, scatter_p = 0, fast_chunks = 0; // KArgs of the same names, as the pass sequence set them
};

// What it decides: the launch's size and the KArgs members that follow from it (enqueue_pass writes them into the pass's KArgs).
struct PassPlan {
  int workgroups = 1;
  int n_waves_resident = 1; // the waves of the launch (lpt_order_kernel's makespan model takes the probe pass's)
  int lanes_cap = 64, tile_granular = 0;
  int heavy_pixels = 0, heavy_lanes = 64;
  int prio_onset = 0, prio_t1 = 0, prio_t2 = 0, prio_t3 = 0;
  int last_launch[4] = {0, 0, 0, 0}; // PtScene.last_launch of a frame pass (pt_debug_last_launch)
};

// Persistent grid: no more workgroups than the chip holds at once; lanes pull pixels from the queue.
PassPlan plan_pass(const PassFacts& f) {
  PassPlan pl;
  const int block_threads = f.block_threads;
  const int waves_per_block = block_threads / 64;
  int per_cu = f.per_cu;
  // (small frames through the grid kernels: below; PT_FLAG_TILE_GRANULAR / PT_FLAG_PIXEL_GRANULAR and the fast mode keep what they ask for)
  // (only the kernels that walk a sphere grid: the headline family's iteration — slab pass, wave-uniform — does not get shorter with fewer
  // lanes: its shard 0/8 took 127 ms that way against 40)
  const bool share_small = f.use_grid && f.lanes_cap >= 0 && !(f.flags & (PT_FLAG_TILE_GRANULAR | PT_FLAG_PIXEL_GRANULAR | PT_FLAG_FAST_RNG));
  // A headline-family launch with fewer than ~1.15 tiles per wave slot (shard 0 of 4 ... 6 of the 1080p frame) is bound by its heaviest
  // tiles' sequential chains, and a chain's iteration takes as long as the waves that share its SIMD make it: four waves per SIMD that
  // take two tiles each, heaviest first, finish before eight that take one.  Cornell-style 1080p x 1024 spp, kernel ms of shard 0 of
  // N = 3 / 4 / 6 at 8 and at 4 workgroups per CU: 63.3 / 57.8 / 43.4 and 60.3 / 51.1 / 42.8 (profiles/r04_blocks_sweep.txt); whole frames
  // and halves (>= 2 tiles per slot) keep the full occupancy, and a launch with half a tile per slot takes four per CU by itself.
  // (Grid and triangle-pool kernels: their own occupancy is the best at every shard count — same file.)
  // (Round 5, with the chain priorities of render_kernel: shard 0 of 3 — 1.3 tiles per slot — 61.2 ms at four workgroups per CU, 54.4 / 57.1 at
  // six / eight; shard 0 of 4 — 1.0 — 45.2 / 47.3 / 48.7: the bound moved from 1.6 to 1.15; profiles/r05_ab_chain_priority.txt.)
  if (f.chain_bound && !f.blocks_per_cu && !f.has_split && f.scatter_p == 0 &&
      (double)f.launch_units < 1.15 * (double)per_cu * waves_per_block * std::max(1, f.num_cus))
    per_cu = std::min(per_cu, 4);
  if (f.blocks_per_cu) per_cu = std::min(per_cu, f.blocks_per_cu); // tuning knob
  // longest remaining chain first (render_kernel): the headline family's frame launches in parity mode, from the middle of the queue on
  if (f.chain_bound && !f.probe && !f.fast_chunks && f.tile_granular && !f.no_chain_prio && f.samples >= 16) {
    pl.prio_onset = f.n_local_pixels / 2;
    pl.prio_t3 = f.samples / 2; pl.prio_t2 = f.samples / 4; pl.prio_t1 = f.samples / 8;
  }
  const int resident_blocks = std::max(1, per_cu) * std::max(1, f.num_cus);
  // one wave per tile is enough, except in the wide phase, where a split tile keeps G waves busy (how many tiles are
  // split is decided on the device, so such a launch simply fills the chip; surplus waves find the queues empty and exit)
  long long wanted = f.has_split ? (long long)resident_blocks : (f.launch_units + waves_per_block - 1) / waves_per_block;
  pl.lanes_cap = 64;
  pl.tile_granular = f.tile_granular;
  // Frames (or shards) that do not fill the chip several times over are bound by their pixels' sequential chains, not by throughput —
  // BASELINE config 1 is 1 406 tiles for 4 096 resident waves, a shard of an 8-GPU job about one tile per wave — and a wave that steps
  // 64 pixels together pays, every iteration, for the LONGEST walk, the largest candidate count and every material among them.  Such a
  // launch fills the chip and gives each wave only `lanes_cap` lanes' worth of pixels at a time (one pixel per lane, refilled from the
  // queue: consecutive positions = neighbouring pixels of one tile row, so the walks stay coherent): fewer lanes per wave = a shorter
  // iteration for the pixels that set the frame time.  Measured on one box (profiles/r04_ab_lanes_cap.txt; rho = pixels per resident
  // lane): config 1 (rho 0.34) 24.5 ms at 64 lanes, 22.0 at 24, 19.2 at 8, 17.9 at 4; shard 0/8 of the 1080p frame (rho 1.0) 70.9 / 61.6 /
  // 60.1 / 76.4 ms at 64 / 32 / 16 / 8; shard 0/8 of the 4K frame (rho 4.0) 201.7 / 209.8 / 218.1 at 64 / 48 / 32: lanes = 16 rho fits all
  // three (rounded to the nearest multiple of 4).  Which lane renders a pixel changes nothing in the image (a pixel's seed is its id).
  if (share_small && f.scatter_p == 0) {
    const long long lanes = (long long)resident_blocks * waves_per_block * 64;
    long long cap = (16 * (long long)f.n_local_pixels + lanes / 2) / lanes; // 16 rho
    cap = std::min<long long>(64, std::max<long long>(4, (cap + 2) / 4 * 4)); // (the nearest multiple of 4: half a tile row)
    if (cap > 24) cap = 64; // (rho 2: 93.9 ms at 32 lanes against 90.9 at 64 — from there on the frame is throughput)
    if (f.lanes_cap > 0) cap = std::min(64, f.lanes_cap); // PtTuning.lanes_cap: forced
    if (cap < 64) {
      pl.lanes_cap = (int)cap;
      pl.tile_granular = 0;
      wanted = std::min<long long>(resident_blocks, ((long long)f.n_local_pixels + cap * waves_per_block - 1) / (cap * waves_per_block));
      wanted = std::max<long long>(wanted, 1);
    }
  }
  // Between the launches that the rule above serves (fewer than 1.5 pixels per resident lane) and the ones that are throughput (6 and
  // more) lie the shards of a multi-GPU job on a big frame — one of 8 GPUs on the 4K frame: 4 pixels per lane — whose time is their
  // heaviest tiles' chains: whole tiles everywhere, except that the head of the cost-sorted queue (one tile per SIMD of the chip) is handed
  // out 16 pixels at a time (lane_acquire: heavy_pixels).  Kernel ms of shard 0 of N, whole tiles / with the narrow head — 4K x 512 spp
  // N = 8 / 6 / 5 / 4: 196.8 / 203.9 / 220.4 / 209.1 -> 162.7 / 169.1 / 217.2 / 208.8; 1080p x 512 spp N = 2 / 3 / 4: 189.3 / 189.2 / 176.2 ->
  // 165.4 / 159.2 / 155.3; whole frames lose (1080p: 382 -> 435 ms), hence the upper bound (profiles/r04_heavy_tiles.txt).
  // Needs the cost-sorted order (the probe pass ran) — and changes nothing in the image: a pixel's seed is its id.
  if (share_small && pl.lanes_cap == 64 && pl.tile_granular && f.has_order && f.scatter_p == 0 && !f.probe && f.heavy_tiles >= 0) {
    const double lanes = (double)resident_blocks * waves_per_block * 64.0, rho = (double)f.n_local_pixels / lanes;
    long long tiles = f.heavy_tiles > 0 ? f.heavy_tiles : (rho >= 1.5 && rho < 6.0 ? 4LL * std::max(1, f.num_cus) : 0);
    tiles = std::min<long long>(tiles, f.n_local_pixels / 64 / 2);
    if (tiles > 0) { pl.heavy_pixels = (int)(tiles * 64); pl.heavy_lanes = 16; }
  }
  if (f.scatter_p > 0) { // triangle-pool kernels: fill the chip and share the pixels out evenly (lane_acquire)
    wanted = std::min<long long>(resident_blocks, ((long long)f.n_local_pixels + block_threads - 1) / block_threads * 64); // (at least one pixel per wave)
    wanted = std::max<long long>(wanted, 1);
    const long long waves = std::min<long long>(wanted, resident_blocks) * waves_per_block;
    pl.lanes_cap = (int)std::min<long long>(64, std::max<long long>(1, ((long long)f.n_local_pixels + waves - 1) / waves));
  }
  pl.workgroups = (int)std::min<long long>(wanted, resident_blocks);
  pl.n_waves_resident = (int)std::min<long long>(wanted, resident_blocks) * waves_per_block;
  pl.last_launch[0] = pl.workgroups; pl.last_launch[1] = pl.lanes_cap; pl.last_launch[2] = pl.heavy_pixels; pl.last_launch[3] = f.queued_walk ? 1 : 0;
  return pl;
}

// the footprint of a pixel in direction space (camera.hpp:93-100 with lens_radius 0: d = llc + s hor + t ver - origin, s in [x / W, (x + 1) / W]):
// KArgs.foot of the camera rays' candidate cache
void pixel_footprint(const Cam& cm, float inv_w, float inv_h, float foot[11]) {
  float base[3], hw[3], vh[3];
  double dmax = 0, lh = 0, lv = 0;
  for (int k = 0; k < 3; k++) {
    base[k] = cm.llc[k] - cm.origin[k]; hw[k] = cm.horizontal[k] * inv_w; vh[k] = cm.vertical[k] * inv_h;
    foot[k] = base[k]; foot[3 + k] = hw[k]; foot[6 + k] = vh[k];
    lh += (double)hw[k] * hw[k]; lv += (double)vh[k] * vh[k];
    dmax += std::fabs((double)cm.llc[k]) + std::fabs((double)cm.origin[k]) + std::fabs((double)cm.horizontal[k]) + std::fabs((double)cm.vertical[k]);
  }
  lh = std::sqrt(lh); lv = std::sqrt(lv);
  // half a pixel each way (the jitter may round to the pixel's far edge), + the binary32 rounding of the camera's own arithmetic and of the centre ray
  foot[9] = (float)((0.5 * (lh + lv)) * 1.001 + 1e-5 * dmax);
  // ... and that rounding term alone, per component (the cache's choice of bins: pt_device.hpp, tri_pool_scan)
  foot[10] = (float)(1e-5 * dmax);
}

// One pass onto the stream: kernel `v` over the pass's KArgs `a` (a copy: what the plan decided is written into it here), sized by `pl`.
int enqueue_pass(const PtScene* s, const PtRenderParams* p, const Variant& v, const PassPlan& pl, int block_threads, KArgs a, hipStream_t st) {
  a.lanes_cap = pl.lanes_cap; a.tile_granular = pl.tile_granular;
  a.heavy_pixels = pl.heavy_pixels; a.heavy_lanes = pl.heavy_lanes;
  a.prio_onset = pl.prio_onset; a.prio_t1 = pl.prio_t1; a.prio_t2 = pl.prio_t2; a.prio_t3 = pl.prio_t3;
  const dim3 grid((unsigned int)pl.workgroups), block((unsigned int)block_threads);
  // The camera rays' candidate cache (pt_device.hpp: TriPrimCtx): triangle-pool kernels, a pinhole camera (the rays of a pixel share
  // their origin), pixel coordinates that fit 16 bits.  One 1 KB line per lane of the launch; every line starts out belonging to no pixel.
  a.tri_cache = nullptr;
  // (sized ahead by pt_accum_create — reserve_tricache; grown here otherwise, BEFORE the queue slot below is taken, and a failed
  // allocation only costs the cache: the image does not depend on it)
  const size_t cache_lanes = (size_t)grid.x * block.x;
  if (v.tri_pool && a.cam.lens_radius == 0.0f && !s->knobs.no_tri_cache && p->width <= 65535 && p->height <= 65535 &&
      grow_tricache(s, cache_lanes) == PT_OK) {
    PT_HIP(hipMemsetAsync(s->ws_tricache.p, 0xff, cache_lanes * PT_TRI_CACHE_WORDS * 4, st));
    a.tri_cache = s->ws_tricache.p;
    pixel_footprint(a.cam, a.inv_w, a.inv_h, a.foot);
  }
  // Queue counters come from a ring of kQueueRing slots.  A slot is reused only after the launch that last used it has
  // finished (more than kQueueRing launches in flight on one scene would otherwise share a dequeue counter and lose or
  // duplicate pixels): the NEW launch's stream waits for that launch's event on the device — the host does not block, so
  // pt_render stays asynchronous however many renders are queued (round 3 synchronised the host here, with the scene's
  // scheduling mutex held).
  const unsigned int slot = s->next_queue % kQueueRing;
  if (s->ring_done[slot]) PT_HIP(hipStreamWaitEvent(st, s->ring_done[slot], 0));
  else PT_HIP(hipEventCreateWithFlags(&s->ring_done[slot], hipEventDisableTiming));
  s->next_queue++; // (only once nothing above can fail any more)
  a.queue = s->queues.p + 2 * slot; // [0] ordinary queue, [1] wide-phase queue
  PT_HIP(hipMemsetAsync(a.queue, 0, 2 * sizeof(unsigned int), st));
  hipLaunchKernelGGL(v.kernel, grid, block, v.shmem, st, a);
  PT_HIP(hipGetLastError());
  s->last_kernels[a.cost ? 0 : 1] = v.tag;
  PT_HIP(hipEventRecord(s->ring_done[slot], st));
  return PT_OK;
}

// One pass of launch_render: the kernel's occupancy, the plan, the enqueue.  chain_bound / queued_walk: the variant's own, or — a fast-mode
// pass after a probe — also what the probe pass of this call ran (the four-workgroup rule of plan_pass, pt_debug_last_launch).
int run_pass(const PtScene* s, const PtRenderParams* p, const Variant& v, bool chain_bound, bool queued_walk, long long launch_units,
             const KArgs& a, hipStream_t st, PassPlan* plan_out = nullptr) {
  PassFacts f;
  f.num_cus = s->num_cus;
  f.per_cu = occupancy_of(s, (const void*)v.kernel, f.block_threads, v.shmem);
  if (f.per_cu < 0) return PT_ERR_HIP;
  // (a kernel variant that does not fit a CU at all — its static + dynamic LDS beyond the device's limit — must not be launched and hoped for)
  if (f.per_cu < 1) return fail(PT_ERR_TOO_LARGE, "pt_render: this scene's kernel variant does not fit a compute unit (LDS " + std::to_string(v.shmem) + " B dynamic + static)");
  f.chain_bound = chain_bound; f.use_grid = v.use_grid; f.queued_walk = queued_walk;
  f.flags = p->flags;
  f.blocks_per_cu = s->knobs.blocks_per_cu; f.lanes_cap = s->knobs.lanes_cap; f.heavy_tiles = s->knobs.heavy_tiles; f.no_chain_prio = s->knobs.no_chain_prio;
  f.launch_units = launch_units; f.n_local_pixels = a.n_local_pixels; f.samples = p->samples;
  f.probe = a.cost != nullptr; f.has_order = a.order != nullptr; f.has_split = a.n_split != nullptr;
  f.tile_granular = a.tile_granular; f.scatter_p = a.scatter_p; f.fast_chunks = a.fast_chunks;
  const PassPlan pl = plan_pass(f);
  if (plan_out) *plan_out = pl;
  if (!f.probe) std::copy(pl.last_launch, pl.last_launch + 4, s->last_launch);
  return enqueue_pass(s, p, v, pl, f.block_threads, a, st);
}

// The frame block that KArgs and AovArgs share: the scene's tables, the camera, the frame's sizes and reciprocals, shard and tile counts
template <typename Args>
void set_frame(Args& a, const PtScene* s, const PtCamera* cam, const PtRenderParams* p) {
  std::memcpy(&a.cam, cam, sizeof(Cam));
  a.blob = s->blob.p; a.mats = s->mats; a.pool = s->pool.p; a.atlas = s->atlas.p;
  a.n_runs = s->n_runs;
  a.width = p->width; a.height = p->height; a.samples = p->samples;
  a.inv_w = 1.0f / (float)p->width; a.inv_h = 1.0f / (float)p->height; // host IEEE division: correctly rounded
  if constexpr (requires { a.width_f; }) { a.width_f = (float)p->width; a.height_f = (float)p->height; } // (KArgs: what v_cvt_f32_i32 gives, RNE)
  a.pinhole = cam_is_pinhole(a.cam) ? 1 : 0;
  a.shard_index = p->shard_index; a.shard_count = p->shard_count;
  a.n_tiles = n_tiles_of(p, &a.tiles_x);
}

// One sample window of a PtAccum (pt_render_accumulate): p->samples is the window's length, fb the accumulator's radiance sums.
struct Window {
  int done;          // samples the state already holds: the window renders [done, done + p->samples)
  unsigned int* rng; // per local pixel: the generator's state after `done` samples
  int* order;        // the accumulator's own heaviest-first tile order (and the cooperative kernels' split) ...
  int* nsplit;
  bool* has_order;   // ... valid once a window has probed
  // a masked window of an adaptive PtAccum (pt_adaptive_window): the per-pixel mask, and the n_active local tiles that hold one of its
  // pixels in dequeue order — the launch sees a frame of that many tiles; no probe, no wide phase, no scene scheduling workspace
  const uint8_t* mask = nullptr;
  const int* active = nullptr;
  int n_active = 0;
};

// (after a pass's n_local_pixels is final: fast mode multiplies it by the chunks per pixel)
void set_scatter(KArgs& a, int scatter_log) {
  a.scatter_log = scatter_log;
  a.scatter_p = (int)scatter_stride((unsigned int)a.n_local_pixels >> 6, 64u >> a.scatter_log /* tiles a wave's 64 pixels come from */);
}

// A render, a sample window or a masked window as a sequence of passes: the early exits (single stream, binned renderer), the optional
// cost probe with the tile order it leaves, then the frame pass — or, in the opt-in fast mode, the chunk pass and its reduction.  Every
// pass takes its KArgs from `base` by value; which kernel it runs is choose_variant's, how it is sized plan_pass's (through run_pass).
int launch_render(const PtScene* s, const PtCamera* cam, const PtRenderParams* p, float* fb, hipStream_t st, const Window* w = nullptr) {
  int cur = -1;
  PT_HIP(hipGetDevice(&cur));
  if (cur != s->device)
    return fail(PT_ERR_INVALID_ARG, "pt_render: the scene lives on device " + std::to_string(s->device) + " but the current device is " +
                                        std::to_string(cur) + " (hipSetDevice to the scene's device first)");
  std::lock_guard<std::mutex> lock(s->sched);
  s->last_kernels[0] = s->last_kernels[1] = KTag{}; // (a pass that does not run leaves family 0)
  s->last_pool_plan = PoolPlan{};
  KArgs base;
  set_frame(base, s, cam, p);
  base.fb = fb;
  base.blob_f4 = s->blob_f4; base.mats_f4 = s->mats_f4 + s->shade_f4 /* staged as one */;
  base.shade_k = s->shade_f4 > 0 ? s->blob_f4 + s->mats_f4 - s->shade_base : 0;
  base.n_hittables = s->n_hittables;
  base.depth = p->depth;
  const bool masked = w && w->mask;
  // tiles this shard owns (a masked window: the tiles it renders)
  const int local_tiles = masked ? w->n_active : local_tiles_of(p);
  if (masked) base.mask = w->mask;
  // pixels no lane owns (edge tiles, padded last tile, depth 0) read as 0 (a window's sums: zeroed by pt_accum_create / _reset)
  if (!w) PT_HIP(hipMemsetAsync(fb, 0, (size_t)pt_framebuffer_floats(p) * sizeof(float), st));
  if (local_tiles <= 0) return PT_OK;
  base.fast_ok = (s->fast_ok && !(p->flags & PT_FLAG_NO_FASTDIV)) ? 1 : 0;
  if (p->flags & PT_FLAG_SINGLE_STREAM) { // the reference's single-task executor: one sequential chain, one lane
    if (p->shard_count != 1) return fail(PT_ERR_INVALID_ARG, "PT_FLAG_SINGLE_STREAM needs shard_count == 1");
    if ((long long)p->width * p->height * p->samples > (1ll << 22))
      return fail(PT_ERR_TOO_LARGE, "PT_FLAG_SINGLE_STREAM is sequential by definition: width * height * samples <= 2^22");
    if (p->depth <= 0) return PT_OK;
    hipLaunchKernelGGL(render_single_stream_kernel, dim3(1), dim3(64), 0, st, base);
    PT_HIP(hipGetLastError());
    s->last_kernels[1].w[0] = KFAM_SINGLE;
    return PT_OK;
  }
  // (sample windows run the persistent kernels: both renderers give the reference's image, and only these resume a pixel)
  if (s->binned && !w && !(p->flags & (PT_FLAG_FORCE_STREAM | PT_FLAG_FAST_RNG))) return launch_binned(s, base, p, local_tiles, st);
  base.n_local_pixels = local_tiles * PT_TILE_PIXELS;
  // The parity-mode kernel variant: the probe pass and the frame pass run it (the fast mode chooses its frame launch's own, below)
  const Variant pv = choose_variant(s, p, local_tiles, false, base.n_local_pixels);
  if (pv.rc) return pv.rc;
  const bool tri_pool = pv.tri_pool, use_grid = pv.use_grid, coop = pv.coop; // (the same in every pass)
  base.coop_prefix = pv.coop_prefix;
  base.plan = pass_pool_plan(s, p, pv); // (the probe pass and the frame pass run pv's kernel; the fast mode's chunk pass sets its own)
  base.samples_total = p->samples;
  if (const char* e = std::getenv("PT_TILE_GROUP")) { const int g = std::atoi(e); if (g == 16 || g == 32) base.tile_group = g; } // (experiment)
  // default: whole tiles for the resident kernels (coherent primary rays), single pixels for the lock-step
  // streaming kernel (a workgroup waits for its slowest lane); either can be forced
  // (the triangle-pool kernels' iterations are long and per-lane: single pixels, like the streaming kernel)
  base.tile_granular = (p->flags & PT_FLAG_TILE_GRANULAR) ? 1 : (p->flags & PT_FLAG_PIXEL_GRANULAR) ? 0 : ((pv.resident && !tri_pool) ? 1 : 0);
  // the triangle-pool kernels' queues deal positions to the tiles with a stride (lane_acquire: scatter_p; set_scatter, per pass)
  const bool scattered = tri_pool && !base.tile_granular && !s->knobs.no_scatter;
  const bool window = w && !(p->flags & PT_FLAG_FAST_RNG); // a parity-mode sample window: resumes from / keeps the per-pixel state
  if (window) { base.samples = w->done + p->samples; base.resume_rng = w->rng; base.resume_spp = w->done; base.keep_state = 1; }

  // ---- the cost probe: heaviest-first tile order from a probe pass (see lpt_order_kernel); pointless for short renders ----
  int probe_spp = std::min(4, p->samples / 16);
  // Tiles are ordered by their ray count — or, where a wave holds a tile until its last pixel is done and pixels differ
  // widely (the sphere-field scenes the grid kernels run: a few glass / mirror pixels per tile), by 64 x their heaviest
  // pixel's, from a deeper probe: 496-hittable scene +3-6 % (same box), Cornell-style -0.8 % (kept on the sum).  (Round 5, with the
  // probe's samples kept: still samples / 64 up to 16 — 1080p x 1024 spp 448 / 409 / 395 / 375 ms at depths 2 / 4 / 8 / 16 and 379 / 387 /
  // 406 at 32 / 64 / 128: an unordered launch runs at half the ordered one's pace; profiles/r05_ab_probe_resume.txt.)
  const bool cost_by_max = s->knobs.lpt_max >= 0 ? s->knobs.lpt_max != 0 : use_grid;
  if (cost_by_max) probe_spp = std::min(std::max(probe_spp, p->samples / 64), s->knobs.probe_spp_max);
  // (the triangle-pool kernels deal every wave a stratified sample of the frame's tiles — lane_acquire, scatter_p — which balances the
  // waves without knowing the costs: the probe only costs there, 1080p x 32 spp 3.12 -> 2.95 s without it; PT_LPT_SCATTER=1 keeps it)
  const bool probe_pays = !scattered || s->knobs.lpt_with_scatter;
  bool probed = false; // the probe pass ran
  KArgs frame = base;  // the frame pass (fast mode: the chunk pass): `base` + the tile order and the probe's samples, where there are any
  if (masked) {
    frame.order = w->active; // (n_split stays NULL: no wide phase)
  } else if (probe_spp >= 1 && local_tiles >= 64 && !(p->flags & PT_FLAG_NO_LPT) && probe_pays) {
    if (int rc = reserve_tiles(s, local_tiles)) return rc; // first render at a new size only (or never: pt_scene_reserve)
    PT_HIP(hipMemsetAsync(s->ws_cost.p, 0, (size_t)local_tiles * sizeof(unsigned int), st));
    KArgs probe = base;
    if (scattered) set_scatter(probe, s->knobs.scatter_log);
    probe.cost = s->ws_cost.p;
    probe.cost_max = (cost_by_max && !coop) ? 1 : 0;
    probe.samples = probe_spp;
    probe.keep_state = 0;
    // the probe's samples are kept (KArgs.resume_rng) — not in the opt-in fast mode, whose chunks are streams of their own
    const bool resume = !(p->flags & PT_FLAG_FAST_RNG) && !s->knobs.no_resume;
    probe.resume_rng = resume ? s->ws_rng.p : nullptr;
    probe.resume_spp = 0;
    // a sample window's probe renders the window's first samples from the accumulator's state, in place; with probe_resume = -1 it
    // only costs (from the pixels' seeds: it writes nothing) and the frame launch renders the whole window
    if (window && resume) { probe.samples = w->done + probe_spp; probe.resume_rng = w->rng; probe.resume_spp = w->done; }
    int* const order_out = w ? w->order : s->ws_order.p;
    int* const nsplit_out = w ? w->nsplit : s->ws_nsplit.p;
    PassPlan probe_plan;
    if (int rc = run_pass(s, p, pv, pv.chain_bound, pv.queued_walk, local_tiles, probe, st, &probe_plan)) return rc;
    probed = true;
    // rough per-iteration instruction counts: traversal (splittable) vs shading + camera + cooperative overhead (not)
    const int forced_logG = s->knobs.wide_logG; // 0: the model picks the group size of the wide phase
    const unsigned int* ranked = s->ws_cost.p;
    if (probe.cost_max && p->shard_count == 1 && !coop) { // tile_dilate_kernel (a shard's neighbours are other ranks' tiles: its own estimates)
      hipLaunchKernelGGL(tile_dilate_kernel, dim3((unsigned int)((local_tiles + 255) / 256)), dim3(256), 0, st, s->ws_cost.p, base.tiles_x, (int)(base.n_tiles / base.tiles_x), s->ws_rank.p);
      PT_HIP(hipGetLastError());
      ranked = s->ws_rank.p;
    }
    // rough per-iteration instruction counts: traversal (splittable) vs shading + camera (not)
    hipLaunchKernelGGL(lpt_order_kernel, dim3(1), dim3(1024), 0, st, ranked, local_tiles, order_out, probe_plan.n_waves_resident,
                       std::max(1.0f, s->traversal_cost), s->knobs.model_fixed, s->knobs.model_chain, forced_logG, coop ? nsplit_out : nullptr);
    PT_HIP(hipGetLastError());
    if (s->knobs.has_split_tiles) { // tuning knob: fixed number of split tiles (< 0: all)
      if (coop) {
        const int k = s->knobs.split_tiles;
        s->nsplit_override = k < 0 ? local_tiles : std::min(k, local_tiles);
        PT_HIP(hipMemcpyAsync(nsplit_out, &s->nsplit_override, sizeof(int), hipMemcpyHostToDevice, st));
      }
    }
    // (A second, ORDERED probe stage of samples / 8 that keeps counting also removes the slow launches tile_dilate_kernel is there for — 1080p x
    // 1024 spp 375 / 407 -> 380.8 +- 1.5 — at the price of the fast ones and of 4 % on chain-bound shards: not kept.)
    if (window) { if (resume) frame.resume_spp = w->done + probe_spp; }
    else if (resume) { frame.resume_rng = s->ws_rng.p; frame.resume_spp = probe_spp; }
    frame.order = order_out;
    frame.n_split = (coop && !(p->flags & PT_FLAG_NO_SPLIT)) ? nsplit_out : nullptr;
    if (w) *w->has_order = true;
  } else if (w && *w->has_order) {
    // a window too short to probe: the order its accumulator kept from its last probed window (same scene, camera and frame: the tiles'
    // costs do not change between windows).  Never the scene's ws_order, which another render on the scene may have rewritten.
    frame.order = w->order;
    frame.n_split = (coop && !(p->flags & PT_FLAG_NO_SPLIT)) ? w->nsplit : nullptr;
  }

  // ---- the frame pass ----
  if (p->flags & PT_FLAG_FAST_RNG) {
    // OPT-IN decorrelated mode (include/pt_render.h): (tile, chunk) work units, per-chunk sums into a workspace, then
    // one ordered reduction.  No wide phase (a chunk is short by construction); the tile order of the probe still applies.
    const int chunks = fast_chunks_of(p->samples);
    if (chunks > 127 || local_tiles >= (1 << 18))
      return fail(PT_ERR_TOO_LARGE, "PT_FLAG_FAST_RNG supports up to 8128 samples per pixel and 2^24 pixels per shard");
    const size_t plane = (size_t)pt_framebuffer_floats(p), need = plane * (size_t)chunks;
    if (int rc = reserve_partial(s, need)) return rc; // first render at a new size only (or never: pt_scene_reserve)
    PT_HIP(hipMemsetAsync(s->ws_partial.p, 0, need * sizeof(float), st)); // pixels no lane owns add 0
    frame.fast_chunks = chunks;
    frame.fast_chunk0 = w ? w->done / PT_FAST_CHUNK_SPP : 0; // (a window starts on a chunk boundary: pt_render_accumulate)
    frame.samples = std::min(p->samples, (int)PT_FAST_CHUNK_SPP);
    frame.fast_stride = (long long)plane;
    frame.fb = s->ws_partial.p;
    frame.n_local_pixels = local_tiles * PT_TILE_PIXELS * chunks;
    if (scattered) set_scatter(frame, s->knobs.scatter_log);
    frame.n_split = nullptr;
    s->last_had_wide_phase = false;
    const Variant fv = choose_variant(s, p, local_tiles, true, frame.n_local_pixels);
    if (fv.rc) return fv.rc;
    frame.plan = pass_pool_plan(s, p, fv);
    s->last_pool_plan = frame.plan;
    // (what the probe pass of this call ran stays set for its chunk pass: run_pass)
    if (int rc = run_pass(s, p, fv, fv.chain_bound || (probed && pv.chain_bound), fv.queued_walk || (probed && pv.queued_walk),
                          (long long)local_tiles * chunks, frame, st))
      return rc;
    if (w) { // a window: its chunks onto the accumulator's running sums, in chunk order, undivided
      hipLaunchKernelGGL(fast_accum_kernel, dim3((unsigned int)((plane + 255) / 256)), dim3(256), 0, st, s->ws_partial.p, fb, (long long)plane,
                         (long long)plane, chunks);
      PT_HIP(hipGetLastError());
      return PT_OK;
    }
    hipLaunchKernelGGL(fast_reduce_kernel, dim3((unsigned int)((plane + 255) / 256)), dim3(256), 0, st, s->ws_partial.p, fb,
                       (long long)plane, (long long)plane, chunks, (float)p->samples);
    PT_HIP(hipGetLastError());
    return PT_OK;
  }
  if (scattered) set_scatter(frame, s->knobs.scatter_log);
  s->last_had_wide_phase = frame.n_split != nullptr;
  s->last_pool_plan = frame.plan;
  return run_pass(s, p, pv, pv.chain_bound, pv.queued_walk, local_tiles, frame, st);
}

// ---- first-hit feature buffers: the AOV pass (aov_kernel) -------------------------------------------------------------------------
// What pt_render_aov refuses, checked on the host before any device call (`depth` and the scheduling flags mean nothing to the pass).
int check_aov_params(const PtRenderParams* p) {
  if (!p) return fail(PT_ERR_INVALID_ARG, "render params are NULL");
  if (p->width <= 0 || p->height <= 0) return fail(PT_ERR_INVALID_ARG, "width and height must be > 0");
  if (int rc = check_shard(p)) return rc;
  if (p->flags & (PT_FLAG_FAST_RNG | PT_FLAG_SINGLE_STREAM))
    return fail(PT_ERR_INVALID_ARG, "the AOV pass is defined on the reference's stream per pixel: no PT_FLAG_FAST_RNG, no PT_FLAG_SINGLE_STREAM");
  return PT_OK;
}

// The launch: which aov_kernel (IMG: u,v tracked through the scan, as the scene's render kernels do; WALK: the sphere-grid walk the
// launcher would pick for a frame of these parameters), one wave per tile of the planes.  Nothing is allocated and none of the scene's
// launch workspaces is read or written.
int launch_aov(const PtScene* s, const PtCamera* cam, const PtRenderParams* p, const PtAovBuffers* b, hipStream_t st) {
  int cur = -1;
  PT_HIP(hipGetDevice(&cur));
  if (cur != s->device) return fail(PT_ERR_INVALID_ARG, "pt_render_aov: the scene lives on another device (hipSetDevice to the scene's device first)");
  AovArgs a;
  set_frame(a, s, cam, p);
  a.albedo = b->albedo; a.normal = b->normal; a.direct = b->direct; a.depth = b->depth; a.coverage = b->coverage; a.id = b->id;
  a.fast_ok = s->fast_ok ? 1 : 0;
  a.local_tiles = tiles_per_shard(a.n_tiles, p->shard_count);
  std::lock_guard<std::mutex> lock(s->sched); // (choose_variant caches its occupancy queries on the scene; last_aov)
  bool queued_walk = false;
  if (s->grid_spheres > 0) {
    PtRenderParams q = *p; // (the scheduling flags are ignored: the walk of an ordinary frame launch)
    q.flags = 0; q.depth = 1;
    const int local_tiles = local_tiles_of(&q);
    const Variant v = choose_variant(s, &q, local_tiles, false, local_tiles * PT_TILE_PIXELS);
    if (v.rc) return v.rc;
    queued_walk = v.queued_walk;
  }
  const auto kernel = s->track_uv ? (queued_walk ? aov_kernel<true, 2> : aov_kernel<true, 1>) : (queued_walk ? aov_kernel<false, 2> : aov_kernel<false, 1>);
  hipLaunchKernelGGL(kernel, dim3((a.local_tiles + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, st, a);
  PT_HIP(hipGetLastError());
  s->last_aov[0] = queued_walk ? 2 : 1; s->last_aov[1] = s->track_uv ? 1 : 0;
  return PT_OK;
}

} // namespace

extern "C" {

int64_t pt_aov_plane_elems(const PtRenderParams* p, int32_t channels) {
  if (check_aov_params(p) || (channels != 1 && channels != 3)) return -1;
  if (p->shard_count == 1) return (int64_t)p->width * p->height * channels;
  return (int64_t)tiles_per_shard(n_tiles_of(p, nullptr), p->shard_count) * PT_TILE_PIXELS * channels;
}

int pt_render_aov(const PtScene* scene, const PtCamera* cam, const PtRenderParams* p, const PtAovBuffers* buffers, void* stream) {
  if (!scene || !cam || !p || !buffers) return fail(PT_ERR_INVALID_ARG, "pt_render_aov: NULL argument");
  if (int rc = check_aov_params(p)) return rc;
  if (p->samples < 1 || p->samples > (1 << 24)) return fail(PT_ERR_INVALID_ARG, "pt_render_aov: need 1 <= samples <= 2^24 (coverage stays exact)");
  if (buffers->struct_size != (int32_t)sizeof(PtAovBuffers)) return fail(PT_ERR_INVALID_ARG, "pt_render_aov: PtAovBuffers.struct_size is not this library's");
  if (!buffers->albedo && !buffers->normal && !buffers->direct && !buffers->depth && !buffers->coverage && !buffers->id)
    return fail(PT_ERR_INVALID_ARG, "pt_render_aov: no plane asked for");
  return launch_aov(scene, cam, p, buffers, (hipStream_t)stream);
}

int pt_scene_reserve(const PtScene* scene, const PtRenderParams* p) {
  if (!scene) return fail(PT_ERR_INVALID_ARG, "pt_scene_reserve: NULL scene");
  int rc = check_params(p);
  if (rc) return rc;
  int cur = -1;
  PT_HIP(hipGetDevice(&cur));
  if (cur != scene->device) return fail(PT_ERR_INVALID_ARG, "pt_scene_reserve: the scene lives on another device");
  std::lock_guard<std::mutex> lock(scene->sched);
  const int local_tiles = local_tiles_of(p);
  if (local_tiles > 0 && (rc = reserve_tiles(scene, local_tiles))) return rc;
  if (p->flags & PT_FLAG_FAST_RNG) {
    const int chunks = fast_chunks_of(p->samples);
    if ((rc = reserve_partial(scene, (size_t)pt_framebuffer_floats(p) * (size_t)chunks))) return rc;
  }
  return PT_OK;
}

int pt_render(const PtScene* scene, const PtCamera* cam, const PtRenderParams* p, float* fb_device, void* stream) {
  if (!scene || !cam || !fb_device) return fail(PT_ERR_INVALID_ARG, "pt_render: NULL argument");
  int rc = check_params(p);
  if (rc) return rc;
  return launch_render(scene, cam, p, fb_device, (hipStream_t)stream);
}

int pt_render_timed(const PtScene* scene, const PtCamera* cam, const PtRenderParams* p, float* fb_device, void* stream,
                    float* kernel_ms) {
  if (!scene || !cam || !fb_device || !kernel_ms) return fail(PT_ERR_INVALID_ARG, "pt_render_timed: NULL argument");
  int rc = check_params(p);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  EventPair ev;
  PT_HIP(hipEventCreate(&ev.e0));
  PT_HIP(hipEventCreate(&ev.e1));
  PT_HIP(hipEventRecord(ev.e0, st));
  rc = launch_render(scene, cam, p, fb_device, st);
  if (rc != PT_OK) return rc;
  PT_HIP(hipEventRecord(ev.e1, st));
  PT_HIP(hipEventSynchronize(ev.e1));
  PT_HIP(hipEventElapsedTime(kernel_ms, ev.e0, ev.e1));
  return PT_OK;
}

int pt_render_host(const PtScene* scene, const PtCamera* cam, const PtRenderParams* p, float* fb_host) {
  if (!scene || !cam || !fb_host) return fail(PT_ERR_INVALID_ARG, "pt_render_host: NULL argument");
  int rc = check_params(p);
  if (rc) return rc;
  size_t bytes = (size_t)pt_framebuffer_floats(p) * sizeof(float);
  float* d = nullptr;
  PT_HIP(hipMalloc((void**)&d, bytes));
  rc = launch_render(scene, cam, p, d, nullptr);
  if (rc == PT_OK) {
    hipError_t e = hipMemcpy(fb_host, d, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(PT_ERR_HIP, std::string("hipMemcpy D2H: ") + hipGetErrorString(e));
  }
  (void)hipFree(d);
  return rc;
}

int pt_unshard_tiles(const float* gathered_device, const PtRenderParams* p, float* fb_device, void* stream) {
  if (!gathered_device || !fb_device) return fail(PT_ERR_INVALID_ARG, "pt_unshard_tiles: NULL argument");
  int rc = check_params(p);
  if (rc) return rc;
  int tiles_x;
  int n_tiles = n_tiles_of(p, &tiles_x);
  int per = tiles_per_shard(n_tiles, p->shard_count);
  dim3 block(256), grid((p->width + 255) / 256, p->height);
  hipLaunchKernelGGL(unshard_kernel, grid, block, 0, (hipStream_t)stream, gathered_device, fb_device, p->width, p->height,
                     tiles_x, p->shard_count, per);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

int pt_tonemap_rgb8(const float* fb_device, int32_t width, int32_t height, uint8_t* rgb8_device, void* stream) {
  if (!fb_device || !rgb8_device || width <= 0 || height <= 0) return fail(PT_ERR_INVALID_ARG, "pt_tonemap_rgb8: bad argument");
  dim3 block(256), grid((width + 255) / 256, height);
  hipLaunchKernelGGL(tonemap_kernel<false>, grid, block, 0, (hipStream_t)stream, fb_device, nullptr, 0, rgb8_device, width, height);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

// ---- the image stages' host prelude: what every stage below checks, tables and records alike.  A stage calls these pieces at its OWN
// positions — the order in which an entry point reports its refusals is its own (tests/test_stage_refusal_order_cpu.py) -------------------
} // extern "C"

namespace {
// an entry point's refusals, in its name
struct Refuse {
  const char* who;
  int operator()(const std::string& what) const { return fail(PT_ERR_INVALID_ARG, std::string(who) + ": " + what); }
  int too_large() const { return fail(PT_ERR_TOO_LARGE, std::string(who) + ": more than 2^30 pixels"); }
};

// a pt_*_params_init's first step: zeros and the struct's size; false for a NULL struct, which is ignored
template <class P>
bool init_params(P* p) {
  if (!p) return false;
  std::memset(p, 0, sizeof *p);
  p->struct_size = (int32_t)sizeof(P);
  return true;
}
template <class P>
bool is_ours(const P* p) { return p->struct_size == (int32_t)sizeof(P); }

constexpr int64_t kMaxPixels = (int64_t)1 << 30;
// the pixels of a frame, or -1 for a frame without pixels or with more than 2^30
int64_t frame_pixels(int32_t width, int32_t height) {
  return width <= 0 || height <= 0 || (int64_t)width * height > kMaxPixels ? -1 : (int64_t)width * height;
}

// the bytes [p, p + bytes) of a plane; a NULL plane meets nothing
struct Span {
  const void* p;
  uintptr_t bytes;
  Span unless_it_is(const void* input) const { return p == input ? Span{nullptr, 0} : *this; } // a written plane that may BE that input: left out
};
using Spans = std::initializer_list<Span>;
bool overlaps(Span a, Span b) {
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  return a.p && b.p && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
// does any of the written spans meet any of the read ones?
bool overlaps(Spans written, Spans read) {
  for (const Span& w : written)
    for (const Span& r : read)
      if (overlaps(w, r)) return true;
  return false;
}
// do the written spans meet one another?
bool overlap_one_another(Spans written) {
  for (const Span* i = written.begin(); i != written.end(); i++)
    for (const Span* j = i + 1; j != written.end(); j++)
      if (overlaps(*i, *j)) return true;
  return false;
}

// A parameter struct's rectangle inside a width x height frame: four zeros mean the whole frame.  False where it leaves the frame or is
// inverted — or, without `allow_empty`, holds no pixel.
struct Rect { int x0, y0, x1, y1; };
template <class P>
bool frame_rect(const P& p, int width, int height, bool allow_empty, Rect& r) {
  r = {p.rect_x0, p.rect_y0, p.rect_x1, p.rect_y1};
  if (!(r.x0 || r.y0 || r.x1 || r.y1)) { r.x1 = width; r.y1 = height; }
  const bool ordered = allow_empty ? r.x0 <= r.x1 && r.y0 <= r.y1 : r.x0 < r.x1 && r.y0 < r.y1;
  return r.x0 >= 0 && r.y0 >= 0 && r.x1 <= width && r.y1 <= height && ordered;
}

// The 32 x 8 tile walk of pt_firefly and pt_spatial_variance: one dimension of at most max_blocks workgroups, each of which walks the
// tiles grid.x apart.  (tiles is at most 2^30: a frame one pixel wide and 2^30 rows high has 2^27.)
static_assert(PT_FIREFLY_TILE_W == PT_SVAR_TILE_W && PT_FIREFLY_TILE_H == PT_SVAR_TILE_H, "TileGrid is either stage's tile");
struct TileGrid {
  int tiles_x, tiles_y, tiles;
  dim3 grid;
  TileGrid(int width, int height, int max_blocks)
      : tiles_x((width + PT_FIREFLY_TILE_W - 1) / PT_FIREFLY_TILE_W), tiles_y((height + PT_FIREFLY_TILE_H - 1) / PT_FIREFLY_TILE_H),
        tiles((int)((int64_t)tiles_x * tiles_y)), grid((unsigned)std::min(tiles, max_blocks)) {}
};

// a kernel's <true> / <false> pair (its LDS path, its vector path), 256 threads per workgroup
template <class... Params, class... Args>
int launch_pair(bool first, void (*k_true)(Params...), void (*k_false)(Params...), dim3 grid, hipStream_t st, Args... args) {
  hipLaunchKernelGGL(first ? k_true : k_false, grid, dim3(256), 0, st, args...);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

// What a pt_debug_last_* getter reports: N words about an entry point's last call.  begin(): a call starts — the words are zeroed and the
// lock is held while it launches and writes `words`; set(): words written under a lock of their own, the others kept.
template <int N>
struct LastRecord {
  std::mutex mutex;
  int32_t words[N] = {};
  std::unique_lock<std::mutex> begin() {
    std::unique_lock<std::mutex> lock(mutex);
    std::memset(words, 0, sizeof words);
    return lock;
  }
  template <class... W>
  void set(int first, W... w) {
    const int32_t v[] = {(int32_t)w...};
    std::lock_guard<std::mutex> lock(mutex);
    std::memcpy(words + first, v, sizeof v);
  }
  int copy_out(const char* who, int32_t* out) {
    if (!out) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
    std::lock_guard<std::mutex> lock(mutex);
    std::memcpy(out, words, sizeof words);
    return PT_OK;
  }
};
// the filters: the read path per iteration (0: not run, 1: global memory, 2: an LDS tile); the other stages: the header's words
LastRecord<8> g_last_denoise, g_last_vdn, g_last_display;
LastRecord<4> g_last_firefly, g_last_svar, g_last_imgerr;

// pt_firefly's and pt_spatial_variance's launch: the record begun, the counts zeroed on the stream, the kernel's LDS pair over the tile walk,
// and the record's words {the read path (1: global memory, 2: LDS), tiles_x, tiles_y, the stage's own fourth word}
template <class Args>
int launch_counted_tiles(LastRecord<4>& last, bool lds, void (*k_true)(Args), void (*k_false)(Args), const TileGrid& tg, uint32_t* counts,
                         hipStream_t st, const Args& a, int32_t fourth) {
  const auto lock = last.begin();
  if (counts) PT_HIP(hipMemsetAsync(counts, 0, 8, st));
  if (const int rc = launch_pair(lds, k_true, k_false, tg.grid, st, a)) return rc;
  const int32_t words[4] = {lds ? 2 : 1, tg.tiles_x, tg.tiles_y, fourth};
  std::memcpy(last.words, words, sizeof words);
  return PT_OK;
}

// ---- the denoisers' host side, once: what pt_denoise and pt_variance_denoise check, decide and launch alike ---------------------------------
// the largest step whose reads come from an LDS-staged tile (profiles/denoise_bench.txt, profiles/variance_denoise_bench.txt: the A/Bs)
constexpr int kFilterLdsMaxStep = 2;
static_assert(PT_DENOISE_DEMODULATE == PT_VDENOISE_DEMODULATE && PT_DENOISE_NO_LDS == PT_VDENOISE_NO_LDS &&
              PT_DENOISE_MAX_ITERATIONS == 8 && PT_VDENOISE_MAX_ITERATIONS == 8, "filter_plan reads either filter's flags and iterations");

// k = 1.0f / (sigma * sigma) in binary32, as the header defines it (host arithmetic: IEEE, no excess precision on this target)
float denoise_k(float sigma) {
  volatile float s2 = sigma * sigma;
  volatile float k = 1.0f / s2;
  return k;
}
bool denoise_k_ok(float k) { return std::isfinite(k) && k > 0.0f; }

struct FilterCall { // a call of either entry point: the fields its parameter struct shares with the other's, and the planes both take
  const char *who, *macro; // "pt_denoise", "PT_DENOISE": for messages
  int32_t width, height, iterations;
  float sigma_color, sigma_normal, sigma_depth, sigma_albedo; // sigma_color: the filter's own colour sigma, here only to be finite
  uint32_t flags;
  const float *albedo, *normal, *depth;
  const float* written[2]; // out and the filter's second output plane, or NULL
  const char* written_names;
  const float* scratch;
  int64_t scratch_floats;
};

struct FilterPlan {
  unsigned terms = 0; // DN_COLOR ... DN_ALBEDO
  float k_n = 0.0f, sd2 = 0.0f, k_a = 0.0f;
  bool demod = false, nd = false, al = false; // nd, al: the launches read the (normal, depth) / (albedo) records
  int32_t width = 0, height = 0, iterations = 0;
  int64_t pixels = 0;
  dim3 grid;
  int staged[8] = {}; // per iteration: the STEP of its kernel (0: taps from global memory)
};

// The checks in the order both entry points report them, after their own NULL and struct_size checks; color_k() converts the filter's
// colour sigma (> 0) where that conversion's error is due and returns what is wrong with it, or NULL.
template <class ColorK>
int filter_plan(const FilterCall& c, ColorK&& color_k, FilterPlan& p) {
  const Refuse bad{c.who};
  if (c.width <= 0 || c.height <= 0) return bad("width and height must be > 0");
  if (c.iterations < 1 || c.iterations > PT_DENOISE_MAX_ITERATIONS) return bad("need 1 <= iterations <= 8");
  for (float s : {c.sigma_color, c.sigma_normal, c.sigma_depth, c.sigma_albedo})
    if (!std::isfinite(s)) return bad("a sigma is not finite");
  if (c.flags & ~(PT_DENOISE_DEMODULATE | PT_DENOISE_NO_LDS)) return bad("unknown flags");
  p = FilterPlan{};
  p.demod = c.flags & PT_DENOISE_DEMODULATE;
  if (p.demod && !c.albedo) return bad(std::string(c.macro) + "_DEMODULATE needs the albedo plane");
  p.width = c.width; p.height = c.height; p.iterations = c.iterations;
  if (c.sigma_color > 0.0f) {
    p.terms |= DN_COLOR;
    if (const char* what = color_k()) return bad(what);
  }
  if (c.sigma_normal > 0.0f && c.normal) {
    p.terms |= DN_NORMAL;
    p.k_n = denoise_k(c.sigma_normal);
    if (!denoise_k_ok(p.k_n)) return bad("1 / sigma_normal^2 leaves binary32");
  }
  if (c.sigma_depth > 0.0f && c.depth) {
    p.terms |= DN_DEPTH;
    volatile float s2 = c.sigma_depth * c.sigma_depth;
    p.sd2 = s2;
    if (!denoise_k_ok(p.sd2)) return bad("sigma_depth^2 leaves binary32");
  }
  if (c.sigma_albedo > 0.0f && c.albedo) {
    p.terms |= DN_ALBEDO;
    p.k_a = denoise_k(c.sigma_albedo);
    if (!denoise_k_ok(p.k_a)) return bad("1 / sigma_albedo^2 leaves binary32");
  }
  p.pixels = (int64_t)c.width * c.height;
  if (p.pixels > kMaxPixels) return bad.too_large();
  if ((uintptr_t)c.scratch % 16) return bad("scratch must be 16-byte aligned");
  const uintptr_t frame = (uintptr_t)p.pixels * 12;
  if (overlaps({{c.written[0], frame}, {c.written[1], frame}, {c.scratch, (uintptr_t)c.scratch_floats * 4}},
               {{c.albedo, frame}, {c.normal, frame}, {c.depth, frame / 3}}))
    return bad(std::string(c.written_names) + " and scratch must not overlap a guide plane");
  p.nd = p.terms & (DN_NORMAL | DN_DEPTH); p.al = p.demod || (p.terms & DN_ALBEDO);
  p.grid = dim3((unsigned)((c.width + 31) / 32), (unsigned)((c.height + 7) / 8));
  // the kernel of an iteration: reads from an LDS-staged tile at the steps 1 and 2 (unless PT_*_NO_LDS), from global memory beyond
  for (int i = 0; i < c.iterations; i++) p.staged[i] = !(c.flags & PT_DENOISE_NO_LDS) && (1 << i) <= kFilterLdsMaxStep ? 1 << i : 0;
  return PT_OK;
}

// a filter kernel's instantiations as [STEP][ND][AL]
#define PT_FILTER_KERNELS(K)                                                                                   \
  {{{K<false, false, 0>, K<false, true, 0>}, {K<true, false, 0>, K<true, true, 0>}},                           \
   {{K<false, false, 1>, K<false, true, 1>}, {K<true, false, 1>, K<true, true, 1>}},                           \
   {{K<false, false, 2>, K<false, true, 2>}, {K<true, false, 2>, K<true, true, 2>}}}

// The iterations: fill(a, i) completes iteration i's arguments — its planes, a.f.g_nd / g_al, a.f.k_color and its own bits of a.f.terms.
template <class Args, class Fill>
int filter_launch(const FilterPlan& p, void (*const (&kernels)[3][2][2])(Args), LastRecord<8>& last, hipStream_t st, Fill&& fill) {
  for (int i = 0; i < p.iterations; i++) {
    Args a;
    a.f.width = p.width; a.f.height = p.height; a.f.step = 1 << i;
    a.f.terms = p.terms; a.f.k_n = p.k_n; a.f.sd2 = p.sd2; a.f.k_a = p.k_a;
    fill(a, i);
    hipLaunchKernelGGL(kernels[p.staged[i]][p.nd ? 1 : 0][p.al ? 1 : 0], p.grid, dim3(256), 0, st, a);
    PT_HIP(hipGetLastError());
    last.words[i] = p.staged[i] ? 2 : 1;
  }
  return PT_OK;
}
} // namespace

extern "C" {

// ---- denoiser: pt_denoise (atrous_pack_kernel, atrous_kernel): its colour ladder k_c(i), its scratch of one colour plane ---------------------

void pt_denoise_params_init(PtDenoiseParams* params, int32_t width, int32_t height) {
  if (!init_params(params)) return;
  params->width = width; params->height = height;
  params->iterations = PT_DENOISE_DEFAULT_ITERATIONS;
  params->sigma_color = PT_DENOISE_DEFAULT_SIGMA_COLOR; params->sigma_normal = PT_DENOISE_DEFAULT_SIGMA_NORMAL;
  params->sigma_depth = PT_DENOISE_DEFAULT_SIGMA_DEPTH; params->sigma_albedo = PT_DENOISE_DEFAULT_SIGMA_ALBEDO;
  params->flags = PT_DENOISE_DEFAULT_FLAGS;
}

// floats of the scratch's colour plane: 3 per pixel, rounded up so that the guide records behind it stay 16-byte aligned
static int64_t denoise_color_floats(int64_t pixels) { return (pixels * 3 + 3) / 4 * 4; }

int64_t pt_denoise_scratch_floats(int32_t width, int32_t height) {
  const int64_t pixels = frame_pixels(width, height);
  return pixels < 0 ? -1 : denoise_color_floats(pixels) + 8 * pixels;
}

int pt_denoise(const PtDenoiseParams* params, const float* color, const float* albedo, const float* normal, const float* depth,
               float* out, float* scratch, void* stream) {
  const Refuse bad{"pt_denoise"};
  if (!params || !color || !out || !scratch) return bad("NULL params, color, out or scratch");
  if (!is_ours(params)) return bad("PtDenoiseParams.struct_size is not this library's");
  const int n_it = params->iterations;
  const int64_t scratch_floats = pt_denoise_scratch_floats(params->width, params->height);
  float k_c[PT_DENOISE_MAX_ITERATIONS] = {};
  FilterPlan plan;
  const int rc = filter_plan({"pt_denoise", "PT_DENOISE", params->width, params->height, n_it, params->sigma_color, params->sigma_normal,
                              params->sigma_depth, params->sigma_albedo, params->flags, albedo, normal, depth, {out, nullptr}, "out", scratch,
                              scratch_floats},
                             [&]() -> const char* {
                               for (int i = 0; i < n_it; i++) {
                                 k_c[i] = denoise_k(std::ldexp(params->sigma_color, -i)); // sigma_color * 2^-i: exact (or rounded once into the denormals, whose k is refused)
                                 if (!denoise_k_ok(k_c[i])) return "1 / sigma_color^2 leaves binary32 at one of the iterations";
                               }
                               return nullptr;
                             }, plan);
  if (rc) return rc;
  const int64_t pixels = plan.pixels;
  const uintptr_t frame = (uintptr_t)pixels * 12;
  if (overlaps({{scratch, (uintptr_t)scratch_floats * 4}}, {{color, frame}, {out, frame}})) return bad("scratch must not overlap color or out");

  hipStream_t st = (hipStream_t)stream;
  float* const plane = scratch; // the colour plane the iterations ping-pong with `out`
  f4* const g_nd = reinterpret_cast<f4*>(scratch + denoise_color_floats(pixels));
  f4* const g_al = g_nd + pixels;
  const auto lock = g_last_denoise.begin();
  if (plan.nd || plan.al) {
    hipLaunchKernelGGL(atrous_pack_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, st, (plan.terms & DN_NORMAL) ? normal : nullptr,
                       (plan.terms & DN_DEPTH) ? depth : nullptr, albedo, plan.nd ? g_nd : nullptr, plan.al ? g_al : nullptr, (long long)pixels);
    PT_HIP(hipGetLastError());
  }
  // Iteration i writes `out` when an even number of iterations follows it and the scratch plane otherwise, so the last one writes `out`.
  // With an odd count the first would read `color` while writing `out`: where the two overlap it reads a copy in the scratch plane.
  const float* src = color;
  if (n_it % 2 == 1 && overlaps(Span{out, frame}, Span{color, frame})) {
    PT_HIP(hipMemcpyAsync(plane, color, (size_t)pixels * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    src = plane;
  }
  static void (*const kernels[3][2][2])(ATrousArgs) = PT_FILTER_KERNELS(atrous_kernel);
  return filter_launch(plan, kernels, g_last_denoise, st, [&](ATrousArgs& a, int i) {
    a.in = src;
    a.out = (n_it - 1 - i) % 2 == 0 ? out : plane;
    a.f.g_nd = g_nd; a.f.g_al = g_al;
    a.f.terms |= (plan.demod && i == 0 ? DN_DEMOD_IN : 0) | (plan.demod && i == n_it - 1 ? DN_REMOD_OUT : 0);
    a.f.k_color = k_c[i];
    src = a.out;
  });
}

int pt_debug_last_denoise(int32_t out[8]) { return g_last_denoise.copy_out("pt_debug_last_denoise", out); }

// ---- variance-guided denoiser: pt_variance_denoise (vdn_pack_kernel, vdn_kernel): its sv2, its variance planes, its scratch of records ------

void pt_variance_denoise_params_init(PtVarianceDenoiseParams* params, int32_t width, int32_t height) {
  if (!init_params(params)) return;
  params->width = width; params->height = height;
  params->iterations = PT_VDENOISE_DEFAULT_ITERATIONS;
  params->sigma_variance = PT_VDENOISE_DEFAULT_SIGMA_VARIANCE; params->sigma_normal = PT_VDENOISE_DEFAULT_SIGMA_NORMAL;
  params->sigma_depth = PT_VDENOISE_DEFAULT_SIGMA_DEPTH; params->sigma_albedo = PT_VDENOISE_DEFAULT_SIGMA_ALBEDO;
  params->flags = PT_VDENOISE_DEFAULT_FLAGS;
}

// per pixel: two working planes of a 16-byte and an 8-byte record (6 floats each) and two 16-byte guide records
int64_t pt_variance_denoise_scratch_floats(int32_t width, int32_t height) {
  const int64_t pixels = frame_pixels(width, height);
  return pixels < 0 ? -1 : 20 * pixels;
}

int pt_variance_denoise(const PtVarianceDenoiseParams* params, const float* color, const float* variance, const float* albedo,
                        const float* normal, const float* depth, float* out, float* variance_out, float* scratch, void* stream) {
  const Refuse bad{"pt_variance_denoise"};
  if (!params || !color || !variance || !out || !scratch) return bad("NULL params, color, variance, out or scratch");
  if (!is_ours(params)) return bad("PtVarianceDenoiseParams.struct_size is not this library's");
  const int64_t scratch_floats = pt_variance_denoise_scratch_floats(params->width, params->height);
  float sv2 = 0.0f;
  FilterPlan plan;
  const int rc = filter_plan({"pt_variance_denoise", "PT_VDENOISE", params->width, params->height, params->iterations, params->sigma_variance,
                              params->sigma_normal, params->sigma_depth, params->sigma_albedo, params->flags, albedo, normal, depth,
                              {out, variance_out}, "out, variance_out", scratch, scratch_floats},
                             [&]() -> const char* {
                               volatile float s2 = params->sigma_variance * params->sigma_variance;
                               sv2 = s2;
                               const bool ok = denoise_k_ok(sv2) && denoise_k_ok(denoise_k(params->sigma_variance));
                               return ok ? nullptr : "sigma_variance^2 or its reciprocal leaves binary32";
                             }, plan);
  if (rc) return rc;
  const int64_t pixels = plan.pixels;
  const uintptr_t frame = (uintptr_t)pixels * 12;
  if (overlaps({{scratch, (uintptr_t)scratch_floats * 4}}, {{color, frame}, {variance, frame}, {out, frame}, {variance_out, frame}}))
    return bad("scratch must not overlap color, variance, out or variance_out");
  if (overlaps({{variance_out, frame}}, {{color, frame}, {out, frame}})) return bad("variance_out must not overlap color or out");

  hipStream_t st = (hipStream_t)stream;
  // scratch: [A0 | A1 | g_nd | g_al] 16-byte records, then [B0 | B1] 8-byte records
  f4* const rec_a[2] = {reinterpret_cast<f4*>(scratch), reinterpret_cast<f4*>(scratch) + pixels};
  f4* const g_nd = rec_a[1] + pixels;
  f4* const g_al = g_nd + pixels;
  f2v* const rec_b[2] = {reinterpret_cast<f2v*>(g_al + pixels), reinterpret_cast<f2v*>(g_al + pixels) + pixels};
  const auto lock = g_last_vdn.begin();
  hipLaunchKernelGGL(vdn_pack_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, st, color, variance, (plan.terms & DN_NORMAL) ? normal : nullptr,
                     (plan.terms & DN_DEPTH) ? depth : nullptr, albedo, rec_a[0], rec_b[0], plan.nd ? g_nd : nullptr, plan.al ? g_al : nullptr,
                     (long long)pixels, plan.demod ? 1 : 0);
  PT_HIP(hipGetLastError());
  static void (*const kernels[3][2][2])(VdnArgs) = PT_FILTER_KERNELS(vdn_kernel);
  return filter_launch(plan, kernels, g_last_vdn, st, [&](VdnArgs& a, int i) {
    const bool last = i == plan.iterations - 1;
    a.in_a = rec_a[i % 2]; a.in_b = rec_b[i % 2];
    a.out_a = rec_a[(i + 1) % 2]; a.out_b = rec_b[(i + 1) % 2];
    a.out_color = out; a.out_var = variance_out;
    a.f.g_nd = g_nd; a.f.g_al = g_al;
    a.f.terms |= (last ? VDN_LAST : 0) | (plan.demod && last ? DN_REMOD_OUT : 0);
    a.f.k_color = sv2;
  });
}

int pt_debug_last_variance_denoise(int32_t out[8]) { return g_last_vdn.copy_out("pt_debug_last_variance_denoise", out); }

// ---- temporal reprojection: PtTemporal, pt_temporal_push (temporal_push_kernel) -------------------------------------------------------
} // extern "C"

struct PtTemporal {
  int32_t width = 0, height = 0;
  long long pixels = 0;
  DevBuf<f4> rec;     // two histories of three planes of `pixels` 16-byte records: a push reads one and writes the other
  int cur = 0;        // the history the next push reads
  int32_t frames = 0; // pushes since create / reset (0: no history)
  PtCamera cam{};     // the camera of the last push
};

namespace {
// fo, hh, vv of a camera (include/pt_render.h): each product and each sum rounded to binary32
struct TemporalConsts { float fo, hh, vv; bool ok; };
TemporalConsts temporal_consts(const PtCamera& c) {
  volatile float g[3], t[3], s;
  for (int i = 0; i < 3; i++) g[i] = c.lower_left_corner[i] - c.origin[i];
  auto dot = [&](const float* a, const float* b) {
    for (int i = 0; i < 3; i++) t[i] = a[i] * b[i];
    s = t[0] + t[1];
    s = s + t[2];
    return (float)s;
  };
  const float gg[3] = {g[0], g[1], g[2]};
  TemporalConsts k;
  k.fo = -dot(gg, c.w);
  k.hh = dot(c.horizontal, c.horizontal);
  k.vv = dot(c.vertical, c.vertical);
  auto good = [](float v) { return std::isfinite(v) && v > 0.0f; };
  k.ok = good(k.fo) && good(k.hh) && good(k.vv);
  return k;
}
} // namespace

extern "C" {

void pt_temporal_params_init(PtTemporalParams* params) {
  if (!init_params(params)) return;
  params->alpha = PT_TEMPORAL_DEFAULT_ALPHA;
  params->tol_depth = PT_TEMPORAL_DEFAULT_TOL_DEPTH;
  params->tol_normal = PT_TEMPORAL_DEFAULT_TOL_NORMAL;
}

// two histories of three 16-byte records per pixel
int64_t pt_temporal_state_bytes(int32_t width, int32_t height) {
  const int64_t pixels = frame_pixels(width, height);
  return pixels < 0 ? -1 : 96 * pixels;
}

int pt_temporal_create(int32_t width, int32_t height, PtTemporal** out) {
  if (!out) return fail(PT_ERR_INVALID_ARG, "pt_temporal_create: out is NULL");
  *out = nullptr;
  const Refuse bad{"pt_temporal_create"};
  if (width <= 0 || height <= 0) return bad("width and height must be > 0");
  if (frame_pixels(width, height) < 0) return bad.too_large();
  std::unique_ptr<PtTemporal> t(new PtTemporal());
  t->width = width; t->height = height; t->pixels = (long long)width * height;
  const hipError_t e = t->rec.alloc((size_t)t->pixels * 6);
  if (e != hipSuccess) return fail(PT_ERR_HIP, std::string("pt_temporal_create: hipMalloc: ") + hipGetErrorString(e));
  *out = t.release();
  return PT_OK;
}

void pt_temporal_destroy(PtTemporal* t) { delete t; }

// (nothing to do on the device: a push without history does not read the records)
int pt_temporal_reset(PtTemporal* t, void* stream) {
  if (!t) return fail(PT_ERR_INVALID_ARG, "pt_temporal_reset: NULL state");
  t->frames = 0;
  return PT_OK;
}

int32_t pt_temporal_frames(const PtTemporal* t) { return t ? t->frames : -1; }

int pt_temporal_push(PtTemporal* t, const PtTemporalParams* params, const PtCamera* cam, const float* color, const float* depth,
                     const float* normal, const int32_t* id, const float* variance_in, float* out_color, float* out_variance,
                     float* out_history, void* stream) {
  const Refuse bad{"pt_temporal_push"};
  // (the arguments that can be judged without the state first: the state is read only once they are sound)
  if (!t || !params || !cam || !color || !depth || !out_color) return bad("NULL state, params, cam, color, depth or out_color");
  if (!is_ours(params)) return bad("PtTemporalParams.struct_size is not this library's");
  if (!(params->alpha > 0.0f && params->alpha <= 1.0f)) return bad("need 0 < alpha <= 1");
  if (!(std::isfinite(params->tol_depth) && params->tol_depth > 0.0f) || !(std::isfinite(params->tol_normal) && params->tol_normal > 0.0f))
    return bad("a tolerance is not a finite number > 0");
  if (params->flags) return bad("unknown flags");
  if (!temporal_consts(*cam).ok) return bad("a degenerate camera (fo, hh or vv is not a finite number > 0)");
  const long long pixels = t->pixels;
  const uintptr_t plane = (uintptr_t)pixels * 4;
  const Spans outs = {{out_color, plane * 3}, {out_variance, plane * 3}, {out_history, plane}};
  if (overlaps(outs, {{depth, plane}, {normal, plane * 3}, {id, plane}})) return bad("an out plane overlaps a guide plane");
  if (overlap_one_another(outs)) return bad("the out planes overlap one another");

  TemporalArgs a;
  a.color = color; a.depth = depth; a.normal = normal; a.id = id; a.var_in = variance_in;
  a.out_color = out_color; a.out_var = out_variance; a.out_hist = out_history;
  a.prev = t->rec.p + (size_t)t->cur * 3 * (size_t)pixels;
  a.next = t->rec.p + (size_t)(1 - t->cur) * 3 * (size_t)pixels;
  a.pixels = pixels; a.width = t->width; a.height = t->height;
  a.has_history = t->frames > 0 ? 1 : 0;
  const PtCamera& pc = a.has_history ? t->cam : *cam;
  const TemporalConsts k = temporal_consts(pc); // (sound: every stored camera passed the check above)
  for (int i = 0; i < 3; i++) {
    a.o[i] = cam->origin[i]; a.llc[i] = cam->lower_left_corner[i]; a.hor[i] = cam->horizontal[i]; a.ver[i] = cam->vertical[i];
    a.po[i] = pc.origin[i]; a.pw[i] = pc.w[i]; a.ph[i] = pc.horizontal[i]; a.pv[i] = pc.vertical[i];
  }
  a.fo = k.fo; a.hh = k.hh; a.vv = k.vv;
  a.alpha = params->alpha; a.tol_depth = params->tol_depth;
  volatile float tn2 = params->tol_normal * params->tol_normal;
  a.tn2 = tn2;
  const dim3 grid((unsigned)((t->width + 31) / 32), (unsigned)((t->height + 7) / 8));
  hipLaunchKernelGGL(temporal_push_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  PT_HIP(hipGetLastError());
  t->cur = 1 - t->cur;
  t->cam = *cam;
  if (t->frames < INT32_MAX) t->frames++;
  return PT_OK;
}

// ---- display stage: PtDisplay, pt_display_meter (display_meter_kernel, display_solve_kernel), pt_display_apply (display_apply_kernel) ----
} // extern "C"

struct PtDisplay {
  DevBuf<unsigned> words; // DISP_WORDS: the working histogram, the last metering's, e, scale, primed
  int32_t frames = 0;     // meterings since create / reset
};

namespace {
// What can be judged of a call without a live object: the params, the frame, the rectangle.  iw2 = 1.0f / (white * white), rounded twice.
int display_check(const char* call, const PtDisplayParams* p, const float* color, int32_t width, int32_t height, float* iw2_out) {
  const Refuse bad{call};
  if (!p || !color) return bad("NULL params or color");
  if (!is_ours(p)) return bad("PtDisplayParams.struct_size is not this library's");
  if (width <= 0 || height <= 0) return bad("width and height must be > 0");
  if ((int64_t)width * height > ((int64_t)1 << 31)) return bad("more than 2^31 pixels");
  if (p->tone != PT_TONE_REFERENCE && p->tone != PT_TONE_REINHARD && p->tone != PT_TONE_ACES) return bad("unknown tone");
  if (p->flags) return bad("unknown flags");
  if (p->lo_permille < 0 || p->hi_permille > 1000 || p->lo_permille >= p->hi_permille) return bad("need 0 <= lo_permille < hi_permille <= 1000");
  if (!(p->adapt_up > 0.0f && p->adapt_up <= 1.0f) || !(p->adapt_down > 0.0f && p->adapt_down <= 1.0f)) return bad("an adaptation rate is outside (0, 1]");
  if (!(p->ev_min >= -32.0f && p->ev_max <= 32.0f && p->ev_min <= p->ev_max)) return bad("need -32 <= ev_min <= ev_max <= 32");
  if (!std::isfinite(p->ev_bias)) return bad("ev_bias is not finite");
  volatile float w2 = p->white * p->white;
  volatile float iw2 = 1.0f / w2;
  if (!(std::isfinite(iw2) && iw2 > 0.0f)) return bad("white: 1 / (white * white) is not a finite binary32 number > 0");
  if (Rect r; !frame_rect(*p, width, height, false, r)) return bad("the metering rectangle is empty or leaves the frame");
  if (iw2_out) *iw2_out = iw2;
  return PT_OK;
}
} // namespace

extern "C" {

void pt_display_params_init(PtDisplayParams* params) {
  if (!init_params(params)) return;
  params->tone = PT_DISPLAY_DEFAULT_TONE;
  params->ev_bias = PT_DISPLAY_DEFAULT_EV_BIAS; params->ev_min = PT_DISPLAY_DEFAULT_EV_MIN; params->ev_max = PT_DISPLAY_DEFAULT_EV_MAX;
  params->lo_permille = PT_DISPLAY_DEFAULT_LO_PERMILLE; params->hi_permille = PT_DISPLAY_DEFAULT_HI_PERMILLE;
  params->adapt_up = PT_DISPLAY_DEFAULT_ADAPT_UP; params->adapt_down = PT_DISPLAY_DEFAULT_ADAPT_DOWN;
  params->white = PT_DISPLAY_DEFAULT_WHITE;
}

int pt_display_create(PtDisplay** out) {
  if (!out) return fail(PT_ERR_INVALID_ARG, "pt_display_create: out is NULL");
  *out = nullptr;
  std::unique_ptr<PtDisplay> d(new PtDisplay());
  const hipError_t e = d->words.alloc(DISP_WORDS);
  if (e != hipSuccess) return fail(PT_ERR_HIP, std::string("pt_display_create: hipMalloc: ") + hipGetErrorString(e));
  std::vector<unsigned> init(DISP_WORDS, 0u);
  const float one = 1.0f;
  std::memcpy(&init[DISP_SCALE], &one, sizeof one);
  PT_HIP(hipMemcpy(d->words.p, init.data(), DISP_WORDS * sizeof(unsigned), hipMemcpyHostToDevice));
  *out = d.release();
  return PT_OK;
}

void pt_display_destroy(PtDisplay* d) { delete d; }

int pt_display_reset(PtDisplay* d, void* stream) {
  if (!d) return fail(PT_ERR_INVALID_ARG, "pt_display_reset: NULL state");
  hipLaunchKernelGGL(display_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d->words.p, 1, 0.0f);
  PT_HIP(hipGetLastError());
  d->frames = 0;
  return PT_OK;
}

int32_t pt_display_frames(const PtDisplay* d) { return d ? d->frames : -1; }

int pt_display_set_exposure(PtDisplay* d, float ev, void* stream) {
  if (!d) return fail(PT_ERR_INVALID_ARG, "pt_display_set_exposure: NULL state");
  if (ev != ev) return fail(PT_ERR_INVALID_ARG, "pt_display_set_exposure: ev is NaN");
  hipLaunchKernelGGL(display_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d->words.p, 0, std::fmin(std::fmax(ev, -32.0f), 32.0f));
  PT_HIP(hipGetLastError());
  return PT_OK;
}

int pt_display_meter(PtDisplay* d, const PtDisplayParams* p, const float* color, int32_t width, int32_t height, void* stream) {
  if (const int rc = display_check("pt_display_meter", p, color, width, height, nullptr)) return rc;
  if (!d) return fail(PT_ERR_INVALID_ARG, "pt_display_meter: NULL state");
  Rect r;
  frame_rect(*p, width, height, false, r);
  const int x0 = r.x0, y0 = r.y0, x1 = r.x1, y1 = r.y1;
  const int64_t n = (int64_t)(x1 - x0) * (y1 - y0); // 1 ... 2^31
  // four pixels per thread where the rectangle is one contiguous, 16-byte aligned range of the frame
  const bool vec = x1 - x0 == width && ((uintptr_t)(color + ((int64_t)y0 * width + x0) * 3) & 15) == 0;
  const int64_t items = vec ? (n + 3) / 4 : n;
  const unsigned blocks = (unsigned)std::min<int64_t>((items + DISP_METER_THREADS - 1) / DISP_METER_THREADS, DISP_METER_MAX_BLOCKS);
  unsigned* const work = d->words.p + DISP_WORK;
  static_assert(DISP_METER_THREADS == 256, "launch_pair's workgroup");
  if (const int rc = launch_pair(vec, display_meter_kernel<true>, display_meter_kernel<false>, dim3(blocks), (hipStream_t)stream, color, work,
                                 (int)width, x0, y0, x1 - x0, (unsigned)n))
    return rc;
  DisplaySolveArgs a;
  a.state = d->words.p;
  a.lo_permille = p->lo_permille; a.hi_permille = p->hi_permille;
  a.ev_bias = p->ev_bias; a.ev_min = p->ev_min; a.ev_max = p->ev_max; a.adapt_up = p->adapt_up; a.adapt_down = p->adapt_down;
  hipLaunchKernelGGL(display_solve_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  PT_HIP(hipGetLastError());
  if (d->frames < INT32_MAX) d->frames++;
  g_last_display.set(0, blocks, DISP_METER_THREADS, (items + (int64_t)blocks * DISP_METER_THREADS - 1) / ((int64_t)blocks * DISP_METER_THREADS),
                     vec ? 4 : 1);
  return PT_OK;
}

int pt_display_apply(const PtDisplay* d, const PtDisplayParams* p, const float* color, int32_t width, int32_t height, uint8_t* rgb8_out,
                     float* linear_out, void* stream) {
  float iw2 = 0.0f;
  if (const int rc = display_check("pt_display_apply", p, color, width, height, &iw2)) return rc;
  const Refuse bad{"pt_display_apply"};
  if (!rgb8_out && !linear_out) return bad("rgb8_out and linear_out are both NULL");
  const uintptr_t values = (uintptr_t)width * (uintptr_t)height * 3;
  if (overlaps({{rgb8_out, values}}, {{color, values * 4}, {linear_out, values * 4}})) return bad("rgb8_out overlaps color or linear_out");
  if (linear_out != color && overlaps(Span{linear_out, values * 4}, Span{color, values * 4})) return bad("linear_out overlaps color without being color");
  const float ev = std::fmin(std::fmax(p->ev_bias, -32.0f), 32.0f);
  const unsigned* state = d ? d->words.p : nullptr;
  // four values per thread where the rows and the planes allow 16-byte loads and stores
  const bool vec = width % 4 == 0 && ((uintptr_t)color & 15) == 0 && ((uintptr_t)linear_out & 15) == 0 && ((uintptr_t)rgb8_out & 3) == 0;
  const long long row_items = vec ? 3ll * width / 4 : 3ll * width;
  const dim3 grid((unsigned)((row_items + 255) / 256), (unsigned)std::min<int32_t>(height, 65535)), block(256);
#define PT_DISPLAY_APPLY(TONE, VEC) \
  hipLaunchKernelGGL((display_apply_kernel<TONE, VEC>), grid, block, 0, (hipStream_t)stream, color, state, ev, iw2, rgb8_out, linear_out, (int)width, (int)height)
  if (p->tone == PT_TONE_REINHARD) { if (vec) PT_DISPLAY_APPLY(PT_TONE_REINHARD, true); else PT_DISPLAY_APPLY(PT_TONE_REINHARD, false); }
  else if (p->tone == PT_TONE_ACES) { if (vec) PT_DISPLAY_APPLY(PT_TONE_ACES, true); else PT_DISPLAY_APPLY(PT_TONE_ACES, false); }
  else { if (vec) PT_DISPLAY_APPLY(PT_TONE_REFERENCE, true); else PT_DISPLAY_APPLY(PT_TONE_REFERENCE, false); }
#undef PT_DISPLAY_APPLY
  PT_HIP(hipGetLastError());
  g_last_display.set(4, grid.x, grid.y, vec ? 4 : 1, p->tone + 1);
  return PT_OK;
}

int pt_display_exposure(const PtDisplay* d, float* ev_host, void* stream) {
  if (!d || !ev_host) return fail(PT_ERR_INVALID_ARG, "pt_display_exposure: NULL argument");
  PT_HIP(hipMemcpyAsync(ev_host, d->words.p + DISP_E, sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
  PT_HIP(hipStreamSynchronize((hipStream_t)stream));
  return PT_OK;
}

int pt_display_histogram(const PtDisplay* d, uint32_t host[257], void* stream) {
  if (!d || !host) return fail(PT_ERR_INVALID_ARG, "pt_display_histogram: NULL argument");
  PT_HIP(hipMemcpyAsync(host, d->words.p + DISP_LAST, DISP_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  PT_HIP(hipStreamSynchronize((hipStream_t)stream));
  return PT_OK;
}

int pt_debug_last_display(int32_t out[8]) { return g_last_display.copy_out("pt_debug_last_display", out); }

// ---- firefly stage (include/pt_post.h): pt_firefly (firefly_kernel) ------------------------------------------------------------------------
void pt_firefly_params_init(PtFireflyParams* params, int32_t width, int32_t height) {
  if (!init_params(params)) return;
  params->width = width; params->height = height;
  params->rank = PT_FIREFLY_DEFAULT_RANK;
  params->k = PT_FIREFLY_DEFAULT_K;
  params->flags = PT_FIREFLY_DEFAULT_FLAGS;
}

int pt_firefly(const PtFireflyParams* params, const float* color, const float* variance, float* out, float* variance_out, uint32_t* counts,
               void* stream) {
  const Refuse bad{"pt_firefly"};
  if (!params || !color || !out) return bad("NULL params, color or out");
  if (!is_ours(params)) return bad("PtFireflyParams.struct_size is not this library's");
  if (params->width <= 0 || params->height <= 0) return bad("width and height must be > 0");
  if (params->rank != 1 && params->rank != 2) return bad("rank must be 1 or 2");
  if (!(std::isfinite(params->k) && params->k > 0.0f)) return bad("k must be finite and > 0");
  if (params->flags & ~(PT_FIREFLY_REPAIR | PT_FIREFLY_NO_LDS)) return bad("unknown flags");
  if (variance_out && !variance) return bad("variance_out needs variance");
  const int64_t pixels = (int64_t)params->width * params->height;
  if (pixels > kMaxPixels) return bad.too_large();
  if ((uintptr_t)counts % 8) return bad("counts must be 8-byte aligned");
  const uintptr_t frame = (uintptr_t)pixels * 12;
  const Span var_out{variance_out, frame};
  if (overlaps({{out, frame}, var_out.unless_it_is(variance), {counts, 8}}, {{color, frame}, {variance, frame}}))
    return bad("out, variance_out and counts must not overlap color or variance (variance_out may be variance itself)");
  if (overlap_one_another({{out, frame}, var_out, {counts, 8}})) return bad("out, variance_out and counts must not overlap one another");

  hipStream_t st = (hipStream_t)stream;
  const bool lds = !(params->flags & PT_FIREFLY_NO_LDS);
  FireflyArgs a;
  a.color = color; a.variance = variance; a.out = out; a.variance_out = variance_out;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.width = params->width; a.height = params->height;
  const TileGrid tg(params->width, params->height, PT_FIREFLY_MAX_BLOCKS);
  a.tiles_x = tg.tiles_x; a.tiles = tg.tiles;
  a.rank = params->rank; a.repair = params->flags & PT_FIREFLY_REPAIR; a.k = params->k;
  return launch_counted_tiles(g_last_firefly, lds, firefly_kernel<true>, firefly_kernel<false>, tg, counts, st, a, variance_out ? 2 : 1);
}

int pt_debug_last_firefly(int32_t out[4]) { return g_last_firefly.copy_out("pt_debug_last_firefly", out); }

// ---- spatial variance estimate (include/pt_spatial_variance.h): pt_spatial_variance (svar_kernel) ----------------------------------------
void pt_spatial_variance_params_init(PtSpatialVarianceParams* params, int32_t width, int32_t height) {
  if (!init_params(params)) return;
  params->width = width; params->height = height;
  params->radius = PT_SVAR_DEFAULT_RADIUS;
  params->min_pairs = PT_SVAR_DEFAULT_MIN_PAIRS;
  params->tol_depth = PT_SVAR_DEFAULT_TOL_DEPTH;
  params->tol_normal = PT_SVAR_DEFAULT_TOL_NORMAL;
  params->flags = PT_SVAR_DEFAULT_FLAGS;
}

int pt_spatial_variance(const PtSpatialVarianceParams* params, const float* color, const float* albedo, const float* normal,
                        const float* depth, const int32_t* id, const float* variance_in, float* variance_out, uint32_t* counts,
                        void* stream) {
  const Refuse bad{"pt_spatial_variance"};
  if (!params || !color || !variance_out) return bad("NULL params, color or variance_out");
  if (!is_ours(params)) return bad("PtSpatialVarianceParams.struct_size is not this library's");
  if (params->width <= 0 || params->height <= 0) return bad("width and height must be > 0");
  if (params->radius < 1 || params->radius > PT_SVAR_MAX_RADIUS) return bad("radius must be 1 ... PT_SVAR_MAX_RADIUS");
  if (params->min_pairs < 1) return bad("min_pairs must be >= 1");
  if (!(std::isfinite(params->tol_depth) && params->tol_depth > 0.0f)) return bad("tol_depth must be finite and > 0");
  if (!(std::isfinite(params->tol_normal) && params->tol_normal > 0.0f)) return bad("tol_normal must be finite and > 0");
  if (params->flags & ~(PT_SVAR_DEMODULATE | PT_SVAR_NO_LDS)) return bad("unknown flags");
  if ((params->flags & PT_SVAR_DEMODULATE) && !albedo) return bad("PT_SVAR_DEMODULATE needs albedo");
  const int64_t pixels = (int64_t)params->width * params->height;
  if (pixels > kMaxPixels) return bad.too_large();
  if ((uintptr_t)counts % 8) return bad("counts must be 8-byte aligned");
  const uintptr_t frame = (uintptr_t)pixels * 12, plane = (uintptr_t)pixels * 4;
  const Span var_out{variance_out, frame};
  if (overlaps({var_out.unless_it_is(variance_in), {counts, 8}},
               {{color, frame}, {albedo, frame}, {normal, frame}, {depth, plane}, {id, plane}, {variance_in, frame}}))
    return bad("variance_out and counts must not overlap color, a guide or variance_in (variance_out may be variance_in itself)");
  if (overlap_one_another({var_out, {counts, 8}})) return bad("variance_out and counts must not overlap one another");

  hipStream_t st = (hipStream_t)stream;
  const bool lds = !(params->flags & PT_SVAR_NO_LDS);
  SvarArgs a;
  a.color = color; a.albedo = albedo; a.normal = normal; a.depth = depth; a.id = id; a.variance_in = variance_in; a.variance_out = variance_out;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.width = params->width; a.height = params->height;
  const TileGrid tg(params->width, params->height, PT_SVAR_MAX_BLOCKS);
  a.tiles_x = tg.tiles_x; a.tiles = tg.tiles;
  a.radius = params->radius; a.min_pairs = params->min_pairs;
  a.demodulate = params->flags & PT_SVAR_DEMODULATE;
  a.tol_depth = params->tol_depth; a.tol_normal = params->tol_normal;
  return launch_counted_tiles(g_last_svar, lds, svar_kernel<true>, svar_kernel<false>, tg, counts, st, a, params->radius);
}

int pt_debug_last_spatial_variance(int32_t out[4]) { return g_last_svar.copy_out("pt_debug_last_spatial_variance", out); }

// ---- image error (include/pt_metrics.h): pt_image_error (imgerr_accumulate_kernel, imgerr_finish_kernel) ---------------------------------
void pt_image_error_params_init(PtImageErrorParams* params, int32_t width, int32_t height) {
  if (!init_params(params)) return;
  params->width = width; params->height = height;
  params->eps = PT_IMAGE_ERROR_DEFAULT_EPS;
}

int64_t pt_image_error_scratch_bytes(void) { return (int64_t)IMGERR_SCRATCH_WORDS * 8; }

int pt_image_error(const PtImageErrorParams* params, const float* a, const float* ref, PtImageErrorResult* result, float* error_plane,
                   void* scratch, void* stream) {
  const Refuse bad{"pt_image_error"};
  if (!params || !a || !ref || !result || !scratch) return bad("NULL params, a, ref, result or scratch");
  if (!is_ours(params)) return bad("PtImageErrorParams.struct_size is not this library's");
  const int width = params->width, height = params->height;
  if (width <= 0 || height <= 0) return bad("width and height must be > 0");
  Rect r;
  if (!frame_rect(*params, width, height, true, r)) return bad("the rectangle leaves the frame");
  const int x0 = r.x0, y0 = r.y0, x1 = r.x1, y1 = r.y1;
  if (!(std::isfinite(params->eps) && params->eps >= 0x1p-126)) return bad("eps must be finite and >= 2^-126");
  if (params->flags & ~PT_IMAGE_ERROR_NO_LDS) return bad("unknown flags");
  const int64_t pixels = (int64_t)width * height;
  if (pixels > kMaxPixels) return bad.too_large();
  if ((uintptr_t)result % 8 || (uintptr_t)scratch % 8) return bad("result and scratch must be 8-byte aligned");
  const uintptr_t scratch_bytes = (uintptr_t)IMGERR_SCRATCH_WORDS * 8;
  if (params->scratch_bytes < (int64_t)scratch_bytes) return bad("scratch_bytes is less than pt_image_error_scratch_bytes()");
  const uintptr_t frame = (uintptr_t)pixels * 12, plane = (uintptr_t)pixels * 4;
  const Spans written = {{error_plane, plane}, {result, sizeof(PtImageErrorResult)}, {scratch, scratch_bytes}};
  if (overlaps(written, {{a, frame}, {ref, frame}})) return bad("error_plane, result and scratch must not overlap an input");
  if (overlap_one_another(written)) return bad("error_plane, result and scratch must not overlap one another");

  hipStream_t st = (hipStream_t)stream;
  const bool lds = !(params->flags & PT_IMAGE_ERROR_NO_LDS);
  ImgErrArgs k;
  k.a = a; k.ref = ref; k.plane = error_plane; k.scratch = static_cast<unsigned long long*>(scratch);
  k.width = width;
  k.x0 = x0; k.y0 = y0; k.x1 = x1; k.y1 = y1;
  const bool whole = error_plane != nullptr; // the plane has a value for every pixel of the frame
  k.wx0 = whole ? 0 : x0; k.wy0 = whole ? 0 : y0; k.ww = whole ? width : x1 - x0;
  k.n = (unsigned)(whole ? pixels : (int64_t)(x1 - x0) * (y1 - y0));
  k.eps = params->eps;
  const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)k.n + 255) / 256, PT_IMGERR_MAX_BLOCKS);
  const auto lock = g_last_imgerr.begin();
  PT_HIP(hipMemsetAsync(scratch, 0, scratch_bytes, st));
  if (blocks) // (an empty rectangle without a plane: nothing to walk)
    if (const int rc = launch_pair(lds, imgerr_accumulate_kernel<true>, imgerr_accumulate_kernel<false>, dim3(blocks), st, k)) return rc;
  hipLaunchKernelGGL(imgerr_finish_kernel, dim3(1), dim3(64), 0, st, k.scratch, result);
  PT_HIP(hipGetLastError());
  const int32_t words[4] = {lds ? 2 : 1, (int32_t)blocks, x1 - x0, y1 - y0};
  std::memcpy(g_last_imgerr.words, words, sizeof words);
  return PT_OK;
}

int pt_debug_last_image_error(int32_t out[4]) { return g_last_imgerr.copy_out("pt_debug_last_image_error", out); }

// ---- encode stage (include/pt_encode.h): pt_encode, pt_display_encode (encode_kernel) ------------------------------------------------------
} // extern "C"

namespace {
LastRecord<8> g_last_encode;

// What both entry points check once the frame has pixels, in the header's order; `in` is the plane the call reads.
int encode_check(const Refuse& bad, const PtEncodeParams* p, const float* in, const uint8_t* rgb8_out) {
  const int64_t pixels = (int64_t)p->width * p->height;
  if (pixels > kMaxPixels) return bad.too_large();
  if (p->transfer != PT_TRANSFER_REFERENCE && p->transfer != PT_TRANSFER_SRGB) return bad("unknown transfer");
  if (p->flags & ~(PT_ENCODE_DITHER | PT_ENCODE_NO_VEC)) return bad("unknown flags");
  if ((p->flags & PT_ENCODE_DITHER) && p->transfer != PT_TRANSFER_SRGB) return bad("PT_ENCODE_DITHER needs PT_TRANSFER_SRGB");
  const uintptr_t values = (uintptr_t)pixels * 3;
  if (overlaps(Span{rgb8_out, values}, Span{in, values * 4})) return bad("rgb8_out overlaps the input");
  return PT_OK;
}

template <int TONE, int MODE>
void encode_launch(bool vec, dim3 grid, hipStream_t st, const EncodeArgs& a) {
  if (vec) hipLaunchKernelGGL((encode_kernel<TONE, MODE, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((encode_kernel<TONE, MODE, false>), grid, dim3(256), 0, st, a);
}
template <int TONE>
void encode_launch(int mode, bool vec, dim3 grid, hipStream_t st, const EncodeArgs& a) {
  if (mode == ENC_DITHER) encode_launch<TONE, ENC_DITHER>(vec, grid, st, a);
  else if (mode == ENC_SRGB) encode_launch<TONE, ENC_SRGB>(vec, grid, st, a);
  else encode_launch<TONE, ENC_REFERENCE>(vec, grid, st, a);
}

// The launch of a checked call; tone: ENCODE_PLAIN (pt_encode) or display_params' tone (pt_display_encode).
int encode_run(const PtEncodeParams* p, int tone, EncodeArgs a, hipStream_t st) {
  const int mode = p->transfer == PT_TRANSFER_REFERENCE ? ENC_REFERENCE : (p->flags & PT_ENCODE_DITHER) ? ENC_DITHER : ENC_SRGB;
  a.width = p->width; a.height = p->height;
  a.phase_x = (unsigned)p->phase_x & 7u; a.phase_y = (unsigned)p->phase_y & 7u;
  // four values per lane where the rows and the planes allow 16-byte loads and 4-byte stores
  const bool vec = !(p->flags & PT_ENCODE_NO_VEC) && p->width % 4 == 0 && ((uintptr_t)a.src & 15) == 0 && ((uintptr_t)a.rgb8 & 3) == 0;
  const long long row_items = vec ? 3ll * p->width / 4 : 3ll * p->width;
  const unsigned gx = (unsigned)((row_items + 255) / 256);
  const dim3 grid(gx, (unsigned)std::min<int64_t>(p->height, std::max<int64_t>(1, PT_ENCODE_MAX_BLOCKS / gx)));
  const auto lock = g_last_encode.begin();
  if (tone == PT_TONE_REINHARD) encode_launch<PT_TONE_REINHARD>(mode, vec, grid, st, a);
  else if (tone == PT_TONE_ACES) encode_launch<PT_TONE_ACES>(mode, vec, grid, st, a);
  else if (tone == PT_TONE_REFERENCE) encode_launch<PT_TONE_REFERENCE>(mode, vec, grid, st, a);
  else encode_launch<ENCODE_PLAIN>(mode, vec, grid, st, a);
  PT_HIP(hipGetLastError());
  const int32_t words[8] = {vec ? 2 : 1, (int32_t)grid.x, (int32_t)grid.y, vec ? 4 : 1, p->transfer + 1, tone != ENCODE_PLAIN,
                            (p->flags & PT_ENCODE_DITHER) != 0, 0};
  std::memcpy(g_last_encode.words, words, sizeof words);
  return PT_OK;
}
} // namespace

extern "C" {

void pt_encode_params_init(PtEncodeParams* params, int32_t width, int32_t height) {
  if (!init_params(params)) return;
  params->width = width; params->height = height;
  params->transfer = PT_ENCODE_DEFAULT_TRANSFER;
  params->flags = PT_ENCODE_DEFAULT_FLAGS;
}

int pt_encode(const PtEncodeParams* params, const float* linear, uint8_t* rgb8_out, void* stream) {
  const Refuse bad{"pt_encode"};
  if (!params || !linear || !rgb8_out) return bad("NULL params, linear or rgb8_out");
  if (!is_ours(params)) return bad("PtEncodeParams.struct_size is not this library's");
  if (params->width <= 0 || params->height <= 0) return bad("width and height must be > 0");
  if (const int rc = encode_check(bad, params, linear, rgb8_out)) return rc;
  EncodeArgs a{};
  a.src = linear; a.rgb8 = rgb8_out;
  return encode_run(params, ENCODE_PLAIN, a, (hipStream_t)stream);
}

int pt_display_encode(const PtDisplay* state, const PtDisplayParams* display_params, const PtEncodeParams* encode_params, const float* color,
                      uint8_t* rgb8_out, void* stream) {
  const Refuse bad{"pt_display_encode"};
  if (!encode_params || !rgb8_out) return bad("NULL encode_params or rgb8_out");
  if (!is_ours(encode_params)) return bad("PtEncodeParams.struct_size is not this library's");
  float iw2 = 0.0f;
  if (const int rc = display_check("pt_display_encode", display_params, color, encode_params->width, encode_params->height, &iw2)) return rc;
  if (const int rc = encode_check(bad, encode_params, color, rgb8_out)) return rc;
  EncodeArgs a{};
  a.src = color; a.rgb8 = rgb8_out;
  a.state = state ? state->words.p : nullptr;
  a.ev = std::fmin(std::fmax(display_params->ev_bias, -32.0f), 32.0f); // pt_display_apply's
  a.iw2 = iw2;
  return encode_run(encode_params, display_params->tone, a, (hipStream_t)stream);
}

int pt_debug_last_encode(int32_t out[8]) { return g_last_encode.copy_out("pt_debug_last_encode", out); }

// ---- progressive rendering: sample windows into a PtAccum (include/pt_render.h) ------------------------------------------------
} // extern "C"

struct PtAccum {
  const PtScene* scene = nullptr;
  PtRenderParams p{};           // the frame (samples: unused)
  int local_tiles = 0;
  size_t fb_floats = 0, rng_words = 0;
  DevBuf<float> sum;            // plain radiance sums, pt_render's framebuffer layout
  DevBuf<unsigned int> rng;     // generator state per local pixel (ws_rng's indexing)
  DevBuf<int> order;            // heaviest-first tile order of the last probed window (never the scene's ws_order)
  DevBuf<int> nsplit;           // ... and the cooperative kernels' split decided with it
  bool has_order = false;
  int32_t done = 0;             // samples the state holds (host-side count; adaptive: the unmasked windows' samples)
  bool cam_bound = false;
  PtCamera cam{};
  // adaptive accumulators (pt_adaptive_create): per-pixel counts and half A, in the frame buffer's layout without the channel
  bool adaptive = false;
  size_t pixels = 0;            // P = fb_floats / 3
  DevBuf<float> half;           // H: radiance sum of half A (fb_floats)
  DevBuf<float> prev;           // the sums before the next window (fb_floats): its contribution for the bookkeeping ...
  bool prev_synced = false;     // ... equal to `sum` (the bookkeeping pass keeps it so; otherwise a window copies it first)
  DevBuf<int> cnt;              // n per pixel
  DevBuf<int> cnt_a;            // a per pixel: samples in half A
  DevBuf<uint8_t> tile_on;      // masked windows: per local tile, holds an active pixel ...
  DevBuf<int> active;           // ... the active tiles in dequeue order ...
  DevBuf<int> n_active;         // ... and how many (device)
  DevBuf<unsigned long long> n_sel; // pt_adaptive_select's count (device)
  int64_t max_n = 0;            // bound on every pixel's n (host-side; 0: nothing rendered)
};

namespace {
struct AccumHeader { // an exported state's header: 160 bytes, then the sections of state_layout
  uint32_t magic, version;
  int32_t width, height, depth, shard_index, shard_count;
  uint32_t flags;
  int32_t samples_done, camera_bound;
  int32_t reserved[6];
  PtCamera cam;
};
static_assert(sizeof(AccumHeader) == PT_ACCUM_HEADER_BYTES, "pt_render.h: PT_ACCUM_HEADER_BYTES");

// the frame of a PtAccum: pt_render's parameter checks with `samples` ignored, and no single-stream executor (no per-pixel state)
int accum_params(const PtRenderParams* p, PtRenderParams& q) {
  if (!p) return fail(PT_ERR_INVALID_ARG, "pt_accum: render params are NULL");
  q = *p;
  q.samples = 1;
  if (int rc = check_params(&q)) return rc;
  if (q.flags & PT_FLAG_SINGLE_STREAM) return fail(PT_ERR_INVALID_ARG, "pt_accum: PT_FLAG_SINGLE_STREAM has one global stream and no per-pixel state to resume");
  return PT_OK;
}

// THE description of an exported state: after the header, in order — format PT_ACCUM_FORMAT: the sums (float), the generator states (u32);
// PT_ADAPTIVE_FORMAT: the same, then half A (float), n and a (i32).  `at` counts from the start of the state; `dev` is the accumulator's
// array (NULL without one, and for the arrays a plain accumulator does not have).
struct StateSection { void* dev; size_t bytes, at; };
enum { SEC_SUM, SEC_RNG, SEC_HALF, SEC_N, SEC_A }; // their order
struct StateLayout {
  int n = 0;
  StateSection s[5];
  size_t bytes = sizeof(AccumHeader); // of the whole state
};
StateLayout state_layout(const PtRenderParams& q, uint32_t format, const PtAccum* acc = nullptr) {
  const size_t F = (size_t)pt_framebuffer_floats(&q) * sizeof(float), R = (size_t)pt_shard_tiles(&q) * PT_TILE_PIXELS * sizeof(unsigned int);
  const size_t P = F / 3; // one i32 per pixel of the frame buffer's layout
  StateLayout l;
  auto add = [&](void* dev, size_t bytes) { l.s[l.n++] = {dev, bytes, l.bytes}; l.bytes += bytes; };
  add(acc ? acc->sum.p : nullptr, F);
  add(acc ? acc->rng.p : nullptr, R);
  if (format == PT_ADAPTIVE_FORMAT) {
    add(acc ? acc->half.p : nullptr, F);
    add(acc ? acc->cnt.p : nullptr, P);
    add(acc ? acc->cnt_a.p : nullptr, P);
  }
  return l;
}

// the header of the accumulator's state, in its own format
AccumHeader header_of(const PtAccum* acc) {
  AccumHeader h;
  std::memset(&h, 0, sizeof h);
  h.magic = PT_ACCUM_MAGIC; h.version = acc->adaptive ? PT_ADAPTIVE_FORMAT : PT_ACCUM_FORMAT;
  h.width = acc->p.width; h.height = acc->p.height; h.depth = acc->p.depth;
  h.shard_index = acc->p.shard_index; h.shard_count = acc->p.shard_count; h.flags = acc->p.flags;
  h.samples_done = acc->done; h.camera_bound = acc->cam_bound ? 1 : 0;
  h.cam = acc->cam;
  return h;
}

// that header, then every section of the format, device to host (pt_accum_export / pt_adaptive_export: `host` holds the layout's bytes)
int export_state(const PtAccum* acc, void* host, hipStream_t st) {
  const AccumHeader h = header_of(acc);
  std::memcpy(host, &h, sizeof h);
  const StateLayout l = state_layout(acc->p, h.version, acc);
  for (int k = 0; k < l.n; k++) PT_HIP(hipMemcpyAsync((char*)host + l.s[k].at, l.s[k].dev, l.s[k].bytes, hipMemcpyDeviceToHost, st));
  PT_HIP(hipStreamSynchronize(st));
  return PT_OK;
}

// a state's header against the accumulator it is imported into: magic, a format `who` accepts (an adaptive accumulator: both), the
// size of that format, the frame parameters
int check_header(const AccumHeader& h, const PtAccum* acc, int64_t bytes, const char* who) {
  if (h.magic != PT_ACCUM_MAGIC || (h.version != PT_ACCUM_FORMAT && !(acc->adaptive && h.version == PT_ADAPTIVE_FORMAT)))
    return fail(PT_ERR_INVALID_ARG, std::string(who) + ": not an exported accumulator state (magic / format version)");
  if (bytes != (int64_t)state_layout(acc->p, h.version).bytes)
    return fail(PT_ERR_INVALID_ARG, std::string(who) + ": the state's size does not fit its format and this accumulator's frame");
  if (h.width != acc->p.width || h.height != acc->p.height || h.depth != acc->p.depth || h.shard_index != acc->p.shard_index ||
      h.shard_count != acc->p.shard_count || h.flags != acc->p.flags)
    return fail(PT_ERR_INVALID_ARG, std::string(who) + ": the state was exported from an accumulator with other frame parameters");
  return PT_OK;
}

// the triangle-pool kernels' candidate cache for every lane they can launch (launch_render would otherwise grow it on a window)
int reserve_tricache(const PtScene* s, uint32_t flags) {
  if (s->tri_pooled <= 0 || s->knobs.no_tri_cache || (flags & PT_FLAG_FORCE_STREAM)) return PT_OK;
  int per_cu = occupancy_of(s, (const void*)tripool_kernel(uv_of(s), (flags & PT_FLAG_FAST_RNG) != 0).kernel, kBlock, 0);
  if (per_cu < 0) return PT_ERR_HIP;
  if (s->knobs.blocks_per_cu) per_cu = std::min(per_cu, s->knobs.blocks_per_cu);
  return grow_tricache(s, (size_t)std::max(1, per_cu) * (size_t)std::max(1, s->num_cus) * kBlock);
}
} // namespace

extern "C" {

int64_t pt_accum_state_bytes(const PtRenderParams* p) {
  PtRenderParams q;
  if (accum_params(p, q)) return -1;
  return (int64_t)state_layout(q, PT_ACCUM_FORMAT).bytes;
}

void pt_accum_destroy(PtAccum* acc) { delete acc; } // (its buffers: DevBuf members)

} // extern "C"
namespace {
AFrame frame_of(const PtAccum* acc) {
  AFrame f;
  f.width = acc->p.width; f.height = acc->p.height; f.shard_index = acc->p.shard_index; f.shard_count = acc->p.shard_count;
  f.n_tiles = n_tiles_of(&acc->p, &f.tiles_x);
  f.pixels = (long long)acc->pixels;
  return f;
}
unsigned int blocks_of(long long n) { return (unsigned int)std::max<long long>(1, (n + 255) / 256); }

// an adaptive accumulator at 0 samples: sums, H, n, a zeroed; every generator state the pixel's seed
int adaptive_clear(PtAccum* acc, hipStream_t st) {
  PT_HIP(hipMemsetAsync(acc->sum.p, 0, acc->fb_floats * sizeof(float), st));
  PT_HIP(hipMemsetAsync(acc->half.p, 0, acc->fb_floats * sizeof(float), st));
  PT_HIP(hipMemsetAsync(acc->prev.p, 0, acc->fb_floats * sizeof(float), st));
  acc->prev_synced = true;
  PT_HIP(hipMemsetAsync(acc->cnt.p, 0, std::max<size_t>(acc->pixels, 1) * sizeof(int), st));
  PT_HIP(hipMemsetAsync(acc->cnt_a.p, 0, std::max<size_t>(acc->pixels, 1) * sizeof(int), st));
  if (acc->rng_words) {
    hipLaunchKernelGGL(adaptive_seed_kernel, dim3(blocks_of((long long)acc->rng_words)), dim3(256), 0, st, frame_of(acc), acc->rng.p, (long long)acc->rng_words);
    PT_HIP(hipGetLastError());
  }
  acc->max_n = 0;
  return PT_OK;
}

int accum_create(const PtScene* scene, const PtRenderParams* p, PtAccum** out, bool adaptive) {
  const char* who = adaptive ? "pt_adaptive_create" : "pt_accum_create";
  if (!out) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": out is NULL");
  *out = nullptr;
  if (!scene) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": NULL scene");
  PtRenderParams q;
  if (int rc = accum_params(p, q)) return rc;
  if (adaptive && (q.flags & PT_FLAG_FAST_RNG)) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_create: PT_FLAG_FAST_RNG is not offered for adaptive sampling");
  int cur = -1;
  PT_HIP(hipGetDevice(&cur));
  if (cur != scene->device) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": the scene lives on another device");
  std::unique_ptr<PtAccum> owner(new PtAccum()); // (an early return frees what was allocated so far)
  PtAccum* const acc = owner.get();
  acc->scene = scene;
  acc->p = q;
  acc->adaptive = adaptive;
  acc->local_tiles = std::max(0, local_tiles_of(&q));
  acc->fb_floats = (size_t)pt_framebuffer_floats(&q);
  acc->rng_words = (size_t)pt_shard_tiles(&q) * PT_TILE_PIXELS;
  auto bad = [&](hipError_t e, const char* what) { return fail(PT_ERR_HIP, std::string(who) + ": " + what + ": " + hipGetErrorString(e)); };
  hipError_t e = hipSuccess; // (a failed allocation: the others are still tried, the last failure is reported)
  for (hipError_t r : {acc->sum.alloc(acc->fb_floats), acc->rng.alloc(acc->rng_words), acc->order.alloc((size_t)acc->local_tiles), acc->nsplit.alloc(2)})
    if (r != hipSuccess) e = r;
  if (e != hipSuccess) return bad(e, "hipMalloc");
  if ((e = hipMemset(acc->sum.p, 0, acc->fb_floats * sizeof(float))) != hipSuccess) return bad(e, "hipMemset");
  if ((e = hipMemset(acc->rng.p, 0, std::max<size_t>(acc->rng_words, 1) * sizeof(unsigned int))) != hipSuccess) return bad(e, "hipMemset");
  if (adaptive) {
    acc->pixels = acc->fb_floats / 3;
    const size_t T = (size_t)acc->local_tiles;
    for (hipError_t r : {acc->half.alloc(acc->fb_floats), acc->prev.alloc(acc->fb_floats), acc->cnt.alloc(acc->pixels), acc->cnt_a.alloc(acc->pixels),
                         acc->tile_on.alloc(T), acc->active.alloc(T), acc->n_active.alloc(1), acc->n_sel.alloc(1)})
      if (r != hipSuccess) e = r;
    if (e != hipSuccess) return bad(e, "hipMalloc");
    if (int rc = adaptive_clear(acc, nullptr)) return rc;
  }
  // The clears above run on the null stream, and neither hipMemset nor hipMemsetAsync has finished when it returns: the first window may
  // be queued on a non-blocking stream, which does not wait for the null stream — a clear still pending there would land on its sums.
  if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) return bad(e, "hipStreamSynchronize");
  {
    // the scene's launch workspaces a window uses (probe costs, tile ranks; the candidate cache): sized now, not by a window
    std::lock_guard<std::mutex> lock(scene->sched);
    int rc = acc->local_tiles > 0 ? reserve_tiles(scene, acc->local_tiles) : PT_OK;
    if (!rc) rc = reserve_tricache(scene, q.flags);
    if (rc) return rc;
  }
  *out = owner.release();
  return PT_OK;
}
} // namespace
extern "C" {

int pt_accum_create(const PtScene* scene, const PtRenderParams* p, PtAccum** out) { return accum_create(scene, p, out, false); }

int pt_accum_reset(PtAccum* acc, void* stream) {
  if (!acc) return fail(PT_ERR_INVALID_ARG, "pt_accum_reset: NULL accumulator");
  if (acc->adaptive) { if (int rc = adaptive_clear(acc, (hipStream_t)stream)) return rc; }
  else PT_HIP(hipMemsetAsync(acc->sum.p, 0, acc->fb_floats * sizeof(float), (hipStream_t)stream));
  acc->done = 0;
  acc->cam_bound = false;
  acc->has_order = false;
  return PT_OK;
}

int32_t pt_accum_samples(const PtAccum* acc) { return acc ? acc->done : -1; }

int pt_render_accumulate(PtAccum* acc, const PtCamera* cam, int32_t samples, void* stream) {
  if (!acc || !cam) return fail(PT_ERR_INVALID_ARG, "pt_render_accumulate: NULL argument");
  if (acc->adaptive) return pt_adaptive_window(acc, cam, samples, nullptr, stream);
  if (samples <= 0) return fail(PT_ERR_INVALID_ARG, "pt_render_accumulate: samples must be > 0");
  if ((int64_t)acc->done + samples > (int64_t)INT32_MAX) return fail(PT_ERR_INVALID_ARG, "pt_render_accumulate: the total would pass INT32_MAX samples");
  if (acc->cam_bound && std::memcmp(&acc->cam, cam, sizeof(PtCamera)) != 0)
    return fail(PT_ERR_INVALID_ARG, "pt_render_accumulate: the camera differs from the one the accumulator's first window was rendered with");
  if ((acc->p.flags & PT_FLAG_FAST_RNG) && acc->done % PT_FAST_CHUNK_SPP != 0)
    return fail(PT_ERR_INVALID_ARG, "pt_render_accumulate: PT_FLAG_FAST_RNG windows start on a multiple of PT_FAST_CHUNK_SPP samples (the last window ended off one)");
  PtRenderParams q = acc->p;
  q.samples = samples;
  Window w{acc->done, acc->rng.p, acc->order.p, acc->nsplit.p, &acc->has_order};
  if (int rc = launch_render(acc->scene, cam, &q, acc->sum.p, (hipStream_t)stream, &w)) return rc;
  acc->done += samples;
  if (!acc->cam_bound) { acc->cam = *cam; acc->cam_bound = true; }
  return PT_OK;
}

int pt_accum_resolve(const PtAccum* acc, float* fb_device, void* stream) {
  if (!acc || !fb_device) return fail(PT_ERR_INVALID_ARG, "pt_accum_resolve: NULL argument");
  if (acc->adaptive ? acc->max_n <= 0 : acc->done <= 0) return fail(PT_ERR_INVALID_ARG, "pt_accum_resolve: no samples rendered yet");
  const long long n = (long long)acc->fb_floats;
  // (adaptive: each pixel by its own count)
  hipLaunchKernelGGL(accum_resolve_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, acc->sum.p, acc->adaptive ? acc->cnt.p : nullptr,
                     (int)acc->done, fb_device, n);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

int pt_accum_tonemap_rgb8(const PtAccum* acc, uint8_t* rgb8_device, void* stream) {
  if (!acc || !rgb8_device) return fail(PT_ERR_INVALID_ARG, "pt_accum_tonemap_rgb8: NULL argument");
  if (acc->adaptive ? acc->max_n <= 0 : acc->done <= 0) return fail(PT_ERR_INVALID_ARG, "pt_accum_tonemap_rgb8: no samples rendered yet");
  if (acc->p.shard_count != 1) return fail(PT_ERR_INVALID_ARG, "pt_accum_tonemap_rgb8: whole frames only (shard_count == 1)");
  dim3 block(256), grid((acc->p.width + 255) / 256, acc->p.height);
  hipLaunchKernelGGL(tonemap_kernel<true>, grid, block, 0, (hipStream_t)stream, acc->sum.p, acc->adaptive ? acc->cnt.p : nullptr, (int)acc->done,
                     rgb8_device, acc->p.width, acc->p.height);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

int pt_accum_export(const PtAccum* acc, void* host, int64_t bytes, void* stream) {
  if (!acc || !host) return fail(PT_ERR_INVALID_ARG, "pt_accum_export: NULL argument");
  if (acc->adaptive) return fail(PT_ERR_INVALID_ARG, "pt_accum_export: an adaptive accumulator exports with pt_adaptive_export");
  if (bytes != pt_accum_state_bytes(&acc->p)) return fail(PT_ERR_INVALID_ARG, "pt_accum_export: the buffer is not pt_accum_state_bytes() long");
  return export_state(acc, host, (hipStream_t)stream);
}

int pt_accum_import(PtAccum* acc, const void* host, int64_t bytes, void* stream) {
  if (!acc || !host) return fail(PT_ERR_INVALID_ARG, "pt_accum_import: NULL argument");
  if (acc->adaptive) return fail(PT_ERR_INVALID_ARG, "pt_accum_import: an adaptive accumulator imports with pt_adaptive_import");
  if (bytes != pt_accum_state_bytes(&acc->p)) return fail(PT_ERR_INVALID_ARG, "pt_accum_import: the state is not pt_accum_state_bytes() long for this accumulator");
  AccumHeader h;
  std::memcpy(&h, host, sizeof h);
  if (int rc = check_header(h, acc, bytes, "pt_accum_import")) return rc;
  if (h.samples_done < 0 || (h.camera_bound != 0) != (h.samples_done > 0)) return fail(PT_ERR_INVALID_ARG, "pt_accum_import: inconsistent header");
  const hipStream_t st = (hipStream_t)stream;
  const StateLayout l = state_layout(acc->p, h.version, acc);
  for (int k = 0; k < l.n; k++) PT_HIP(hipMemcpyAsync(l.s[k].dev, (const char*)host + l.s[k].at, l.s[k].bytes, hipMemcpyHostToDevice, st));
  PT_HIP(hipStreamSynchronize(st)); // (the caller's buffer may go as soon as this returns)
  acc->done = h.samples_done;
  acc->cam_bound = h.camera_bound != 0;
  acc->cam = h.cam;
  acc->has_order = false; // (the next window long enough to probe orders the tiles again)
  return PT_OK;
}

// ---- adaptive sampling: per-pixel sample counts (include/pt_render.h) ----------------------------------------------------------
int pt_adaptive_create(const PtScene* scene, const PtRenderParams* p, PtAccum** out) { return accum_create(scene, p, out, true); }

int64_t pt_adaptive_state_bytes(const PtRenderParams* p) {
  PtRenderParams q;
  if (accum_params(p, q) || (q.flags & PT_FLAG_FAST_RNG)) return -1;
  return (int64_t)state_layout(q, PT_ADAPTIVE_FORMAT).bytes;
}

static int adaptive_only(const PtAccum* acc, const char* who) {
  if (!acc) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": NULL accumulator");
  if (!acc->adaptive) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": not an adaptive accumulator (pt_adaptive_create)");
  return PT_OK;
}

int pt_adaptive_window(PtAccum* acc, const PtCamera* cam, int32_t samples, const uint8_t* mask_device, void* stream) {
  if (int rc = adaptive_only(acc, "pt_adaptive_window")) return rc;
  if (!cam) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_window: NULL camera");
  if (samples <= 0) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_window: samples must be > 0");
  // (the kernels count a window from a nominal start of 1: see below)
  if (acc->max_n + samples > (int64_t)INT32_MAX || samples >= INT32_MAX)
    return fail(PT_ERR_INVALID_ARG, "pt_adaptive_window: a pixel's total could pass INT32_MAX samples");
  if (acc->cam_bound && std::memcmp(&acc->cam, cam, sizeof(PtCamera)) != 0)
    return fail(PT_ERR_INVALID_ARG, "pt_adaptive_window: the camera differs from the one the accumulator's first window was rendered with");
  const hipStream_t st = (hipStream_t)stream;
  const AFrame f = frame_of(acc);
  // Every window resumes from the state (pt_adaptive_create seeded it), whatever its pixels' counts: the kernels read the sample index
  // only to stop and for the chain-priority poll, so a window runs from a nominal start of 1 to 1 + samples (with done = 0 it would seed).
  Window w{1, acc->rng.p, acc->order.p, acc->nsplit.p, &acc->has_order};
  if (mask_device) {
    if (acc->local_tiles <= 0) return PT_OK;
    hipLaunchKernelGGL(adaptive_tiles_kernel, dim3(blocks_of(acc->local_tiles)), dim3(256), 0, st, f, mask_device, acc->local_tiles, acc->tile_on.p);
    PT_HIP(hipGetLastError());
    hipLaunchKernelGGL(adaptive_compact_kernel, dim3(1), dim3(1024), 0, st, acc->tile_on.p, acc->has_order ? acc->order.p : nullptr, acc->local_tiles,
                       acc->active.p, acc->n_active.p);
    PT_HIP(hipGetLastError());
    int n_active = 0;
    PT_HIP(hipMemcpyAsync(&n_active, acc->n_active.p, sizeof(int), hipMemcpyDeviceToHost, st));
    PT_HIP(hipStreamSynchronize(st)); // (the launch is sized by the active tiles)
    if (n_active <= 0) return PT_OK;  // an empty mask: nothing to render
    w.mask = mask_device; w.active = acc->active.p; w.n_active = n_active;
  }
  PtRenderParams q = acc->p;
  q.samples = samples;
  // S before the window is `prev`, which the last bookkeeping pass left equal to the sums (copied here only where none ran since)
  if (!acc->prev_synced) PT_HIP(hipMemcpyAsync(acc->prev.p, acc->sum.p, acc->fb_floats * sizeof(float), hipMemcpyDeviceToDevice, st));
  acc->prev_synced = false;
  if (int rc = launch_render(acc->scene, cam, &q, acc->sum.p, st, &w)) return rc;
  hipLaunchKernelGGL(adaptive_book_kernel, dim3(blocks_of(f.pixels)), dim3(256), 0, st, f, mask_device, acc->sum.p, acc->prev.p, acc->half.p,
                     acc->cnt.p, acc->cnt_a.p, (int)samples);
  PT_HIP(hipGetLastError());
  acc->prev_synced = true;
  if (!mask_device) acc->done += samples;
  acc->max_n += samples;
  if (!acc->cam_bound) { acc->cam = *cam; acc->cam_bound = true; }
  return PT_OK;
}

// A new image that continues every pixel's stream: pt_accum_reset without the re-seeding.  Every window of an adaptive accumulator
// resumes from the stored state, so this is memsets and host bookkeeping: no kernel.
int pt_adaptive_next_frame(PtAccum* acc, void* stream) {
  if (int rc = adaptive_only(acc, "pt_adaptive_next_frame")) return rc;
  const hipStream_t st = (hipStream_t)stream;
  PT_HIP(hipMemsetAsync(acc->sum.p, 0, acc->fb_floats * sizeof(float), st));
  PT_HIP(hipMemsetAsync(acc->half.p, 0, acc->fb_floats * sizeof(float), st));
  PT_HIP(hipMemsetAsync(acc->prev.p, 0, acc->fb_floats * sizeof(float), st));
  acc->prev_synced = true;
  PT_HIP(hipMemsetAsync(acc->cnt.p, 0, std::max<size_t>(acc->pixels, 1) * sizeof(int), st));
  PT_HIP(hipMemsetAsync(acc->cnt_a.p, 0, std::max<size_t>(acc->pixels, 1) * sizeof(int), st));
  acc->max_n = 0;
  acc->done = 0;
  acc->cam_bound = false;
  acc->has_order = false;
  return PT_OK;
}

int pt_adaptive_counts(const PtAccum* acc, int32_t* counts_device, void* stream) {
  if (int rc = adaptive_only(acc, "pt_adaptive_counts")) return rc;
  if (!counts_device) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_counts: NULL argument");
  PT_HIP(hipMemcpyAsync(counts_device, acc->cnt.p, acc->pixels * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return PT_OK;
}

int pt_adaptive_error(const PtAccum* acc, float* err_device, void* stream) {
  if (int rc = adaptive_only(acc, "pt_adaptive_error")) return rc;
  if (!err_device) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_error: NULL argument");
  const AFrame f = frame_of(acc);
  hipLaunchKernelGGL(adaptive_error_kernel, dim3(blocks_of(f.pixels)), dim3(256), 0, (hipStream_t)stream, f, acc->sum.p, acc->half.p, acc->cnt.p, acc->cnt_a.p, err_device);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

int pt_variance_estimate(const PtAccum* acc, float* variance_device, void* stream) {
  if (int rc = adaptive_only(acc, "pt_variance_estimate")) return rc;
  if (!variance_device) return fail(PT_ERR_INVALID_ARG, "pt_variance_estimate: NULL argument");
  if (acc->max_n <= 0) return fail(PT_ERR_INVALID_ARG, "pt_variance_estimate: no samples rendered yet");
  const AFrame f = frame_of(acc);
  hipLaunchKernelGGL(variance_estimate_kernel, dim3(blocks_of(f.pixels)), dim3(256), 0, (hipStream_t)stream, f, acc->sum.p, acc->half.p, acc->cnt.p,
                     acc->cnt_a.p, variance_device);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

int pt_adaptive_select(const PtAccum* acc, float threshold, int32_t min_spp, int32_t max_spp, uint32_t flags, uint8_t* mask_device,
                       int64_t* n_active, void* stream) {
  if (int rc = adaptive_only(acc, "pt_adaptive_select")) return rc;
  if (!mask_device || !n_active) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_select: NULL argument");
  if (flags & ~PT_ADAPTIVE_DILATE) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_select: unknown flags");
  if ((flags & PT_ADAPTIVE_DILATE) && acc->p.shard_count != 1)
    return fail(PT_ERR_INVALID_ARG, "pt_adaptive_select: PT_ADAPTIVE_DILATE needs whole frames (a shard's neighbours are other shards' pixels)");
  const hipStream_t st = (hipStream_t)stream;
  const AFrame f = frame_of(acc);
  PT_HIP(hipMemsetAsync(acc->n_sel.p, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(adaptive_select_kernel, dim3(blocks_of(f.pixels)), dim3(256), 0, st, f, acc->sum.p, acc->half.p, acc->cnt.p, acc->cnt_a.p, threshold,
                     (int)min_spp, (int)max_spp, (flags & PT_ADAPTIVE_DILATE) ? 1 : 0, mask_device, acc->n_sel.p);
  PT_HIP(hipGetLastError());
  unsigned long long n = 0;
  PT_HIP(hipMemcpyAsync(&n, acc->n_sel.p, sizeof n, hipMemcpyDeviceToHost, st));
  PT_HIP(hipStreamSynchronize(st));
  *n_active = (int64_t)n;
  return PT_OK;
}

int pt_adaptive_export(const PtAccum* acc, void* host, int64_t bytes, void* stream) {
  if (int rc = adaptive_only(acc, "pt_adaptive_export")) return rc;
  if (!host) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_export: NULL argument");
  if (bytes != pt_adaptive_state_bytes(&acc->p)) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_export: the buffer is not pt_adaptive_state_bytes() long");
  return export_state(acc, host, (hipStream_t)stream);
}

int pt_adaptive_import(PtAccum* acc, const void* host, int64_t bytes, void* stream) {
  if (int rc = adaptive_only(acc, "pt_adaptive_import")) return rc;
  if (!host) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_import: NULL argument");
  if (bytes < (int64_t)sizeof(AccumHeader)) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_import: shorter than a state header");
  AccumHeader h;
  std::memcpy(&h, host, sizeof h);
  if (int rc = check_header(h, acc, bytes, "pt_adaptive_import")) return rc;
  const bool plain = h.version == PT_ACCUM_FORMAT;
  const StateLayout l = state_layout(acc->p, h.version, acc); // (a plain state: the sums and the generator states)
  const char* in = (const char*)host;
  const AFrame f = frame_of(acc);
  std::vector<int> n, na;
  int64_t max_n = 0;
  if (plain) { // upgrade: every pixel of the frame at samples_done, nothing in half A
    if (h.samples_done < 0 || (h.camera_bound != 0) != (h.samples_done > 0)) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_import: inconsistent header");
    n.assign(acc->pixels, 0);
    for (size_t i = 0; i < acc->pixels; i++) { int x, y; if (aframe_xy(f, (long long)i, x, y)) n[i] = h.samples_done; }
    na.assign(acc->pixels, 0);
    max_n = h.samples_done;
  } else {
    n.resize(acc->pixels); na.resize(acc->pixels);
    std::memcpy(n.data(), in + l.s[SEC_N].at, l.s[SEC_N].bytes);
    std::memcpy(na.data(), in + l.s[SEC_A].at, l.s[SEC_A].bytes);
    int64_t min_n = INT32_MAX;
    for (size_t i = 0; i < acc->pixels; i++) {
      if (na[i] < 0 || na[i] > n[i]) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_import: a pixel's counts are not 0 <= a <= n");
      int x, y;
      if (aframe_xy(f, (long long)i, x, y)) min_n = std::min<int64_t>(min_n, n[i]);
      max_n = std::max<int64_t>(max_n, n[i]);
    }
    if (h.samples_done < 0 || (acc->pixels && h.samples_done > min_n) || (h.camera_bound != 0) != (max_n > 0))
      return fail(PT_ERR_INVALID_ARG, "pt_adaptive_import: inconsistent header");
  }
  const hipStream_t st = (hipStream_t)stream;
  PT_HIP(hipMemcpyAsync(acc->sum.p, in + l.s[SEC_SUM].at, l.s[SEC_SUM].bytes, hipMemcpyHostToDevice, st));
  if (plain && h.samples_done == 0) { // (a plain state at 0 samples holds no generator states: the seeds)
    if (acc->rng_words) {
      hipLaunchKernelGGL(adaptive_seed_kernel, dim3(blocks_of((long long)acc->rng_words)), dim3(256), 0, st, f, acc->rng.p, (long long)acc->rng_words);
      PT_HIP(hipGetLastError());
    }
  } else {
    PT_HIP(hipMemcpyAsync(acc->rng.p, in + l.s[SEC_RNG].at, l.s[SEC_RNG].bytes, hipMemcpyHostToDevice, st));
  }
  if (plain) PT_HIP(hipMemsetAsync(acc->half.p, 0, acc->fb_floats * sizeof(float), st));
  else PT_HIP(hipMemcpyAsync(acc->half.p, in + l.s[SEC_HALF].at, l.s[SEC_HALF].bytes, hipMemcpyHostToDevice, st));
  PT_HIP(hipMemcpyAsync(acc->cnt.p, n.data(), acc->pixels * sizeof(int), hipMemcpyHostToDevice, st));
  PT_HIP(hipMemcpyAsync(acc->cnt_a.p, na.data(), acc->pixels * sizeof(int), hipMemcpyHostToDevice, st));
  PT_HIP(hipStreamSynchronize(st)); // (the caller's buffer and the host counts may go as soon as this returns)
  acc->done = h.samples_done;
  acc->max_n = max_n;
  acc->cam_bound = h.camera_bound != 0;
  acc->cam = h.cam;
  acc->has_order = false;
  acc->prev_synced = false; // (the next window copies the imported sums)
  return PT_OK;
}

#ifdef PT_BIN_DEBUG
extern "C" int pt_debug_bin_fallbacks(unsigned int* out) { // -DPT_BIN_DEBUG: per generation (rays, waves) that scanned the pooled run in full
  PT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bin_fb), 4096 * sizeof(unsigned int)));
  return PT_OK;
}
#endif
#ifdef PT_STAMPS_BLOCKS
extern "C" int pt_debug_blocks(unsigned long long* out, int n_blocks) { // -DPT_STAMPS_BLOCKS: (where, start, end) of the last frame launch's workgroups
  PT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_blocks), (size_t)std::min(n_blocks, 8192) * 3 * sizeof(unsigned long long)));
  return PT_OK;
}
#endif
#ifdef PT_STAMPS
int pt_debug_stamps(unsigned long long* out8, int reset) { // diagnostic build only; not part of include/pt_render.h
  if (out8) PT_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_stamps), 8 * sizeof(unsigned long long)));
  if (reset) { unsigned long long z[8] = {0}; PT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof z)); }
  return PT_OK;
}
#ifdef PT_STAMPS_TRI
int pt_debug_tri(unsigned long long* out8, int reset) { // -DPT_STAMPS_TRI: counters of the triangle pool (pt_device.hpp: PT_TRI_COUNT)
  if (out8) PT_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_tri), 16 * sizeof(unsigned long long)));
  if (reset) { unsigned long long z[16] = {0}; PT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_tri), z, sizeof z)); }
  return PT_OK;
}
#endif
#ifdef PT_STAMPS_RUNS
int pt_debug_runs(unsigned long long* out16, int reset) { // -DPT_STAMPS_RUNS: cycles per run of the hittable list (pt_device.hpp: hit_world)
  if (out16) PT_HIP(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_runs), 16 * sizeof(unsigned long long)));
  if (reset) { unsigned long long z[16] = {0}; PT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_runs), z, sizeof z)); }
  return PT_OK;
}
#endif
#ifdef PT_STAMPS_WALK
int pt_debug_walk(unsigned long long* out8, int reset) { // -DPT_STAMPS_WALK: counters of the sphere-grid walk (pt_device.hpp: walk_ctr)
  if (out8) PT_HIP(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_walk), 8 * sizeof(unsigned long long)));
  if (reset) { unsigned long long z[8] = {0}; PT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_walk), z, sizeof z)); }
  return PT_OK;
}
#endif
#endif

// ---- probes: host arrays in/out ------------------------------------------------------------------------

int pt_debug_bounce(const PtScene* scene, const PtBounceIn* in, PtBounceOut* out, int32_t n) {
  if (!scene || !in || !out || n < 0) return fail(PT_ERR_INVALID_ARG, "pt_debug_bounce: bad argument");
  if (n == 0) return PT_OK;
  DevBuf<PtBounceIn> din;
  DevBuf<PtBounceOut> dout;
  PT_HIP(din.alloc(n));
  PT_HIP(dout.alloc(n));
  PT_HIP(hipMemcpy(din.p, in, (size_t)n * sizeof(PtBounceIn), hipMemcpyHostToDevice));
  dim3 block(64), grid((n + 63) / 64);
  const bool qw = scene->knobs.grid_walk == 2; // PtTuning.grid_walk = 2: the probe walks sphere grids through the pair queue, like the kernels it stands for
  const auto kernel = scene->track_uv ? (qw ? bounce_kernel<true, 2> : bounce_kernel<true, 1>) : (qw ? bounce_kernel<false, 2> : bounce_kernel<false, 1>);
  hipLaunchKernelGGL(kernel, grid, block, 0, nullptr, scene->blob.p, scene->n_runs, scene->mats, scene->pool.p, scene->atlas.p, din.p, dout.p, n, scene->fast_ok ? 1 : 0);
  PT_HIP(hipGetLastError());
  PT_HIP(hipMemcpy(out, dout.p, (size_t)n * sizeof(PtBounceOut), hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_debug_schedule(const PtScene* scene, int32_t out[2]) {
  if (!scene || !out) return fail(PT_ERR_INVALID_ARG, "pt_debug_schedule: NULL argument");
  out[0] = out[1] = 0;
  PT_HIP(hipDeviceSynchronize());
  std::lock_guard<std::mutex> lock(scene->sched); // last_had_wide_phase / ws_nsplit belong to the launch path
  if (!scene->last_had_wide_phase) return PT_OK;
  int v[2] = {0, 0};
  PT_HIP(hipMemcpy(v, scene->ws_nsplit.p, sizeof v, hipMemcpyDeviceToHost));
  out[0] = v[0]; out[1] = v[0] > 0 ? (1 << v[1]) : 0;
  return PT_OK;
}

int pt_debug_last_launch(const PtScene* scene, int32_t out[4]) {
  if (!scene || !out) return fail(PT_ERR_INVALID_ARG, "pt_debug_last_launch: NULL argument");
  std::lock_guard<std::mutex> lock(scene->sched);
  for (int k = 0; k < 4; k++) out[k] = scene->last_launch[k];
  return PT_OK;
}

int pt_debug_plan_pass(const int64_t facts[20], int32_t out[14]) {
  if (!facts || !out) return fail(PT_ERR_INVALID_ARG, "pt_debug_plan_pass: NULL argument");
  for (int k = 0; k < 20; k++)
    if (k != 11 && (facts[k] < INT32_MIN || facts[k] > INT32_MAX)) return fail(PT_ERR_INVALID_ARG, "pt_debug_plan_pass: a fact does not fit 32 bits");
  if (facts[0] < 1 || facts[0] > 65536 || facts[1] < 1 || facts[1] > 64 || facts[2] < 64 || facts[2] % 64 != 0 || facts[2] > 1024 || facts[11] < 0 ||
      facts[11] > (1ll << 40) || facts[12] < 0 || facts[13] < 1 || facts[18] < 0 || facts[19] < 0)
    return fail(PT_ERR_INVALID_ARG, "pt_debug_plan_pass: need 1 <= CUs <= 65536, 1 <= workgroups per CU <= 64, block threads a multiple of 64 up to 1024, "
                                    "samples >= 1, 0 <= launch units <= 2^40, counts >= 0");
  PtTuning t;
  tuning_defaults(t);
  t.blocks_per_cu = (int32_t)facts[7]; t.lanes_cap = (int32_t)facts[8]; t.heavy_tiles = (int32_t)facts[9]; t.chain_priority = facts[10] ? -1 : 0;
  const Knobs knobs(t); // (the PtTuning fields as a scene resolves them)
  PassFacts f;
  f.num_cus = (int)facts[0]; f.per_cu = (int)facts[1]; f.block_threads = (int)facts[2];
  f.chain_bound = facts[3] != 0; f.use_grid = facts[4] != 0; f.queued_walk = facts[5] != 0;
  f.flags = (uint32_t)facts[6];
  f.blocks_per_cu = knobs.blocks_per_cu; f.lanes_cap = knobs.lanes_cap; f.heavy_tiles = knobs.heavy_tiles; f.no_chain_prio = knobs.no_chain_prio;
  f.launch_units = facts[11]; f.n_local_pixels = (int)facts[12]; f.samples = (int)facts[13];
  f.probe = facts[14] != 0; f.has_order = facts[15] != 0; f.has_split = facts[16] != 0;
  f.tile_granular = facts[17] != 0; f.scatter_p = (int)facts[18]; f.fast_chunks = (int)facts[19];
  const PassPlan pl = plan_pass(f);
  const int words[14] = {pl.workgroups, pl.n_waves_resident, pl.lanes_cap, pl.tile_granular, pl.heavy_pixels, pl.heavy_lanes, pl.prio_onset,
                         pl.prio_t1, pl.prio_t2, pl.prio_t3, pl.last_launch[0], pl.last_launch[1], pl.last_launch[2], pl.last_launch[3]};
  for (int k = 0; k < 14; k++) out[k] = words[k];
  return PT_OK;
}

int pt_debug_last_kernels(const PtScene* scene, int32_t out[24]) {
  if (!scene || !out) return fail(PT_ERR_INVALID_ARG, "pt_debug_last_kernels: NULL argument");
  std::lock_guard<std::mutex> lock(scene->sched);
  for (int pass = 0; pass < 2; pass++)
    for (int k = 0; k < 12; k++) out[12 * pass + k] = scene->last_kernels[pass].w[k];
  return PT_OK;
}

static void pool_plan_words(const PoolPlan& pl, int32_t out[4]) { out[0] = pl.one != 0; out[1] = pl.n; out[2] = pl.x_off; out[3] = pl.oct_off; }

int pt_debug_last_pool_plan(const PtScene* scene, int32_t out[4]) {
  if (!scene || !out) return fail(PT_ERR_INVALID_ARG, "pt_debug_last_pool_plan: NULL argument");
  std::lock_guard<std::mutex> lock(scene->sched);
  pool_plan_words(scene->last_pool_plan, out);
  return PT_OK;
}

int pt_debug_last_pool_word(const PtScene* scene, int32_t* out) {
  if (!scene || !out) return fail(PT_ERR_INVALID_ARG, "pt_debug_last_pool_word: NULL argument");
  std::lock_guard<std::mutex> lock(scene->sched);
  *out = scene->last_pool_plan.one;
  return PT_OK;
}

int pt_debug_pool_plan(const PtSceneDesc* desc, const PtTuning* tuning, const PtRenderParams* params, int32_t out[12]) {
  if (!desc || !params || !out) return fail(PT_ERR_INVALID_ARG, "pt_debug_pool_plan: NULL argument");
  if (int rc = check_params(params)) return rc;
  PtTuning tun;
  std::string err;
  if (int rc = resolve_tuning(tuning, tun, err)) return fail(rc, err);
  ptf::Flat flat;
  if (int rc = flatten_tuned(desc, tun, flat, err)) return fail(rc, err);
  PtScene s; // (never meets a device: facts only)
  set_scene_facts(&s, desc, tun, flat);
  PoolPlan pl = s.pool_plan;
  pl.one = 0;
  int32_t mats = 0, lds = 0;
  // Only the headline family reads the plan, and choosing among its kernels asks the device nothing (no sphere grid: no occupancy query)
  if (s.rectbox_only && s.mats_simple && s.grid_spheres == 0 && s.tri_pooled == 0 && !(params->flags & PT_FLAG_SINGLE_STREAM)) {
    const int local_tiles = local_tiles_of(params);
    const Variant v = choose_variant(&s, params, local_tiles, (params->flags & PT_FLAG_FAST_RNG) != 0, local_tiles * PT_TILE_PIXELS);
    if (v.rc) return v.rc;
    pl = pass_pool_plan(&s, params, v);
    lds = v.tag.w[0] == KFAM_RENDER ? v.tag.w[2] : 0;
    mats = v.tag.w[0] == KFAM_RENDER ? v.tag.w[10] : 0;
  }
  pool_plan_words(pl, out);
  out[4] = pl.pool_off; std::memcpy(&out[5], &pl.bmax, 4);
  out[6] = pl.kind; out[7] = pl.off; out[8] = pl.count;
  out[9] = s.pool_plan.one != 0; out[10] = lds; out[11] = mats;
  return PT_OK;
}

int pt_debug_last_aov(const PtScene* scene, int32_t out[2]) {
  if (!scene || !out) return fail(PT_ERR_INVALID_ARG, "pt_debug_last_aov: NULL argument");
  std::lock_guard<std::mutex> lock(scene->sched);
  out[0] = scene->last_aov[0]; out[1] = scene->last_aov[1];
  return PT_OK;
}

int pt_debug_camera_rays(const PtCamera* cam, int32_t width, int32_t height, const int32_t* xy, const uint32_t* rng_in,
                         PtCameraRay* out, int32_t n) {
  if (!cam || !xy || !rng_in || !out || n < 0 || width <= 0 || height <= 0)
    return fail(PT_ERR_INVALID_ARG, "pt_debug_camera_rays: bad argument");
  if (n == 0) return PT_OK;
  DevBuf<int32_t> dxy;
  DevBuf<uint32_t> drng;
  DevBuf<PtCameraRay> dout;
  PT_HIP(dxy.alloc((size_t)n * 2));
  PT_HIP(drng.alloc(n));
  PT_HIP(dout.alloc(n));
  PT_HIP(hipMemcpy(dxy.p, xy, (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice));
  PT_HIP(hipMemcpy(drng.p, rng_in, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
  Cam c;
  std::memcpy(&c, cam, sizeof c);
  hipLaunchKernelGGL(camera_rays_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, c, width, height, dxy.p, drng.p, dout.p, n);
  PT_HIP(hipGetLastError());
  PT_HIP(hipMemcpy(out, dout.p, (size_t)n * sizeof(PtCameraRay), hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_debug_math(int32_t op, const float* a, const float* b, float* out, int64_t n) {
  if (!a || !out || n < 0 || op < 0 || op > 15) return fail(PT_ERR_INVALID_ARG, "pt_debug_math: bad argument");
  if ((op == 4 || op == 8 || op == 9 || op == 12 || op == 13) && !b) return fail(PT_ERR_INVALID_ARG, "pt_debug_math: op needs two operands");
  if (n == 0) return PT_OK;
  DevBuf<float> da, db, dout;
  PT_HIP(da.alloc(n));
  PT_HIP(dout.alloc(n));
  PT_HIP(hipMemcpy(da.p, a, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  if (b) {
    PT_HIP(db.alloc(n));
    PT_HIP(hipMemcpy(db.p, b, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, op, da.p, b ? db.p : nullptr, dout.p, (long long)n);
  PT_HIP(hipGetLastError());
  PT_HIP(hipMemcpy(out, dout.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_debug_sphere_texel(const float* n_xyz, int64_t n, float freq, int32_t width, int32_t height, int32_t* out_ij, int32_t* exact_ij, uint8_t* took_fast,
                          float* uv4) {
  if (!n_xyz || !out_ij || !exact_ij || !took_fast || n < 0 || width < 1 || height < 1) return fail(PT_ERR_INVALID_ARG, "pt_debug_sphere_texel: bad argument");
  if (n == 0) return PT_OK;
  DevBuf<float> dn;
  DevBuf<int32_t> da, db;
  DevBuf<uint8_t> df;
  DevBuf<float> duv;
  if (uv4) PT_HIP(duv.alloc(4 * n));
  PT_HIP(dn.alloc(3 * n));
  PT_HIP(da.alloc(2 * n));
  PT_HIP(db.alloc(2 * n));
  PT_HIP(df.alloc(n));
  PT_HIP(hipMemcpy(dn.p, n_xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(sphere_texel_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, dn.p, (long long)n, freq, (uint32_t)width, (uint32_t)height, da.p, db.p, df.p, uv4 ? duv.p : nullptr);
  PT_HIP(hipGetLastError());
  PT_HIP(hipMemcpy(out_ij, da.p, (size_t)n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
  PT_HIP(hipMemcpy(exact_ij, db.p, (size_t)n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
  PT_HIP(hipMemcpy(took_fast, df.p, (size_t)n, hipMemcpyDeviceToHost));
  if (uv4) PT_HIP(hipMemcpy(uv4, duv.p, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost));
  return PT_OK;
}

} // extern "C"
