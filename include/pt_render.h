/*
 * pt_render.h — C-ABI drop-in boundary of the MI355X-native render() hot path.
 *
 * What it replaces (all citations are into the reference tree, triSYCL/path_tracer):
 *
 *   render<width,height,samples>(sycl::queue&, sycl::buffer<color,2>&,
 *                                std::vector<hittable_t>&, camera&)      include/render.hpp:141-160
 *
 * The reference has no FFI/plugin layer; its boundary is that one C++ function
 * template plus a hidden third input, the process-global image-texture atlas
 * (include/texture.hpp:71,126-131,157).  This header states the same boundary as a
 * plain C ABI (pointers + sizes, no C++/torch types) so any host — the C++20
 * facade in path_tracer_amd/include/pt/, the Python ctypes mirror in
 * path_tracer_amd/, or the reference's own render.hpp through the adapter of
 * INTEGRATION.md (which needs what the reference does not expose today: read access to
 * camera's ten private fields, camera.hpp:23-51, and to image_texture's fields) — can
 * bind it.  The facade's render<W,H,S>(frame_buf, hittables, cam) keeps the reference's
 * argument order but has no sycl::queue& / sycl::buffer& (there is no SYCL here).
 *
 * The scene crosses the boundary as three small tables (hittables, materials,
 * textures) + the RGB8 atlas; tags keep the reference's std::variant index order
 * (render.hpp:22-23, material.hpp:133-135, texture.hpp:154, rectangle.hpp:130,
 * constant_medium.hpp:10) so dumps are debuggable against the reference.
 * pt_scene_create() flattens those tables into per-kind 16-byte-aligned record
 * arrays + an order-preserving run table in HBM (see DESIGN.md "Data layout").
 *
 * All floating point is IEEE binary32, no contraction; RNG is xorshift32
 * (include/xorshift.hpp:72-74) seeded with the pixel's linear id (render.hpp:130-132).
 */
#ifndef PT_RENDER_H
#define PT_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): PtTuning's word 9 is tri_binned (was tri_Mg, dead since round 5), tri_cache appended; pt_scene_device_bytes, pt_build_id.
 * The table structs (PtHittable / PtMaterial / PtTexture / PtCamera / PtRenderParams) are those of version 1: scene fixtures written
 * under version 1 load unchanged (path_tracer_amd/scene_io.py).                                                                    */
#define PT_ABI_VERSION 2

/* ---- tags: same numbering as the reference's variant alternatives ---------- */

/* hittable_t = variant<sphere, xy_rect, triangle, box, constant_medium>  render.hpp:22-23 */
enum {
  PT_HIT_SPHERE = 0,          /* sphere.hpp:26-117 (static + moving)             */
  PT_HIT_XY_RECT = 1,         /* rectangle.hpp:16-52                              */
  PT_HIT_TRIANGLE = 2,        /* triangle.hpp:58-122 (Moller-Trumbore strategy)   */
  PT_HIT_BOX = 3,             /* box.hpp:10-56                                    */
  PT_HIT_CONSTANT_MEDIUM = 4, /* constant_medium.hpp:16-83                        */
  /* Extension: classes exist (rectangle.hpp:54,92) but are not hittable_t
   * alternatives in the reference; offered as top-level hittables here.        */
  PT_HIT_XZ_RECT = 5,
  PT_HIT_YZ_RECT = 6,
  PT_HIT_KIND_COUNT = 7
};

/* _triangle<IntersectionStrategy> (triangle.hpp:102-103): moller_trumbore_triangle_intersec is the default and the only one
 * main.cpp instantiates; badouel_ray_triangle_intersec (triangle.hpp:14-56) is the alternative the header ships.        */
enum { PT_TRI_MOLLER_TRUMBORE = 0, PT_TRI_BADOUEL = 1 };

/* material_t = variant<lambertian, metal, dielectric, lightsource, isotropic>  material.hpp:133-135 */
enum {
  PT_MAT_LAMBERTIAN = 0,
  PT_MAT_METAL = 1,
  PT_MAT_DIELECTRIC = 2,
  PT_MAT_LIGHTSOURCE = 3,
  PT_MAT_ISOTROPIC = 4
};

/* texture_t = variant<checker_texture, solid_texture, image_texture>  texture.hpp:154 */
enum { PT_TEX_CHECKER = 0, PT_TEX_SOLID = 1, PT_TEX_IMAGE = 2 };

/* ---- scene description tables (host memory, caller-owned, read-only) ------- */

/* One hittable, 64 bytes.  f[] by kind:
 *  SPHERE           f[0..2]=center0 f[3..5]=center1 f[6]=radius f[7]=time0 f[8]=time1
 *                   (static sphere: center1=center0, time0=time1=0  sphere.hpp:30-36)
 *  XY_RECT          f[0]=x0 f[1]=x1 f[2]=y0 f[3]=y1 f[4]=k          rectangle.hpp:21
 *  XZ_RECT          f[0]=x0 f[1]=x1 f[2]=z0 f[3]=z1 f[4]=k          rectangle.hpp:59
 *  YZ_RECT          f[0]=y0 f[1]=y1 f[2]=z0 f[3]=z1 f[4]=k          rectangle.hpp:97
 *  TRIANGLE         f[0..2]=v0 f[3..5]=v1 f[6..8]=v2                triangle.hpp:107
 *  BOX              f[0..2]=p0 (min) f[3..5]=p1 (max)               box.hpp:15
 *  CONSTANT_MEDIUM  f[0..8]=boundary in SPHERE or BOX layout (boundary_kind),
 *                   f[9]=neg_inv_density (= -1/d, constant_medium.hpp:20);
 *                   material = the isotropic phase function         constant_medium.hpp:21
 */
typedef struct PtHittable {
  int32_t kind;
  int32_t material;      /* index into PtSceneDesc.materials */
  int32_t boundary_kind; /* CONSTANT_MEDIUM only: PT_HIT_SPHERE or PT_HIT_BOX */
  int32_t strategy;      /* TRIANGLE only: the template argument of _triangle<> (triangle.hpp:102-103): PT_TRI_MOLLER_TRUMBORE
                          * (= `triangle`, what main.cpp builds) or PT_TRI_BADOUEL (triangle.hpp:14-56); 0 elsewhere      */
  float f[12];
} PtHittable;

/* One material, 32 bytes.
 *  LAMBERTIAN   texture = albedo                              material.hpp:11-31
 *  METAL        color = albedo, param = fuzz (already clamped to [0,1], material.hpp:37)
 *  DIELECTRIC   color = albedo, param = ref_idx               material.hpp:55-95
 *  LIGHTSOURCE  texture = emit                                material.hpp:97-111
 *  ISOTROPIC    texture = albedo                              material.hpp:113-131
 */
typedef struct PtMaterial {
  int32_t kind;
  int32_t texture; /* index into PtSceneDesc.textures, or -1 */
  float color[3];
  float param;
  int32_t reserved[2];
} PtMaterial;

/* One texture, 48 bytes.
 *  SOLID    color0                                            texture.hpp:18-29
 *  CHECKER  color0 = odd (sines < 0), color1 = even           texture.hpp:32-52
 *  IMAGE    width,height,offset (in texels into the atlas),freq  texture.hpp:67-152
 */
typedef struct PtTexture {
  int32_t kind;
  float color0[3];
  float color1[3];
  uint32_t width, height;
  uint32_t offset;
  float freq;
  int32_t reserved;
} PtTexture;

typedef struct PtSceneDesc {
  const PtHittable* hittables; /* list order == traversal order (render.hpp:37) */
  int32_t n_hittables;
  const PtMaterial* materials;
  int32_t n_materials;
  const PtTexture* textures;
  int32_t n_textures;
  int32_t reserved;
  /* RGB8 atlas, rows top-down; texel 0 is the {0,0,1} load-failure fallback
   * (texture.hpp:157).  May be NULL/0 when no image texture is used.          */
  const uint8_t* atlas;
  uint64_t atlas_bytes;
} PtSceneDesc;

/* camera, 96 bytes: the private fields of camera.hpp:23-51 in declaration order.
 * pt_camera_init() is the 9-argument constructor camera.hpp:67-87.             */
typedef struct PtCamera {
  float origin[3];
  float lower_left_corner[3];
  float horizontal[3];
  float vertical[3];
  float u[3], v[3], w[3];
  float lens_radius;
  float time0, time1;
} PtCamera;

/* Pixels are grouped into 8x8 tiles (one 64-lane wavefront per tile).  Tile g =
 * ty*tiles_x + tx belongs to shard g % shard_count, local index g / shard_count. */
#define PT_TILE 8
#define PT_TILE_PIXELS 64

enum {
  PT_FLAG_NONE = 0,
  PT_FLAG_NO_LDS = 1u << 0,       /* A/B switch: fetch primitives with scalar loads instead of LDS */
  PT_FLAG_FORCE_STREAM = 1u << 1, /* use the LDS-tile streaming kernel even when the scene fits in LDS */
  PT_FLAG_NO_FASTDIV = 1u << 2,   /* plain IEEE division for every rect/box side (no shared reciprocal) */
  PT_FLAG_TILE_GRANULAR = 1u << 3,  /* waves dequeue whole 8x8 tiles (default when the scene is LDS/scalar-cache resident) */
  PT_FLAG_FORCE_COOP = 1u << 7,     /* use the cooperative kernels even where the launcher's heuristic would not */
  PT_FLAG_NO_SPLIT = 1u << 8,       /* cooperative kernels, but no tile is rendered several lanes per pixel */
  PT_FLAG_NO_COOP = 1u << 6,        /* never split a ray's primitive list over idle lanes (tail acceleration off) */
  PT_FLAG_NO_LPT = 1u << 5,         /* skip the cost-probe pass: tiles are dequeued in raster order */
  PT_FLAG_PIXEL_GRANULAR = 1u << 4, /* lanes dequeue single pixels (default for the LDS-tile streaming kernel) */
  /* OPT-IN, NOT THE REFERENCE'S IMAGE: decorrelated RNG streams.  The reference gives a pixel ONE xorshift32 stream for all
   * of its samples (render.hpp:95-101,130-133), which makes a pixel a sequential chain and bounds any schedule by the
   * heaviest pixel.  With this flag a pixel's samples are cut into chunks of PT_FAST_CHUNK_SPP; chunk c of pixel id draws
   * from its own stream seeded pt_fast_seed(id, c), chunks are rendered as independent work units and their sums are added
   * in chunk order (deterministic run to run).  Same estimator, different random numbers: judged by PSNR / mean against
   * the parity image, never bit for bit, never the default.                                                             */
  PT_FLAG_FAST_RNG = 1u << 9,
  /* The reference's OTHER executor (render.hpp:113-122, built with USE_SINGLE_TASK for FPGA targets): ONE LocalPseudoRNG
   * with its default seed (xorshift.hpp:18) shared by all pixels, visited x-outer / y-inner, every draw of every sample of
   * every pixel taken from that one stream in order.  Sequential by definition — a pixel's first state depends on how
   * many numbers all earlier pixels drew — so it runs as ONE lane; offered for parity completeness on small frames
   * (width * height * samples <= 2^22), not for speed.  Needs shard_count == 1.                                         */
  PT_FLAG_SINGLE_STREAM = 1u << 10,
};

/* PT_FLAG_FAST_RNG: samples per chunk; pt_fast_seed() below gives the xorshift32 seed of chunk `chunk` of the pixel with
 * linear id `pixel`: h = pixel * 0x9E3779B1 + chunk * 0x85EBCA77 + 0x165667B1; h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15;
 * h *= 0x846CA68B; h ^= h >> 16; 0 is mapped to 1 (a zero xorshift state is stuck).                                       */
#define PT_FAST_CHUNK_SPP 64

typedef struct PtRenderParams {
  int32_t width, height; /* template args of render<> (render.hpp:141)           */
  int32_t samples;       /* spp, template arg                                    */
  int32_t depth;         /* 50 in the reference (render.hpp:144)                 */
  int32_t shard_index;   /* this GPU's shard, 0 <= shard_index < shard_count     */
  int32_t shard_count;   /* 1 = whole frame                                      */
  uint32_t flags;
  int32_t reserved;
} PtRenderParams;

/* Opaque device-resident flattened scene.  Renders of one PtScene may be queued back to back (each launch gets its
 * own work-queue slot) but must be ORDERED with respect to each other — same stream, or synchronised by the caller —
 * and issued by one host thread at a time: the scene owns a small grow-only scheduling workspace (per-tile costs,
 * tile order) that consecutive renders reuse.  For concurrent renders create one PtScene per stream.            */
typedef struct PtScene PtScene;

/* ---- error codes (the reference returns void and asserts; we return codes) -- */
enum {
  PT_OK = 0,
  PT_ERR_INVALID_ARG = 1,
  PT_ERR_BAD_SCENE = 2,   /* tag / index out of range in the tables */
  PT_ERR_HIP = 3,         /* a HIP runtime call failed; see pt_last_error() */
  PT_ERR_NO_DEVICE = 4,
  PT_ERR_TOO_LARGE = 5
};

int pt_abi_version(void);
const char* pt_error_string(int code);
const char* pt_last_error(void); /* thread-local detail of the last failure */

/* camera(look_from, look_at, vup, vfov_deg, aspect, aperture, focus_dist, t0, t1)
 * camera.hpp:67-87.  Host-side arithmetic only.                                 */
int pt_camera_init(PtCamera* cam, const float look_from[3], const float look_at[3],
                   const float vup[3], float vfov_deg, float aspect_ratio,
                   float aperture, float focus_dist, float time0, float time1);

/* Validate + flatten + upload to the current HIP device.  Replaces the
 * sycl::buffer wrapping of hittables and image_texture::freeze()
 * (render.hpp:146-148).  Unlike freeze() it may be called any number of times. */
int pt_scene_create(const PtSceneDesc* desc, PtScene** out_scene);
void pt_scene_destroy(PtScene* scene);
/* Device memory the scene's DATA occupies: record blob + material table + the triangle pools' tables + texture atlas
 * (launch workspaces — tile orders, candidate caches — come on top and are sized by the frame).  -1 for NULL.      */
int64_t pt_scene_device_bytes(const PtScene* scene);
/* Which kernels this library was built from: the first 16 hex digits of the sha256 over its kernel sources
 * (csrc/Makefile) — what bench.py and tools/pmc_summary.py stamp PMC recordings with.                               */
const char* pt_build_id(void);

/* ---- tuning --------------------------------------------------------------------------------------------------------------
 * PERFORMANCE-ONLY knobs: every setting gives the same image bit for bit (tests/test_abi_cpu.py, the GPU parity suite runs
 * several of them); they choose which exact culling structures pt_scene_create builds and how launches are scheduled.  A
 * zero-initialised struct with struct_size set (pt_tuning_init) is the library's defaults.  pt_scene_create(desc, out) is
 * pt_scene_create_tuned(desc, NULL, out): the defaults with the PT_* environment variables applied on top — the override
 * channel of tools/ and of A/B runs (tools/README.md lists them).  A caller that passes a PtTuning gets EXACTLY that: the
 * environment is not consulted.  Fields (0 = default unless said otherwise):
 *   sphere_grid        -1: no culling grid for runs of small spheres (PT_NO_GRID)
 *   grid_margin/cell   the grid's margin in median radii / cell edge in (median radius + margin) (PT_GRID_M, PT_GRID_CELL; 0.5, 3.0)
 *   slab_pools         -1: no slab pools for rect / box stretches (PT_NO_BOXCULL); 1: a pool for every stretch of >= 2
 *                      (PT_POOL_ALWAYS: also where the cost model says it does not pay)
 *   tri_pool           -1: no triangle pool (PT_NO_TRICULL)
 *   tri_min_run        shortest triangle run that gets a pool (PT_TRI_MIN; 4096; PT_TRICULL=1 means 256)
 *   tri_M, tri_cell    the pool's slack 1/M (grid boxes grow with 1/M, bands with M) and its grid cell in median grown boxes (PT_TRI_M,
 *                      PT_TRI_CELL; 6, 0.30 — round 6, after the grid's slack was re-derived; 12, 0.22 before)
 *   tri_binned         scenes with ONE pooled triangle run render in GENERATIONS (round 6; csrc/pt_binned.hpp): every live pixel traces one
 *                      ray per generation and the rays are sorted by direction bin, so that a bin's list of grazing candidates is read once
 *                      for 64 rays — 1: on (PT_TRI_BINNED); 0: off: measured, it does not beat the persistent kernel yet (docs/EXPERIMENTS.md).
 *                      Such renders have returned only when the frame is done (the number of generations is known on the device only)
 *   sphere_merge       a sphere run of more than two spheres also tests, through its lists, the static spheres of later short sphere runs
 *                      that only rect / box / short triangle runs separate it from (the resident kernels then skip those runs: a short run
 *                      costs ~600 cycles per sphere, a list entry ~100) — 0: yes; -1: every run where it stands (PT_NO_SPHERE_MERGE; the A/B)
 *   tri_cache          triangle-pool kernels, pinhole cameras: a lane keeps the grazing candidates of its pixel's camera rays (built by the
 *                      pixel's first sample with the filters widened to the pixel's footprint) and every later camera ray of the pixel tests
 *                      those instead of enumerating its direction-map list — 0: yes; -1: no (PT_NO_TRI_CACHE; the A/B)
 *   tri_res[0..2], tri_rho[0..1] + tri_rho2   the pool's direction maps: resolution per cube-map face and the largest rho / R a map
 *                      serves, per rho class (PT_TRI_RES=a,b,c PT_TRI_RHO=a,b,c; {128, 64, 32} since round 6 — camera rays take their candidates from the pixel's cache: tri_cache —, {2.12, 4, 16}; a negative rho: no such
 *                      map; rays with rho beyond the last class stream every band record)
 *   tri_budget_mb      MiB the direction maps may take together (PT_TRI_BUDGET_MB; 1600, for all of a scene's pooled runs): a map over budget is built coarser or not at all
 *   generic_materials  1: no material-specialised kernels (PT_NO_MATSPEC)
 *   blocks_per_cu      cap on resident workgroups per CU (PT_BLOCKS_PER_CU)
 *   cold_state         -1: the cold lane state stays in registers (PT_NO_COLD_LDS)
 *   wide_log2_group    forced log2 group size of the cooperative kernels' wide phase (PT_WIDE_LOGG; 0: the model picks)
 *   split_tiles_mode / split_tiles   mode 1: `split_tiles` tiles go through the wide phase (< 0: all) (PT_SPLIT_TILES)
 *   lpt_by_max         1 / -1: order tiles by their heaviest pixel / by their ray count (PT_LPT_MAX; 0: by kernel family)
 *   probe_spp_max      depth cap of the cost probe (PT_PROBE_SPP_MAX; 16)
 *   grid_min_tiles     frames (shards) of fewer tiles keep the cooperative kernels and the lists (PT_GRID_MIN_TILES; 0)
 *   model_fixed/chain  constants of the makespan model (PT_MODEL_FIXED, PT_MODEL_CHAIN; 2400, 2400)
 *   scatter_log        triangle-pool kernels: log2 of the pixels of one tile a wave takes together (PT_SCATTER_LOG; 0)
 *   scatter_mode       -1: whole tiles per wave (PT_NO_SCATTER); 1: with the cost probe (PT_LPT_SCATTER)
 *   lanes_cap          sphere-grid kernels on frames that do not fill the chip: lanes of a wave that take pixels (PT_LANES_CAP=n; 0: 16 x
 *                      pixels per resident lane, whole tiles from 24 on; -1 or PT_LANES_CAP=0: whole tiles always)
 *   grid_walk          which sphere-grid walk: 1 wave-synchronous (each lane tests its candidate in place), 2 through the LDS pair queue
 *                      (64 pairs per batch); 0: the launcher's rule (PT_GRID_WALK).  Only the LDS-resident ordinary kernels have walk 2:
 *                      the scalar-cache, fast-mode and cold-state kernels (scenes up to 10 KB without image textures) walk in place
 *   heavy_tiles        sphere-grid kernels on launches bound by their heaviest tiles' chains (1.5 ... 6 pixels per resident lane): the first
 *                      n tiles of the cost-sorted order are handed out 16 pixels at a time, a quarter tile per wave (PT_HEAVY_TILES=n;
 *                      0: one tile per SIMD of the chip in that range, none outside; -1: never)
 *   probe_resume       the cost probe's samples are the frame's first samples — the frame launch starts every pixel from the radiance sum and
 *                      the generator state the probe left (same stream, same order of additions) — 0: yes; -1: the probe's samples are
 *                      thrown away and rendered again, as before round 5 (PT_NO_PROBE_RESUME; the A/B)
 *   chain_priority     headline-family frame launches (no sphere grid, no cooperative phase): from the middle of the tile queue on, a wave
 *                      raises its issue priority by the samples its slowest pixel still has to render — the longest remaining chain first;
 *                      changes no value, only when a pixel is rendered — 0: yes; -1: never (PT_NO_CHAIN_PRIO; the A/B)                        */
typedef struct PtTuning {
  int32_t struct_size; /* sizeof(PtTuning) of the caller's header */
  int32_t sphere_grid;
  float grid_margin, grid_cell;
  int32_t slab_pools;
  int32_t tri_pool, tri_min_run;
  float tri_M;
  int32_t tri_binned; /* (round 6: took the place of tri_Mg, dead since round 5) */
  float tri_cell;
  int32_t tri_res[3];
  int32_t generic_materials;
  int32_t blocks_per_cu, cold_state, wide_log2_group, split_tiles_mode, split_tiles, lpt_by_max, probe_spp_max, grid_min_tiles;
  float model_fixed, model_chain;
  int32_t scatter_log, scatter_mode;
  int32_t lanes_cap, grid_walk;
  int32_t heavy_tiles;
  float tri_rho[2];      /* (round 5; these four took the place of reserved words: the struct's size is unchanged) */
  int32_t tri_budget_mb;
  float tri_rho2;
  int32_t probe_resume;  /* (round 5, the last reserved word) */
  int32_t chain_priority; /* (round 5: appended — a caller built against the shorter struct passes its own struct_size and gets the default) */
  int32_t tri_cache;      /* (round 6: appended) */
  int32_t sphere_merge;   /* (round 6: appended) */
} PtTuning;
void pt_tuning_init(PtTuning* t);     /* zero + struct_size: the library's defaults                                          */
void pt_tuning_from_env(PtTuning* t); /* the defaults with the PT_* environment applied: what pt_scene_create(desc, out) uses */
int pt_scene_create_tuned(const PtSceneDesc* desc, const PtTuning* tuning, PtScene** out_scene);

/* Number of floats the caller must provide to pt_render for these params:
 * shard_count==1: height*width*3 laid out [y][x][rgb], y=0 = bottom scan-line
 * (render.hpp:105, main.cpp:41).  shard_count>1: pt_shard_tiles()*64*3 laid
 * out [local_tile][ly*8+lx][rgb].                                              */
int64_t pt_framebuffer_floats(const PtRenderParams* p);
/* Seed of the fast mode's stream for (pixel, chunk) — see PT_FLAG_FAST_RNG; never 0. Host function, no GPU needed. */
uint32_t pt_fast_seed(uint32_t pixel, uint32_t chunk);

int32_t pt_shard_tiles(const PtRenderParams* p); /* ceil(n_tiles / shard_count) */

/* Optional: size the scene's per-launch workspaces (tile cost / order arrays and per-pixel generator states of the heaviest-first schedule; the fast
 * mode's partial sums) for these parameters NOW, so that no later pt_render() with parameters that need no more
 * allocates or frees device memory (hipMalloc / hipFree synchronise the device; without this call the first render at
 * a new size does it).  Call it with the scene's device current.                                                     */
int pt_scene_reserve(const PtScene* scene, const PtRenderParams* params);

/* The hot path.  Asynchronous on `stream` (a hipStream_t, or NULL for the
 * default stream) like queue.submit (render.hpp:151); fb_device is device
 * memory, fully overwritten (discard_write, render.hpp:152) — and READ BACK
 * while the render runs: the cost-probe pass leaves every pixel's radiance sum
 * of its first samples there and the frame launch carries on from it
 * (PtTuning.probe_resume), so the buffer must be ordinary readable device memory
 * and holds intermediate sums until the stream has passed the call.  The first
 * render of a scene at a new frame size grows the scene's workspaces (hipMalloc,
 * which synchronises); call pt_scene_reserve first where that matters.          */
int pt_render(const PtScene* scene, const PtCamera* cam, const PtRenderParams* p,
              float* fb_device, void* stream);

/* Same, timed: brackets the kernel launch with HIP events recorded on `stream`
 * and returns the kernel's duration (synchronises `stream`: blocks until done). */
int pt_render_timed(const PtScene* scene, const PtCamera* cam, const PtRenderParams* p,
                    float* fb_device, void* stream, float* kernel_ms);

/* Convenience: render into host memory (allocates, renders, copies back, syncs). */
int pt_render_host(const PtScene* scene, const PtCamera* cam, const PtRenderParams* p,
                   float* fb_host);

/* Root-side un-interleave after the RCCL gather: gathered is
 * [shard_count][pt_shard_tiles][64][3] device floats -> fb [height][width][3].
 * Asynchronous on `stream`, allocates nothing.                                  */
int pt_unshard_tiles(const float* gathered_device, const PtRenderParams* p,
                     float* fb_device, void* stream);

/* Output stage of main.cpp:33-59: sqrt gamma, clamp [0,0.999], *256 -> u8,
 * vertical flip; rgb8_device is [height][width][3], row 0 = top.  Asynchronous
 * on `stream`, allocates nothing.                                             */
int pt_tonemap_rgb8(const float* fb_device, int32_t width, int32_t height,
                    uint8_t* rgb8_device, void* stream);

/* ---- progressive rendering: one frame rendered in sample windows -------------------------------------------------------------------
 * Added without an ABI version change (PT_ABI_VERSION stays 2): a caller detects the feature by the presence of these symbols.
 *
 * A PtAccum holds the device-resident per-pixel state of one frame: the plain radiance sum (float3, laid out like pt_render's frame
 * buffer: [y][x][3], or [local tile][64][3] for shards) and the xorshift32 generator state (u32 per local pixel, indexed like the
 * scheduler's per-pixel states: local tile * 64 + ly * 8 + lx).  pt_render_accumulate renders the samples [done, done + samples) of
 * every pixel into it: a window that starts at 0 seeds the generator with the pixel's linear id (render.hpp:130-132), a later one
 * resumes from the saved state — the reference's single stream per pixel, summed in order (render.hpp:95-102).
 *
 * CONTRACT: after any sequence of windows totalling N samples, pt_accum_resolve writes the same bits that pt_render writes with
 * samples = N and the same scene, camera, depth, shard and flags — for every split, N windows of 1 sample included.  (PT_FLAG_FAST_RNG:
 * the same holds against pt_render's fast mode, under the window rule below.)
 *
 * Binding.  The accumulator is bound at create to the scene and to the frame parameters (width, height, depth, shard, flags; `samples`
 * is ignored), and by its first window to that window's camera: a later window whose PtCamera differs (byte compare of the 96 bytes)
 * returns PT_ERR_INVALID_ARG.  The scene must outlive the accumulator and stay the same scene: the state means nothing against other
 * tables.  Windows are stream-ordered like renders of one PtScene (same stream, or synchronised by the caller; one host thread at a
 * time); they share the scene's launch workspaces with its other renders, never its tile order: the accumulator keeps its own.
 *
 * Rejected (PT_ERR_INVALID_ARG): samples <= 0 or a total past INT32_MAX; PT_FLAG_SINGLE_STREAM (one global stream, no per-pixel state);
 * pt_accum_resolve / pt_accum_tonemap_rgb8 at 0 samples; pt_accum_tonemap_rgb8 with shard_count > 1 (pt_tonemap_rgb8's frame layout).
 * PT_FLAG_FAST_RNG: a window may only START on a multiple of PT_FAST_CHUNK_SPP samples (once one ends off a multiple, the next is
 * refused) and holds at most 8 128 samples (PT_ERR_TOO_LARGE, as pt_render); the total is not capped.
 *
 * Scheduling.  A window long enough for pt_render's cost probe (16 samples and more) probes with its own length, starting from the
 * state; a shorter one dequeues tiles in the heaviest-first order the accumulator kept from its last probed window (raster order
 * before the first).  Scenes with PtTuning.tri_binned render their windows with the persistent kernels (the same image).
 *
 * Device memory: pt_accum_create allocates the state (pt_accum_state_bytes, less the header) and sizes the scene's launch workspaces
 * for the frame; pt_render_accumulate allocates nothing, except in fast mode, whose chunk workspace pt_scene_reserve sizes (called
 * with samples = the largest window).
 *
 * Export format (pt_accum_export / pt_accum_import; host byte order): a PT_ACCUM_HEADER_BYTES header — u32 magic PT_ACCUM_MAGIC, u32 format
 * PT_ACCUM_FORMAT, i32 width, height, depth, shard_index, shard_count, u32 flags, i32 samples done, i32 camera bound (0 / 1), 6 reserved
 * words (0), the bound PtCamera (96 bytes) — then pt_framebuffer_floats() floats of sums, then pt_shard_tiles() * 64 u32 generator
 * states.  Import refuses a state whose header does not match the accumulator's frame parameters.                                   */
#define PT_ACCUM_MAGIC 0x43415450u /* "PTAC" */
#define PT_ACCUM_FORMAT 1
#define PT_ACCUM_HEADER_BYTES 160
typedef struct PtAccum PtAccum; /* device-resident per-pixel state of a frame rendered in sample windows */
/* Validates the parameters (before any device call), allocates and zeroes the state on the current device (the scene's). */
int pt_accum_create(const PtScene* scene, const PtRenderParams* p, PtAccum** out);
void pt_accum_destroy(PtAccum* acc);
/* Back to 0 samples: same scene and frame parameters; the camera binding and the kept tile order are released (a camera that moved
 * starts a new image: the next window binds its camera).  Asynchronous on `stream`. */
int pt_accum_reset(PtAccum* acc, void* stream);
int32_t pt_accum_samples(const PtAccum* acc); /* samples rendered so far (host-side count; -1 for NULL) */
/* Render samples [done, done + samples) of every pixel; asynchronous on `stream` like pt_render. */
int pt_render_accumulate(PtAccum* acc, const PtCamera* cam, int32_t samples, void* stream);
/* fb = sum / done (correctly rounded, as render.hpp:102), pt_render's layout and bits; fb_device: pt_framebuffer_floats() floats.
 * Asynchronous on `stream`, allocates nothing. */
int pt_accum_resolve(const PtAccum* acc, float* fb_device, void* stream);
/* resolve + the output stage of pt_tonemap_rgb8 in one pass (whole frames): rgb8_device is [height][width][3], row 0 = top.
 * Asynchronous on `stream`, allocates nothing. */
int pt_accum_tonemap_rgb8(const PtAccum* acc, uint8_t* rgb8_device, void* stream);
/* Host function, no GPU: bytes of an exported state for these frame parameters (samples ignored); < 0 for invalid ones. */
int64_t pt_accum_state_bytes(const PtRenderParams* p);
/* Checkpoint into host memory of exactly pt_accum_state_bytes() bytes (synchronises `stream`). */
int pt_accum_export(const PtAccum* acc, void* host, int64_t bytes, void* stream);
/* Restore a checkpoint (validates the header; synchronises `stream`).  The next window resumes from it. */
int pt_accum_import(PtAccum* acc, const void* host, int64_t bytes, void* stream);

/* ---- adaptive sampling: progressive rendering with a sample count per pixel -----------------------------------------------------------
 * Added without an ABI version change, like PtAccum: a caller detects the feature by the presence of these symbols.
 *
 * An ADAPTIVE accumulator (pt_adaptive_create) is a PtAccum that also keeps, per pixel, its sample count n, how many of those samples
 * are in "half A" (a) and the radiance sum of half A (H).  A pixel's work in a window depends only on its sum and its generator state,
 * never on the sample index, so a pixel that reaches n samples through any pattern of windows is the reference's render at n samples.
 *
 * CONTRACT: after any sequence of windows, masked or not, pixel p resolves to the same bits that pt_render writes at p with
 * samples = n_p (same scene, camera, depth, flags and shard) — for every kernel family, with or without the cost probe, for shards and
 * across a checkpoint.  A pixel with n_p = 0 resolves to 0.  Plain accumulators keep every behaviour and every exported byte.
 *
 * Per-pixel arrays (masks: u8, counts: i32, errors: f32) hold one element per pixel in the frame buffer's layout without the channel:
 * [height][width] for whole frames, [local tile][64] (ly * 8 + lx) for shards.  Padding pixels of a shard are ignored (mask 0, count 0).
 *
 * Window.  pt_adaptive_window renders `samples` more samples of every pixel whose mask byte is nonzero (mask_device = NULL: every pixel);
 * the other pixels keep their sum, generator state and counts bit for bit.  pt_render_accumulate on an adaptive accumulator is the same
 * call with a NULL mask.  A masked window renders the local tiles that hold an active pixel, in the accumulator's kept heaviest-first
 * order (raster order before its first probed window), without the cost probe or the cooperative wide phase; it SYNCHRONISES `stream`
 * once, to read the active-tile count that sizes its launch.  A window with an empty mask is a no-op.  After each window a bookkeeping
 * pass puts it into half A or half B of each pixel it rendered: with D = the window's contribution to the sum (S after - S before,
 * binary32), if a < n - a then H += D and a += samples (ties go to half B); then n += samples.
 * Rejected (PT_ERR_INVALID_ARG): a plain accumulator; samples <= 0; a per-pixel total that could pass INT32_MAX; a camera other than the
 * bound one.
 *
 * Error (Dammertz et al. 2010, the two-half-buffer estimate), per pixel: +inf where a == 0 or a == n; otherwise, with the correctly
 * rounded binary32 means I = S / (float)n and A = H / (float)a per channel,
 *   err = ((|I.x - A.x| + |I.y - A.y|) + |I.z - A.z|) / (1e-4f + sqrt((I.x + I.y) + I.z)).
 * Select: noisy(q) = n_q < max_spp && !(err_q <= threshold) (NaN and inf stay noisy); pixel p is active when n_p < max_spp and
 * n_p < min_spp, or noisy(p), or (PT_ADAPTIVE_DILATE) a pixel of p's 8-neighbourhood inside the frame is noisy.  A negative threshold
 * keeps every pixel active up to max_spp.  PT_ADAPTIVE_DILATE with shard_count > 1 is refused.
 *
 * pt_adaptive_create refuses PT_FLAG_FAST_RNG and PT_FLAG_SINGLE_STREAM before any device call and seeds every pixel's generator state
 * with its linear id (the state of a pixel at 0 samples), so that every window resumes from the state.  pt_accum_reset restores that and
 * zeroes n, a and H.  pt_accum_samples returns the samples of the windows rendered without a mask (every pixel has at least these).
 * pt_accum_resolve and pt_accum_tonemap_rgb8 divide each pixel by its own n_p (the same correctly rounded division; 0 where n_p = 0);
 * they are refused only before the first window.  pt_accum_export / pt_accum_import refuse adaptive accumulators.
 *
 * Export format PT_ADAPTIVE_FORMAT (pt_adaptive_export / pt_adaptive_import; host byte order): the PT_ACCUM_HEADER_BYTES header of
 * pt_accum_export with format = PT_ADAPTIVE_FORMAT (samples done = the unmasked windows' samples), then F floats of sums, R u32 generator
 * states, F floats of H, P i32 counts n and P i32 counts a (F = pt_framebuffer_floats, R = pt_shard_tiles * 64, P = F / 3).
 * pt_adaptive_import also takes a PT_ACCUM_FORMAT state of a plain accumulator with the same frame parameters: every pixel gets
 * n = samples done, a = 0, H = 0 (start uniform, continue adaptively).  It validates the header and 0 <= a <= n on the host.         */
#define PT_ADAPTIVE_FORMAT 2
#define PT_ADAPTIVE_DILATE 1u
/* Validates the parameters (before any device call) and allocates the state on the current device; destroyed with pt_accum_destroy. */
int pt_adaptive_create(const PtScene* scene, const PtRenderParams* p, PtAccum** out);
/* `samples` more samples of each pixel whose mask byte is nonzero (NULL: every pixel: asynchronous on `stream` like
 * pt_render_accumulate); a mask synchronises `stream` once. */
int pt_adaptive_window(PtAccum* acc, const PtCamera* cam, int32_t samples, const uint8_t* mask_device, void* stream);
/* Per-pixel sample counts n (P i32).  Asynchronous on `stream`, allocates nothing. */
int pt_adaptive_counts(const PtAccum* acc, int32_t* counts_device, void* stream);
/* Per-pixel error estimate (P f32; the formula above).  Asynchronous on `stream`, allocates nothing. */
int pt_adaptive_error(const PtAccum* acc, float* err_device, void* stream);
/* The next window's mask (P u8: 1 active, 0 not) by the rule above; synchronises `stream`: n_active is a host value. */
int pt_adaptive_select(const PtAccum* acc, float threshold, int32_t min_spp, int32_t max_spp, uint32_t flags,
                       uint8_t* mask_device, int64_t* n_active, void* stream);
/* Host function, no GPU: bytes of an exported adaptive state for these frame parameters; < 0 for invalid ones. */
int64_t pt_adaptive_state_bytes(const PtRenderParams* p);
/* Checkpoint into host memory of exactly pt_adaptive_state_bytes() bytes (synchronises `stream`). */
int pt_adaptive_export(const PtAccum* acc, void* host, int64_t bytes, void* stream);
/* Restore a PT_ADAPTIVE_FORMAT checkpoint, or upgrade a plain PT_ACCUM_FORMAT one (synchronises `stream`). */
int pt_adaptive_import(PtAccum* acc, const void* host, int64_t bytes, void* stream);

/* ---- first-hit feature buffers (AOVs): guide images for denoisers, mattes for compositing --------------------------------------------
 * Added without an ABI version change, like PtAccum: a caller detects the feature by the presence of these symbols.
 *
 * DEFINITION.  The AOV pass of n samples is the reference's render at DEPTH 1, with the first bounce's record kept instead of thrown
 * away.  Pixel p owns one xorshift32 stream, seeded with its linear id exactly as pt_render seeds it (render.hpp:130-132).  Sample s
 * draws its camera ray from the stream (render.hpp:96-99), runs ONE iteration of the bounce loop (render.hpp:58-89: traversal, emitted,
 * scatter — with every draw a constant_medium or the scatter takes) and leaves the stream where that bounce left it.  In terms of the
 * probes below: pt_debug_camera_rays -> pt_debug_bounce (attenuation in = 1,1,1) -> PtBounceOut.rng_state -> the next sample.  Sample
 * 0's camera ray is the beauty pass's first camera ray; later ones are other draws over the same pixel footprint, lens and shutter.
 * The pass needs nothing from the beauty pass and costs one ray per sample.
 *
 * Per-sample terms, each a field of that sample's PtBounceOut, with hit = (status != PT_BOUNCE_MISS):
 *   albedo    color: the new attenuation if scattered, the emitted colour if absorbed, the sky if missed
 *   normal    hit ? normal : 0
 *   depth     hit ? t : 0
 *   coverage  hit ? 1 : 0
 *   direct    status == PT_BOUNCE_SCATTERED ? 0 : color — the depth-1 radiance: the bits pt_render writes with depth = 1
 *   id        `hittable` of SAMPLE 0 only (-1: miss)
 * Each float channel is a binary32 sum from +0 in sample order, divided once by (float)samples, correctly rounded (render.hpp:102).
 *
 * Layout.  3-channel planes are laid out like pt_render's frame buffer ([y][x][3], y = 0 the bottom scan-line, or [local tile][64][3]
 * for shards), 1-channel planes like pt_adaptive_counts ([height][width], or [local tile][64]); pt_aov_plane_elems gives the element
 * counts.  Padding pixels of a shard get 0, and -1 in `id`.  A NULL plane is not written.
 *
 * Rejected (PT_ERR_INVALID_ARG, before any device call): a NULL scene, camera, params or buffers; a struct_size other than
 * sizeof(PtAovBuffers); all six planes NULL; samples < 1 or > 1 << 24 (coverage stays exact); width or height <= 0; bad shard fields;
 * PT_FLAG_FAST_RNG or PT_FLAG_SINGLE_STREAM.  `depth` and the scheduling flags are ignored.
 *
 * Asynchronous on `stream` like pt_render; allocates nothing and touches none of the scene's launch workspaces, so it may sit between
 * any two renders of the scene on their stream without disturbing them.                                                              */
typedef struct PtAovBuffers { /* device pointers; NULL = plane not wanted */
  int32_t struct_size, reserved;
  float* albedo;   /* 3 ch */
  float* normal;   /* 3 ch */
  float* direct;   /* 3 ch */
  float* depth;    /* 1 ch */
  float* coverage; /* 1 ch */
  int32_t* id;     /* 1 ch */
} PtAovBuffers;
/* Host function, no GPU: elements of a plane of `channels` (1 or 3) channels for these parameters (samples ignored); < 0 for invalid ones. */
int64_t pt_aov_plane_elems(const PtRenderParams* p, int32_t channels);
/* The pass defined above; asynchronous on `stream`, allocates nothing. */
int pt_render_aov(const PtScene* scene, const PtCamera* cam, const PtRenderParams* p, const PtAovBuffers* buffers, void* stream);

/* ---- denoiser: the edge-avoiding a-trous wavelet filter, guided by the feature buffers ---------------------------------------------
 * Added without an ABI version change, like PtAccum: a caller detects the feature by the presence of these symbols.
 *
 * The filter of Dammertz, Sewtz, Hanika and Lensch (HPG 2010) over a finished frame, defined here operation by operation: every value
 * is IEEE binary32, every operation below is rounded once, nothing is fused, and the order of operations is the one written.
 *
 * Scope.  Whole frames only: color, albedo, normal and out are [height][width][3], depth is [height][width], y = 0 the bottom row — the
 * layouts pt_render and pt_render_aov write with shard_count = 1.  The filter reads neighbours, so a multi-GPU job filters after
 * pt_unshard_tiles; there is no shard parameter.  No scene is involved.  albedo, normal and depth are optional (NULL).  `out` may be
 * `color`.  The call is asynchronous on `stream` like pt_render_aov and allocates nothing: the caller supplies `scratch`,
 * pt_denoise_scratch_floats(width, height) floats of device memory, 16-byte aligned.
 *
 * Terms.  A term is OFF — contributes x = 0 — when its sigma is <= 0 or its plane is NULL (normal, depth, albedo).
 *
 * DEFINITION.  c_0 = color (with PT_DENOISE_DEMODULATE: c_0 = color / (albedo + 1e-3f) per channel).  Iteration i = 0 ... iterations - 1
 * has step s = 2^i and makes c_(i+1) from c_i; for pixel p = (x, y):
 *   sum = (0, 0, 0), wsum = 0
 *   for dy = -2 ... 2 (outer), for dx = -2 ... 2 (inner): tap q = (x + s dx, y + s dy); a tap outside the frame is skipped
 *     h   = K[dy + 2] * K[dx + 2],  K = {1/16, 1/4, 3/8, 1/4, 1/16}                                      (exact)
 *     x_c = ((dr * dr + dg * dg) + db * db) * k_c(i)      d. = c_i(p) - c_i(q) per channel;  k_c(i) = 1.0f / (sg * sg), sg = sigma_color * 2^-i
 *     x_n = ((dnx * dnx + dny * dny) + dnz * dnz) * k_n   dn = normal(p) - normal(q);        k_n = 1.0f / (sigma_normal * sigma_normal)
 *     x_d = (dz * dz) / (sd2 * (z_p * z_p) + 1e-12f)      dz = depth(p) - depth(q), z_p = depth(p);  sd2 = sigma_depth * sigma_depth
 *     x_a = ((dar * dar + dag * dag) + dab * dab) * k_a   da = albedo(p) - albedo(q);        k_a = 1.0f / (sigma_albedo * sigma_albedo)
 *     x   = ((x_c + x_n) + x_d) + x_a
 *     if !(x < 80.0f) the tap is skipped (NaN included); otherwise w = h * pt_exp_neg(x),
 *       sum.ch = sum.ch + w * c_i(q).ch for ch = r, g, b (the product rounded, then the sum), wsum = wsum + w
 *   c_(i+1)(p) = sum / wsum per channel (correctly rounded division); where wsum == 0 — no tap was accepted — c_(i+1)(p) = c_i(p)
 * out = c_iterations (with PT_DENOISE_DEMODULATE: out = c_iterations * (albedo + 1e-3f) per channel).
 * The colour sigma halves per iteration (the paper's schedule: what one level has smoothed, the next must not take for an edge) by an
 * exact scaling; the depth term is relative to the centre's depth, so the scene's scale does not matter; with demodulation, texture
 * detail (checker, image textures) lives in the albedo and is not blurred.
 *
 * pt_exp_neg(x), 0 <= x < 80, is e^-x by:  k = rintf(x * 0x1.715476p+0f)  (round half to even; 0 <= k <= 115);
 *   r = (x - k * 0x1.62e4p-1f) - k * 0x1.7f7d1cp-20f  (the first product is exact: the constant has 16 significant bits);  t = -r;
 *   q = 0x1.6c16c2p-10f; q = q * t + 0x1.111112p-7f; q = q * t + 0x1.555556p-5f; q = q * t + 0x1.555556p-3f; q = q * t + 0.5f;
 *   q = q * t + 1.0f; q = q * t + 1.0f  (the degree-6 Taylor polynomial of e^t, every product and every sum rounded);  result = ldexpf(q, -k)
 *   (exact: the result is a normal number).  Truncation on |r| <= ln2 / 2: 0.3466^7 / 5040 = 1.2e-7; with the rounding of the reduction
 *   and of the polynomial the relative error against e^-x stays under 1e-6 (derived, then swept: tests/test_denoise_cpu.py).
 *
 * Containment.  With the colour term on, a tap whose colour is NaN or inf has x = NaN or inf and is skipped, and a pixel whose own colour
 * is not finite accepts no tap, its centre included (inf - inf = NaN), and keeps its value: a NaN or inf pixel stays where it is and
 * never spreads.  Every finite pixel accepts at least its centre tap (x = 0, w = 3/8 * 3/8).  The same holds for a non-finite guide value
 * whose term is on.
 *
 * Rejected (PT_ERR_INVALID_ARG, on the host, before any device call): a NULL params, color, out or scratch; a struct_size other than
 * sizeof(PtDenoiseParams); width or height <= 0; iterations outside 1 ... PT_DENOISE_MAX_ITERATIONS; a sigma that is not finite; a
 * sigma > 0 whose k (for sigma_color: any of its k_c(i); for sigma_depth: sd2) is not a finite binary32 number > 0; PT_DENOISE_DEMODULATE
 * without an albedo plane; flags other than PT_DENOISE_DEMODULATE and PT_DENOISE_NO_LDS; `out` or `scratch` overlapping a guide plane; `scratch` overlapping
 * `color` or `out`, or not 16-byte aligned.  More than 2^30 pixels: PT_ERR_TOO_LARGE.                                                 */
#define PT_DENOISE_DEMODULATE 1u
#define PT_DENOISE_NO_LDS 2u /* A/B switch, same bits: every iteration reads its taps from global memory (default: the steps 1 and 2 read an LDS-staged tile) */
#define PT_DENOISE_MAX_ITERATIONS 8
/* The defaults (pt_denoise_params_init), chosen for what progressive and adaptive renders stop at — 8 to 64 samples per pixel, where one
 * path that reaches a light moves a pixel by a unit of radiance or more: five levels (a 65 x 65 footprint); the halving colour sigma
 * from 32 in demodulated units (2 at the last level: the early levels are led by the guides, the colour term takes over as the noise
 * shrinks; lower it for cleaner input); normals within ~0.5 of each other; depth within ~20 %; no albedo term (demodulation has taken
 * the albedo out already); demodulation on.  tests/test_denoise_cpu.py holds them to a measured quality (profiles/denoise_bench.txt). */
#define PT_DENOISE_DEFAULT_ITERATIONS 5
#define PT_DENOISE_DEFAULT_SIGMA_COLOR 32.0f
#define PT_DENOISE_DEFAULT_SIGMA_NORMAL 0.5f
#define PT_DENOISE_DEFAULT_SIGMA_DEPTH 0.2f
#define PT_DENOISE_DEFAULT_SIGMA_ALBEDO 0.0f
#define PT_DENOISE_DEFAULT_FLAGS PT_DENOISE_DEMODULATE
typedef struct PtDenoiseParams {
  int32_t struct_size; /* sizeof(PtDenoiseParams) of the caller's header */
  int32_t width, height;
  int32_t iterations;  /* 1 ... PT_DENOISE_MAX_ITERATIONS */
  float sigma_color, sigma_normal, sigma_depth, sigma_albedo; /* <= 0: term off */
  uint32_t flags;      /* PT_DENOISE_DEMODULATE, PT_DENOISE_NO_LDS */
  int32_t reserved;
} PtDenoiseParams;
/* Host function, no GPU: struct_size + the defaults above for a frame of width x height. */
void pt_denoise_params_init(PtDenoiseParams* params, int32_t width, int32_t height);
/* Host function, no GPU: floats of `scratch` for a frame of width x height — one colour plane (the iterations ping-pong between it and
 * `out`) and two 16-byte guide records per pixel, (normal, depth) and (albedo, 0), packed by a prepass; < 0 for invalid sizes. */
int64_t pt_denoise_scratch_floats(int32_t width, int32_t height);
/* The filter defined above; asynchronous on `stream`, allocates nothing. */
int pt_denoise(const PtDenoiseParams* params, const float* color, const float* albedo, const float* normal, const float* depth,
               float* out, float* scratch, void* stream);
/* How the LAST pt_denoise of this process read its taps, per iteration: out[i] = 0 iteration not run, 1 from global memory, 2 from an
 * LDS-staged tile (the steps 1 and 2, unless PT_DENOISE_NO_LDS: profiles/denoise_bench.txt).  The bits do not depend on it.  For tests. */
int pt_debug_last_denoise(int32_t out[8]);

/* ---- variance-guided denoiser: the a-trous filter with a per-pixel colour tolerance taken from the adaptive half buffers ---------------
 * Added without an ABI version change, like PtAccum: a caller detects the feature by the presence of these symbols.  pt_denoise and
 * everything about it stay as they are.
 *
 * pt_denoise weighs colour differences against one sigma_color, which fits one noise level; an adaptive frame holds pixels from a few to a
 * thousand samples.  This filter is the spatial half of SVGF (Schied et al., HPG 2017): the colour difference is measured in units of
 * the pixel's own estimated standard deviation, the variance is smoothed by a 3 x 3 Gaussian before it is used, and it is propagated
 * through the levels (the variance of a weighted mean), so that each level sees the noise the previous one left.
 *
 * VARIANCE ESTIMATE (pt_variance_estimate).  Writes a 3-channel plane in the frame buffer's layout — pt_framebuffer_floats() floats:
 * [y][x][3] for whole frames, [local tile][64][3] for shards, padding pixels 0 — from an adaptive accumulator's sums S, half sums H and
 * counts n, a.  Per pixel and channel, every value binary32 and every operation rounded once:
 *   where a == 0 || a == n: +inf ("no estimate yet", the convention of pt_adaptive_error); otherwise, with b = n - a,
 *   A = H / (float)a;  B = (S - H) / (float)b;  d = A - B;  f = ((float)a * (float)b) / ((float)n * (float)n);  var = (d * d) * f
 * Why: the two halves are independent means of a and b samples of one distribution of variance s2, so Var(A - B) = s2 (1/a + 1/b) =
 * s2 n / (a b), while the resolved pixel S / n has variance s2 / n: (A - B)^2 * a b / n^2 estimates the variance of the resolved pixel
 * (with equal halves it is ((A - B) / 2)^2).  One squared difference is a noisy estimate — hence the filter's prefilter.
 * Asynchronous on `stream`, allocates nothing.  Rejected (PT_ERR_INVALID_ARG): a NULL argument, a plain (non-adaptive) accumulator, a call
 * before the accumulator's first window.
 *
 * THE FILTER (pt_variance_denoise).  Scope: pt_denoise's — whole frames only, no scene involved; color, variance, albedo, normal, out and
 * variance_out are [height][width][3], depth is [height][width]; albedo, normal and depth are optional (NULL), variance_out is optional;
 * `out` may be `color` and `variance_out` may be `variance` (the planes are read completely, by a prepass, before the first is written);
 * asynchronous on `stream`; allocates nothing: the caller supplies `scratch`, pt_variance_denoise_scratch_floats(width, height) floats
 * of device memory, 16-byte aligned.  `variance` is required: the variance of the pixel's MEAN per channel, from pt_variance_estimate or
 * from anywhere else.
 *
 * DEFINITION.  Every value is IEEE binary32, every operation below is rounded once, nothing is fused, and the order of operations is the
 * one written.  Terms not named here — K, h, x_n, x_d, x_a, k_n, sd2, k_a, pt_exp_neg, when a guide term is off — are pt_denoise's, verbatim.
 *   m   = albedo + 1e-3f per channel with PT_VDENOISE_DEMODULATE, else 1
 *   c_0 = color / m
 *   v_0 = sanitised(variance) / (m * m): a variance value that is not (>= 0 && < +inf) — negative, NaN, inf — is taken as +0 first.  (The
 *         filter then knows nothing about that pixel's noise beyond its neighbours' estimates, and is conservative there.)
 * Iteration i = 0 ... iterations - 1 has step s = 2^i and makes c_(i+1), v_(i+1) from c_i, v_i; for pixel p = (x, y):
 *   the prefilter, always at a distance of ONE pixel, whatever the step:
 *     vs = (0, 0, 0), gs = 0
 *     for dy = -1 ... 1 (outer), for dx = -1 ... 1 (inner): q = (x + dx, y + dy); a q outside the frame is skipped
 *       g = G[dy + 1] * G[dx + 1],  G = {1/4, 1/2, 1/4}   (exact);   vs.ch = vs.ch + g * v_i(q).ch;   gs = gs + g
 *     vbar.ch = vs.ch / gs
 *   the colour scale, three divisions per pixel and none per tap:
 *     iv.ch = 1.0f / (sv2 * vbar.ch + 1e-8f),  sv2 = sigma_variance * sigma_variance
 *   sum = (0, 0, 0), vsum = (0, 0, 0), wsum = 0
 *   for dy = -2 ... 2 (outer), for dx = -2 ... 2 (inner): tap q = (x + s dx, y + s dy); a tap outside the frame is skipped
 *     x_c = ((dr * dr) * iv.r + (dg * dg) * iv.g) + (db * db) * iv.b      d. = c_i(p) - c_i(q) per channel
 *     x   = ((x_c + x_n) + x_d) + x_a
 *     if !(x < 80.0f) the tap is skipped (NaN included); otherwise w = h * pt_exp_neg(x),
 *       sum.ch = sum.ch + w * c_i(q).ch;   vsum.ch = vsum.ch + (w * w) * v_i(q).ch;   wsum = wsum + w
 *   c_(i+1)(p) = sum / wsum,  v_(i+1)(p) = vsum / (wsum * wsum)  per channel; where wsum == 0 both keep their value
 * out = c_iterations * m;  variance_out (if not NULL) = v_iterations * (m * m) — the filtered frame's residual variance, under the
 * filter's assumption that the taps are independent.
 * The colour term is ON when sigma_variance > 0; when it is off x_c = 0, the prefilter is not needed, the filter is guide-only and the
 * variance is only propagated.  The 1e-8f keeps iv finite where the estimate is 0 (a pixel whose halves agree, a sanitised value): such a
 * pixel accepts only taps within ~1e-3 of its colour — it is left nearly alone rather than blurred on no evidence.
 *
 * Containment.  pt_denoise's: with the colour term on, a tap whose colour is NaN or inf has x = NaN or inf and is skipped, and a pixel whose
 * own colour is not finite accepts no tap, its centre included, and keeps its value and its variance: a NaN or inf colour stays where it
 * is and never spreads.  Every finite pixel accepts at least its centre tap (x = 0), so wsum is 0 or >= 9/64.  The same holds for a
 * non-finite guide value whose term is on.  A non-finite VARIANCE of the caller's never enters: it is sanitised to 0.  The prefilter is not edge-aware
 * (SVGF's is not either): no COLOUR is ever averaged across an edge the guides reject, but a pixel next to such an edge takes part of
 * its tolerance from the variance on the other side.
 *
 * Rejected (PT_ERR_INVALID_ARG, on the host, before any device call): a NULL params, color, variance, out or scratch; a struct_size
 * other than sizeof(PtVarianceDenoiseParams); width or height <= 0; iterations outside 1 ... PT_VDENOISE_MAX_ITERATIONS; a sigma that
 * is not finite; sigma_variance > 0 whose sv2 or 1.0f / sv2 is not a finite binary32 number > 0; a guide sigma > 0 whose k (sigma_depth:
 * sd2) is not one; PT_VDENOISE_DEMODULATE without an albedo plane; flags other than PT_VDENOISE_DEMODULATE and PT_VDENOISE_NO_LDS; `out`,
 * `variance_out` or `scratch` overlapping a guide plane; `scratch` overlapping color, variance, out or variance_out, or not 16-byte
 * aligned; `variance_out` overlapping `color` or `out`.  More than 2^30 pixels: PT_ERR_TOO_LARGE.                                      */
#define PT_VDENOISE_DEMODULATE 1u
#define PT_VDENOISE_NO_LDS 2u /* A/B switch, same bits: every iteration reads from global memory (default: the steps 1 and 2 read an LDS-staged tile) */
#define PT_VDENOISE_MAX_ITERATIONS 8
/* The defaults (pt_variance_denoise_params_init): pt_denoise's five levels, guide sigmas and demodulation; sigma_variance — the colour
 * tolerance in standard deviations of the prefiltered estimate — is the value of {2, 3, 4} with the smallest worst-case MSE ratio over
 * 8, 32 and 128 spp frames (tests/test_variance_denoise_cpu.py measures it; profiles/variance_denoise_bench.txt records the sweep). */
#define PT_VDENOISE_DEFAULT_ITERATIONS 5
#define PT_VDENOISE_DEFAULT_SIGMA_VARIANCE 2.0f
#define PT_VDENOISE_DEFAULT_SIGMA_NORMAL 0.5f
#define PT_VDENOISE_DEFAULT_SIGMA_DEPTH 0.2f
#define PT_VDENOISE_DEFAULT_SIGMA_ALBEDO 0.0f
#define PT_VDENOISE_DEFAULT_FLAGS PT_VDENOISE_DEMODULATE
typedef struct PtVarianceDenoiseParams {
  int32_t struct_size; /* sizeof(PtVarianceDenoiseParams) of the caller's header */
  int32_t width, height;
  int32_t iterations;  /* 1 ... PT_VDENOISE_MAX_ITERATIONS */
  float sigma_variance, sigma_normal, sigma_depth, sigma_albedo; /* <= 0: term off */
  uint32_t flags;      /* PT_VDENOISE_DEMODULATE, PT_VDENOISE_NO_LDS */
  int32_t reserved;
} PtVarianceDenoiseParams;
/* The per-channel variance of each resolved pixel of an adaptive accumulator (the formula above); variance_device: pt_framebuffer_floats() floats.
 * Asynchronous on `stream`, allocates nothing. */
int pt_variance_estimate(const PtAccum* acc, float* variance_device, void* stream);
/* Host function, no GPU: struct_size + the defaults above for a frame of width x height. */
void pt_variance_denoise_params_init(PtVarianceDenoiseParams* params, int32_t width, int32_t height);
/* Host function, no GPU: floats of `scratch` for a frame of width x height, 20 per pixel — two working planes the iterations ping-pong
 * between, each a 16-byte record (c.r, c.g, c.b, v.r) and an 8-byte record (v.g, v.b) per pixel, so that a tap's colour and variance are
 * two loads, and pt_denoise's two 16-byte guide records per pixel, (normal, depth) and (albedo, 0); < 0 for invalid sizes. */
int64_t pt_variance_denoise_scratch_floats(int32_t width, int32_t height);
/* The filter defined above; asynchronous on `stream`, allocates nothing. */
int pt_variance_denoise(const PtVarianceDenoiseParams* params, const float* color, const float* variance, const float* albedo,
                        const float* normal, const float* depth, float* out, float* variance_out, float* scratch, void* stream);
/* How the LAST pt_variance_denoise of this process read its taps, per iteration: out[i] = 0 iteration not run, 1 from global memory, 2 from
 * an LDS-staged tile (the steps 1 and 2, unless PT_VDENOISE_NO_LDS).  The bits do not depend on it.  For tests. */
int pt_debug_last_variance_denoise(int32_t out[8]);

/* ---- temporal reprojection: a frame's history carried across camera moves ------------------------------------------------------------
 * Added without an ABI version change, like PtAccum: a caller detects the feature by the presence of these symbols.  Nothing above changes.
 *
 * The temporal half of SVGF (Schied et al., HPG 2017), whose spatial half is pt_variance_denoise: each frame of a sequence is blended
 * into the history of the frames before it, fetched for every pixel through the PREVIOUS camera and rejected where the guides say the
 * surface is another one.  Two pieces are needed, and both are here: the reprojection (PtTemporal), and frames that do not repeat their
 * random numbers (pt_adaptive_next_frame) — pt_render and pt_accum_reset seed a pixel's generator with its linear id, so two frames from
 * the same or a nearby camera carry the SAME noise and no image-space accumulator could average them.
 *
 * NEXT FRAME (pt_adaptive_next_frame).  Adaptive accumulators only (PT_ERR_INVALID_ARG for NULL or a plain accumulator).  Starts a new
 * image that CONTINUES every pixel's stream: S, H, n, a and the unmasked sample count are zeroed, the camera binding and the kept tile
 * order are released exactly as pt_accum_reset releases them, and the per-pixel generator states are KEPT.  Asynchronous on `stream`,
 * allocates nothing, launches no kernel (an adaptive accumulator's windows always resume from the stored state).
 * CONTRACT, to the bit: let s_p be pixel p's generator state at the call.  After any sequence of windows, masked or not, totalling n_p
 * samples under the newly bound camera, S_p is the binary32 sum from +0, in sample order, of the n_p sample colours the reference's loop
 * (render.hpp:95-101) produces when its generator starts at s_p; the pixel resolves to S_p / (float)n_p; and the pixel's state is where
 * that loop left it.  Such a frame is the reference's estimator on a LATER PART of the pixel's stream: it equals pt_render's image at no
 * sample count.  pt_adaptive_export / pt_adaptive_import work unchanged afterwards.
 * (Declared `extern`, which changes nothing for a C or C++ caller: the eight entry points adaptive sampling was introduced with are
 * told from later ones by their plain one-word declarations.)
 *
 * THE HISTORY (PtTemporal).  Scope: pt_denoise's — whole frames only, no scene involved; planes [height][width](x3), y = 0 the bottom row;
 * pt_temporal_push is asynchronous on `stream` and allocates nothing (pt_temporal_create is the only allocation: pt_temporal_state_bytes
 * of device memory, two histories of 48 bytes per pixel — a push reads one and writes the other).  depth, normal and id are
 * pt_render_aov's planes for the same camera: the mean t along the UN-NORMALISED camera ray, 0 where missed; the mean normal; the
 * hittable of sample 0.  normal, id, variance_in, out_variance and out_history are optional (NULL).  out_color may be color and
 * out_variance may be variance_in.  Pushes of one PtTemporal are stream-ordered like renders of one PtScene.
 *
 * State.  Per pixel: c, the accumulated colour (also the first moment); m2, the accumulated second moment; N, the history length as a
 * float (0: unusable); z, n, k: the depth, normal and id pushed with the frame (0 for a NULL plane) — stored as three 16-byte records,
 * (c.rgb, N), (m2.rgb, z), (n.xyz, bits of k), so that a tap is three 16-byte loads.  The history also keeps the camera of the last push.
 *
 * Host-side constants, from the previous camera (primed):  g = lower_left_corner' - origin' per component;
 *   fo = -((g.x w'.x + g.y w'.y) + g.z w'.z);   hh = (h'.x h'.x + h'.y h'.y) + h'.z h'.z  (h' = horizontal');   vv likewise from vertical'.
 * A camera whose fo, hh or vv is not a finite number > 0 is refused (when it is pushed: a stored camera is always sound).
 *
 * DEFINITION.  Every value is IEEE binary32, every operation below is rounded once, nothing is fused, and the order of operations is the
 * one written.  For pixel p = (x, y) of a W x H frame, with C = color(p), z = depth(p), n = normal(p), k = id(p):
 *   finite(C) = every channel has |C.ch| < inf.
 *   !finite(C):  out_color = C, out_variance = +inf, out_history = 0; stored record: c = m2 = 0, N = 0.  (A NaN or inf stays where it is and
 *                never enters a history.)
 *   No usable history (the first push, or the first after pt_temporal_reset):  N = 1, alpha_p = 1, c = C, m2 = C * C.
 *   Otherwise:
 *     sc = ((float)x + 0.5f) / (float)W;   tc = ((float)y + 0.5f) / (float)H
 *     dir = ((lower_left_corner + sc * horizontal) + tc * vertical) - origin           per component, the camera of this push
 *     hit = z > 0                                                                      (NaN: false)
 *     d   = hit ? ((origin + z * dir) - origin') : dir      (a missed pixel reprojects as a direction: the sky is at infinity)
 *     cp  = -((d.x w'.x + d.y w'.y) + d.z w'.z);   r = fo / cp;   te = cp / fo
 *     s'  = (((d.x h'.x + d.y h'.y) + d.z h'.z) * r) / hh + 0.5f;   t' likewise with vertical', vv
 *     fx  = s' * (float)W - 0.5f;   fy = t' * (float)H - 0.5f
 *     usable = cp > 0 && fx >= -1 && fx < W && fy >= -1 && fy < H                      (NaN fails)
 *     x0 = floorf(fx), y0 = floorf(fy), ax = fx - x0, ay = fy - y0
 *     hc = hm = (0, 0, 0), hN = 0, bs = 0
 *     for j = 0, 1 (outer), i = 0, 1 (inner): q = (x0 + i, y0 + j); a q outside the frame is skipped
 *       b = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay)
 *       consistent(q) = N'(q) >= 1
 *                    && (hit ? (z'(q) > 0 && fabsf(z'(q) - te) <= tol_depth * te) : !(z'(q) > 0))
 *                    && (id == NULL     || k'(q) == k)
 *                    && (normal == NULL || ((dn.x dn.x + dn.y dn.y) + dn.z dn.z) <= tol_normal * tol_normal),   dn = n - n'(q)
 *       if consistent: hc.ch = hc.ch + b * c'(q).ch;  hm.ch = hm.ch + b * m2'(q).ch;  hN = hN + b * N'(q);  bs = bs + b
 *     if !(usable && bs > 0.01f): as "no usable history".
 *     Else:
 *       hcn = hc / bs;  hmn = hm / bs;  N = fminf(hN / bs + 1.0f, 65536.0f);  alpha_p = fmaxf(1.0f / N, alpha)
 *       c = hcn + alpha_p * (C - hcn);   m2 = hmn + alpha_p * (C * C - hmn)
 *   Then, for every pixel with finite(C):
 *     out_color = c;  out_history = N
 *     out_variance = N >= 4 ? fmaxf(m2 - c * c, 0) * alpha_p : (variance_in ? variance_in(p) : +inf)
 * te is the depth the pixel's surface would have had in the previous frame, in that frame's units, so the depth test compares like with
 * like.  The variance is that of the accumulated mean: s^2 / N while alpha_p = 1 / N, and within a factor 2 (on the safe side) once the
 * exponential floor `alpha` holds.  The +inf is pt_variance_estimate's "no estimate" value, which pt_variance_denoise sanitises; a young
 * history (N < 4) passes the caller's own estimate through.  A camera that turned away (cp <= 0), a disoccluded surface (every tap
 * inconsistent) and a pixel that reprojects outside the previous frame all start a new history of length 1.
 * Cameras with a lens (lens_radius > 0) reproject through the lens centre; the consistency tests reject what that gets wrong.
 *
 * Rejected (PT_ERR_INVALID_ARG, on the host, before any device call): a NULL state, params, cam, color, depth or out_color; a struct_size
 * other than sizeof(PtTemporalParams); alpha outside (0, 1]; a tolerance that is not finite and > 0; flags (none is defined); a degenerate
 * camera (above); an out plane overlapping a guide plane (depth, normal, id) or another out plane.  pt_temporal_create: width or height <= 0;
 * more than 2^30 pixels: PT_ERR_TOO_LARGE.
 *
 * Out of scope: shards (gather first, as for the denoisers); checkpointing the history; SVGF's 3 x 3 fallback search; moving geometry
 * other than what the guides already reject.  profiles/temporal_bench.txt holds the measured cost.                                   */
#define PT_TEMPORAL_DEFAULT_ALPHA 0.1f
#define PT_TEMPORAL_DEFAULT_TOL_DEPTH 0.1f
#define PT_TEMPORAL_DEFAULT_TOL_NORMAL 0.5f
/* NEXT FRAME above; asynchronous on `stream`, allocates nothing, launches no kernel. */
extern int pt_adaptive_next_frame(PtAccum* acc, void* stream);
typedef struct PtTemporal PtTemporal; /* device-resident history of one image sequence; 2 x 48 bytes per pixel */
typedef struct PtTemporalParams {
  int32_t struct_size; /* sizeof(PtTemporalParams) of the caller's header */
  float alpha, tol_depth, tol_normal;
  uint32_t flags;      /* none defined: 0 */
  int32_t reserved[3];
} PtTemporalParams;
/* Host function, no GPU: struct_size + the defaults above (alpha 0.1, tol_depth 0.1, tol_normal 0.5). */
void pt_temporal_params_init(PtTemporalParams* params);
/* Host function, no GPU: device bytes of the state of a width x height sequence; < 0 for invalid sizes. */
int64_t pt_temporal_state_bytes(int32_t width, int32_t height);
/* Allocates the state on the current device (the only allocation); no history yet. */
int pt_temporal_create(int32_t width, int32_t height, PtTemporal** out);
void pt_temporal_destroy(PtTemporal* state);
/* Forget the history: the next push starts one.  Asynchronous on `stream` (host bookkeeping only). */
int pt_temporal_reset(PtTemporal* state, void* stream);
/* Pushes since create / reset (host-side count; -1 for NULL). */
int32_t pt_temporal_frames(const PtTemporal* state);
int pt_temporal_push(PtTemporal* state, const PtTemporalParams* params, const PtCamera* cam, const float* color, const float* depth,
                     const float* normal, const int32_t* id, const float* variance_in, float* out_color, float* out_variance,
                     float* out_history, void* stream);

/* ---- display stage: histogram auto-exposure and filmic tone curves ---------------------------------------------------------------------
 * Added without an ABI version change, like PtAccum: a caller detects the feature by the presence of these symbols.  Nothing above changes:
 * pt_tonemap_rgb8 and pt_accum_tonemap_rgb8 stay the reference's output stage.
 *
 * The end of the interactive chain render -> guides -> temporal -> filter -> DISPLAY: the frame is metered with a luminance histogram on the
 * device, an exposure is solved from it (with eye adaptation across the frames of a sequence), and exposure, a tone curve and the existing
 * quantiser are applied — without a round trip to the host between metering and applying.
 *
 * Scope.  pt_denoise's — whole frames only, no scene involved: color and linear_out are [height][width][3], y = 0 the bottom row (the layout
 * pt_render writes with shard_count = 1); rgb8_out is [height][width][3] bytes, row 0 = top (pt_tonemap_rgb8's).  pt_display_meter,
 * pt_display_set_exposure, pt_display_reset and pt_display_apply are asynchronous on `stream` and allocate nothing (pt_display_create is the
 * only allocation); calls on one PtDisplay are stream-ordered like renders of one PtScene.
 *
 * DEFINITION.  Every float value is IEEE binary32 unless binary64 is named, every operation below is rounded once, nothing is fused, the
 * order of operations is the one written, and divisions are the correctly rounded ones.
 *
 * Luminance (Rec. 709).  Y = (0.2126f * R + 0.7152f * G) + 0.0722f * B.
 *
 * Metering histogram.  256 uint32 bins, 8 per octave over the 32 octaves [2^-16, 2^16), keyed on the bit pattern of Y (no logarithm):
 *   a pixel whose Y is NaN, +-inf, negative or +-0 is not binned: it is counted in `rejected`;
 *   otherwise bin = clamp((int)(bits(Y) >> 20) - ((127 - 16) << 3), 0, 255)  (denormals and Y < 2^-16: bin 0; Y >= 2^16: bin 255).
 * Only the pixels of the metering rectangle [x0, x1) x [y0, y1) are read (frame coordinates: y = 0 the bottom row); PtDisplayParams' rect of
 * four zeros means the whole frame.  Counts are integers: the histogram does not depend on the order the hardware adds them in.
 *
 * Solve (integers and one binary64 division).  N = the sum of the bins; lo_n = (uint64)N * lo_permille / 1000, hi_n likewise from
 * hi_permille.  Walking the bins in ascending order, bin b holds the ranks [r_b, r_b + count_b), r_b = the sum of the bins below it, and
 * contributes c_b = the number of its ranks inside [lo_n, hi_n).  Its value, in 1/65536 octave, is the log2 of the geometric centre of
 * the bin:  value_b = 65536 * ((b >> 3) - 16) + LOGC[b & 7],  LOGC[j] = round(65536 * log2(1 + (2j + 1) / 16)) = PT_DISPLAY_LOGC below.
 *   S = sum of c_b * value_b (int64; |S| < 2^53 since N <= 2^31),  C = sum of c_b
 *   C == 0 (nothing binned, or an empty band): the exposure stays as it is.  Otherwise
 *   t   = (float)(((double)S / (double)C) * 0x1p-16)                     the mean log2 luminance of the band
 *   e_t = fminf(fmaxf((PT_DISPLAY_LOG2_KEY - t) + ev_bias, ev_min), ev_max)   the target exposure in stops
 *
 * Adaptation.  The first metering since create or reset that solves (C > 0) sets e = e_t.  Later ones set e = e + (e_t - e) * a, with
 * a = adapt_up when e_t > e, else adapt_down (1 = instant).  pt_display_set_exposure sets e = fminf(fmaxf(ev, -32), 32) and counts as a
 * first metering: the next one adapts from it.  e lives in device memory; nothing on the way to pt_display_apply reads it on the host.
 *
 * Scale.  k = ceilf(e);  scale = ldexpf(pt_exp_neg((k - e) * 0x1.62e430p-1f), (int)k)  — 2^e: k - e is exact and lies in [0, 1), inside
 * pt_exp_neg's domain (pt_denoise's function, verbatim); an integer e gives exactly 2^e and e == 0 exactly 1.
 *
 * Curve, per channel.  x = c * scale;  if !(x >= 0): x = +0 (NaN and negative values);  if x > 0x1p20f: x = 0x1p20f;  then
 *   PT_TONE_REFERENCE  y = x
 *   PT_TONE_REINHARD   y = (x * (1.0f + x * iw2)) / (1.0f + x),  iw2 = 1.0f / (white * white) computed once on the host (extended
 *                      Reinhard: `white` is the input that maps to 1)
 *   PT_TONE_ACES       y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f)       (Narkowicz's fit of the ACES film curve)
 *
 * Output.  rgb8_out = pt_tonemap_rgb8's quantiser of y (sqrt, clamp to [0, 0.999], * 256, truncate, int(NaN) = 0) with its vertical flip;
 * linear_out = y, not flipped, in the frame buffer's layout.  The transfer stays the reference's gamma 2.  PT_TONE_REFERENCE at e = 0 gives
 * pt_tonemap_rgb8's bytes exactly, for every input.  With state == NULL pt_display_apply takes e = fminf(fmaxf(ev_bias, -32), 32): the
 * manual, stateless use.
 *
 * Rejected (PT_ERR_INVALID_ARG, on the host, before any device call and before the state is read): a NULL params, color or (pt_display_meter,
 * pt_display_set_exposure, pt_display_reset, pt_display_exposure, pt_display_histogram) state; both outputs NULL; a struct_size other than
 * sizeof(PtDisplayParams); width or height <= 0 or more than 2^31 pixels; an unknown tone; flags (none is defined);
 * lo_permille >= hi_permille or either outside [0, 1000]; an adaptation rate outside (0, 1]; ev_min > ev_max or either outside [-32, 32];
 * an ev_bias that is not finite, an ev that is NaN; a `white` whose iw2 is not a finite binary32 number > 0; a rectangle that is not all zeros and is
 * empty or leaves the frame; rgb8_out overlapping color or linear_out; linear_out overlapping color without being color.                  */
#define PT_TONE_REFERENCE 0
#define PT_TONE_REINHARD 1
#define PT_TONE_ACES 2
#define PT_DISPLAY_LOG2_KEY (-0x1.3ca9c6p+1f) /* log2(0.18): the band's geometric mean is exposed to middle grey */
#define PT_DISPLAY_LOGC {5732, 16248, 25711, 34312, 42196, 49472, 56229, 62534}
/* The defaults (pt_display_params_init); DESIGN.md gives the reason for each: the ACES curve; no bias; the full +-16 stop range; the band
 * from the 40th to the 95th percentile (shadows do not drive the exposure, the brightest 5 % — emitters — do not either); instant
 * adaptation (a still image has no history); white 4 (Reinhard only). */
#define PT_DISPLAY_DEFAULT_TONE PT_TONE_ACES
#define PT_DISPLAY_DEFAULT_EV_BIAS 0.0f
#define PT_DISPLAY_DEFAULT_EV_MIN -16.0f
#define PT_DISPLAY_DEFAULT_EV_MAX 16.0f
#define PT_DISPLAY_DEFAULT_LO_PERMILLE 400
#define PT_DISPLAY_DEFAULT_HI_PERMILLE 950
#define PT_DISPLAY_DEFAULT_ADAPT_UP 1.0f
#define PT_DISPLAY_DEFAULT_ADAPT_DOWN 1.0f
#define PT_DISPLAY_DEFAULT_WHITE 4.0f
typedef struct PtDisplay PtDisplay; /* device-resident metering state: the histogram, `rejected`, e, scale */
typedef struct PtDisplayParams {
  int32_t struct_size; /* sizeof(PtDisplayParams) of the caller's header */
  int32_t tone;        /* PT_TONE_* */
  uint32_t flags;      /* none defined: 0 */
  float ev_bias, ev_min, ev_max;
  int32_t lo_permille, hi_permille;
  float adapt_up, adapt_down;
  float white;
  int32_t rect_x0, rect_y0, rect_x1, rect_y1; /* the metering rectangle; four zeros: the whole frame */
  int32_t reserved;
} PtDisplayParams;
/* Host function, no GPU: struct_size + the defaults above. */
void pt_display_params_init(PtDisplayParams* params);
/* Allocates the state on the current device (the only allocation): no exposure yet (e = 0, scale = 1), empty histogram. */
int pt_display_create(PtDisplay** out);
void pt_display_destroy(PtDisplay* state);
/* Back to the state after create: the next metering is instant. */
int pt_display_reset(PtDisplay* state, void* stream);
/* Meterings since create / reset (host-side count; -1 for NULL). */
int32_t pt_display_frames(const PtDisplay* state);
/* Histogram, solve and adaptation; asynchronous on `stream`: nothing comes back to the host. */
int pt_display_meter(PtDisplay* state, const PtDisplayParams* params, const float* color, int32_t width, int32_t height, void* stream);
/* A manual exposure, in stops. */
int pt_display_set_exposure(PtDisplay* state, float ev, void* stream);
/* Exposure, curve and quantiser in one pass; either output may be NULL, state may be NULL (e = ev_bias), linear_out may be color. */
int pt_display_apply(const PtDisplay* state, const PtDisplayParams* params, const float* color, int32_t width, int32_t height,
                     uint8_t* rgb8_out, float* linear_out, void* stream);
/* For inspection and tests; both SYNCHRONISE `stream`: the exposure e, and the last metering's 256 bins followed by `rejected`. */
int pt_display_exposure(const PtDisplay* state, float* ev_host, void* stream);
int pt_display_histogram(const PtDisplay* state, uint32_t host[257], void* stream);
/* The launch geometry of the LAST pt_display_meter and pt_display_apply of this process: out[0] = the metering kernel's workgroups,
 * out[1] = its threads per workgroup, out[2] = the trips a thread makes through its metering loop, out[3] = the pixels it takes per trip
 * (4, as three 16-byte loads, where the metered pixels are one contiguous 16-byte aligned range — a whole frame, a rectangle as wide as
 * the frame —, else 1: a frame of more than out[0] * out[1] * out[3] pixels takes the loop more than once), out[4] / out[5] = the apply
 * kernel's grid (x, y), out[6] = the values a thread of it takes per row (4 where the width is a multiple of 4 and the planes are 16-byte
 * aligned, rgb8_out 4-byte; else 1), out[7] = its tone + 1; zeros before the first call.  The bits do not depend on any of it.  For tests. */
int pt_debug_last_display(int32_t out[8]);

/* ---- function-level probes (parity tests call these; not used by render) ---- */

/* One iteration of the bounce loop render.hpp:58-89 per record: hit_world,
 * emitted, scatter (or sky).  n records in, n out; host pointers.              */
typedef struct PtBounceIn {
  float origin[3];
  float dir[3];
  float time;
  uint32_t rng_state;
  float attenuation[3];
} PtBounceIn;

enum { PT_BOUNCE_MISS = 0, PT_BOUNCE_SCATTERED = 1, PT_BOUNCE_ABSORBED = 2 };

typedef struct PtBounceOut {
  int32_t status;     /* PT_BOUNCE_* */
  int32_t hittable;   /* index of the nearest hittable, -1 on miss */
  int32_t material;   /* material index of the hit, -1 on miss */
  int32_t front_face;
  float t;
  float p[3];
  float normal[3];
  float u, v;         /* 0 unless the scene has an image texture */
  float color[3];     /* MISS: attenuation*sky; ABSORBED: emitted; SCATTERED: new attenuation */
  float sc_origin[3]; /* scattered ray (SCATTERED only) */
  float sc_dir[3];
  float sc_time;
  uint32_t rng_state; /* generator state after the bounce */
} PtBounceOut;

int pt_debug_bounce(const PtScene* scene, const PtBounceIn* in, PtBounceOut* out, int32_t n);

/* First camera ray of a pixel: render.hpp:96-99 + camera.hpp:93-100.
 * rng_state in/out; ray out.                                                   */
typedef struct PtCameraRay {
  float origin[3];
  float dir[3];
  float time;
  uint32_t rng_state;
} PtCameraRay;
int pt_debug_camera_rays(const PtCamera* cam, int32_t width, int32_t height,
                         const int32_t* xy /*[n][2]*/, const uint32_t* rng_in,
                         PtCameraRay* out, int32_t n);

/* Host-only view of what pt_scene_create() uploads (no GPU needed): the flattened blob
 * ([n_runs run headers (device kind, first record offset, count, first hittable)] then the
 * per-kind 16-byte records) and the material table (4 x 16 bytes each, texture inlined).
 * Pass NULL buffers to query the sizes.  flags_out: bit0 = has image texture, bit1 = has medium, bit2 = a triangle run
 * carries a triangle pool (exact culling tables for long runs of Moller-Trumbore triangles; csrc/pt_tripool.hpp).        */
int pt_debug_flatten(const PtSceneDesc* desc, float* blob_out, int64_t blob_cap_f4, int32_t* n_blob_f4,
                     int32_t* n_runs, float* mats_out, int64_t mats_cap_f4, int32_t* flags_out);
/* the same for an explicit PtTuning (NULL: defaults + environment, i.e. pt_debug_flatten) */
int pt_debug_flatten_tuned(const PtSceneDesc* desc, const PtTuning* tuning, float* blob_out, int64_t blob_cap_f4, int32_t* n_blob_f4,
                           int32_t* n_runs, float* mats_out, int64_t mats_cap_f4, int32_t* flags_out);

/* Host-only statistics of the triangle pool pt_scene_create() would build (no GPU needed): out[0] = triangles in pooled runs,
 * out[1] = triangles whose band covers every direction in the first map ("slivers"), out[2] = entries of the first direction map,
 * out[3] = of the other two together, in units of 1024 (0: not built), out[4] = the three maps' resolutions, 10 bits each, out[5] = 1000 x mean
 * grid cells per triangle, out[6] = blob size in 16-byte records (always), out[7] = spheres that sit in a sphere culling grid (always). */
int pt_debug_tri_pool(const PtSceneDesc* desc, int32_t out[8]);
/* The tables of the scene's triangle pools (host-only, like pt_debug_flatten): the second buffer pt_scene_create uploads beside the blob
 * (pt_flatten.hpp: put_tri_pool says what the pools' headers in the blob point at).  pool_out may be NULL to query the size (in 16-byte
 * records); tuning NULL = defaults + environment.                                                                                       */
int pt_debug_flatten_pool(const PtSceneDesc* desc, const PtTuning* tuning, float* pool_out, int64_t pool_cap_f4, int64_t* n_pool_f4);

/* What the scheduler decided for the LAST render of this scene (blocks until that render is done): out[0] = tiles sent
 * through the wide phase, out[1] = lanes per pixel there (0 when the render had no cost-probe pass or used a kernel
 * without that phase).  For tuning the makespan model (csrc/pt_render.hip: lpt_order_kernel) and for tests.            */
int pt_debug_schedule(const PtScene* scene, int32_t out[2]);

/* What the launcher decided for the LAST frame launch of this scene (csrc/pt_render.hip: plan_pass): out[0] = workgroups launched,
 * out[1] = lanes of a wave that take pixels (PtTuning.lanes_cap's rule; 64 = whole tiles), out[2] = queue positions at the head of the
 * cost-sorted order that are handed out 16 pixels at a time (PtTuning.heavy_tiles' rule; 0 = none), out[3] = 1 if the sphere-grid walk
 * through the LDS pair queue was picked.  For tests of those rules.                                                                  */
int pt_debug_last_launch(const PtScene* scene, int32_t out[4]);

/* The launcher's geometry rules for ONE pass (csrc/pt_render.hip: plan_pass), host-only: no scene, no device call, so the rules can be
 * checked without a GPU and on a "chip" of any size.  Detected by its presence, like the entry points above that were added later.
 * facts[0] = CUs, [1] = the kernel's resident workgroups per CU, [2] = threads per workgroup; the kernel variant: [3] chain-bound (the
 * headline family), [4] walks a sphere grid, [5] walks it through the pair queue; [6] = PtRenderParams.flags; PtTuning fields as a scene
 * takes them: [7] blocks_per_cu, [8] lanes_cap, [9] heavy_tiles, [10] != 0: chain_priority = -1; [11] = work units in the queue (tiles;
 * PT_FLAG_FAST_RNG: tiles x chunks), [12] = local pixels (64 x tiles; fast mode: x chunks), [13] = PtRenderParams.samples; the pass:
 * [14] != 0 the cost probe, [15] != 0 a tile order exists, [16] != 0 a wide phase exists, [17] != 0 whole tiles per wave, [18] = the
 * scatter stride of the triangle-pool kernels (0: none), [19] = fast-mode chunks per pixel (0: parity mode).
 * out[0] = workgroups, [1] = their waves, [2] = lanes of a wave that take pixels, [3] = whole tiles per wave after that cap, [4] / [5] =
 * queue positions of the narrow head and the lanes that take them, [6] = queue position from which the chain priorities act, [7..9] =
 * their thresholds for priority 1, 2, 3, [10..13] = what pt_debug_last_launch reports after a frame pass of these facts.               */
int pt_debug_plan_pass(const int64_t facts[20], int32_t out[14]);

/* Which kernel instantiations the LAST pt_render / pt_render_accumulate of this scene launched: out[0..11] the cost-probe pass,
 * out[12..23] the frame pass.  Word 0 of a pass is the kernel family — 0 no such pass, 1 render_kernel, 2 render_kernel_stream,
 * 3 the single-stream kernel (PT_FLAG_SINGLE_STREAM), 4 the binned renderer's step / finish pair — and the words after it are that
 * family's template arguments in the template's order (csrc/pt_device.hpp; unused words 0): render_kernel UV, LDS, MLDS, COOP, CL, FAST,
 * BADOUEL, GRID, TRIPOOL, MATS, BLOCK; render_kernel_stream UV, FAST, BADOUEL; binned UV, MATS.  The launcher takes a kernel and its
 * tag from one constant (csrc/pt_render.hip: picked_of), so the tag is the kernel that ran.  For tests (tests/kernel_variant_cases.py). */
int pt_debug_last_kernels(const PtScene* scene, int32_t out[24]);

/* The pool plan the LAST frame pass of this scene was given (csrc/pt_device.hpp: PoolPlan): out[0] = 1 if the pass's kernel took the
 * scene's ONE slab pool from its kernel arguments instead of walking the run list (a rect / box-only scene whose first run heads a pool
 * with an octant table that spans every run, rendered by an LDS-resident kernel compiled for such scenes, rays allowed to be regular),
 * out[1] = the pool's entries, out[2] / out[3] = the 16-byte-record offsets in the blob of its exact entries and of its octant table's
 * first record.  out[1..3] say what the scene's blob holds whether or not out[0] claims it.  For tests (tests/test_gpu_pool_plan.py).   */
int pt_debug_last_pool_plan(const PtScene* scene, int32_t out[4]);

/* The plan's first word as that pass's kernel read it (csrc/pt_device.hpp: PoolPlan.one), which says what the kernel DID with a claimed
 * pool: 0 = no plan, the run list was walked; 2 = the pool is one chunk of the slab pass (<= 16 entries) and the kernel took it from its
 * arguments; 1 = claimed, but larger than one chunk: the LDS-resident rect / box-only kernels hold no chunk loop on that path and walked
 * the run list record by record.  (pt_debug_last_pool_plan's out[0] is 1 for both claimed kinds.)  For tests (tests/test_gpu_headline_flags.py). */
int pt_debug_last_pool_word(const PtScene* scene, int32_t* out);

/* The same derivation host-only — no device call — for the frame pass of a render of `desc` with `params` (tuning NULL = defaults +
 * environment): out[0..3] as above; out[4] = offset of the pool's slab entries, out[5] = the bits of its largest |coordinate|,
 * out[6..8] = the first run's header (device kind, first record, count); out[9] = 1 if the SCENE allows the plan (whatever kernel and
 * flags), out[10] / out[11] = the LDS and MATS template arguments of the kernel the launcher would pick (0 where another kernel family
 * runs).  Scenes that are not rects and boxes under lambertian / light materials never read a plan: out[0] = 0 without asking further. */
int pt_debug_pool_plan(const PtSceneDesc* desc, const PtTuning* tuning, const PtRenderParams* params, int32_t out[12]);

/* The SHADE TABLE of the flattened scene (csrc/pt_flatten.hpp: Flat::shade), host-only: one 16-byte record per hittable of a small scene
 * of rects and boxes under lambertian / light materials over solid textures — (the material's colour, one word: bits 0-1 a rect's axis,
 * bit 2 box, bits 4-6 the material kind, bits 8-30 the hittable's index) — from which the kernels of such scenes shade a hit.  The
 * record of the hittable whose records start at blob offset `off` (16-byte records) is record (off >> 1) - *base; records no hittable
 * maps to are zero.  *n_f4 = the table's records (0: the scene has none); table_out may be NULL to query.  For tests.                 */
int pt_debug_shade_table(const PtSceneDesc* desc, const PtTuning* tuning, float* table_out, int64_t table_cap_f4, int32_t* n_f4, int32_t* base);

/* Which aov_kernel the LAST pt_render_aov of this scene launched: out[0] = its sphere-grid walk (1 wave-synchronous, 2 through the LDS pair
 * queue; scenes without a sphere grid: 1), out[1] = 1 if u,v are tracked through the scan; both 0 before the first pass.  For tests.  */
int pt_debug_last_aov(const PtScene* scene, int32_t out[2]);

/* Device math used by the kernel, elementwise over host arrays.
 * op: 0 sin 1 cos 2 log 3 pow5 4 atan2(a,b) 5 asin 6 fmod(a,1) 7 sqrt 8 div(a,b)
 *     9 the shared-reciprocal exact quotient a/b used for rect/box sides (pt_device.hpp: div_exact)
 *     10 the reciprocal 1/a of the ray context, correctly rounded for 2^-40 <= |a| <= 2^40 (rcp_rn_guarded)
 *     11 the square root of a = 0 or 2^-60 <= a <= 4 as the RNG's unit_vec / in_unit_disk take it (sqrt_rn_unit)
 *     12 a / sqrt(b) as the sky of a regular ray takes unit_vector(d).y (b = d.d in [3 * 2^-80, 3 * 2^80]; sky_unit_y)
 *     13 the checker texture's decision `sin(a) sin(b) sin(1) < 0` as 1.0 / 0.0 (texture.hpp:43-45; checker_sines_negative)
 *     14 / 15 sin / cos through the fused form the unit-ball sampler uses (pt_math.hpp: sincosf_)                            */
int pt_debug_math(int32_t op, const float* a, const float* b, float* out, int64_t n);

/* The texel (column i, row j) an image texture of width x height texels and frequency freq selects on a sphere whose unit normal at the
 * hit is n (n_xyz: 3 floats per entry) — texture.hpp:140-157 over sphere.hpp:13-24.  out_ij = what the render kernels take (the texel
 * straight from the normal where that is provably unambiguous, the reference's chain otherwise: pt_device.hpp sphere_texel_fast),
 * exact_ij = the reference's chain alone, took_fast = 1 where the short form decided.  2 ints per entry.  uv4 (optional, 4 floats per
 * entry): (u, v) of the reference's chain, then (u, v) of the binary32 approximations — their deviation is what the short form's
 * margin must cover.  For tests.                                                                                                       */
int pt_debug_sphere_texel(const float* n_xyz, int64_t n, float freq, int32_t width, int32_t height, int32_t* out_ij, int32_t* exact_ij,
                          uint8_t* took_fast, float* uv4);

#ifdef __cplusplus
}
#endif
#endif /* PT_RENDER_H */
