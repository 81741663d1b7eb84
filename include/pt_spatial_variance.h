/*
 * pt_spatial_variance.h — the spatial variance estimate: a per-pixel noise estimate for frames that have no other.
 *
 * Declared in a header of its own for the reason pt_post.h is one: pt_render.h's and pt_post.h's declarations are pinned one for one by
 * their ABI tables and stream-contract tables.  The stage is exported from the same libpt_render.so and listed in a table of its own
 * (path_tracer_amd/abi.py: SPATIAL_VARIANCE_SIGNATURES), which is held to this header by the same two rules.  Error codes, pt_last_error
 * and the conventions — device pointers, whole frames [height][width][3] with y = 0 the bottom row, a `void* stream` that is a
 * hipStream_t — are pt_render.h's.  A caller detects the stage by the presence of its symbols; PT_ABI_VERSION does not change.
 */
#ifndef PT_SPATIAL_VARIANCE_H
#define PT_SPATIAL_VARIANCE_H

#include "pt_render.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- spatial variance estimate (SVGF's fourth piece: Schied et al., HPG 2017, section 4.2) ------------------------------------------------
 * pt_variance_denoise needs the variance of every pixel's mean.  pt_variance_estimate gives one for an adaptive accumulator only, and
 * every producer of a variance plane writes +inf — "no estimate" — somewhere: pt_variance_estimate where a half buffer is empty,
 * pt_temporal_push where a history is younger than 4 frames and the caller had no estimate, pt_firefly for a repaired pixel.
 * pt_variance_denoise sanitises those to +0 and leaves such a pixel nearly alone.  This stage estimates the variance of a pixel from the
 * frame itself: from the squared differences of ADJACENT pixels in a (2 radius + 1)^2 window, over the pixels of the window that lie on
 * the centre's surface by the guides.  Given a variance plane it fills only the pixels that have no estimate (fill mode); given none it
 * makes the whole plane, so that a plain frame — render(), a plain accumulator, a frame from disk — can be variance-filtered.
 *
 * Why differences and not moments: the variance about the window's mean takes every shading gradient for noise; the difference of two
 * adjacent pixels sees a gradient g as g^2 against the 2 sigma^2 of the noise.  For independent pixels of equal variance
 * E[(X - Y)^2] = 2 sigma^2, hence the 2 in the divisor.  What the guides do not separate is still taken for noise: a texture, a shadow
 * edge, and above all what a mirror or a glass shows — a stated limit of the stage (DESIGN.md section 1 has the figures).
 *
 * Scope.  pt_firefly's — whole frames only, no scene involved, no shards (gather and unshard first): color, albedo, normal, variance_in
 * and variance_out are [height][width][3] float, depth is [height][width] float, id is [height][width] int32; the guides are
 * pt_render_aov's planes for the frame's camera.  albedo, normal, depth, id, variance_in and counts are optional (NULL).  variance_out may
 * BE variance_in (each pixel reads and writes only its own variance) and must not overlap any other plane.  pt_spatial_variance is
 * asynchronous on `stream` and allocates nothing.
 *
 * DEFINITION.  Every value is IEEE binary32, every operation below is rounded once, nothing is fused, the order of operations is the one
 * written, and the divisions are the correctly rounded ones.
 *   m(q).ch  = DEMODULATE ? albedo(q).ch + 1e-3f : 1          e(q).ch = color(q).ch / m(q).ch
 *   usable(q)      : q inside the frame, and fabsf(e(q).ch) < +inf for each channel (NaN fails)
 *   consistent(q|p): usable(q)
 *                 && (depth  == NULL || (z_p > 0 ? (z_q > 0 && fabsf(z_q - z_p) <= tol_depth * z_p) : !(z_q > 0)))
 *                 && (id     == NULL || k_q == k_p)
 *                 && (normal == NULL || ((dn.x dn.x + dn.y dn.y) + dn.z dn.z) <= tol_normal * tol_normal),  dn = n_p - n_q
 *         (pt_temporal_push's three tests with te = z_p, verbatim; the default tolerances are its 0.1 and 0.5)
 * For pixel p = (x, y), r = radius:
 *   keep(p) = variance_in != NULL && every channel of variance_in(p) is (>= 0 && < +inf)         (pt_variance_denoise's sanitising test)
 *   keep(p):   variance_out(p) = variance_in(p), the bits kept
 *   otherwise: ssd = (+0, +0, +0), np = 0
 *     for dy = -r ... r (outer), dx = -r ... r (inner): q = (x + dx, y + dy); skip unless consistent(q|p)
 *       if dx < r and consistent(q'|p),  q'  = (x + dx + 1, y + dy):  d = e(q) - e(q');   ssd.ch = ssd.ch + d.ch * d.ch;   np = np + 1
 *       if dy < r and consistent(q''|p), q'' = (x + dx, y + dy + 1):  d = e(q) - e(q'');  ssd.ch = ssd.ch + d.ch * d.ch;   np = np + 1
 *     usable(p) && np >= min_pairs:  variance_out.ch = (ssd.ch / (2.0f * (float)np)) * (m(p).ch * m(p).ch);   estimated += 1
 *     else:                          variance_out    = +inf  ("no estimate", the convention everywhere);       holes += 1
 * Both members of a pair lie inside the window and on p's surface; p itself takes part only as one of the window's pixels, and need not
 * be consistent with itself (a NaN normal at p fails every normal test: np = 0, a hole).  With DEMODULATE the estimate is made on the
 * demodulated colour and scaled back by m(p)^2, the variance of m X being m^2 that of X.
 * What this leaves open elsewhere is fixed here.  d.ch * d.ch (or d itself) may overflow to +inf: then ssd.ch and variance_out.ch are +inf
 * (NaN where m(p).ch * m(p).ch is 0), the pixel still counts as estimated, and pt_variance_denoise sanitises the channel like any other
 * "no estimate".  A z_p that is NaN is not > 0: p is taken as a miss and is consistent with the q whose z_q is not > 0 (a NaN among
 * them).  tol_depth * z_p may overflow to +inf and then accepts every z_q > 0.  A -0 in variance_in is >= 0: the pixel is kept, the -0
 * with it.  A NaN, a negative or an infinite channel in variance_in makes the WHOLE pixel one to estimate.  A 1 x 1 frame has no pair:
 * one hole (unless it is kept).  The window is clipped by the frame: a pixel outside is never consistent.
 *
 * Counts.  counts (if not NULL) is a device uint32[2], 8-byte aligned: {estimated, holes} of this call; the kept pixels are the rest.
 * The call zeroes it on `stream` and the kernel adds to it with integer atomics (both counts in one 64-bit add, once per workgroup), so
 * the result does not depend on the order of the adds.  Nothing is read back: the caller copies the eight bytes when it wants them.
 *
 * Rejected (PT_ERR_INVALID_ARG, on the host, before any device call): a NULL params, color or variance_out; a struct_size other than
 * sizeof(PtSpatialVarianceParams); width or height <= 0; a radius outside 1 ... PT_SVAR_MAX_RADIUS; min_pairs < 1; a tol_depth or
 * tol_normal that is not finite and > 0; flags other than PT_SVAR_DEMODULATE and PT_SVAR_NO_LDS; PT_SVAR_DEMODULATE without albedo; a
 * counts that is not 8-byte aligned; variance_out (unless it is variance_in itself) or counts overlapping color, a guide or variance_in;
 * variance_out and counts overlapping one another.  More than 2^30 pixels: PT_ERR_TOO_LARGE.
 *
 * Out of scope: shards; radii above PT_SVAR_MAX_RADIUS; edge-aware weights in place of the accept / reject tests; a temporal estimate
 * (pt_temporal_push has one).  profiles/spatial_variance_bench.txt holds the measured cost and the quality record.                     */
#define PT_SVAR_DEMODULATE 1u /* estimate on color / (albedo + 1e-3f), scale back by m(p)^2; requires albedo */
#define PT_SVAR_NO_LDS 2u     /* A/B switch, same bits: every pixel of the window is read from global memory (default: from an LDS-staged tile) */
#define PT_SVAR_MAX_RADIUS 3
/* The workgroup's tile, for callers that size tests by it: PT_SVAR_TILE_W x PT_SVAR_TILE_H pixels, one lane each, staged with a halo of
 * PT_SVAR_MAX_RADIUS pixels. */
#define PT_SVAR_TILE_W 32
#define PT_SVAR_TILE_H 8
/* The defaults (pt_spatial_variance_params_init): the setting of the sweep {radius 2, 3} x {min_pairs 2, 4, 8} with the smallest worst
 * ratio MSE(filtered) / MSE(noisy) over 8, 32 and 128 spp Cornell frames; the tolerances are
 * PT_TEMPORAL_DEFAULT_TOL_DEPTH and PT_TEMPORAL_DEFAULT_TOL_NORMAL.  The defaults demodulate, as pt_variance_denoise's do, and the record
 * was made so: without it the 128 spp frame comes out of the filter worse than it went in.  A caller without an albedo plane clears the
 * flag. */
#define PT_SVAR_DEFAULT_RADIUS 2
#define PT_SVAR_DEFAULT_MIN_PAIRS 4
#define PT_SVAR_DEFAULT_TOL_DEPTH 0.1f
#define PT_SVAR_DEFAULT_TOL_NORMAL 0.5f
#define PT_SVAR_DEFAULT_FLAGS PT_SVAR_DEMODULATE
typedef struct PtSpatialVarianceParams {
  int32_t struct_size; /* sizeof(PtSpatialVarianceParams) of the caller's header */
  int32_t width, height;
  int32_t radius;      /* the window is (2 radius + 1)^2 pixels; 1 ... PT_SVAR_MAX_RADIUS */
  int32_t min_pairs;   /* the smallest number of pairs that gives an estimate; >= 1 */
  float tol_depth, tol_normal; /* the consistency tolerances; finite, > 0 */
  uint32_t flags;      /* PT_SVAR_DEMODULATE, PT_SVAR_NO_LDS */
  int32_t reserved[2];
} PtSpatialVarianceParams;
/* Host function, no GPU: struct_size + the defaults above for a frame of width x height. */
void pt_spatial_variance_params_init(PtSpatialVarianceParams* params, int32_t width, int32_t height);
/* The stage defined above; asynchronous on `stream`, allocates nothing. */
int pt_spatial_variance(const PtSpatialVarianceParams* params, const float* color, const float* albedo, const float* normal,
                        const float* depth, const int32_t* id, const float* variance_in, float* variance_out, uint32_t* counts,
                        void* stream);
/* How the LAST pt_spatial_variance of this process ran: out[0] = 0 not run, 1 the window from global memory (PT_SVAR_NO_LDS), 2 from an
 * LDS-staged tile; out[1] / out[2] = the frame's tiles (x, y) of PT_SVAR_TILE_W x PT_SVAR_TILE_H pixels, which the workgroups walk;
 * out[3] = the radius.  The bits do not depend on the path.  For tests. */
int pt_debug_last_spatial_variance(int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* PT_SPATIAL_VARIANCE_H */
