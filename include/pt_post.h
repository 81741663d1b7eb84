/*
 * pt_post.h — image-space stages added after include/pt_render.h was closed to new entry points.
 *
 * pt_render.h's declarations are pinned one for one by the ABI table and by the stream-contract table; stages added from here on are
 * declared in this header, exported from the same libpt_render.so, and listed in tables of their own (path_tracer_amd/abi.py:
 * POST_SIGNATURES), which are held to this header by the same two rules.  Error codes, pt_last_error and the conventions — device pointers,
 * whole frames [height][width][3] with y = 0 the bottom row, a `void* stream` that is a hipStream_t — are pt_render.h's.  A caller detects a
 * stage by the presence of its symbols; PT_ABI_VERSION does not change.
 */
#ifndef PT_POST_H
#define PT_POST_H

#include "pt_render.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- firefly stage: clamp outliers to their neighbours, repair NaN / inf ---------------------------------------------------------------
 * Between render and the filters of the chain render -> guides -> temporal -> filter -> display.  Every stage of that chain passes a
 * firefly through: the a-trous filters contain a non-finite pixel where it is and no tap matches a finite outlier, pt_temporal_push stores
 * a non-finite colour with N = 0, the display stage counts it as rejected.  This stage compares every pixel's luminance with the largest
 * (rank 1) or second largest (rank 2) luminance among its up to eight neighbours, scales a brighter pixel down to k times that, and
 * optionally replaces a pixel that is not finite by the mean of its finite neighbours.
 *
 * THE CLAMP IS BIASED: it only ever removes energy, so the mean of clamped frames is darker than the mean of the frames.  It is therefore off
 * by default everywhere — no other entry point calls it, and every host takes it as an explicit option.
 *
 * Scope.  pt_denoise's — whole frames only, no scene involved, no shards (gather and unshard first): color, variance, out and variance_out
 * are [height][width][3].  variance (the variance of each pixel's mean per channel: pt_variance_estimate's plane, or a temporal one),
 * variance_out and counts are optional (NULL).  `out` must not overlap `color` (a pixel reads its neighbours); variance_out may BE variance
 * (each pixel reads and writes only its own value).  pt_firefly is asynchronous on `stream` and allocates nothing.
 *
 * DEFINITION.  Every value is IEEE binary32, every operation below is rounded once, nothing is fused, the order of operations is the one
 * written, and the division is the correctly rounded one.
 *   Y(c)      = (0.2126f * R + 0.7152f * G) + 0.0722f * B        the display stage's luminance, verbatim
 *   finite(q) : fabsf(ch) < +inf for each of q's three colour channels (NaN fails)
 * For pixel p = (x, y):
 *   m1 = m2 = -inf, n = 0, sum = (+0, +0, +0)
 *   for dy = -1 ... 1 (outer), for dx = -1 ... 1 (inner), (dx, dy) != (0, 0): q = (x + dx, y + dy); a q outside the frame or with
 *   !finite(q) is skipped; otherwise
 *     n = n + 1;   sum.ch = sum.ch + c(q).ch;   Yq = Y(c(q))
 *     if (Yq > m1) { m2 = m1; m1 = Yq; } else if (Yq > m2) m2 = Yq;
 *   m = rank == 1 ? m1 : m2
 *   finite(p):   Yp = Y(c(p)),  L = k * m
 *     if n >= rank && Yp > L && Yp > 0:   s = (L > 0 ? L : +0) / Yp
 *          out.ch = c(p).ch * s;   variance_out.ch = variance(p).ch * (s * s);   clamped += 1
 *     else out = c(p), variance_out = variance(p)
 *   !finite(p), PT_FIREFLY_REPAIR set and n > 0:
 *          out.ch = sum.ch / (float)n;   variance_out.ch = +inf  ("no estimate", pt_adaptive_error's convention);   repaired += 1
 *   otherwise out = c(p), variance_out = variance(p)                      (copies: the bits of a NaN are kept)
 * What this leaves open elsewhere is fixed here: Y of a finite pixel may overflow to +-inf (never to NaN: each product is smaller in
 * magnitude than its channel, and +-inf plus a finite value is +-inf) and is compared as it is — a Yp of +inf above a finite L gives s = +0;
 * a neighbour whose Yq is -inf counts in n and sum and never becomes m1 or m2, so m may be -inf with n >= rank, and then L = -inf and a pixel
 * of positive luminance is scaled by s = +0; ties (Yq == m1) go to m2; a pixel that is not brighter than L, or whose luminance is zero or
 * negative, is never touched; -0 channels scale to -0.  The variance of a clamped pixel is scaled like the variance of s * X; a variance value
 * is never tested: NaN, inf and negative values are multiplied or copied like any other.  A 1 x 1 frame and a frame of non-finite pixels only
 * have n = 0 everywhere and come back unchanged.
 *
 * Counts.  counts (if not NULL) is a device uint32[2], 8-byte aligned: {clamped, repaired} of this call.  The call zeroes it on `stream`
 * and the kernel adds to it with integer atomics (both counts in one 64-bit add), so the result does not depend on the order of the adds.  Nothing is read back: the caller
 * copies the eight bytes when it wants them.
 *
 * Rejected (PT_ERR_INVALID_ARG, on the host, before any device call): a NULL params, color or out; a struct_size other than
 * sizeof(PtFireflyParams); width or height <= 0; a rank other than 1 or 2; a k that is not finite or not > 0; flags other than
 * PT_FIREFLY_REPAIR and PT_FIREFLY_NO_LDS; variance_out without variance; out, variance_out (unless it is variance itself) or counts
 * overlapping color or variance; out, variance_out and counts overlapping one another.  More than 2^30 pixels: PT_ERR_TOO_LARGE.          */
#define PT_FIREFLY_REPAIR 1u
#define PT_FIREFLY_NO_LDS 2u /* A/B switch, same bits: every neighbour is read from global memory (default: from an LDS-staged tile) */
/* The workgroup's tile, for callers that size tests by it: PT_FIREFLY_TILE_W x PT_FIREFLY_TILE_H pixels, one lane each, staged with a halo
 * of one pixel. */
#define PT_FIREFLY_TILE_W 32
#define PT_FIREFLY_TILE_H 8
/* The defaults (pt_firefly_params_init): the parameter-free rule — the largest neighbour, k = 1, repair on — is the one setting of the sweep
 * {rank 1, 2} x {k 1, 2} over 4 ... 128 spp frames that never had a larger error than the frame it was given. */
#define PT_FIREFLY_DEFAULT_RANK 1
#define PT_FIREFLY_DEFAULT_K 1.0f
#define PT_FIREFLY_DEFAULT_FLAGS PT_FIREFLY_REPAIR
typedef struct PtFireflyParams {
  int32_t struct_size; /* sizeof(PtFireflyParams) of the caller's header */
  int32_t width, height;
  int32_t rank;        /* 1: the largest neighbour, 2: the second largest */
  float k;             /* the limit is k times that neighbour's luminance; finite, > 0 */
  uint32_t flags;      /* PT_FIREFLY_REPAIR, PT_FIREFLY_NO_LDS */
  int32_t reserved[2];
} PtFireflyParams;
/* Host function, no GPU: struct_size + the defaults above for a frame of width x height. */
void pt_firefly_params_init(PtFireflyParams* params, int32_t width, int32_t height);
/* The stage defined above; asynchronous on `stream`, allocates nothing. */
int pt_firefly(const PtFireflyParams* params, const float* color, const float* variance, float* out, float* variance_out,
               uint32_t* counts, void* stream);
/* How the LAST pt_firefly of this process ran: out[0] = 0 not run, 1 neighbours from global memory (PT_FIREFLY_NO_LDS), 2 from an LDS-staged
 * tile; out[1] / out[2] = the frame's tiles (x, y) of PT_FIREFLY_TILE_W x PT_FIREFLY_TILE_H pixels, which the workgroups walk; out[3] = the planes it wrote
 * (1: out, 2: out and variance_out).  The bits do not depend on it.  For tests. */
int pt_debug_last_firefly(int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* PT_POST_H */
