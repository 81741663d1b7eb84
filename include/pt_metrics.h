/*
 * pt_metrics.h — image error on the device: exact, order-independent sums of the differences of two frames.
 *
 * Declared in a header of its own for the reason pt_post.h and pt_spatial_variance.h are: the older headers' declarations are pinned one
 * for one by their ABI tables and stream-contract tables.  The stage is exported from the same libpt_render.so and listed in a table of
 * its own (path_tracer_amd/abi.py: METRICS_SIGNATURES), which is held to this header by the same two rules.  Error codes, pt_last_error
 * and the conventions — device pointers, whole frames [height][width][3] with y = 0 the bottom row, a `void* stream` that is a
 * hipStream_t — are pt_render.h's.  A caller detects the stage by the presence of its symbols; PT_ABI_VERSION does not change.
 */
#ifndef PT_METRICS_H
#define PT_METRICS_H

#include "pt_render.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- image error ---------------------------------------------------------------------------------------------------------------------------
 * Every stage after the renderer is justified by a ratio of mean squared errors against a reference frame.  pt_image_error is the
 * instrument: it compares frame `a` against frame `ref` inside a rectangle and leaves, on the device, the sums of the squared, absolute
 * and relative squared differences per channel, the largest absolute difference and the numbers of pixels that took part and that did
 * not.  A floating-point sum over two million pixels depends on the order of its additions; this project defines every result to the
 * bit, so each sum here is the EXACT real sum of its terms, rounded once.  That does not depend on an order, a grid or an implementation.
 *
 * Scope.  pt_firefly's — whole frames only, no scene involved, no shards (gather and unshard first): a and ref are [height][width][3]
 * float, error_plane (optional, NULL) is [height][width] float.  a may BE ref (every difference is then +0).  error_plane must overlap
 * neither input, result or scratch.  pt_image_error is asynchronous on `stream` and allocates nothing: the caller passes `scratch`,
 * pt_image_error_scratch_bytes() bytes of device memory, 8-byte aligned, which the call zeroes itself on `stream` — repeated calls need
 * no host step — and whose contents afterwards mean nothing.  Nothing comes back to the host: `result` is a DEVICE PtImageErrorResult,
 * 8-byte aligned, which the caller copies when it wants the numbers.
 *
 * DEFINITION.  The rectangle is the pixels x0 <= x < x1, y0 <= y < y1; a rect of four zeros is the whole frame (the display stage's
 * convention for its metering rectangle); x0 == x1 or y0 == y1 otherwise is an EMPTY rectangle, which is allowed.
 * For a pixel p of the rectangle and ch = r, g, b:
 *   d.ch = a(p).ch - ref(p).ch                          binary32, rounded once; a subnormal difference is kept, not flushed
 *   p TAKES PART iff a(p).ch, ref(p).ch and d.ch are finite for all three channels (3e38f - (-3e38f) is not: such a pixel does not)
 *   a pixel of the rectangle that does not take part is counted in `skipped` and enters no sum and no maximum
 * For a pixel that takes part, in binary64, each operation rounded once, nothing fused:
 *   sq.ch  = (double)d.ch * (double)d.ch                exact: 24 x 24 bits
 *   ab.ch  = fabs((double)d.ch)                         exact; a difference of -0 counts as +0
 *   rel.ch = sq.ch / ((double)ref(p).ch * (double)ref(p).ch + eps)      the product is exact, the sum and the quotient are rounded once
 *            (the relative squared error of the denoising literature — Rousselle et al. 2011 and the relMSE of the Monte Carlo denoisers
 *            since: (a - ref)^2 / (ref^2 + eps), averaged over pixels and channels —, here with eps = PT_IMAGE_ERROR_DEFAULT_EPS)
 * Results:
 *   sum_sq[ch], sum_abs[ch], sum_rel[ch] = the exact real sum of the terms over the pixels taking part, rounded ONCE to binary64,
 *                                          round-to-nearest-even (a sum at or above 2^1024 - 2^970 gives +inf, as that rounding does)
 *   max_abs[ch] = the largest fabsf(d.ch), binary32; +0 where no pixel takes part
 *   pixels      = the pixels taking part;  skipped = the other pixels of the rectangle
 * error_plane (if not NULL), for EVERY pixel of the frame, binary32, each operation rounded once, nothing fused:
 *   taking part:                            ((d.r * d.r + d.g * d.g) + d.b * d.b) / 3.0f    (may overflow to +inf; the correctly rounded division)
 *   skipped, or outside the rectangle:      +inf
 * Corners.  An empty rectangle, or a rectangle whose every pixel is skipped: every sum and maximum is +0, pixels = 0.  a == ref as
 * pointers: every sum and maximum +0, pixels = the finite pixels.  With eps >= 2^-126 (required) no term can overflow: rel < 2^256 / eps.
 *
 * Derived figures are the HOST's, ordinary binary64 arithmetic on the copied result in the order written (path_tracer_amd/render.py:
 * ImageError, pt::image_error_result): MSE = ((sum_sq[0] + sum_sq[1]) + sum_sq[2]) / (3.0 * pixels), MAE and relMSE likewise from
 * sum_abs and sum_rel, PSNR = 10 log10(peak^2 / MSE) against a stated peak.  pixels = 0 gives NaN.
 *
 * The accumulator and its bound.  Each of the nine sums is a fixed-point number of PT_IMAGE_ERROR_WORDS 64-bit words, word j weighing
 * 2^(32 j - 1074): the grid of binary64's smallest subnormal, on which every finite binary64 lies.  A term's 53-bit significand,
 * shifted to its place, overlaps at most three words and adds one chunk < 2^32 to each with an integer add.  Integer adds commute, so
 * the words do not depend on the order of the terms.  A sum has at most 2^30 terms (one per pixel), so no word exceeds
 * 2^30 (2^32 - 1) < 2^62: it cannot overflow, whatever the frame.  The highest word a chunk touches is 65; carries out of it reach word
 * 66 at most, and 68 words leave one to spare.  A last pass propagates the carries, finds the leading bit and rounds once.
 *
 * Rejected (PT_ERR_INVALID_ARG, on the host, before any device call): a NULL params, a, ref, result or scratch; a struct_size other
 * than sizeof(PtImageErrorParams); width or height <= 0; a rect that is not four zeros and not 0 <= x0 <= x1 <= width,
 * 0 <= y0 <= y1 <= height; an eps that is not finite or < 2^-126; flags other than PT_IMAGE_ERROR_NO_LDS; a result or scratch that is
 * not 8-byte aligned; params.scratch_bytes < pt_image_error_scratch_bytes(); error_plane, result or scratch overlapping an input or one another.
 * More than 2^30 pixels: PT_ERR_TOO_LARGE (the accumulator's bound above).
 *
 * Out of scope: shards; SSIM, FLIP and perceptual metrics; per-tile maps beyond the per-pixel plane.  profiles/metrics_bench.txt holds
 * the measured cost.                                                                                                                  */
#define PT_IMAGE_ERROR_NO_LDS 1u /* A/B switch, same bits: every chunk is added to `scratch` with a global atomic (default: to a workgroup's accumulators in LDS, flushed once) */
#define PT_IMAGE_ERROR_WORDS 68  /* 64-bit words per accumulator */
#define PT_IMAGE_ERROR_SUMS 9    /* accumulators: sum_sq, sum_abs, sum_rel x 3 channels */
#define PT_IMAGE_ERROR_DEFAULT_EPS 1e-4
typedef struct PtImageErrorParams {
  int32_t struct_size; /* sizeof(PtImageErrorParams) of the caller's header */
  int32_t width, height;
  int32_t rect_x0, rect_y0, rect_x1, rect_y1; /* four zeros: the whole frame */
  uint32_t flags;      /* PT_IMAGE_ERROR_NO_LDS */
  double eps;          /* relMSE's; finite, >= 2^-126 */
  int64_t scratch_bytes; /* the bytes behind `scratch`; >= pt_image_error_scratch_bytes() (params_init leaves 0: the caller states what it has) */
  int32_t reserved[2];
} PtImageErrorParams;
typedef struct PtImageErrorResult {
  double sum_sq[3], sum_abs[3], sum_rel[3];
  uint64_t pixels, skipped;
  float max_abs[3];
  uint32_t reserved;
} PtImageErrorResult;
/* Host function, no GPU: struct_size + the defaults above (the whole frame, eps = PT_IMAGE_ERROR_DEFAULT_EPS) for a frame of width x height. */
void pt_image_error_params_init(PtImageErrorParams* params, int32_t width, int32_t height);
/* Host function, no GPU: the bytes of `scratch` a call needs — the same for every frame. */
int64_t pt_image_error_scratch_bytes(void);
/* The stage defined above; asynchronous on `stream`, allocates nothing. */
int pt_image_error(const PtImageErrorParams* params, const float* a, const float* ref, PtImageErrorResult* result, float* error_plane,
                   void* scratch, void* stream);
/* How the LAST pt_image_error of this process ran: out[0] = 0 not run, 1 global atomics only (PT_IMAGE_ERROR_NO_LDS), 2 accumulators in
 * LDS; out[1] = the workgroups of the accumulating kernel; out[2] / out[3] = the rectangle's width and height in pixels.  The bits do
 * not depend on the path.  For tests. */
int pt_debug_last_image_error(int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* PT_METRICS_H */
