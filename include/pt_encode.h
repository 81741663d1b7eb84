/*
 * pt_encode.h — the encode stage: linear light to 8-bit codes by the exact sRGB transfer, with an ordered dither in linear light.
 *
 * Declared in a header of its own for the reason pt_post.h, pt_spatial_variance.h and pt_metrics.h are: the older headers' declarations
 * are pinned one for one by their ABI tables and stream-contract tables.  The stage is exported from the same libpt_render.so and listed
 * in a table of its own (path_tracer_amd/abi.py: ENCODE_SIGNATURES), which is held to this header by the same two rules.  Error codes,
 * pt_last_error and the conventions — device pointers, whole frames [height][width][3] with y = 0 the bottom row, a `void* stream` that
 * is a hipStream_t — are pt_render.h's.  A caller detects the stage by the presence of its symbols; PT_ABI_VERSION does not change.
 */
#ifndef PT_ENCODE_H
#define PT_ENCODE_H

#include "pt_render.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- encode stage ---------------------------------------------------------------------------------------------------------------------------
 * The last step of the chain render -> guides -> firefly -> temporal -> variance -> filter -> display.  Every other 8-bit image of this
 * library goes through the reference's quantiser (sqrt, clamp to 0.999, * 256, truncate): a gamma-2 transfer, where every consumer of a
 * PNG assumes sRGB — linear 0.18 is written as code 108 and an sRGB viewer expects 118.  This stage writes the code of the real sRGB
 * function, correctly rounded, for every binary32 input, and needs no pow for it: an 8-bit code is a step function of its input, so the
 * encoder is fully defined by the 255 binary32 numbers at which the code steps.  The sRGB exponent is 2.4 = 12/5, so "x >= EOTF(v)" is
 * the rational inequality x^5 >= ((v + 0.055) / 1.055)^12, which integer arithmetic decides exactly: every entry of the two tables
 * below is verified that way (tests/test_encode_cpu.py; tools/encode_tables.py derives them), with no libm and no tolerance.
 *
 * THE STAGE IS OPT-IN: no other entry point calls it, pt_tonemap_rgb8 and pt_display_apply write the bytes they always wrote, and every
 * host takes it as an explicit option.
 *
 * Scope.  Whole frames only, no scene involved, no shards (gather and unshard first): linear (pt_encode) and color (pt_display_encode)
 * are [height][width][3] float with row 0 the BOTTOM row; rgb8_out is [height][width][3] bytes with row 0 the TOP row, which is
 * pt_tonemap_rgb8's flip.  rgb8_out must not overlap the input.  pt_encode and pt_display_encode are asynchronous on `stream` and
 * allocate nothing: the tables live in the code object.
 *
 * TABLES.  EOTF(v) = v / 12.92 for v <= 0.04045, else ((v + 0.055) / 1.055)^2.4: IEC 61966-2-1's decoding function.  The branch is
 * chosen by v, and every v used is a rational.
 *   M[c], c = 1 ... 255 = the smallest binary32 x with x >= EOTF((2c - 1) / 510): the boundary between the codes c - 1 and c
 *                         (PT_SRGB8_THRESHOLDS, 255 values)
 *   L[0] = +0;  L[c], c = 1 ... 255 = the smallest binary32 x with x >= EOTF(c / 255): the light a display shows for code c; L[255] is
 *                         exactly 1.0f  (PT_SRGB8_LEVELS, 256 values)
 * Both are strictly increasing, and L[c] < M[c + 1] < L[c + 1] for every c.
 *
 * DEFINITION, per channel value x of the pixel at column px and frame row py (py = 0 the bottom row).  Every value is IEEE binary32,
 * every operation is rounded once, nothing is fused, and the division is the correctly rounded one.
 *   PT_TRANSFER_REFERENCE            code = the reference's quantise(x), verbatim: what pt_tonemap_rgb8 writes
 *   PT_TRANSFER_SRGB, no dither      code = the number of j in 1 ... 255 with M[j] <= x        (binary32 comparisons: NaN gives 0,
 *                                    negatives and +-0 give 0, +inf gives 255)
 *   PT_TRANSFER_SRGB + PT_ENCODE_DITHER
 *     !(x > 0):   code = 0                              (NaN, negatives, +-0)
 *     x >= 1.0f:  code = 255
 *     otherwise   c = the number of j in 1 ... 254 with L[j] <= x                 (L[c] <= x < L[c + 1])
 *                 f = (x - L[c]) / (L[c + 1] - L[c])                              two subtractions and the division, each rounded once
 *                 t = ((float)B((px + phase_x) & 7, (py + phase_y) & 7) + 0.5f) * 0x1p-6f                                    exact
 *                 code = c + (f >= t)
 *     B(u, v) = sum over i = 0 ... 2 of ((((u ^ v) >> i) & 1) << (2 (2 - i) + 1)) | (((v >> i) & 1) << (2 (2 - i)))
 *   B is the 8 x 8 Bayer matrix — row v = 0 is 0 32 8 40 2 34 10 42 —, a permutation of 0 ... 63.  One t serves all three channels of a
 *   pixel, so neutral greys stay neutral.  `& 7` acts on the two's-complement int32 sum (which wraps), so negative phases are defined.
 *   x == L[c] gives f = +0 and code c: encode(L[c]) == c for every c, with and without dither.  The dither picks between the two
 *   neighbouring codes by the position of x between their decoded levels, so over any aligned 8 x 8 patch of one value x the mean of
 *   L[code] differs from x by at most (L[c + 1] - L[c]) / 64.
 *
 * The fused call.  pt_display_encode(state, display_params, encode_params, color, rgb8_out, stream) is pt_encode(encode_params, ...)
 * applied to the linear_out of pt_display_apply(state, display_params, color, encode_params->width, encode_params->height, ...): the
 * same bytes, and the plane between them is never written.  `state` may be NULL, as it may there (the stateless exposure 2^ev_bias).
 * With PT_TRANSFER_REFERENCE it writes pt_display_apply's rgb8_out.
 *
 * Rejected (PT_ERR_INVALID_ARG unless stated, on the host, before any device call), each call in this order:
 *   pt_encode:          a NULL params, linear or rgb8_out; a struct_size other than sizeof(PtEncodeParams); width or height <= 0; more
 *                       than 2^30 pixels (PT_ERR_TOO_LARGE); an unknown transfer; flags other than PT_ENCODE_DITHER and
 *                       PT_ENCODE_NO_VEC; PT_ENCODE_DITHER with PT_TRANSFER_REFERENCE; rgb8_out overlapping linear.
 *   pt_display_encode:  a NULL encode_params or rgb8_out; a struct_size other than sizeof(PtEncodeParams); then everything
 *                       pt_display_apply refuses about display_params, color and the frame size, in its order and with its words; then
 *                       pt_encode's list from "more than 2^30 pixels" on, with color in the place of linear.
 *
 * How a lane finds its code is the kernel's business (path_tracer_amd/csrc/pt_encode.hpp); the tables define the bits.
 * Out of scope: 16-bit output; other transfers (Rec. 709, PQ); blue-noise or animated patterns; white balance; shards.
 * profiles/encode_bench.txt holds the measured cost.                                                                                  */
#define PT_TRANSFER_REFERENCE 0 /* the reference's quantise(): sqrt, clamp to 0.999, * 256, truncate */
#define PT_TRANSFER_SRGB 1      /* the tables below */
#define PT_ENCODE_DITHER 1u     /* the ordered dither in linear light; PT_TRANSFER_SRGB only */
#define PT_ENCODE_NO_VEC 2u     /* A/B switch, same bits: one value per lane (default: four, where the width is a multiple of 4 and the planes are aligned) */
/* The defaults (pt_encode_params_init): the sRGB transfer, no dither, phase (0, 0). */
#define PT_ENCODE_DEFAULT_TRANSFER PT_TRANSFER_SRGB
#define PT_ENCODE_DEFAULT_FLAGS 0u
/* M[1 ... 255] */
#define PT_SRGB8_THRESHOLDS { \
  0x1.3e4568p-13f, 0x1.dd681cp-12f, 0x1.8dd6c2p-11f, 0x1.167cbcp-10f, 0x1.660e16p-10f, 0x1.b59f70p-10f, 0x1.029866p-9f, 0x1.2a6112p-9f, \
  0x1.5229bep-9f, 0x1.79f26cp-9f, 0x1.a1e5a2p-9f, 0x1.cbf736p-9f, 0x1.f86806p-9f, 0x1.13a0c0p-8f, 0x1.2c4666p-8f, 0x1.46297ap-8f, \
  0x1.614e62p-8f, 0x1.7db96ep-8f, 0x1.9b6edap-8f, 0x1.ba72cep-8f, 0x1.dac95ep-8f, 0x1.fc768cp-8f, 0x1.0fbf22p-7f, 0x1.21f236p-7f, \
  0x1.34d664p-7f, 0x1.486d90p-7f, 0x1.5cb98ep-7f, 0x1.71bc34p-7f, 0x1.877748p-7f, 0x1.9dec90p-7f, 0x1.b51dc8p-7f, 0x1.cd0ca8p-7f, \
  0x1.e5bae2p-7f, 0x1.ff2a1ep-7f, 0x1.0cae04p-6f, 0x1.1a291ep-6f, 0x1.28072cp-6f, 0x1.3648f8p-6f, 0x1.44ef4cp-6f, 0x1.53faf0p-6f, \
  0x1.636ca6p-6f, 0x1.734530p-6f, 0x1.838552p-6f, 0x1.942dc6p-6f, 0x1.a53f48p-6f, 0x1.b6ba96p-6f, 0x1.c8a064p-6f, 0x1.daf16ap-6f, \
  0x1.edae5cp-6f, 0x1.006bf8p-5f, 0x1.0a3768p-5f, 0x1.1439d8p-5f, 0x1.1e73a0p-5f, 0x1.28e514p-5f, 0x1.338e8ap-5f, 0x1.3e7058p-5f, \
  0x1.498acep-5f, 0x1.54de44p-5f, 0x1.606b08p-5f, 0x1.6c316ep-5f, 0x1.7831c8p-5f, 0x1.846c64p-5f, 0x1.90e194p-5f, 0x1.9d91a4p-5f, \
  0x1.aa7ce6p-5f, 0x1.b7a3a6p-5f, 0x1.c50630p-5f, 0x1.d2a4d4p-5f, 0x1.e07fdcp-5f, 0x1.ee9794p-5f, 0x1.fcec48p-5f, 0x1.05bf20p-4f, \
  0x1.0d26e4p-4f, 0x1.14ad96p-4f, 0x1.1c5356p-4f, 0x1.24184ep-4f, 0x1.2bfc9ep-4f, 0x1.34006ap-4f, 0x1.3c23d8p-4f, 0x1.446708p-4f, \
  0x1.4cca20p-4f, 0x1.554d40p-4f, 0x1.5df08ep-4f, 0x1.66b42ap-4f, 0x1.6f9836p-4f, 0x1.789cd6p-4f, 0x1.81c228p-4f, 0x1.8b0852p-4f, \
  0x1.946f72p-4f, 0x1.9df7acp-4f, 0x1.a7a11ep-4f, 0x1.b16beap-4f, 0x1.bb5832p-4f, 0x1.c56614p-4f, 0x1.cf95b2p-4f, 0x1.d9e72ap-4f, \
  0x1.e45aa0p-4f, 0x1.eef02ep-4f, 0x1.f9a7f8p-4f, 0x1.02410ep-3f, 0x1.07bf5cp-3f, 0x1.0d4ef6p-3f, 0x1.12efecp-3f, 0x1.18a24cp-3f, \
  0x1.1e6628p-3f, 0x1.243b8ap-3f, 0x1.2a2286p-3f, 0x1.301b2ap-3f, 0x1.362584p-3f, 0x1.3c41a2p-3f, 0x1.426f96p-3f, 0x1.48af6cp-3f, \
  0x1.4f0132p-3f, 0x1.5564fap-3f, 0x1.5bdad0p-3f, 0x1.6262c2p-3f, 0x1.68fce0p-3f, 0x1.6fa938p-3f, 0x1.7667d8p-3f, 0x1.7d38cep-3f, \
  0x1.841c2ap-3f, 0x1.8b11f6p-3f, 0x1.921a44p-3f, 0x1.993520p-3f, 0x1.a06298p-3f, 0x1.a7a2bap-3f, 0x1.aef594p-3f, 0x1.b65b34p-3f, \
  0x1.bdd3a8p-3f, 0x1.c55efcp-3f, 0x1.ccfd3ep-3f, 0x1.d4ae7cp-3f, 0x1.dc72c4p-3f, 0x1.e44a22p-3f, 0x1.ec34a4p-3f, 0x1.f43258p-3f, \
  0x1.fc434ap-3f, 0x1.0233c4p-2f, 0x1.064f8ep-2f, 0x1.0a750cp-2f, 0x1.0ea444p-2f, 0x1.12dd3ap-2f, 0x1.171ff8p-2f, 0x1.1b6c82p-2f, \
  0x1.1fc2e0p-2f, 0x1.242316p-2f, 0x1.288d2cp-2f, 0x1.2d012ap-2f, 0x1.317f12p-2f, 0x1.3606eep-2f, 0x1.3a98c4p-2f, 0x1.3f3498p-2f, \
  0x1.43da70p-2f, 0x1.488a56p-2f, 0x1.4d444cp-2f, 0x1.52085cp-2f, 0x1.56d688p-2f, 0x1.5baedap-2f, 0x1.609154p-2f, 0x1.657e00p-2f, \
  0x1.6a74e2p-2f, 0x1.6f7600p-2f, 0x1.748162p-2f, 0x1.79970ap-2f, 0x1.7eb702p-2f, 0x1.83e14ep-2f, 0x1.8915f2p-2f, 0x1.8e54f8p-2f, \
  0x1.939e64p-2f, 0x1.98f23cp-2f, 0x1.9e5084p-2f, 0x1.a3b944p-2f, 0x1.a92c82p-2f, 0x1.aeaa42p-2f, 0x1.b4328cp-2f, 0x1.b9c564p-2f, \
  0x1.bf62d0p-2f, 0x1.c50ad4p-2f, 0x1.cabd7ap-2f, 0x1.d07ac6p-2f, 0x1.d642bap-2f, 0x1.dc1562p-2f, 0x1.e1f2bep-2f, 0x1.e7dad6p-2f, \
  0x1.edcdb0p-2f, 0x1.f3cb50p-2f, 0x1.f9d3bcp-2f, 0x1.ffe6fcp-2f, 0x1.03028ap-1f, 0x1.061704p-1f, 0x1.0930eep-1f, 0x1.0c504ep-1f, \
  0x1.0f7524p-1f, 0x1.129f72p-1f, 0x1.15cf3ep-1f, 0x1.190488p-1f, 0x1.1c3f54p-1f, 0x1.1f7fa4p-1f, 0x1.22c57cp-1f, 0x1.2610dcp-1f, \
  0x1.2961c8p-1f, 0x1.2cb844p-1f, 0x1.301452p-1f, 0x1.3375f4p-1f, 0x1.36dd2cp-1f, 0x1.3a49fep-1f, 0x1.3dbc6cp-1f, 0x1.413478p-1f, \
  0x1.44b226p-1f, 0x1.483578p-1f, 0x1.4bbe70p-1f, 0x1.4f4d12p-1f, 0x1.52e15ep-1f, 0x1.567b5ap-1f, 0x1.5a1b06p-1f, 0x1.5dc064p-1f, \
  0x1.616b7ap-1f, 0x1.651c48p-1f, 0x1.68d2d0p-1f, 0x1.6c8f16p-1f, 0x1.70511ep-1f, 0x1.7418e6p-1f, 0x1.77e674p-1f, 0x1.7bb9cap-1f, \
  0x1.7f92eap-1f, 0x1.8371d6p-1f, 0x1.875690p-1f, 0x1.8b411ep-1f, 0x1.8f317ep-1f, 0x1.9327b6p-1f, 0x1.9723c6p-1f, 0x1.9b25b0p-1f, \
  0x1.9f2d7ap-1f, 0x1.a33b24p-1f, 0x1.a74eb0p-1f, 0x1.ab6822p-1f, 0x1.af877cp-1f, 0x1.b3acbep-1f, 0x1.b7d7eep-1f, 0x1.bc090cp-1f, \
  0x1.c0401cp-1f, 0x1.c47d20p-1f, 0x1.c8c018p-1f, 0x1.cd090ap-1f, 0x1.d157f6p-1f, 0x1.d5ace0p-1f, 0x1.da07cap-1f, 0x1.de68b4p-1f, \
  0x1.e2cfa4p-1f, 0x1.e73c9ap-1f, 0x1.ebaf98p-1f, 0x1.f028a2p-1f, 0x1.f4a7bap-1f, 0x1.f92ce2p-1f, 0x1.fdb81cp-1f }
/* L[0 ... 255] */
#define PT_SRGB8_LEVELS { \
  0x0p+0f, 0x1.3e4568p-12f, 0x1.3e4568p-11f, 0x1.dd681cp-11f, 0x1.3e4568p-10f, 0x1.8dd6c2p-10f, 0x1.dd681cp-10f, 0x1.167cbcp-9f, \
  0x1.3e4568p-9f, 0x1.660e16p-9f, 0x1.8dd6c2p-9f, 0x1.b6a31cp-9f, 0x1.e1e31ep-9f, 0x1.07c38cp-8f, 0x1.1fcc2cp-8f, 0x1.390ffcp-8f, \
  0x1.53936ep-8f, 0x1.6f5adep-8f, 0x1.8c6a96p-8f, 0x1.aac6c2p-8f, 0x1.ca7382p-8f, 0x1.eb74e2p-8f, 0x1.06e76cp-7f, 0x1.18c2a6p-7f, \
  0x1.2b4e0ap-7f, 0x1.3e8b7cp-7f, 0x1.527cd8p-7f, 0x1.6723f0p-7f, 0x1.7c8294p-7f, 0x1.929a8ap-7f, 0x1.a96d92p-7f, 0x1.c0fd68p-7f, \
  0x1.d94bbep-7f, 0x1.f25a46p-7f, 0x1.061552p-6f, 0x1.135f40p-6f, 0x1.210bbap-6f, 0x1.2f1b8ep-6f, 0x1.3d8f84p-6f, 0x1.4c6868p-6f, \
  0x1.5ba6fcp-6f, 0x1.6b4c04p-6f, 0x1.7b5842p-6f, 0x1.8bcc76p-6f, 0x1.9ca95ap-6f, 0x1.adefaap-6f, 0x1.bfa022p-6f, 0x1.d1bb74p-6f, \
  0x1.e4425ap-6f, 0x1.f73586p-6f, 0x1.054ad6p-5f, 0x1.0f31bcp-5f, 0x1.194fccp-5f, 0x1.23a560p-5f, 0x1.2e32cap-5f, 0x1.38f860p-5f, \
  0x1.43f678p-5f, 0x1.4f2d64p-5f, 0x1.5a9d76p-5f, 0x1.664702p-5f, 0x1.722a58p-5f, 0x1.7e47c8p-5f, 0x1.8a9fa4p-5f, 0x1.97323ap-5f, \
  0x1.a3ffdap-5f, 0x1.b108d0p-5f, 0x1.be4d6cp-5f, 0x1.cbcdfap-5f, 0x1.d98ac8p-5f, 0x1.e7841ep-5f, 0x1.f5ba4ap-5f, 0x1.0216ccp-4f, \
  0x1.096f28p-4f, 0x1.10e65ep-4f, 0x1.187c92p-4f, 0x1.2031eap-4f, 0x1.280688p-4f, 0x1.2ffa92p-4f, 0x1.380e2ap-4f, 0x1.404176p-4f, \
  0x1.489496p-4f, 0x1.5107aep-4f, 0x1.599ae0p-4f, 0x1.624e50p-4f, 0x1.6b2220p-4f, 0x1.741672p-4f, 0x1.7d2b66p-4f, 0x1.866120p-4f, \
  0x1.8fb7c2p-4f, 0x1.992f6ap-4f, 0x1.a2c83cp-4f, 0x1.ac8256p-4f, 0x1.b65ddcp-4f, 0x1.c05aeep-4f, 0x1.ca79aap-4f, 0x1.d4ba30p-4f, \
  0x1.df1ca4p-4f, 0x1.e9a122p-4f, 0x1.f447cap-4f, 0x1.ff10bcp-4f, 0x1.04fe0cp-3f, 0x1.0a8500p-3f, 0x1.101d46p-3f, 0x1.15c6eep-3f, \
  0x1.1b820ap-3f, 0x1.214ea6p-3f, 0x1.272cd4p-3f, 0x1.2d1ca2p-3f, 0x1.331e20p-3f, 0x1.39315ap-3f, 0x1.3f5660p-3f, 0x1.458d44p-3f, \
  0x1.4bd610p-3f, 0x1.5230d4p-3f, 0x1.589da2p-3f, 0x1.5f1c84p-3f, 0x1.65ad8ap-3f, 0x1.6c50c4p-3f, 0x1.73063ep-3f, 0x1.79ce08p-3f, \
  0x1.80a82ep-3f, 0x1.8794c0p-3f, 0x1.8e93ccp-3f, 0x1.95a560p-3f, 0x1.9cc988p-3f, 0x1.a40054p-3f, 0x1.ab49d0p-3f, 0x1.b2a60cp-3f, \
  0x1.ba1512p-3f, 0x1.c196f4p-3f, 0x1.c92bbep-3f, 0x1.d0d37cp-3f, 0x1.d88e3ep-3f, 0x1.e05c10p-3f, 0x1.e83cfep-3f, 0x1.f03116p-3f, \
  0x1.f83868p-3f, 0x1.002980p-2f, 0x1.044074p-2f, 0x1.086116p-2f, 0x1.0c8b70p-2f, 0x1.10bf88p-2f, 0x1.14fd60p-2f, 0x1.194504p-2f, \
  0x1.1d9676p-2f, 0x1.21f1c0p-2f, 0x1.2656e6p-2f, 0x1.2ac5eep-2f, 0x1.2f3ee0p-2f, 0x1.33c1c2p-2f, 0x1.384e9ap-2f, 0x1.3ce56cp-2f, \
  0x1.418642p-2f, 0x1.463122p-2f, 0x1.4ae60ep-2f, 0x1.4fa510p-2f, 0x1.546e2ep-2f, 0x1.59416cp-2f, 0x1.5e1ed2p-2f, 0x1.630664p-2f, \
  0x1.67f82ap-2f, 0x1.6cf42ap-2f, 0x1.71fa68p-2f, 0x1.770aecp-2f, 0x1.7c25bcp-2f, 0x1.814adcp-2f, 0x1.867a54p-2f, 0x1.8bb42ap-2f, \
  0x1.90f862p-2f, 0x1.964702p-2f, 0x1.9ba012p-2f, 0x1.a10394p-2f, 0x1.a67194p-2f, 0x1.abea12p-2f, 0x1.b16d16p-2f, 0x1.b6faa6p-2f, \
  0x1.bc92c6p-2f, 0x1.c2357ep-2f, 0x1.c7e2d4p-2f, 0x1.cd9acap-2f, 0x1.d35d6ap-2f, 0x1.d92ab8p-2f, 0x1.df02b8p-2f, 0x1.e4e572p-2f, \
  0x1.ead2eap-2f, 0x1.f0cb26p-2f, 0x1.f6ce2cp-2f, 0x1.fcdc02p-2f, 0x1.017a56p-1f, 0x1.048c18p-1f, 0x1.07a34ap-1f, 0x1.0abff0p-1f, \
  0x1.0de20ap-1f, 0x1.11099cp-1f, 0x1.1436a8p-1f, 0x1.176934p-1f, 0x1.1aa13ep-1f, 0x1.1ddeccp-1f, 0x1.2121dep-1f, 0x1.246a7ap-1f, \
  0x1.27b8a0p-1f, 0x1.2b0c54p-1f, 0x1.2e6598p-1f, 0x1.31c470p-1f, 0x1.3528dcp-1f, 0x1.3892e2p-1f, 0x1.3c0280p-1f, 0x1.3f77bep-1f, \
  0x1.42f29ap-1f, 0x1.46731ap-1f, 0x1.49f93ep-1f, 0x1.4d850cp-1f, 0x1.511682p-1f, 0x1.54ada6p-1f, 0x1.584a7ap-1f, 0x1.5becfep-1f, \
  0x1.5f9538p-1f, 0x1.63432ap-1f, 0x1.66f6d4p-1f, 0x1.6ab03cp-1f, 0x1.6e6f62p-1f, 0x1.72344ap-1f, 0x1.75fef4p-1f, 0x1.79cf66p-1f, \
  0x1.7da5a0p-1f, 0x1.8181a6p-1f, 0x1.856378p-1f, 0x1.894b1cp-1f, 0x1.8d3892p-1f, 0x1.912bdep-1f, 0x1.952502p-1f, 0x1.992400p-1f, \
  0x1.9d28dap-1f, 0x1.a13392p-1f, 0x1.a5442ep-1f, 0x1.a95aacp-1f, 0x1.ad7712p-1f, 0x1.b19960p-1f, 0x1.b5c198p-1f, 0x1.b9efc0p-1f, \
  0x1.be23d6p-1f, 0x1.c25ddep-1f, 0x1.c69ddcp-1f, 0x1.cae3d2p-1f, 0x1.cf2fc0p-1f, 0x1.d381acp-1f, 0x1.d7d994p-1f, 0x1.dc377ep-1f, \
  0x1.e09b6cp-1f, 0x1.e5055ep-1f, 0x1.e97558p-1f, 0x1.edeb5cp-1f, 0x1.f2676cp-1f, 0x1.f6e98cp-1f, 0x1.fb71bcp-1f, 0x1p+0f }
typedef struct PtEncodeParams {
  int32_t struct_size; /* sizeof(PtEncodeParams) of the caller's header */
  int32_t width, height;
  int32_t transfer;    /* PT_TRANSFER_REFERENCE, PT_TRANSFER_SRGB */
  uint32_t flags;      /* PT_ENCODE_DITHER, PT_ENCODE_NO_VEC */
  int32_t phase_x, phase_y; /* the dither pattern's offset in pixels; any int32 */
  int32_t reserved;
} PtEncodeParams;
/* Host function, no GPU: struct_size + the defaults above for a frame of width x height. */
void pt_encode_params_init(PtEncodeParams* params, int32_t width, int32_t height);
/* The stage defined above; asynchronous on `stream`, allocates nothing. */
int pt_encode(const PtEncodeParams* params, const float* linear, uint8_t* rgb8_out, void* stream);
/* pt_display_apply's exposure and tone curve and the stage above in one pass; asynchronous on `stream`, allocates nothing. */
int pt_display_encode(const PtDisplay* state, const PtDisplayParams* display_params, const PtEncodeParams* encode_params, const float* color,
                      uint8_t* rgb8_out, void* stream);
/* How the LAST pt_encode or pt_display_encode of this process ran: out[0] = 0 not run, 1 one value per lane, 2 four values per lane (one
 * 16-byte load, one 4-byte store); out[1] / out[2] = the grid (x: workgroups along a row, y: workgroups that walk the rows); out[3] = the
 * values per lane — a workgroup takes 256 * out[3] values of a row per trip; out[4] = transfer + 1; out[5] = 1 fused
 * (pt_display_encode), 0 not; out[6] = 1 with PT_ENCODE_DITHER, 0 without; out[7] = 0.  The bits do not depend on the path.  For tests. */
int pt_debug_last_encode(int32_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* PT_ENCODE_H */
