/* crt_vfilter.h -- C ABI of libcrt_vfilter.so: a variance-guided a-trous filter on device buffers, HIP for gfx950.
 *
 * No reference counterpart. The last stage of trace -> accumulate -> filter for a caller who accumulates: the spatial half of SVGF
 * (spatiotemporal variance-guided filtering). crtt_accumulate (crt_temporal.h) keeps, beside the colour, a moments plane {m1, m2, N, variance} of
 * the luminance; this filter reads it: it blurs where the signal is still noisy and keeps shadow and texture edges where it has converged. The
 * luminance stop of every tap follows the local standard deviation, and the variance is carried through the passes. A library of its own beside
 * libcrt_hip.so, libcrt_denoise.so and libcrt_temporal.so, stateless like the latter two: every buffer is the caller's; the library creates and
 * destroys no HIP object, allocates nothing, copies nothing and never waits on the host.
 *
 * Conventions: crtv_filter returns 0, a negative CRTV_E_* code (the values of CrtStatus) or a positive hipError_t when a launch fails;
 * crtv_error_string explains either. The argument checks need no GPU: the library loads and answers them on a machine without one.
 *
 * Definition. Every value is float32 arithmetic without contraction (a*b + c is a multiply, then an add); / and sqrtf are correctly rounded;
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z and luma(c) = (0.299f*c.x + 0.587f*c.y) + 0.114f*c.z as in crt_denoise.h; fmaxf is C's (a NaN is
 * dropped). t, n = a pixel's distance and stored normal; a pixel is a HIT iff t <= 99998.0f (so a NaN t is no hit). den, per channel, of the albedo
 * word's byte b (r = bits 0-7, g = 8-15, b = 16-23): b == 0 ? 1.0f : (float)b / 255.0f under CRTV_DEMODULATE, 1.0f without it; ld = luma(den)
 * (exactly 1.0f without the flag). {m1, m2, N, variance} = a pixel's moments. K[0..2] = 0.375f, 0.25f, 0.0625f; G[0..2] = 0.25f, 0.125f, 0.0625f.
 * The geometry stops of a tap q of a centre c at step s: fabsf(t_q - t_c) <= (depthTol * t_c) * (float)s and dot3(n_q, n_c) >= normalCos and,
 * under CRTV_MATCH_INSTANCE, instance_q == instance_c. Every comparison with a NaN is false. A tap that does not count contributes NOTHING: it is
 * selected away, as in crt_temporal.h, not multiplied by zero, so a NaN in a neighbour heals instead of spreading.
 *   1. The estimate writes the working image I0 = {r, g, b, var}:
 *      a pixel that is no hit: {color.rgb, 0};
 *      a hit pixel with N_c >= minHistory: var = variance_c where that is >= 0, else 0 (the temporal estimate);
 *      any other hit pixel, the spatial estimate: dy = -3..3 outside, dx = -3..3 inside, q = (x + dx, y + dy), s = 1; taps outside the frame are
 *        skipped; the centre always counts; another tap counts iff it is a hit, passes the geometry stops and m1_q and m2_q are finite. Over the
 *        counted taps, in tap order, from 0: S1 += m1_q; S2 += m2_q; n += 1.0f. Then a = S1 / n; v = S2 / n - a * a; var = v > 0 ? v : 0;
 *        var = var * (4.0f / fmaxf(N_c, 1.0f)).
 *      Under CRTV_DEMODULATE a hit pixel then gets rgb = rgb / den per channel and var = var / (ld * ld).
 *   2. Pass p = 0 .. iterations-1 with step s = 1 << p, input image I (pass 0: I0; later: the pass before). A pixel that is no hit copies I.
 *      For a hit centre c at (x, y):
 *      the prefiltered variance: over the 3 x 3 pixels q = (x + dx, y + dy), dy = -1..1 outside, dx = -1..1 inside (at distance 1 whatever s is),
 *        those inside the frame that are hits with var_q >= 0 count: gsum += var_q * g and gw += g with g = G[|dy|] * G[|dx|], from 0, in that
 *        order; gv = gsum / gw, or 0 when nothing counts; sd = lumaSigma * sqrtf(gv) + lumaFloor.
 *      the taps: dy = -2..2 outside, dx = -2..2 inside at q = (x + dx*s, y + dy*s), k = K[|dy|] * K[|dx|]. The centre counts with w = k. Another
 *        tap counts iff it lies in the frame, is a hit, passes the geometry stops, var_q >= 0 and xl < 1 with
 *        xl = fabsf(luma(I_q) - luma(I_c)) / sd (so 0 / 0 does not count); its w = k * ((1 - xl) * (1 - xl)).
 *      Over the counted taps, in tap order, from 0: sum += I_q.rgb * w per channel; vsum += var_q * (w * w); wsum += w.
 *      The pass writes {sum / wsum, vsum / (wsum * wsum)}.
 *   3. The last pass stores out = {rgb * den, color.a} for hit pixels and color exactly for pixels that are no hit and, where outVariance is
 *      given, var * (ld * ld) there for hit pixels and 0 for the others.
 *   The working images alternate between `scratch` and `out` so that the last pass lands in `out`; neither needs to be initialised; color,
 *   moments and the guides are only read. The polynomial weight stands where SVGF has exp(-xl): expf on the device is not correctly rounded,
 *   and this project compares bit for bit.
 *
 * crtv_filter ENQUEUES 1 + `iterations` launches on `stream` (a hipStream_t; NULL: HIP's null stream) AND RETURNS: no synchronisation.
 * Errors, all before anything is enqueued:
 *   CRTV_E_BAD_ARGUMENT  a NULL struct, color, moments, geometry, out or scratch; a plane that a flag needs missing (ids for MATCH_INSTANCE,
 *                        albedo for DEMODULATE, under CRTV_GUIDES_PLANES); ids or albedo given under CRTV_GUIDES_SURFACE; out, scratch or
 *                        outVariance equal to each other or to any input; iterations outside 1..5; an unknown flag or guide layout;
 *                        !(depthTol >= 0); a normalCos that is not finite; !(lumaSigma >= 0) or !(lumaFloor >= 0) or an infinite one of the
 *                        two; a NaN minHistory; width or height < 1
 *   CRTV_E_OUT_OF_RANGE  width or height > 16384
 *
 * The kernels: crtv_estimate_kernel, then crtv_pass_kernel once per pass; one lane per pixel, 256-lane workgroups over 32 x 8 tiles. For steps
 * up to CRTV_STAGE_MAX_STEP a pass's workgroup first stages its tile and a halo of 2 * step pixels -- geometry, {I.rgb, var} and the instance id,
 * 36 B per pixel -- in LDS and takes its 9 + 25 taps from there; beyond that step the taps are row reads through L1 / L2. The estimate's 7 x 7
 * window is taken likewise from a tile staged with a halo of 3 (only by workgroups that have a pixel in need of the spatial estimate) or as row
 * reads. CRTV_STAGE_MAX_STEP=0|1|2|4 and CRTV_ESTIMATE_TAPS=l1|lds in the environment (read by every call) override the built-in choices: for
 * measurements. The bits are the same whichever is chosen. */
#ifndef CRT_VFILTER_H
#define CRT_VFILTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CRTV_OK = 0, CRTV_E_BAD_ARGUMENT = -2, CRTV_E_OUT_OF_RANGE = -3 };   /* same values as CrtStatus */
enum { CRTV_GUIDES_PLANES = 0, CRTV_GUIDES_SURFACE = 1 };                   /* the two layouts of crt_denoise.h */
enum { CRTV_DEMODULATE = 1, CRTV_MATCH_INSTANCE = 2 };

/* 56 bytes (LP64): width 0, height 4, color 8, moments 16, guides 24 (4 bytes of padding behind it), geometry 32, ids 40, albedo 48 */
typedef struct {
    int32_t width, height;
    const void* color;      /* float4[W*H], row-major, e.g. crtt_accumulate's history colour; never written */
    const void* moments;    /* float4[W*H] {m1, m2, N, variance}, as crtt_accumulate writes it; never written */
    int32_t guides;         /* PLANES: geometry = float4[W*H] (CRT_GBUFFER_GEOMETRY), ids = 16-B records (CRT_GBUFFER_IDS, may be NULL
                               without MATCH_INSTANCE), albedo = uint32[W*H] (CRT_GBUFFER_ALBEDO, may be NULL without DEMODULATE).
                               SURFACE: geometry = CrtSurfaceHit[W*H] (48 B, what crt_shade_rays writes); ids and albedo must be NULL */
    const void *geometry, *ids, *albedo;
} CrtvFrame;

/* 28 bytes */
typedef struct {
    int32_t iterations;     /* 1..5 */
    uint32_t flags;         /* CRTV_DEMODULATE | CRTV_MATCH_INSTANCE */
    float depthTol;         /* >= 0, relative to the centre's distance, times the step */
    float normalCos;        /* finite */
    float lumaSigma;        /* >= 0, finite: the luminance stop in standard deviations */
    float lumaFloor;        /* >= 0, finite: added to the stop, so that a converged pixel still has one */
    float minHistory;       /* no NaN: a hit pixel with N below it takes the spatial estimate */
} CrtvParams;

size_t crtv_scratch_bytes(int32_t width, int32_t height, int32_t iterations);   /* W*H*16 for every valid count; else 0 */
int crtv_filter(const CrtvFrame* f, const CrtvParams* p, void* out /* float4[W*H] */, void* outVariance /* float[W*H] or NULL */, void* scratch,
                void* stream);
const char* crtv_error_string(int rc);

#ifdef __cplusplus
}
#endif

#endif
