/* crt_denoise.h -- C ABI of libcrt_denoise.so: a G-buffer-guided a-trous denoiser on device buffers, HIP for gfx950.
 *
 * No reference counterpart (upstream traces one sample per pixel and filters nothing). A library of its own beside libcrt_hip.so: the filter
 * is a pure function of device buffers -- no session, no scene, no state, no allocation. Every buffer is the caller's; the library creates
 * and destroys no HIP object (no device or pinned buffer, no event, no stream) and never waits on the host. Whoever accumulates stochastic
 * samples over crt_shade_rays / crt_trace_rays has a noisy float4 image and, beside it, exact normals, distances, ids and albedo: the planes
 * of a CRT_RENDER_GBUFFER frame (crt_api.h) or the CrtSurfaceHit records of crt_shade_rays (crt_types.h). Both are taken as they lie.
 *
 * Conventions: crtd_denoise returns 0, a negative CRTD_E_* code (the values of CrtStatus) or a positive hipError_t when a launch fails;
 * crtd_error_string explains either. The argument checks need no GPU: the library loads and answers them on a machine without one.
 *
 * Definition. Every value is float32 arithmetic without contraction (a*b + c is a multiply, then an add);
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z as in crt_api.h. t, n = a pixel's distance and stored normal (GEOMETRY: n.x, n.y, n.z, t);
 * a pixel is a HIT iff t <= 99998.0f (so a NaN t is no hit). K[0..2] = 0.375f, 0.25f, 0.0625f.
 *   Demodulation (CRTD_DEMODULATE): per channel, with the albedo word's byte b (r = bits 0-7, g = 8-15, b = 16-23):
 *     den = b == 0 ? 1.0f : (float)b / 255.0f. The input of pass 0 is color.rgb / den for hit pixels and color.rgb for the others; the last
 *     pass stores result.rgb * den for hit pixels.
 *   Pass p = 0 .. iterations-1 with step s = 1 << p, input image I (pass 0: color, demodulated as above; later: the pass before):
 *     for a hit centre c at (x, y): sum = (0, 0, 0), wsum = 0; dy = -2..2 outside, dx = -2..2 inside: the tap q = (x + dx*s, y + dy*s) is
 *     skipped when it lies outside the frame; k = K[|dy|] * K[|dx|]; m = 1 at the centre; otherwise m = 1 iff q is a hit and
 *     fabsf(t_q - t_c) <= (depthTol * t_c) * (float)s and dot3(n_q, n_c) >= normalCos and, with CRTD_MATCH_INSTANCE, instance_q == instance_c
 *     and, with CRTD_LUMA_STOP, fabsf(L_q - L_c) <= lumaTol where L = (0.299f*r + 0.587f*g) + 0.114f*b of I; else m = 0. w = m ? k : 0;
 *     sum += I_q.rgb * w per channel, then wsum += w, in tap order. The pass writes sum / wsum.
 *   A pixel that is no hit copies I. Alpha is the centre's color.a throughout. At the end a pixel that is no hit holds color exactly.
 *   NaNs get what these expressions give: every comparison with a NaN is false, and a NaN colour reaches every sum it is a tap of (NaN * 0).
 *   Passes alternate between `out` and `scratch` so that the last one lands in `out`; neither needs to be initialised; color and the guides
 *   are only read.
 *
 * crtd_denoise ENQUEUES `iterations` launches on `stream` (a hipStream_t; NULL: HIP's null stream) AND RETURNS: no synchronisation.
 * Errors, all before anything is enqueued:
 *   CRTD_E_BAD_ARGUMENT  a NULL struct, color, geometry or out; a plane that a flag needs missing (ids for MATCH_INSTANCE, albedo for
 *                        DEMODULATE, under CRTD_GUIDES_PLANES); ids or albedo given under CRTD_GUIDES_SURFACE; scratch NULL with
 *                        iterations >= 2; out or scratch equal to color, to each other or to a guide; iterations outside 1..6; an unknown
 *                        flag or guide layout; !(depthTol >= 0); a normalCos that is not finite; CRTD_LUMA_STOP with !(lumaTol >= 0);
 *                        width or height < 1
 *   CRTD_E_OUT_OF_RANGE  width or height > 16384
 *
 * The kernel: one launch per pass, one lane per pixel, 256-lane workgroups over 32 x 8 tiles. For steps up to CRTD_STAGE_MAX_STEP the
 * workgroup first stages its tile and a halo of 2 * step pixels -- geometry, the pass's input colour (demodulated once per pixel in pass 0)
 * and the instance id, 32 B per pixel -- in LDS and takes its 25 taps from there; beyond that step the taps are row reads through L1 / L2.
 * CRTD_STAGE_MAX_STEP=0|1|2|4 in the environment (read by every call) overrides the built-in threshold: for measurements. */
#ifndef CRT_DENOISE_H
#define CRT_DENOISE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CRTD_OK = 0, CRTD_E_BAD_ARGUMENT = -2, CRTD_E_OUT_OF_RANGE = -3 };   /* same values as CrtStatus */
enum { CRTD_GUIDES_PLANES = 0, CRTD_GUIDES_SURFACE = 1 };
enum { CRTD_DEMODULATE = 1, CRTD_MATCH_INSTANCE = 2, CRTD_LUMA_STOP = 4 };

typedef struct {
    int32_t width, height;
    const void* color;      /* float4[W*H], row-major; never written */
    int32_t guides;         /* PLANES: geometry = float4[W*H] (CRT_GBUFFER_GEOMETRY), ids = 16-B records (CRT_GBUFFER_IDS, may be NULL
                               without MATCH_INSTANCE), albedo = uint32[W*H] (CRT_GBUFFER_ALBEDO, may be NULL without DEMODULATE).
                               SURFACE: geometry = CrtSurfaceHit[W*H] (48 B, what crt_shade_rays writes); ids and albedo must be NULL */
    const void *geometry, *ids, *albedo;
} CrtdFrame;

typedef struct { int32_t iterations; uint32_t flags; float depthTol, normalCos, lumaTol; } CrtdParams;

size_t crtd_scratch_bytes(int32_t width, int32_t height, int32_t iterations);   /* 0 for iterations == 1, else W*H*16 */
int crtd_denoise(const CrtdFrame* f, const CrtdParams* p, void* out /* float4[W*H] */, void* scratch, void* stream);
const char* crtd_error_string(int rc);

#ifdef __cplusplus
}
#endif

#endif
