/* crt_upsample.h -- C ABI of libcrt_upsample.so: guided (joint-bilateral) upsampling of a low-resolution pass on device buffers, HIP for gfx950.
 *
 * No reference counterpart. A stochastic pass (ambient occlusion, one shade_rays sample per pixel) traced at every 2nd or 4th pixel of a frame costs
 * a quarter or a sixteenth of the full pass; this call brings it to full resolution, guided by the FULL-resolution G-buffer the Trace launch
 * writes anyway. The ray generation makes the guides free: pixel (i, j) of a W x H frame looks through cx = i / W, so pixel (X, Y) of a
 * W/F x H/F frame has, bit for bit, the ray of pixel (F*X, F*Y) of the full frame. A low sample therefore SITS ON a full-resolution pixel, and its
 * guide is that pixel's G-buffer entry: there is no second set of guides. A library of its own beside libcrt_hip.so and the four image libraries
 * (crt_denoise.h, crt_temporal.h, crt_vfilter.h, crt_motion.h), stateless like them: every buffer is the caller's; the library creates and
 * destroys no HIP object, allocates nothing, copies nothing and never waits on the host.
 *
 * Conventions: crtu_upsample and crtu_low_size return 0, a negative CRTU_E_* code (the values of CrtStatus) or, crtu_upsample only, a positive
 * hipError_t when the launch fails; crtu_error_string explains either. The argument checks need no GPU: the library loads and answers them on a
 * machine without one.
 *
 * The low image. factor F is 2 or 4; offsetX, offsetY lie in 0 .. F-1; low sample (X, Y) sits on full pixel (F*X + offsetX, F*Y + offsetY).
 * LW = (W - offsetX + F - 1) / F and LH = (H - offsetY + F - 1) / F (crtu_low_size), so every low sample's pixel lies in the frame. The offset
 * exists so that a caller can rotate the sampled pixel from frame to frame under temporal accumulation.
 *
 * Definition. Every value is float32 arithmetic without contraction (a*b + c is a multiply, then an add); / is correctly rounded;
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; t, n = a pixel's distance and stored normal; a pixel is a HIT iff t <= 99998.0f (so a NaN t is no
 * hit); den, per channel, of the albedo word's byte b (r = bits 0-7, g = 8-15, b = 16-23): b == 0 ? 1.0f : (float)b / 255.0f -- all as in
 * crt_vfilter.h. Every comparison with a NaN is false. For the full pixel c = (x, y) with guide values t_c, n_c and instance_c:
 *   1. The four taps. X0 = floor((x - offsetX) / F), Y0 = floor((y - offsetY) / F): a floor, so X0 = -1 left of the first sample.
 *      fx = (float)((x - offsetX) - X0*F) / (float)F, fy likewise (exact). The taps, in tap order: (X0, Y0), (X0+1, Y0), (X0, Y0+1), (X0+1, Y0+1);
 *      their bilinear weights b = (1-fx)*(1-fy), fx*(1-fy), (1-fx)*fy, fx*fy (exact: multiples of 1/16). A tap outside 0..LW-1 x 0..LH-1 does
 *      not EXIST. A tap whose b == 0 does not count, so a pixel that carries a sample takes that sample alone.
 *   2. A tap q with guide pixel g = (F*X + offsetX, F*Y + offsetY) and value v_q (1 or 4 channels) COUNTS iff it exists, b > 0, every channel of
 *      v_q is finite, and
 *        c is a hit:  g is a hit, fabsf(t_g - t_c) <= depthTol * t_c, dot3(n_g, n_c) >= normalCos and, under CRTU_MATCH_INSTANCE,
 *                     instance_g == instance_c;
 *        c is no hit: g is no hit (sky interpolates among sky).
 *      A tap that does not count contributes NOTHING: it is selected away, not multiplied by zero, so a NaN heals instead of spreading.
 *   3. If at least one tap counts: over the counted taps, in tap order, from 0: sum += v_q * b per channel; wsum += b. out = sum / wsum per
 *      channel. The state is CRTU_STATE_INTERPOLATED.
 *   4. If none counts, the nearest surviving tap. The candidates are the existing taps with finite v_q, whatever their b. If c is a hit and at
 *      least one candidate's guide is a hit with a d = fabsf(t_g - t_c) that is no NaN: the candidate with the smallest such d, the first in tap
 *      order winning a tie. Otherwise the first candidate in tap order. out = v_q of the chosen tap; the state is CRTU_STATE_NEAREST. With no
 *      candidate at all out = 0 per channel and the state is CRTU_STATE_EMPTY.
 *   5. Under CRTU_MODULATE (channels 4 only) a hit pixel's out.rgb is multiplied by den per channel; out.a stays as computed.
 *   6. outState, where given, receives the state word of every pixel: the caller can re-trace the NEAREST and EMPTY pixels at full resolution.
 *   low and the guides are only read; out and outState need not be initialised.
 *
 * crtu_upsample ENQUEUES ONE launch on `stream` (a hipStream_t; NULL: HIP's null stream) AND RETURNS: no synchronisation.
 * Errors, all before anything is enqueued:
 *   CRTU_E_BAD_ARGUMENT  a NULL struct, low, geometry or out; a plane that a flag needs missing (ids for MATCH_INSTANCE, albedo for MODULATE,
 *                        under CRTU_GUIDES_PLANES); ids or albedo given under CRTU_GUIDES_SURFACE; an unknown flag or guide layout; channels
 *                        other than 1 or 4; MODULATE with channels 1; a factor other than 2 or 4; an offset outside 0 .. factor-1, or one that
 *                        is not below the frame's width (offsetX) or height (offsetY); out or outState equal to each other or to an input;
 *                        !(depthTol >= 0); a normalCos that is NaN; width or height < 1.
 *                        depthTol = +inf with normalCos = -inf is legal: the unguided call (of hit pixels among hit pixels).
 *   CRTU_E_OUT_OF_RANGE  width or height > 16384
 * crtu_low_size refuses what crtu_upsample refuses of its arguments, and a NULL lowWidth or lowHeight.
 *
 * The kernel: crtu_upsample_kernel, one lane per full pixel, 256-lane workgroups over 32 x 8 tiles. A tile touches at most
 * (32/F + 2) x (8/F + 2) low samples -- 18 x 6 at factor 2, 10 x 4 at factor 4. In the staged form the workgroup first stages those samples in
 * LDS -- guide {n, t}, instance and the 1 or 4 value channels -- and each lane takes its four taps from there; in the other form each lane
 * gathers its taps' guides and values through L1. CRTU_TAPS=l1|lds in the environment (read by every call) overrides the built-in choice: for
 * measurements. The bits are the same whichever is chosen. */
#ifndef CRT_UPSAMPLE_H
#define CRT_UPSAMPLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CRTU_OK = 0, CRTU_E_BAD_ARGUMENT = -2, CRTU_E_OUT_OF_RANGE = -3 };   /* same values as CrtStatus */
enum { CRTU_GUIDES_PLANES = 0, CRTU_GUIDES_SURFACE = 1 };                   /* the two layouts of crt_denoise.h */
enum { CRTU_MATCH_INSTANCE = 1, CRTU_MODULATE = 2 };
enum { CRTU_STATE_INTERPOLATED = 0, CRTU_STATE_NEAREST = 1, CRTU_STATE_EMPTY = 2 };

/* 40 bytes (LP64): width 0, height 4, guides 8 (4 bytes of padding behind it), geometry 16, ids 24, albedo 32 */
typedef struct {
    int32_t width, height;  /* of the FULL-resolution frame, whose guides these are */
    int32_t guides;         /* PLANES: geometry = float4[W*H] (CRT_GBUFFER_GEOMETRY), ids = 16-B records (CRT_GBUFFER_IDS, may be NULL
                               without MATCH_INSTANCE), albedo = uint32[W*H] (CRT_GBUFFER_ALBEDO, may be NULL without MODULATE).
                               SURFACE: geometry = CrtSurfaceHit[W*H] (48 B, what crt_shade_rays writes); ids and albedo must be NULL */
    const void *geometry, *ids, *albedo;
} CrtuFrame;

/* 24 bytes (LP64): low 0, channels 8, factor 12, offsetX 16, offsetY 20 */
typedef struct {
    const void* low;        /* float[LW*LH] (channels 1) or float4[LW*LH] (channels 4), row-major; never written */
    int32_t channels;       /* 1 or 4 */
    int32_t factor;         /* 2 or 4 */
    int32_t offsetX, offsetY;   /* 0 .. factor-1: low sample (X, Y) sits on full pixel (factor*X + offsetX, factor*Y + offsetY) */
} CrtuLow;

/* 12 bytes: flags 0, depthTol 4, normalCos 8 */
typedef struct {
    uint32_t flags;         /* CRTU_MATCH_INSTANCE | CRTU_MODULATE */
    float depthTol;         /* >= 0 (+inf allowed), relative to the centre's distance */
    float normalCos;        /* no NaN (-inf allowed) */
} CrtuParams;

int crtu_low_size(int32_t width, int32_t height, int32_t factor, int32_t offsetX, int32_t offsetY, int32_t* lowWidth, int32_t* lowHeight);
int crtu_upsample(const CrtuFrame* f, const CrtuLow* l, const CrtuParams* p, void* out /* float[W*H] or float4[W*H], as channels says */,
                  void* outState /* uint32[W*H] or NULL */, void* stream);
const char* crtu_error_string(int rc);

#ifdef __cplusplus
}
#endif

#endif
