/* crt_present.h -- C ABI of libcrt_present.so: the last step of the chain on device buffers -- compose, tone-map, FXAA and RGBA8 -- and the
 * ID views of the G-buffer. HIP for gfx950.
 *
 * The stages that follow Trace in a frame (upstream's RGBA8 render target, PostProcess, the FXAA extension, the packed bytes of
 * crt_read_output_rgba8) exist in libcrt_hip.so for the frame's own one-sample colour only. crtp_present applies the same stages -- the same
 * functions, csrc/crt_post.h, compiled into both libraries -- to any float4 image on the device: a denoised, accumulated or upsampled pass,
 * optionally multiplied by an ambient-occlusion plane and an exposure first. On the plain colour of a frame it gives the frame's own bits (see
 * "Consequence"). crtp_view turns a plane of the G-buffer, a float plane or a state plane into a picture. A library of its own beside
 * libcrt_hip.so and the seven image libraries (crt_denoise.h, crt_temporal.h, crt_vfilter.h, crt_motion.h, crt_upsample.h, crt_select.h),
 * stateless like them: every buffer is the caller's; the library creates and destroys no HIP object, allocates nothing, copies nothing and
 * never waits on the host.
 *
 * Conventions: every call returns 0, a negative CRTP_E_* code (the values of CrtStatus) or a positive hipError_t when a launch fails;
 * crtp_error_string explains either. The argument checks need no GPU: the library loads and answers them on a machine without one. Each call
 * ENQUEUES its launch on `stream` (a hipStream_t; NULL: HIP's null stream) AND RETURNS: no synchronisation. Errors come before anything is
 * enqueued.
 *
 * Definition. Every value is float32 arithmetic without contraction (a*b + c is a multiply, then an add); / and sqrtf are correctly rounded;
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; every comparison with a NaN is false. A pixel's index is k = y*W + x.
 *   unorm8(v)      u = v * 255.0f; 0 where u is a NaN or u <= 0; 255 where u >= 255; else (uint32)rintf(u) (ties to even)
 *   quantize1(v)   (float)unorm8(v) / 255.0f; quantize3 per component
 *   pack_rgba8(c)  unorm8(c.x) | unorm8(c.y) << 8 | unorm8(c.z) << 16 | 0xFF000000
 *   post_pixel(c, x, y, W, H)   upstream's PostProcess as crt_api.h defines CRT_RENDER_POSTPROCESS: saturation 1.2 about
 *                  P = sqrtf((c.x*c.x)*0.299f + ((c.y*c.y)*0.587f) + ((c.z*c.z)*0.114f)); Reinhard on l = dot3(c, (0.2126, 0.7152, 0.0722)) with
 *                  white 0.8: c * ((l * (1 + l / (0.8f*0.8f))) / (1 + l) / l); powf(c, 1/1.55f); powf(c, 1/1.2f); times the vignette
 *                  powf(((u*(1-v)) * (v*(1-u))) * 15, 0.15f) with u = (float)x / (float)W, v = (float)y / (float)H
 *   fxaa(S, x, y)  what crt_fxaa_kernel computes at (x, y) over the image S up to the value it chooses (rgbA or rgbB), every read clamped to
 *                  the edge: four diagonal neighbours and the centre, a direction clamped to +-8 pixels, four bilinear taps at +-1/6 and +-1/2
 *                  of it. The oracle's orc_fxaa restates it operation for operation.
 * All five are csrc/crt_post.h's functions: one text, two libraries.
 *
 * 1. crtp_present. Per pixel, with c = color[k].rgb (alpha is ignored):
 *      1. CRTP_HEAL: a component of c that is not finite becomes 0.0f.
 *      2. ao != NULL: f = (1.0f - aoStrength) + aoStrength * ao[k]; under CRTP_HEAL a non-finite f becomes 1.0f; c = c * f per component. With
 *         ao == NULL the step does not exist (no multiply by 1).
 *      3. exposure != 1.0f: c = c * exposure per component. With exposure == 1.0f the step does not exist.
 *      4. CRTP_UNORM8: c = quantize3(c) -- the store and load through upstream's render target.
 *      5. CRTP_FXAA: call the image of the values after step 4 S. c = fxaa(S, x, y): steps 1-4 at every pixel, then the filter.
 *      6. CRTP_POST: c = post_pixel(c, x, y, W, H).
 *      7. CRTP_UNORM8 and (CRTP_POST or CRTP_FXAA): c = quantize3(c) again -- the frame's rule (finish_pixel, the tail of crt_fxaa_kernel).
 *      8. outColor[k] = {c, 1.0f} and outBytes[k] = pack_rgba8(c), each where given; the bytes saturate and round whether or not CRTP_UNORM8
 *         is set.
 *    Consequence: with ao == NULL, exposure == 1.0f, no CRTP_HEAL and color = the float frame of crt_render(flags 0), outColor and outBytes
 *    equal crt_read_output and crt_read_output_rgba8 of crt_render with CRT_RENDER_POSTPROCESS (CRTP_POST), CRT_RENDER_UNORM8 (CRTP_UNORM8)
 *    and CRT_RENDER_FXAA (CRTP_FXAA) set alike, bit for bit, for all eight combinations.
 *    The kernel: one launch of 256-lane workgroups over 32 x 8 tiles, the four flags template parameters; whether there is an AO plane and an
 *    exposure are kernel-uniform branches. Without CRTP_FXAA a lane reads 16 (+ 4) bytes and writes 16 and/or 4. With CRTP_FXAA the workgroup
 *    first stages S over its tile and a halo of CRTP_FXAA_HALO = 5 pixels in LDS (42 x 18 texels, {S, 0} as 16 bytes each: 12096 bytes) -- a
 *    tap lies at most 5 pixels left of or above and 4 right of or below its pixel -- and the filter reads LDS; CRTP_TAPS=l1 in the environment
 *    (read by every call; anything but l1 or lds means the built-in choice, lds) makes each tap recompute S from color and ao through L1
 *    instead. Both give the same values.
 *    scratch: crtp_scratch_bytes(width, height, flags) bytes of the caller's; the shipped kernels need none, so it is 0 for every input and
 *    scratch is then not looked at.
 *    CRTP_E_BAD_ARGUMENT  a NULL struct or color; both outputs NULL; an output equal to color, to ao or to the other output (for any flags: the
 *                         filter reads neighbours); scratch NULL or equal to any other buffer when crtp_scratch_bytes is not 0; an unknown
 *                         flag; a non-finite aoStrength or exposure; aoStrength outside 0..1; !(exposure > 0); width or height < 1
 *    CRTP_E_OUT_OF_RANGE  width or height > 16384
 *
 * 2. crtp_view. The frame's guides in one of the two layouts of crt_denoise.h: CRTP_GUIDES_PLANES (geometry float4[W*H] = {n, t}; ids 16-byte
 *    records {int32 instance, uint32 triIndex, u, v}; albedo uint32[W*H] = 0xFF000000 | b << 16 | g << 8 | r) or CRTP_GUIDES_SURFACE (geometry
 *    = CrtSurfaceHit[W*H] of 48 bytes, which hold all three; ids and albedo must be NULL). Every mode is defined in bytes r, g, b:
 *    outBytes[k] = r | g << 8 | b << 16 | 0xFF000000 and outColor[k] = {(float)r / 255.0f, (float)g / 255.0f, (float)b / 255.0f, 1.0f}. A
 *    pixel is a HIT iff t <= 99998.0f (a NaN t is no hit). magenta = 255, 0, 255.
 *      CRTP_VIEW_NORMAL    geometry. hit: unorm8(n * 0.5f + 0.5f) per component; else 0, 0, 0
 *      CRTP_VIEW_DEPTH     geometry, scale. hit: r = g = b = unorm8(scale / (t + scale)); else 0, 0, 0
 *      CRTP_VIEW_INSTANCE  ids. instance >= 0: the low three bytes (r lowest) of hash((uint32)instance); else 0, 0, 0
 *      CRTP_VIEW_TRIANGLE  ids. instance >= 0: likewise of hash((uint32)instance * 0x9E3779B1u + triIndex); else 0, 0, 0
 *      CRTP_VIEW_ALBEDO    albedo. the word's r, g, b bytes: w & 255, (w >> 8) & 255, (w >> 16) & 255
 *      CRTP_VIEW_SCALAR    plane = float[W*H], lo, hi. v = plane[k]; a NaN: magenta; else r = g = b = unorm8((v - lo) / (hi - lo))
 *      CRTP_VIEW_STATE     plane = uint32[W*H]. 0 (CRTU_STATE_INTERPOLATED): 32, 32, 32; 1 (CRTU_STATE_NEAREST): 255, 160, 0; 2
 *                          (CRTU_STATE_EMPTY): 255, 0, 0; 3 (CRTS_STATE_RETRACED): 0, 200, 80; any other word: magenta
 *    hash(h): h *= 0x9E3779B1u; h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16 (uint32 arithmetic). No mode
 *    uses a transcendental. One launch, one lane per pixel.
 *    CRTP_E_BAD_ARGUMENT  a NULL struct; both outputs NULL; an unknown mode or layout; a plane the mode needs is NULL (geometry for NORMAL and
 *                         DEPTH; under PLANES ids for INSTANCE and TRIANGLE and albedo for ALBEDO; under SURFACE geometry for those; plane
 *                         for SCALAR and STATE); ids or albedo given under SURFACE; DEPTH with a scale that is not finite or not > 0; SCALAR
 *                         with lo or hi not finite or !(lo < hi); an output equal to geometry, ids, albedo, plane or the other output; width
 *                         or height < 1
 *    CRTP_E_OUT_OF_RANGE  width or height > 16384 */
#ifndef CRT_PRESENT_H
#define CRT_PRESENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CRTP_OK = 0, CRTP_E_BAD_ARGUMENT = -2, CRTP_E_OUT_OF_RANGE = -3 };   /* same values as CrtStatus */
enum { CRTP_GUIDES_PLANES = 0, CRTP_GUIDES_SURFACE = 1 };                   /* the two layouts of crt_denoise.h */
enum { CRTP_UNORM8 = 1, CRTP_POST = 2, CRTP_FXAA = 4, CRTP_HEAL = 8 };      /* CrtpPresent.flags */
enum { CRTP_VIEW_NORMAL = 0, CRTP_VIEW_DEPTH = 1, CRTP_VIEW_INSTANCE = 2, CRTP_VIEW_TRIANGLE = 3, CRTP_VIEW_ALBEDO = 4, CRTP_VIEW_SCALAR = 5,
       CRTP_VIEW_STATE = 6 };                                               /* CrtpView.mode */
enum { CRTP_FXAA_HALO = 5 };            /* the pixels around a tile the FXAA form stages */

/* 40 bytes (LP64): width 0, height 4, color 8, ao 16, aoStrength 24, exposure 28, flags 32, 4 bytes of tail padding */
typedef struct {
    int32_t width, height;
    const void* color;      /* float4[W*H]; alpha is ignored; never written */
    const void* ao;         /* float[W*H] or NULL */
    float aoStrength;       /* 0 .. 1 */
    float exposure;         /* finite, > 0; 1.0f: no such step */
    uint32_t flags;         /* CRTP_UNORM8 | CRTP_POST | CRTP_FXAA | CRTP_HEAL */
} CrtpPresent;

/* 64 bytes (LP64): width 0, height 4, guides 8, mode 12, geometry 16, ids 24, albedo 32, plane 40, scale 48, lo 52, hi 56, 4 bytes of tail padding */
typedef struct {
    int32_t width, height;
    int32_t guides;         /* CRTP_GUIDES_PLANES or CRTP_GUIDES_SURFACE */
    int32_t mode;           /* CRTP_VIEW_* */
    const void* geometry;   /* PLANES: float4[W*H]. SURFACE: CrtSurfaceHit[W*H] (48 B) */
    const void* ids;        /* PLANES: 16-B records; NULL under SURFACE */
    const void* albedo;     /* PLANES: uint32[W*H]; NULL under SURFACE */
    const void* plane;      /* SCALAR: float[W*H]. STATE: uint32[W*H] */
    float scale;            /* DEPTH: finite, > 0 */
    float lo, hi;           /* SCALAR: finite, lo < hi */
} CrtpView;

size_t crtp_scratch_bytes(int32_t width, int32_t height, uint32_t flags);
int crtp_present(const CrtpPresent* p, void* outColor /* float4[W*H] or NULL */, void* outBytes /* uint32[W*H] or NULL */, void* scratch,
                 void* stream);
int crtp_view(const CrtpView* v, void* outColor /* float4[W*H] or NULL */, void* outBytes /* uint32[W*H] or NULL */, void* stream);
const char* crtp_error_string(int rc);

#ifdef __cplusplus
}
#endif

#endif
