/* crt_temporal.h -- C ABI of libcrt_temporal.so: temporal reprojection and accumulation on device buffers, HIP for gfx950.
 *
 * No reference counterpart (upstream traces one sample per pixel per frame and keeps nothing). The stage between the tracer and the filter of
 * crt_denoise.h: trace -> accumulate -> filter. Each frame's noisy float4 image is blended into a history that is fetched where the pixel's
 * surface was in the previous frame, and dropped where that place shows something else. A library of its own beside libcrt_hip.so and
 * libcrt_denoise.so, stateless like the latter: every buffer is the caller's, history included; the library creates and destroys no HIP object,
 * allocates nothing, copies nothing and never waits on the host.
 *
 * Conventions: crtt_accumulate returns 0, a negative CRTT_E_* code (the values of CrtStatus) or a positive hipError_t when the launch fails;
 * crtt_error_string explains either. The argument checks and crtt_camera need no GPU: the library loads and answers them on a machine without one.
 *
 * Cameras. RayGen's direction of pixel (i, j) is normalize(invView * (invProj * (cx, cy, 1, 1) / w, 1)) with cx = 2i/W - 1, cy = 2j/H - 1 and
 * w the fourth component of invProj * (cx, cy, 1, 1). With A = invView * invProj that is normalize((1/w) * A[rows 0..2] * (cx, cy, 1, 1)): the
 * unnormalised direction is a 3 x 3 map of (i, j, 1), and the inverse of that map takes a world-space vector from the camera back to pixel
 * coordinates. The kernel knows no matrix convention: it sees CrttCamera values only, and crtt_camera (host only) makes them:
 *   toRay    = sign * [A col 0, A col 1, A col 2 + A col 3](rows 0..2) * S, S = {{2/W, 0, -1}, {0, 2/H, -1}, {0, 0, 1}} taking (i, j, 1) to
 *              (cx, cy, 1), sign = the sign of w at the frame's centre; row-major, toRay[3r + c]
 *   toScreen = toRay^-1, row-major; both are computed in double and rounded to float32
 *   for a world point P: u = toScreen * (P - pos); its pixel coordinates are (u.x / u.z, u.y / u.z), and it is in front of the camera iff u.z > 0
 * crtt_camera returns CRTT_E_BAD_ARGUMENT for a NULL pointer, width or height < 1, a non-finite input, a w of zero at the centre, a w whose sign
 * differs among the four corners (i, j) = (0, 0), (W, 0), (0, H), (W, H), or a singular (or non-finite) toRay.
 *
 * Definition. Every value is float32 arithmetic without contraction (a*b + c is a multiply, then an add); / and sqrtf are correctly rounded;
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z and luma(c) = (0.299f*c.x + 0.587f*c.y) + 0.114f*c.z as in crt_denoise.h; a matrix times a vector
 * is one dot3 per row. min(a, b) = a < b ? a : b and max(a, b) = a > b ? a : b (so a NaN b is taken); fminf / fmaxf are C's (a NaN is dropped).
 *   Per pixel (x, y): g = {n, t} its guide, c = its color; HIT iff t <= 99998.0f (so a NaN t is no hit); L = luma(c.rgb).
 *     next->geometry = g; next->instance = the pixel's instance (when that plane is given); out.a = c.a. out is next->color.
 *   No history (prev == NULL, a pixel that is no hit, or any "no history" below): out.rgb = c.rgb, moments = {L, L*L, HIT ? 1 : 0, 0}.
 *   Reprojection of a hit pixel: d = toRay_cur * (x, y, 1), then d = d / sqrtf(dot3(d, d)) per component;
 *     v = (pos_cur - pos_prev) + d*t per component; dist = sqrtf(dot3(v, v)); u = toScreen_prev * v.
 *     No history unless u.z > 0 and fx = u.x / u.z >= -1 and fx < W and fy = u.y / u.z >= -1 and fy < H (every comparison with a NaN is false).
 *     x0 = (int)floorf(fx), ax = fx - floorf(fx); y0 and ay likewise.
 *   Taps (dx, dy) = (0,0), (1,0), (0,1), (1,1) at q = (x0 + dx, y0 + dy): a tap outside the frame is skipped; its weight is
 *     b = (dx ? ax : 1 - ax) * (dy ? ay : 1 - ay). A tap counts iff its prev->geometry is a hit and fabsf(t_q - dist) <= depthTol * dist and
 *     dot3(n_q, n) >= normalCos and, under CRTT_MATCH_INSTANCE, prev->instance_q == the pixel's instance, and N_q >= 1 and every one of
 *     prev->color_q.rgb, m1_q and m2_q is finite ({m1, m2, N, variance} = prev->moments). A tap that does not count contributes NOTHING: it is
 *     selected away, not multiplied by zero, so a NaN in the history heals instead of spreading. Over the taps that count, in tap order, from
 *     0: sums of color.rgb*b, m1*b, m2*b, N*b and b (wsum). No history unless wsum > 0.01f; else h.rgb, m1_h, m2_h, N_h = each sum / wsum.
 *   CRTT_CLAMP: mn = +inf, mx = -inf per channel; over the 3 x 3 pixels around (x, y) that lie inside the frame, row-major:
 *     mn = min(mn, cur->color_q), mx = max(mx, cur->color_q); then per channel h = min(max(h, mn), mx).
 *   Blend: N = fminf(N_h + 1, maxHistory); a = fmaxf(alpha, 1 / N), am = fmaxf(momentsAlpha, 1 / N);
 *     out.rgb = h*(1 - a) + c*a per channel; m1 = m1_h*(1 - am) + L*am; m2 = m2_h*(1 - am) + (L*L)*am;
 *     variance = m2 - m1*m1 where that is > 0, else 0; moments = {m1, m2, N, variance}.
 *
 * crtt_accumulate ENQUEUES one launch on `stream` (a hipStream_t; NULL: HIP's null stream) AND RETURNS: no synchronisation. cur and prev are
 * only read; every pixel of next->color, next->moments, next->geometry and (when given) next->instance is written, none needs initialising. The
 * history keeps its guides as {n, t} float4 and int32 planes whatever layout cur uses, written from the values the kernel has loaded: nobody
 * copies the previous frame's G-buffer. next->camera and prev->camera: only prev->camera is read (the caller keeps next's camera = cur's).
 * Errors, all before anything is enqueued:
 *   CRTT_E_BAD_ARGUMENT  a NULL cur, next or p; a NULL cur->color or cur->geometry; a NULL color, moments or geometry of next, or of a prev
 *                        that is given; a plane that needs another missing: cur->ids (under CRTT_GUIDES_PLANES) when next->instance is given
 *                        or under CRTT_MATCH_INSTANCE, next->instance under CRTT_MATCH_INSTANCE, prev->instance of a prev that is given under
 *                        CRTT_MATCH_INSTANCE; ids given under CRTT_GUIDES_SURFACE; any plane of next equal to another plane of next or to any
 *                        plane of prev or cur; an unknown flag or guide layout; alpha or momentsAlpha outside (0, 1]; !(maxHistory >= 1) or an
 *                        infinite one; !(depthTol >= 0); a normalCos that is not finite; width or height < 1
 *   CRTT_E_OUT_OF_RANGE  width or height > 16384
 *
 * The kernel: one launch, one lane per pixel, 256-lane workgroups over 32 x 8 tiles. A lane loads its pixel, reprojects, then issues the loads
 * of its four taps together (addresses clamped; what must not count is chosen away afterwards). Two choices were measured and can
 * be overridden in the environment, read by every call: CRTT_TAPS=all|gated (the taps' colour and moments loaded unconditionally, or only behind
 * the geometry test) and CRTT_CLAMP_TAPS=l1|lds (the 3 x 3 neighbourhood of CRTT_CLAMP as row reads through L1, or from a tile staged in LDS
 * with a halo of 1). The bits are the same whichever is chosen. */
#ifndef CRT_TEMPORAL_H
#define CRT_TEMPORAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CRTT_OK = 0, CRTT_E_BAD_ARGUMENT = -2, CRTT_E_OUT_OF_RANGE = -3 };   /* same values as CrtStatus */
enum { CRTT_GUIDES_PLANES = 0, CRTT_GUIDES_SURFACE = 1 };
enum { CRTT_MATCH_INSTANCE = 1, CRTT_CLAMP = 2 };
enum { CRTT_PLANE_COLOR = 0, CRTT_PLANE_MOMENTS = 1, CRTT_PLANE_GEOMETRY = 2, CRTT_PLANE_INSTANCE = 3 };   /* crtt_history_bytes */

/* 84 bytes, alignment 4 */
typedef struct { float pos[3]; float toRay[9]; float toScreen[9]; } CrttCamera;

/* 128 bytes (LP64): width 0, height 4, color 8, guides 16 (4 bytes of padding behind it), geometry 24, ids 32, camera 40, 4 bytes of tail padding */
typedef struct {
    int32_t width, height;
    const void* color;      /* float4[W*H], row-major: the frame's noisy radiance; never written */
    int32_t guides;         /* PLANES: geometry = float4[W*H] (CRT_GBUFFER_GEOMETRY), ids = 16-B records (CRT_GBUFFER_IDS; may be NULL when
                               next->instance is NULL). SURFACE: geometry = CrtSurfaceHit[W*H] (48 B, what crt_shade_rays writes); ids must be NULL */
    const void *geometry, *ids;
    CrttCamera camera;      /* the camera the frame was shot with */
} CrttFrame;

/* 120 bytes (LP64): color 0, moments 8, geometry 16, instance 24, camera 32, 4 bytes of tail padding */
typedef struct {
    void* color;            /* float4[W*H]: the accumulated radiance; a is the last frame's */
    void* moments;          /* float4[W*H]: {m1, m2, N, variance} of the luminance; N = frames accumulated, 0 for a pixel that is no hit */
    void* geometry;         /* float4[W*H]: {n, t} */
    void* instance;         /* int32[W*H]; may be NULL without CRTT_MATCH_INSTANCE */
    CrttCamera camera;      /* the camera those planes were made with */
} CrttHistory;

/* 24 bytes */
typedef struct {
    uint32_t flags;         /* CRTT_MATCH_INSTANCE | CRTT_CLAMP */
    float alpha;            /* (0, 1]: the least share of the new frame in the colour */
    float momentsAlpha;     /* (0, 1]: the same for the moments */
    float maxHistory;       /* >= 1, finite: N stops growing there */
    float depthTol;         /* >= 0, relative to the reprojected distance */
    float normalCos;        /* finite */
} CrttParams;

int crtt_camera(const float invView[16], const float invProj[16], const float pos[3], int32_t width, int32_t height, CrttCamera* out);
size_t crtt_history_bytes(int32_t width, int32_t height, int plane);   /* W*H*16 for colour, moments and geometry, W*H*4 for instance; else 0 */
int crtt_accumulate(const CrttFrame* cur, const CrttHistory* prev /* NULL: reset */, const CrttHistory* next, const CrttParams* p, void* stream);
const char* crtt_error_string(int rc);

#ifdef __cplusplus
}
#endif

#endif
