/* crt_motion.h -- C ABI of libcrt_motion.so: temporal reprojection and accumulation that follows moving instances, HIP for gfx950.
 *
 * No reference counterpart. crtt_accumulate (crt_temporal.h) fetches the history where the world point a pixel sees now lay on the previous
 * camera's screen, which is where the SURFACE was only if the surface stood still. crtm_accumulate takes, beside the same arguments, one record
 * per instance saying where a point of that instance was in the previous frame, and reprojects through it. A library of its own beside
 * libcrt_temporal.so, stateless like it: every buffer is the caller's, the motion table included; the library creates and destroys no HIP object,
 * allocates nothing, copies nothing and never waits on the host. It uses crt_temporal.h's types as they are -- a history written by either library
 * is a valid `prev` for the other, and crtt_camera makes the cameras -- and restates its blend; wherever nothing moves the two agree in every bit.
 *
 * Conventions: crtm_accumulate returns 0, a negative CRTT_E_* code or a positive hipError_t when the launch fails; crtm_motion and crtm_motions
 * return 0 or a CRTT_E_* code; crtm_error_string explains either. The argument checks, crtm_motion and crtm_motions need no GPU.
 *
 * Motion records. An instance's inverseTransform is a CrtMatrix4 (crt_types.h): row-major, row-vector convention, p_local = p_world * inverse.
 * The fourth COLUMN of either input is never read, as the trace kernel never reads it when a ray enters an instance (crt_device.h: xform_xyz and
 * mat3mul use columns 0..2 only): the map is p_local = p_world * A + b with A = rows 0..2 and b = row 3 of columns 0..2, whatever column 3 holds
 * (only the STATIC comparison below and the finiteness check look at all 16 elements). With T = curInverse * inverse(prevInverse) under that
 * reading -- L = A_cur * A_prev^-1, the row T[3] = (b_cur - b_prev) * A_prev^-1 -- a point of the instance at world position p now was at
 * p * T in the previous frame. crtm_motion (host only, in double, rounded to float32 at the end) makes
 *   point[4k + j]  = T[j][k] for j < 3, point[4k + 3] = T[3][k]:  previous.k = dot3(point[4k .. 4k+2], p) + point[4k+3]
 *   normal[3k + j] = (L^-1)[k][j], L^-1 = A_prev * A_cur^-1:      a normal n now was (before normalising) m.k = dot3(normal[3k .. 3k+2], n)
 *   kind = CRTM_NEW when prevInverse is NULL (point and normal are the identity's), CRTM_STATIC with the identity's point and normal when the two
 *   inputs are equal in all 16 float bit patterns, CRTM_MOVING otherwise.
 * CRTT_E_BAD_ARGUMENT: a NULL curInverse or out, a non-finite element of either input, a singular A_prev or L (|det| <= 1e-12 * the product of
 * the rows' lengths), a result that is not finite in float32. A refusal writes nothing. crtm_motions does the same over two arrays of
 * CrtMeshInstance records (80-B stride, the matrix first): out[i] for i < curCount from prev[i] and cur[i], CRTM_NEW for i >= prevCount; the
 * first refusal is returned (records before it are written). A NULL array goes with a count of 0 only.
 *
 * Definition. crtm_accumulate is crtt_accumulate's definition (crt_temporal.h) word for word -- the same float32 arithmetic without contraction,
 * dot3, taps, stops, select-away, clamp and blend -- with these differences. kind(x, y) = table[i].kind for the pixel's instance id i; an id < 0 or
 * >= count, or a NULL table, is CRTM_STATIC, and so is a kind that is none of the three.
 *   CRTM_STATIC: exactly crt_temporal.h: v = (pos_cur - pos_prev) + d*t, and the normal test uses n.
 *   CRTM_NEW:    no history.
 *   CRTM_MOVING, per component: P = pos_cur + d*t; Pp.k = dot3(point[4k], point[4k+1], point[4k+2], P) + point[4k+3]; v = Pp - pos_prev;
 *                m.k = dot3(normal[3k .. 3k+2], n), then m = m / sqrtf(dot3(m, m)). dist, u, the on-screen test and the taps follow from this v; the
 *                normal test is dot3(n_q, m) >= normalCos (a NaN m makes it false). Everything else is unchanged; next->geometry keeps the
 *                current frame's {n, t}.
 *   m->vectors, when given, is written at EVERY pixel: {fx - x, fy - y, dist, state} (x, y as floats). state 2: history kept; state 1:
 *                reprojected on the previous screen but no history; state 0, with zeros in the other three: not a hit, no prev, CRTM_NEW or off
 *                screen. A screen-space motion-vector plane for callers that warp other buffers.
 *
 * crtm_accumulate ENQUEUES one launch on `stream` AND RETURNS, as crtt_accumulate does. The table is only read (by the launch: it must stay
 * valid and unchanged until the launch has run). Errors, all before anything is enqueued: every refusal of crtt_accumulate, with its code; and
 *   CRTT_E_BAD_ARGUMENT  a NULL m; a NULL table with count != 0 or a table with count 0; count > 65536; a table with cur->ids missing under
 *                        CRTT_GUIDES_PLANES; vectors equal to any plane of cur, prev or next
 *
 * The kernel: crt_temporal.h's, in the two forms DESIGN.md 4l measured as best and no other (taps gated behind the geometry test; the clamp's
 * neighbourhood from an LDS tile with a halo of 1), plus, in round one, the lane's `kind` and -- only in a wave with a moving lane -- its
 * matrices, as plain vector loads through L1. Without CRTT_CLAMP the kernel is launched with 28 KiB of dynamic LDS it never touches, which holds it
 * to the 5 waves per SIMD at which it measures fastest. */
#ifndef CRT_MOTION_H
#define CRT_MOTION_H

#include "crt_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { CRTM_STATIC = 0, CRTM_MOVING = 1, CRTM_NEW = 2 };
enum { CRTM_MAX_COUNT = 65536 };

/* 88 bytes, alignment 4 */
typedef struct { uint32_t kind; float point[12]; float normal[9]; } CrtmMotion;

/* 24 bytes (LP64): table 0, count 8 (4 bytes of padding behind it), vectors 16 */
typedef struct {
    const void* table;      /* CrtmMotion[count] in device memory, or NULL with count 0; never written */
    uint32_t count;
    void* vectors;          /* float4[W*H] or NULL */
} CrtmMotionArgs;

int crtm_motion(const float prevInverse[16] /* NULL: CRTM_NEW */, const float curInverse[16], CrtmMotion* out);   /* host only */
int crtm_motions(const void* prevInstances, uint32_t prevCount, const void* curInstances, uint32_t curCount, CrtmMotion* out);   /* host only */
int crtm_accumulate(const CrttFrame* cur, const CrttHistory* prev /* NULL: reset */, const CrttHistory* next, const CrttParams* p,
                    const CrtmMotionArgs* m, void* stream);
const char* crtm_error_string(int rc);

#ifdef __cplusplus
}
#endif

#endif
