/* crt_select.h -- C ABI of libcrt_select.so: selective re-tracing on device buffers -- compact, gather, scatter -- HIP for gfx950.
 *
 * No reference counterpart. The step between the image libraries and the point queries of crt_api.h: a mask or a crtu_upsample state plane becomes
 * an ordered, padded list of pixel indices (crts_compact); listed pixels, or the pixels a low-resolution pass sits on, become the positions and
 * normals crt_trace_ao and the ray queries take (crts_points); and what was traced for them goes back into the full image (crts_scatter). The
 * number of selected items is known only on the device, and every query takes its n on the host; so the list has a fixed CAPACITY the caller
 * chooses, and the entries behind the selected ones are CRTS_NONE. crts_points turns a CRTS_NONE entry into an all-zero row, crt_trace_ao defines
 * that an item whose normal is exactly (0, 0, 0) traces nothing, and crts_scatter skips the entry: the whole chain is enqueued with host-known
 * sizes and nobody waits for the device. The list is in ASCENDING order, so that the re-traced rays keep the coherence of pixel order.
 * A library of its own beside libcrt_hip.so and the five image libraries (crt_denoise.h, crt_temporal.h, crt_vfilter.h, crt_motion.h,
 * crt_upsample.h), stateless like them: every buffer is the caller's, scratch included; the library creates and destroys no HIP object, allocates
 * nothing, copies nothing and never waits on the host.
 *
 * Conventions: every call returns 0, a negative CRTS_E_* code (the values of CrtStatus) or a positive hipError_t when a launch fails;
 * crts_error_string explains either. The argument checks need no GPU: the library loads and answers them on a machine without one. Each call
 * ENQUEUES its launches on `stream` (a hipStream_t; NULL: HIP's null stream) AND RETURNS: no synchronisation. Errors come before anything is
 * enqueued.
 *
 * Definition. Every value is float32 arithmetic without contraction (a*b + c is a multiply, then an add); / and sqrtf are correctly rounded;
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z as in crt_denoise.h; a matrix times a vector is one dot3 per row; every comparison with a NaN is
 * false. A pixel's index is k = y*W + x.
 *
 * 1. crts_compact. words: n items of wordBytes 1 (uint8: a bool or byte mask) or 4 (uint32: a crtu_upsample state plane), aligned to wordBytes
 *    only. Item k is SELECTED iff words[k] < 32 && ((values >> words[k]) & 1). For the upsample's plane values = 1 << CRTU_STATE_NEAREST |
 *    1 << CRTU_STATE_EMPTY = 6; for a mask values = 2. total = the number of selected items.
 *      list[j], j < min(total, capacity): the index of the j-th selected item in ascending order;
 *      list[j], min(total, capacity) <= j < capacity: CRTS_NONE;
 *      counts = {total, min(total, capacity)}.
 *    Every entry of list and counts is written; neither needs initialising. total > capacity is no error: the first `capacity` selected items are
 *    listed and counts shows it. scratch: crts_scratch_bytes(n) bytes of the caller's, aligned to 4, not initialised; calls in flight at the
 *    same time need different scratch buffers (and calls on one stream may share one).
 *    The kernels, three launches: crts_count_kernel, one 256-lane workgroup per chunk of CRTS_CHUNK items, writes the chunk's number of selected
 *    items to scratch; crts_scan_kernel, ONE workgroup, turns the chunk sums into exclusive offsets, CRTS_SCAN of them per round with a carry in
 *    a register, and writes counts; crts_write_kernel, one workgroup per chunk again, selects again and writes each selected index at its
 *    chunk's offset + its rank in the chunk (wave ballots, mbcnt, the wave sums through LDS), and the workgroup whose number is j / CRTS_CHUNK
 *    writes the CRTS_NONE of entry j. No kernel waits for another workgroup, there is no atomic, and every entry has one writer: the bits do
 *    not depend on scheduling.
 *    CRTS_E_BAD_ARGUMENT  a NULL struct, words, list, counts or scratch; wordBytes other than 1 or 4; n < 1 or capacity < 1; two of words, list,
 *                         counts, scratch equal
 *    CRTS_E_OUT_OF_RANGE  n or capacity > CRTS_MAX_ITEMS = 2^28 (16384 x 16384)
 *    crts_scratch_bytes(n) is 0 for an n crts_compact refuses, else > 0 and monotone in n.
 *
 * 2. crts_points. The frame: width, height, the guide layout and geometry of crt_denoise.h ({n, t} per pixel: float4[W*H] under
 *    CRTS_GUIDES_PLANES, the first 16 bytes of CrtSurfaceHit[W*H] records of 48 bytes under CRTS_GUIDES_SURFACE) and the CrttCamera of
 *    crt_temporal.h, made by crtt_camera: the kernel knows no matrix convention. The items, `count` of them, in one of two forms:
 *      list != NULL: item j is pixel k = list[j], uint32, as crts_compact writes it; factor, offsetX and offsetY are not looked at;
 *      list == NULL: the grid of a low-resolution pass. factor F is 1, 2 or 4; offsetX, offsetY lie in 0 .. F-1 and below width, height;
 *                    LW = (W - offsetX + F - 1) / F, LH likewise (crtu_low_size's, and W, H at factor 1); count must be LW*LH; item j is low
 *                    sample (X, Y) = (j % LW, j / LW), which sits on pixel (x, y) = (F*X + offsetX, F*Y + offsetY).
 *    Per item, with (x, y) = (k % W, k / W) and g = {n, t} the pixel's guide:
 *      d = toRay * ((float)x, (float)y, 1.0f), then d = d / sqrtf(dot3(d, d)) per component (crt_temporal.h's reprojection line);
 *      the pixel is a HIT iff t <= 99998.0f (so a NaN t is no hit);
 *      a hit:    positions[j] = {pos.x + d.x*t, pos.y + d.y*t, pos.z + d.z*t, t}; normals[j] = {n', 0} with n' = dot3(n, d) > 0 ? -n : n (the
 *                stored normal turned towards the viewer; -n flips the sign bit of each component); dirs[j] = {d, 0};
 *      no hit:   positions[j] = {0, 0, 0, t}; normals[j] = {0, 0, 0, 0}; dirs[j] = {d, 0};
 *      an entry that is CRTS_NONE, or any entry >= W*H: positions[j] = normals[j] = dirs[j] = {0, 0, 0, 0}. No entry makes the kernel read
 *                outside the frame.
 *    positions, normals and dirs (which may be NULL) are float4[count]: positions as rows of stride 4 is a points argument of crt_trace_ao and
 *    an origins argument of crt_trace_rays. Every row is written; list and the frame are only read. One launch, one lane per item.
 *    CRTS_E_BAD_ARGUMENT  a NULL struct, geometry, positions or normals; an unknown guide layout; width or height < 1; count < 1; under
 *                         list == NULL a factor other than 1, 2, 4, an offset outside 0 .. factor-1 or not below the width (offsetX) or height
 *                         (offsetY), or a count other than LW*LH; an output equal to list, to geometry or to another output
 *    CRTS_E_OUT_OF_RANGE  width or height > 16384; count > CRTS_MAX_ITEMS
 *
 * 3. crts_scatter. For j < count with k = list[j] < n: out[k] = values[j] -- float (channels 1) or float4 (channels 4), as in crtu_upsample --
 *    and, where outState is given, outState[k] = stateWord (CRTS_STATE_RETRACED = 3 next to the upsample's 0, 1 and 2). An entry >= n is
 *    skipped, CRTS_NONE among them; nothing else of out and outState is touched. A list with duplicates is legal; which of their values ends up
 *    in out is unspecified (crts_compact writes none). One launch, one lane per entry.
 *    CRTS_E_BAD_ARGUMENT  a NULL struct, list, values or out; channels other than 1 or 4; count < 1 or n < 1; out or outState equal to list, to
 *                         values or to each other
 *    CRTS_E_OUT_OF_RANGE  count or n > CRTS_MAX_ITEMS */
#ifndef CRT_SELECT_H
#define CRT_SELECT_H

#include <stddef.h>
#include <stdint.h>
#include "crt_temporal.h"   /* CrttCamera */

#ifdef __cplusplus
extern "C" {
#endif

enum { CRTS_OK = 0, CRTS_E_BAD_ARGUMENT = -2, CRTS_E_OUT_OF_RANGE = -3 };   /* same values as CrtStatus */
enum { CRTS_GUIDES_PLANES = 0, CRTS_GUIDES_SURFACE = 1 };                   /* the two layouts of crt_denoise.h */
enum { CRTS_STATE_RETRACED = 3 };                                           /* behind CRTU_STATE_INTERPOLATED, NEAREST and EMPTY */
enum { CRTS_CHUNK = 2048 };             /* items per workgroup of crts_compact's counting and writing launches */
enum { CRTS_SCAN = 256 };               /* chunk sums per round of its scanning launch: above CRTS_CHUNK * CRTS_SCAN items it takes a second */
enum { CRTS_MAX_ITEMS = 1 << 28 };
#define CRTS_NONE 0xFFFFFFFFu           /* a list entry that names no item; -1 as int32 */

/* 24 bytes (LP64): words 0, wordBytes 8, values 12, n 16, capacity 20 */
typedef struct {
    const void* words;      /* uint8[n] (wordBytes 1) or uint32[n] (wordBytes 4); never written */
    int32_t wordBytes;      /* 1 or 4 */
    uint32_t values;        /* bit v set: a word of value v is selected (v < 32) */
    int32_t n;              /* 1 .. CRTS_MAX_ITEMS */
    int32_t capacity;       /* 1 .. CRTS_MAX_ITEMS: the entries of list */
} CrtsCompact;

/* 112 bytes (LP64): width 0, height 4, guides 8 (4 bytes of padding behind it), geometry 16, camera 24, 4 bytes of tail padding */
typedef struct {
    int32_t width, height;
    int32_t guides;         /* PLANES: geometry = float4[W*H] (CRT_GBUFFER_GEOMETRY). SURFACE: geometry = CrtSurfaceHit[W*H] (48 B) */
    const void* geometry;
    CrttCamera camera;      /* the camera the frame was shot with (crtt_camera) */
} CrtsFrame;

/* 24 bytes (LP64): list 0, count 8, factor 12, offsetX 16, offsetY 20 */
typedef struct {
    const void* list;       /* uint32[count], or NULL: the grid form */
    int32_t count;          /* 1 .. CRTS_MAX_ITEMS; LW*LH in the grid form */
    int32_t factor;         /* the grid form: 1, 2 or 4 */
    int32_t offsetX, offsetY;   /* the grid form: 0 .. factor-1 */
} CrtsItems;

/* 48 bytes (LP64): list 0, values 8, out 16, outState 24, count 32, channels 36, n 40, stateWord 44 */
typedef struct {
    const void* list;       /* uint32[count] */
    const void* values;     /* float[count] or float4[count] */
    void* out;              /* float[n] or float4[n] */
    void* outState;         /* uint32[n] or NULL */
    int32_t count;          /* 1 .. CRTS_MAX_ITEMS */
    int32_t channels;       /* 1 or 4 */
    int32_t n;              /* 1 .. CRTS_MAX_ITEMS: the items of out */
    uint32_t stateWord;
} CrtsScatter;

size_t crts_scratch_bytes(int32_t n);
int crts_compact(const CrtsCompact* c, void* list /* uint32[capacity] */, void* counts /* uint32[2] */, void* scratch, void* stream);
int crts_points(const CrtsFrame* f, const CrtsItems* items, void* positions /* float4[count] */, void* normals /* float4[count] */,
                void* dirs /* float4[count] or NULL */, void* stream);
int crts_scatter(const CrtsScatter* s, void* stream);
const char* crts_error_string(int rc);

#ifdef __cplusplus
}
#endif

#endif
