// crt_ao.h -- ambient occlusion on device points and on G-buffer frames (crt_trace_ao, crt_frame_ao): the kernels' arguments and declarations.
// The kernels are compiled in a translation unit of their own (crt_ao.hip, the third of libcrt_hip.so) and launched from crt_ao_host.h through
// crt_query_host.h: the device code of the other two units is the same with and without them. What crt_ao_kernel shares with the other
// queries on device buffers -- the persistent grid, the claim, the cull decision, ctl: crt_query.h. The definition of every value is in
// include/crt_api.h (crt_trace_ao).
#pragma once
#include "crt_query.h"

// ---- crt_ao_kernel<SOURCE, TLAS> ---------------------------------------------------------------------------------------------------
// One fused kernel: a lane owns one item (a point, or a pixel of a G-buffer frame), builds its sample rays in registers -- a direction is
// one 16-byte load from the 4 KiB table, flipped into the normal's hemisphere -- traces each with the any-hit traversal bounded by
// query_bound(radius), and reduces num / den itself. No ray is ever stored: the materialised route writes and reads 28 B per sample ray.
//   SOURCE  CRT_AO_POINTS: chunk c = items 64 c .. 64 c + 63 of the position / normal arrays.
//           CRT_AO_FRAME:  chunk c = one 8 x 8 pixel tile of the rows this rank owns (tile c % tilesX of owned tile row c / tilesX); the
//                          item is the pixel's first hit in the GEOMETRY plane: P = cameraPos + raygen_dir * t, n the plane's normal
//                          turned towards the viewer. A miss (t > 99998: instance -1 carries t = 99999) is no item.
//   Idle    a chunk without an item that traces (zero normals, misses: a tile of sky) stores its 1.0f's and claims the next.
//   Cull    once per chunk, on the ray origin o = P + n * bias every sample of a lane shares; only the lanes that trace take part.
//   Regs    num, den and the sample counter live across the traversals; the lane number is taken again behind each one, and the item
//           itself (P, n) is loaded again per sample (an L1 hit) instead of being carried.
// q.ctl: the query context's ctl[2], ctl[3] (crt_debug_ao_stats): crt_debug_rays_stats keeps reading its own.
#define CRT_AO_POINTS 0
#define CRT_AO_FRAME 1
#define CRT_AO_TABLE_SIZE 256
struct CrtAoArgs {
    const float* __restrict__ positions; const float* __restrict__ normals;   // POINTS
    const float4* __restrict__ geometry;         // FRAME: the slot's GEOMETRY plane {normal.xyz, t}
    float* __restrict__ out;                     // one float per item: n floats, or the W x H plane
    CrtQueryArgs q;
    uint32_t positionStride, normalStride;       // POINTS, in floats; 0: one value for every point (a wave-uniform load)
    uint32_t n, chunks;                          // n <= 2^30 (FRAME: unused / owned tiles)
    uint32_t samples, step;                      // N of {1, 2, 4, ..., 64} and 256 / N
    uint32_t seedMul;                            // seed * 0x9E3779B9u
    float radius, bias;
};
// F: the G-buffer frame's matrices, camera and geometry in plain row-interleaved order (FRAME only; POINTS ignores it)
template <int SOURCE, bool TLAS> __global__ void crt_ao_kernel(CrtDevScene S0, CrtAoArgs A, CrtFrame F);

// ---- crt_ao_filter_kernel (CRT_AO_FILTER) ----------------------------------------------------------------------------------------------
// 5 x 5 cross-bilateral mean of the raw AO plane, guided by the GEOMETRY plane (t and the normal as stored): one lane per pixel, whole
// frames only. Definition: include/crt_api.h.
__global__ void crt_ao_filter_kernel(const float* __restrict__ raw, const float4* __restrict__ geometry, float* __restrict__ out, int width, int height,
                                     float depthTol, float normalCos);
