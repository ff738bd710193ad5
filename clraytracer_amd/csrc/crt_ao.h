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

// ---- the device half: what a unit that COMPILES crt_ao_kernel's text needs (crt_ao.hip; crt_inclusive.hip for the box test of
// CRT_AO_INCLUSIVE). Such a unit defines CRT_AO_DEVICE_TABLE -- the name of its copy of the direction table: every unit's device code is
// linked on its own, the host-side handles are not -- in front of this header; crt_shim.hip, which only launches, does not. ----
#ifdef CRT_AO_DEVICE_TABLE
// the direction table in device memory: 256 rows of 16 bytes (tools/make_ao_table.py); 4 KiB, resident in the vector L1 after the first wave
struct alignas(16) CrtAoDir { float x, y, z, w; };
#define CRT_AO_TABLE_DECL __device__ const CrtAoDir CRT_AO_DEVICE_TABLE[CRT_AO_TABLE_SIZE]
#include "crt_ao_table.h"
#undef CRT_AO_TABLE_DECL

__device__ __forceinline__ uint32_t lowbias32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// FRAME: pixel of lane `lane` in chunk `chunk` -- tile chunk % tilesX of the chunk / tilesX'th tile row this rank owns (deal_tile's band
// arithmetic without the XCD interleave: chunks are claimed, not dealt), rows of 8 pixels inside the tile
__device__ __forceinline__ void ao_pixel(const CrtFrame& F, uint32_t chunk, uint32_t lane, int& px, int& py)
{
    const int k = (int)chunk / F.tilesX, tx = (int)chunk - k * F.tilesX;
    const int bandK = k / F.tileRowsPerBand;
    const int tileRow = (F.rank + bandK * F.nRanks) * F.tileRowsPerBand + (k - bandK * F.tileRowsPerBand);
    px = tx * CRT_TILE + (int)(lane & 7u);
    py = tileRow * CRT_TILE + (int)(lane >> 3);
}

// Where the lane's result goes: `k` = the item's index (a point's index, a pixel's y W + x), false: the lane has no item (past n, outside the frame)
template <int SOURCE>
__device__ __forceinline__ bool ao_index(const CrtAoArgs& A, const CrtFrame& F, uint32_t chunk, uint32_t lane, uint32_t& k)
{
    if constexpr (SOURCE == CRT_AO_POINTS) { k = chunk * CRT_BLOCK + lane; return k < A.n; }
    else {
        int px, py;
        ao_pixel(F, chunk, lane, px, py);
        k = (uint32_t)py * (uint32_t)F.width + (uint32_t)px;
        return px < F.width && py < F.height;
    }
}

// The lane's item: position, normal (FRAME: turned towards the viewer) and index; true when it traces -- it exists, is no miss and its normal
// is not exactly (0, 0, 0)
template <int SOURCE>
__device__ __forceinline__ bool ao_item(const CrtAoArgs& A, const CrtFrame& F, uint32_t chunk, uint32_t lane, uint32_t& k, v3& P, v3& n)
{
    P = mk3(0.0f, 0.0f, 0.0f); n = P;
    if (!ao_index<SOURCE>(A, F, chunk, lane, k)) return false;
    if constexpr (SOURCE == CRT_AO_POINTS) {
        P = load_xyz(A.positions, A.positionStride, k);
        n = load_xyz(A.normals, A.normalStride, k);
    } else {
        int px, py;
        ao_pixel(F, chunk, lane, px, py);
        const float4 gm = A.geometry[k];
        if (gm.w > 99998.0f) return false;                        // a miss (t = 99999), or a hit beyond upstream's InfMinusOne: its normal is 0 anyway
        const v3 dir = raygen_dir(F, px, py);
        P = add3(mk3(F.camPos[0], F.camPos[1], F.camPos[2]), scale3(dir, gm.w));
        n = mk3(gm.x, gm.y, gm.z);
        if (dot3(n, dir) > 0.0f) n = neg3(n);
    }
    return !(n.x == 0.0f && n.y == 0.0f && n.z == 0.0f);
}

// The kernel's text, written once: crt_ao_kernel (crt_ao.hip) and crt_ao_inclusive_kernel (crt_inclusive.hip) are one-line wrappers that
// own the LDS stack and pass it in. (Arguments by value, as the kernels take them: by reference the same text allocates registers differently.)
//   INCLUSIVE  closest_hit's TR_INCLUSIVE: intersect_aabb<true> for every box test; nothing else differs.
template <int SOURCE, bool TLAS, bool INCLUSIVE>
__device__ __forceinline__ void crt_ao_body(CrtDevScene S0, CrtAoArgs A, CrtFrame F, crt_lds_u32_ptr s_stack)
{
    LaneCounters lc = {};                        // COUNT = false: never read
    for (;;) {
        uint32_t chunk;
        if (claim_chunk(A.q, A.chunks, chunk)) break;
        const uint32_t lane = opaque_lane();
        float ao = 1.0f;
        {
            uint32_t k; v3 P, n;
            const bool traces = ao_item<SOURCE>(A, F, chunk, lane, k, P, n);
            if (__ballot(traces) != 0 && traces) {
                // the chunk's cull decision, on the origin every sample of the lane shares
                const v3 o0 = add3(P, scale3(n, A.bias));
                CrtDevScene S = S0;
                const bool noCull = cull_decision(A.q, o0, lane, S);
                const float best0 = query_bound(A.radius);
                float num = 0.0f, den = 0.0f;
                for (uint32_t s = 0; s < A.samples; ++s) {
                    // the item once more (an L1 hit), behind the traversal of the sample before
                    uint32_t chunk2 = chunk, lane2;
                    chunk_lane_again(chunk2, lane2);
                    uint32_t k2; v3 P2, n2;
                    (void)ao_item<SOURCE>(A, F, chunk2, lane2, k2, P2, n2);
                    const v3 o = add3(P2, scale3(n2, A.bias));
                    const uint32_t h = lowbias32(k2 ^ A.seedMul);
                    const uint32_t j = (h + s * A.step) & (CRT_AO_TABLE_SIZE - 1u);
                    const crt_f32x4 t = *reinterpret_cast<const crt_f32x4*>(&CRT_AO_DEVICE_TABLE[j]);      // one 16-byte vector load
                    v3 d = mk3((h & 0x100u) ? -t.x : t.x, (h & 0x200u) ? -t.y : t.y, (h & 0x400u) ? -t.z : t.z);
                    if (dot3(d, n2) < 0.0f) d = neg3(d);
                    const float w = dot3(d, n2);
                    const CrtStackT<TLAS ? CRT_TLAS_PARK : 0> stack = { s_stack + lane2, S0.stackOverflow };
                    constexpr unsigned kOcclusion = TR_ANYHIT | opt_if(TLAS, TR_TLAS) | opt_if(INCLUSIVE, TR_INCLUSIVE)
                                                  | opt_if(policy::ao_divides(SOURCE == CRT_AO_FRAME, TLAS), TR_DIVIDE)
                                                  | opt_if(policy::kDeviceQueryOffset32, TR_OFFSET32);
                    const Closest c = closest_hit<kOcclusion>(S, o, d, stack, lc, best0, noCull);
                    const float occ = c.anyHit ? 1.0f : 0.0f;
                    num += w * occ; den += w;
                }
                ao = den > 0.0f ? 1.0f - num / den : 1.0f;
            }
        }
        // the item's index once more, behind the traversals
        uint32_t chunk3 = chunk, lane3;
        chunk_lane_again(chunk3, lane3);
        uint32_t k3;
        if (ao_index<SOURCE>(A, F, chunk3, lane3, k3)) A.out[k3] = ao;
    }
}
#endif
