// crt_ao.hip -- crt_ao_kernel and crt_ao_filter_kernel, the kernels of crt_trace_ao / crt_frame_ao (declarations and description: crt_ao.h);
// third translation unit of libcrt_hip.so.
// Build: with crt_shim.hip and crt_rays.hip, same flags (Makefile).
#include <hip/hip_runtime.h>
#include "../../include/crt_api.h"
#include "crt_ao.h"

// the direction table in device memory: 256 rows of 16 bytes (tools/make_ao_table.py); 4 KiB, resident in the vector L1 after the first wave
struct alignas(16) CrtAoDir { float x, y, z, w; };
#define CRT_AO_TABLE_DECL __device__ const CrtAoDir crt_ao_table_dev[CRT_AO_TABLE_SIZE]
#include "crt_ao_table.h"

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

template <int SOURCE, bool TLAS>
__global__ __launch_bounds__(CRT_BLOCK, CRT_WAVES_PER_SIMD) void crt_ao_kernel(CrtDevScene S0, CrtAoArgs A, CrtFrame F)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
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
                    const crt_f32x4 t = *reinterpret_cast<const crt_f32x4*>(&crt_ao_table_dev[j]);      // one 16-byte vector load
                    v3 d = mk3((h & 0x100u) ? -t.x : t.x, (h & 0x200u) ? -t.y : t.y, (h & 0x400u) ? -t.z : t.z);
                    if (dot3(d, n2) < 0.0f) d = neg3(d);
                    const float w = dot3(d, n2);
                    const CrtStackT<TLAS ? CRT_TLAS_PARK : 0> stack = { (crt_lds_u32_ptr)s_stack + lane2, S0.stackOverflow };
                    const Closest c = closest_hit<false, false, true, TLAS>(S, o, d, stack, lc, best0, noCull);
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

template __global__ void crt_ao_kernel<CRT_AO_POINTS, false>(CrtDevScene, CrtAoArgs, CrtFrame);
template __global__ void crt_ao_kernel<CRT_AO_POINTS, true>(CrtDevScene, CrtAoArgs, CrtFrame);
template __global__ void crt_ao_kernel<CRT_AO_FRAME, false>(CrtDevScene, CrtAoArgs, CrtFrame);
template __global__ void crt_ao_kernel<CRT_AO_FRAME, true>(CrtDevScene, CrtAoArgs, CrtFrame);

// one workgroup per 8 x 8 tile of the whole frame, one lane per pixel
__global__ __launch_bounds__(CRT_BLOCK) void crt_ao_filter_kernel(const float* __restrict__ raw, const float4* __restrict__ geometry, float* __restrict__ out,
                                                                  int width, int height, float depthTol, float normalCos)
{
    const int tilesX = (width + CRT_TILE - 1) / CRT_TILE;
    const int ty = (int)blockIdx.x / tilesX, tx = (int)blockIdx.x - ty * tilesX;
    const int x = tx * CRT_TILE + (int)(threadIdx.x & 7u), y = ty * CRT_TILE + (int)(threadIdx.x >> 3);
    if (x >= width || y >= height) return;
    const size_t c = (size_t)y * (size_t)width + (size_t)x;
    const float4 gc = geometry[c];
    if (gc.w > 99998.0f) { out[c] = 1.0f; return; }               // a miss stays 1
    const v3 nc = mk3(gc.x, gc.y, gc.z);
    float sum = 0.0f, cnt = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= height) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= width) continue;
            const size_t q = (size_t)yy * (size_t)width + (size_t)xx;
            float m = 1.0f;
            if ((dx | dy) != 0) {
                const float4 gn = geometry[q];
                const bool hit = !(gn.w > 99998.0f);
                m = (hit && fabsf(gn.w - gc.w) <= depthTol * gc.w && dot3(mk3(gn.x, gn.y, gn.z), nc) >= normalCos) ? 1.0f : 0.0f;
            }
            sum += raw[q] * m; cnt += m;
        }
    }
    out[c] = sum / cnt;
}
