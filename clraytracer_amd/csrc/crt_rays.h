// crt_rays.h -- batched ray queries on device buffers (crt_trace_rays): the kernel's arguments and its declaration.
// The kernel is compiled in a translation unit of its own (crt_rays.hip, linked into the same libcrt_hip.so) and launched from crt_query_host.h: the
// device code of crt_shim.hip -- every kernel that existed before -- is then the same with and without it, and tools/kernel_resources.py lists the
// units separately. What it shares with the other queries on device buffers -- the persistent grid, the claim, the cull decision, ctl: crt_query.h.
#pragma once
#include "crt_query.h"

// ---- crt_rays_kernel<ANYHIT, TLAS>: closest hit or occlusion, with an optional distance bound -------
// The production twin of crt_query_kernel; a lane owns one ray, chunk c = rays 64 c .. 64 c + 63.
//   ANYHIT  CRT_RAYS_OCCLUDED: one byte per ray, closest_hit's any-hit form (as shadow rays); else one CrtRayHit per ray.
//   Bound   query_bound(tmax[k]), 99999 without a tmax array.
//   Cull    per chunk on the rays' origins.
// q.ctl: the query context's ctl[0], ctl[1] (crt_debug_rays_stats).
struct CrtRaysArgs {
    const float* __restrict__ origins; const float* __restrict__ dirs; const float* __restrict__ tmax;   // tmax: or null
    void* __restrict__ out;
    CrtQueryArgs q;
    uint32_t originStride, dirStride;            // in floats; 0: one value for every ray (a wave-uniform load)
    uint32_t n, chunks;                          // n <= 2^30
};
template <bool ANYHIT, bool TLAS> __global__ void crt_rays_kernel(CrtDevScene S0, CrtRaysArgs A);

// The kernel's text, written once: crt_rays_kernel (crt_rays.hip) and crt_rays_inclusive_kernel (crt_inclusive.hip, the box test of
// CRT_RAYS_INCLUSIVE) are one-line wrappers that own the LDS stack and pass it in. (Arguments by value, as the kernels take them: by reference the same
// text allocates registers differently.)
//   INCLUSIVE  closest_hit's TR_INCLUSIVE: intersect_aabb<true> for every box test; nothing else differs.
template <bool ANYHIT, bool TLAS, bool INCLUSIVE>
__device__ __forceinline__ void crt_rays_body(CrtDevScene S0, CrtRaysArgs A, crt_lds_u32_ptr s_stack)
{
    constexpr unsigned kRay = opt_if(ANYHIT, TR_ANYHIT) | opt_if(TLAS, TR_TLAS) | opt_if(INCLUSIVE, TR_INCLUSIVE) | opt_if(policy::kDeviceQueryDivides, TR_DIVIDE)
                            | opt_if(policy::kDeviceQueryOffset32, TR_OFFSET32);
    LaneCounters lc = {};                        // no TR_COUNT: never read
    for (;;) {
        uint32_t chunk;
        if (claim_chunk(A.q, A.chunks, chunk)) break;
        const uint32_t lane = opaque_lane();
        const CrtStackT<TLAS ? CRT_TLAS_PARK : 0> stack = { s_stack + lane, S0.stackOverflow };
        const uint32_t k = chunk * CRT_BLOCK + lane;
        if (k < A.n) {
            const v3 o = load_xyz(A.origins, A.originStride, k);
            const v3 d = load_xyz(A.dirs, A.dirStride, k);
            float best0 = 99999.0f;
            if (A.tmax) best0 = query_bound(A.tmax[k]);
            CrtDevScene S = S0;
            const bool noCull = cull_decision(A.q, o, lane, S);
            const Closest c = closest_hit<kRay>(S, o, d, stack, lc, best0, noCull);
            // the ray's index once more, behind the traversal (as lane_pixel_again does for the pixel)
            uint32_t chunk2 = chunk, lane2;
            chunk_lane_again(chunk2, lane2);
            const size_t k2 = (size_t)(chunk2 * CRT_BLOCK + lane2);
            if constexpr (ANYHIT) static_cast<uint8_t*>(A.out)[k2] = c.anyHit ? (uint8_t)1 : (uint8_t)0;
            else {
                CrtRayHit h;
                // (t: Closest::distance IS the hit's t -- Traversal::pop_next / finish store tr.t in both -- so hit.t need not stay alive)
                if (c.anyHit) { h.t = c.distance; h.u = c.hit.u; h.v = c.hit.v; h.triIndex = c.hit.tri; h.instance = c.hitInstance; }
                else { h.t = 99999.0f; h.u = 0.0f; h.v = 0.0f; h.triIndex = 0; h.instance = -1; }      // whatever the bound was
                static_cast<CrtRayHit*>(A.out)[k2] = h;
            }
        }
    }
}
