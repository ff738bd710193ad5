// crt_rays.hip -- crt_rays_kernel, the kernel of crt_trace_rays (declaration and description: crt_rays.h); second translation unit of libcrt_hip.so.
// Build: with crt_shim.hip, same flags (Makefile).
#include <hip/hip_runtime.h>
#include "../../include/crt_api.h"
#include "crt_rays.h"

template <bool ANYHIT, bool TLAS>
__global__ __launch_bounds__(CRT_BLOCK, CRT_WAVES_PER_SIMD) void crt_rays_kernel(CrtDevScene S0, CrtRaysArgs A)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    LaneCounters lc = {};                        // COUNT = false: never read
    for (;;) {
        uint32_t chunk;
        if (claim_chunk(A.q, A.chunks, chunk)) break;
        const uint32_t lane = opaque_lane();
        const CrtStackT<TLAS ? CRT_TLAS_PARK : 0> stack = { (crt_lds_u32_ptr)s_stack + lane, S0.stackOverflow };
        const uint32_t k = chunk * CRT_BLOCK + lane;
        if (k < A.n) {
            const v3 o = load_xyz(A.origins, A.originStride, k);
            const v3 d = load_xyz(A.dirs, A.dirStride, k);
            float best0 = 99999.0f;
            if (A.tmax) best0 = query_bound(A.tmax[k]);
            CrtDevScene S = S0;
            const bool noCull = cull_decision(A.q, o, lane, S);
            const Closest c = closest_hit<false, false, ANYHIT, TLAS>(S, o, d, stack, lc, best0, noCull);
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

template __global__ void crt_rays_kernel<false, false>(CrtDevScene, CrtRaysArgs);
template __global__ void crt_rays_kernel<false, true>(CrtDevScene, CrtRaysArgs);
template __global__ void crt_rays_kernel<true, false>(CrtDevScene, CrtRaysArgs);
template __global__ void crt_rays_kernel<true, true>(CrtDevScene, CrtRaysArgs);
