// crt_rays.hip -- crt_rays_kernel, the kernel of crt_trace_rays (declaration and description: crt_rays.h); second translation unit of libcrt_hip.so.
// Build: with crt_shim.hip, same flags (Makefile).
#include <hip/hip_runtime.h>
#include "../../include/crt_api.h"
#include "crt_rays.h"

// element k of a ray array: three dwords per lane at the given stride, or (stride 0) one scalar load for the wave
__device__ __forceinline__ v3 load_ray_xyz(const float* __restrict__ p, uint32_t stride, uint32_t k)
{
    if (stride == 0) {
        typedef const float __attribute__((address_space(4)))* crt_const_f32_ptr;
        const crt_const_f32_ptr q = (crt_const_f32_ptr)p;
        return mk3(q[0], q[1], q[2]);
    }
    const float* e = p + (size_t)k * (size_t)stride;
    return mk3(e[0], e[1], e[2]);
}
template <bool ANYHIT, bool TLAS>
__global__ __launch_bounds__(CRT_BLOCK, CRT_WAVES_PER_SIMD) void crt_rays_kernel(CrtDevScene S0, CrtRaysArgs A)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    LaneCounters lc = {};                        // COUNT = false: never read
    for (;;) {
        uint32_t chunk = 0;
        if ((threadIdx.x & 63) == 0) chunk = atomicAdd(&A.ctl[0], 1u);
        chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk);
        if (chunk >= A.chunks) break;
        // (opaque per chunk: what derives from the lane number -- stack addresses, the ray's index -- is recomputed where it is used
        // instead of being hoisted out of this loop and kept in registers through the traversal, which then spills)
        uint32_t lane = threadIdx.x & 63u;
        asm volatile("" : "+v"(lane));
        const CrtStackT<TLAS ? CRT_TLAS_PARK : 0> stack = { (crt_lds_u32_ptr)s_stack + lane, S0.stackOverflow };
        const uint32_t k = chunk * CRT_BLOCK + lane;
        if (k < A.n) {
            const v3 o = load_ray_xyz(A.origins, A.originStride, k);
            const v3 d = load_ray_xyz(A.dirs, A.dirStride, k);
            float best0 = 99999.0f;
            if (A.tmax) { const float tm = A.tmax[k]; best0 = !(tm >= 99999.0f) ? tm : 99999.0f; }
            const bool beyond = !(sqrt((double)o.x * (double)o.x + (double)o.y * (double)o.y + (double)o.z * (double)o.z) <= A.cullOriginLimit);
            const bool noCull = __ballot(beyond) != 0;          // wave-uniform
            CrtDevScene S = S0;
            if (noCull) {
                S.instBounds = A.noCullBounds; S.tlas = nullptr; S.tlasNodes = 0; S.alwaysList = nullptr; S.numAlways = 0;
                if ((int)lane == __ffsll((long long)__ballot(1)) - 1) atomicAdd(&A.ctl[1], 1u);      // one vector atomic per affected chunk
            }
            const Closest c = closest_hit<false, false, ANYHIT, TLAS>(S, o, d, stack, lc, best0, noCull);
            // the ray's index once more, behind the traversal (as lane_pixel_again does for the pixel)
            uint32_t chunk2 = chunk, lane2 = threadIdx.x & 63u;
            asm volatile("" : "+s"(chunk2), "+v"(lane2));
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
