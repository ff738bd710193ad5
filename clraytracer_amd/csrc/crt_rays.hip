// crt_rays.hip -- crt_rays_kernel, the kernel of crt_trace_rays (declaration, description and body: crt_rays.h); second translation unit of libcrt_hip.so.
// Build: with crt_shim.hip, same flags (Makefile).
#include <hip/hip_runtime.h>
#include "../../include/crt_api.h"
#include "crt_rays.h"

template <bool ANYHIT, bool TLAS>
__global__ __launch_bounds__(CRT_BLOCK, CRT_WAVES_PER_SIMD) void crt_rays_kernel(CrtDevScene S0, CrtRaysArgs A)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    crt_rays_body<ANYHIT, TLAS, false>(S0, A, (crt_lds_u32_ptr)s_stack);
}

template __global__ void crt_rays_kernel<false, false>(CrtDevScene, CrtRaysArgs);
template __global__ void crt_rays_kernel<false, true>(CrtDevScene, CrtRaysArgs);
template __global__ void crt_rays_kernel<true, false>(CrtDevScene, CrtRaysArgs);
template __global__ void crt_rays_kernel<true, true>(CrtDevScene, CrtRaysArgs);
