// crt_shade.hip -- crt_shade_kernel, the kernel of crt_shade_rays (declaration, description and body: crt_shade.h); sixth translation unit of libcrt_hip.so.
// Build: with crt_shim.hip, same flags (Makefile).
#include <hip/hip_runtime.h>
#include "../../include/crt_api.h"
#include "crt_shade.h"

template <int WHAT, bool TLAS>
__global__ __launch_bounds__(CRT_BLOCK, CRT_WAVES_PER_SIMD) void crt_shade_kernel(CrtDevScene S0, CrtShadeArgs A)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    crt_shade_body<WHAT, TLAS>(S0, A, (crt_lds_u32_ptr)s_stack);
}

template __global__ void crt_shade_kernel<CRT_SHADE_RADIANCE, false>(CrtDevScene, CrtShadeArgs);
template __global__ void crt_shade_kernel<CRT_SHADE_RADIANCE, true>(CrtDevScene, CrtShadeArgs);
template __global__ void crt_shade_kernel<CRT_SHADE_SURFACE, false>(CrtDevScene, CrtShadeArgs);
template __global__ void crt_shade_kernel<CRT_SHADE_SURFACE, true>(CrtDevScene, CrtShadeArgs);
template __global__ void crt_shade_kernel<CRT_SHADE_BOTH, false>(CrtDevScene, CrtShadeArgs);
template __global__ void crt_shade_kernel<CRT_SHADE_BOTH, true>(CrtDevScene, CrtShadeArgs);
