// crt_inclusive.hip -- crt_rays_inclusive_kernel and crt_ao_inclusive_kernel, the kernels of crt_trace_rays / crt_trace_ao / crt_frame_ao under
// the inclusive box test (declarations and description: crt_inclusive.h; bodies: crt_rays.h, crt_ao.h); fourth translation unit of libcrt_hip.so.
// Build: with the other units, same flags (Makefile).
#include <hip/hip_runtime.h>
#include "../../include/crt_api.h"
#define CRT_AO_DEVICE_TABLE crt_ao_inclusive_table_dev
#include "crt_inclusive.h"

template <bool ANYHIT, bool TLAS>
__global__ __launch_bounds__(CRT_BLOCK, CRT_WAVES_PER_SIMD) void crt_rays_inclusive_kernel(CrtDevScene S0, CrtRaysArgs A)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    crt_rays_body<ANYHIT, TLAS, true>(S0, A, (crt_lds_u32_ptr)s_stack);
}

template __global__ void crt_rays_inclusive_kernel<false, false>(CrtDevScene, CrtRaysArgs);
template __global__ void crt_rays_inclusive_kernel<false, true>(CrtDevScene, CrtRaysArgs);
template __global__ void crt_rays_inclusive_kernel<true, false>(CrtDevScene, CrtRaysArgs);
template __global__ void crt_rays_inclusive_kernel<true, true>(CrtDevScene, CrtRaysArgs);

template <int SOURCE, bool TLAS>
__global__ __launch_bounds__(CRT_BLOCK, CRT_WAVES_PER_SIMD) void crt_ao_inclusive_kernel(CrtDevScene S0, CrtAoArgs A, CrtFrame F)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    crt_ao_body<SOURCE, TLAS, true>(S0, A, F, (crt_lds_u32_ptr)s_stack);
}

template __global__ void crt_ao_inclusive_kernel<CRT_AO_POINTS, false>(CrtDevScene, CrtAoArgs, CrtFrame);
template __global__ void crt_ao_inclusive_kernel<CRT_AO_POINTS, true>(CrtDevScene, CrtAoArgs, CrtFrame);
template __global__ void crt_ao_inclusive_kernel<CRT_AO_FRAME, false>(CrtDevScene, CrtAoArgs, CrtFrame);
template __global__ void crt_ao_inclusive_kernel<CRT_AO_FRAME, true>(CrtDevScene, CrtAoArgs, CrtFrame);
