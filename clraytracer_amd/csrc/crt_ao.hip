// crt_ao.hip -- crt_ao_kernel and crt_ao_filter_kernel, the kernels of crt_trace_ao / crt_frame_ao (declarations, description and body: crt_ao.h);
// third translation unit of libcrt_hip.so.
// Build: with crt_shim.hip and crt_rays.hip, same flags (Makefile).
#include <hip/hip_runtime.h>
#include "../../include/crt_api.h"
#define CRT_AO_DEVICE_TABLE crt_ao_table_dev
#include "crt_ao.h"

template <int SOURCE, bool TLAS>
__global__ __launch_bounds__(CRT_BLOCK, CRT_WAVES_PER_SIMD) void crt_ao_kernel(CrtDevScene S0, CrtAoArgs A, CrtFrame F)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    crt_ao_body<SOURCE, TLAS, false>(S0, A, F, (crt_lds_u32_ptr)s_stack);
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
