// crt_shade_host.h -- shaded ray queries on device buffers: crt_shade_rays and its statistics.
// Part of the one translation unit crt_shim.hip (included there behind crt_ao_host.h; launch_query and query_stats: crt_query_host.h);
// everything here has internal linkage. The kernel: crt_shade.h (declared, described), crt_shade.hip (compiled).
#pragma once
namespace {

typedef void CrtShadeKernel(CrtDevScene, CrtShadeArgs);
// [2 * (WHAT - 1) + TLAS]
static CrtShadeKernel* const kShadeKernels[6] = { crt_shade_kernel<CRT_SHADE_RADIANCE, false>, crt_shade_kernel<CRT_SHADE_RADIANCE, true>,
                                                  crt_shade_kernel<CRT_SHADE_SURFACE, false>, crt_shade_kernel<CRT_SHADE_SURFACE, true>,
                                                  crt_shade_kernel<CRT_SHADE_BOTH, false>, crt_shade_kernel<CRT_SHADE_BOTH, true> };

// Enqueue-and-return like crt1_trace_rays: every check comes before the first thing that is queued (launch_query).
int crt1_shade_rays(const CrtRayBatch* rays, const CrtShadeParams* params, uint32_t numInstances, float* radiance, CrtSurfaceHit* surface, hipStream_t stream)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!rays || !params) return CRT_E_BAD_ARGUMENT;
    if (!std::isfinite(params->sunAngle) || params->flags != 0) return CRT_E_BAD_ARGUMENT;
    if (rays->n == 0) return CRT_OK;
    if (!rays->origins || !rays->dirs || (!radiance && !surface)) return CRT_E_BAD_ARGUMENT;
    if (rays->originStride == 1 || rays->originStride == 2 || rays->dirStride == 1 || rays->dirStride == 2) return CRT_E_BAD_ARGUMENT;
    if (numInstances > CRT_MAX_INSTANCES || !g.sceneValid) return CRT_E_BAD_ARGUMENT;
    if (rays->n > CRT_RAYS_MAX) return CRT_E_OUT_OF_RANGE;
    CrtShadeArgs A;
    A.origins = rays->origins; A.dirs = rays->dirs; A.tmax = rays->tmax;
    A.radiance = reinterpret_cast<float4*>(radiance); A.surface = surface;
    A.originStride = rays->originStride; A.dirStride = rays->dirStride; A.n = (uint32_t)rays->n;
    A.lightY = (float)sin((double)params->sunAngle);      // as fill_frame
    A.lightZ = (float)cos((double)params->sunAngle);
    const int what = (radiance ? CRT_SHADE_RADIANCE : 0) | (surface ? CRT_SHADE_SURFACE : 0);
    return launch_query(g.rayQuery.shade, kShadeKernels, false, what - 1, numInstances, (rays->n + CRT_BLOCK - 1) / CRT_BLOCK, stream,
                        no_query_step, no_query_step, A);
}

int crt1_debug_shade_stats(uint64_t out[3]) { return query_stats(&QueryContext::shade, out); }

} // namespace
