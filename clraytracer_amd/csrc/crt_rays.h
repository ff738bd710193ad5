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
