// crt_rays.h -- batched ray queries on device buffers (crt_trace_rays): the kernel's arguments and its declaration.
// The kernel is compiled in a translation unit of its own (crt_rays.hip, linked into the same libcrt_hip.so) and launched from crt_frame.h: the device
// code of crt_shim.hip -- every kernel that existed before -- is then the same with and without it, and tools/kernel_resources.py lists the two units
// separately. The traversal is shared text: closest_hit of crt_device.h.
#pragma once
#include "crt_device.h"

// ---- batched ray queries on device buffers (crt_trace_rays): closest hit or occlusion, with an optional distance bound -------
// The production twin of crt_query_kernel: no counters, the plain kernels' budget (64 VGPRs, 8 waves/SIMD), rays and results
// stay on the device. A PERSISTENT grid -- as many one-wave workgroups as are resident at once, whatever n is -- claims 64-ray
// chunks from a device counter (one atomicAdd by lane 0, shared through readfirstlane) until they are gone: explicit rays are
// ragged work, and a statically dealt tail would idle behind one long ray. The overflow area is owned per workgroup, so it is
// bounded by the grid too.
//   ANYHIT  CRT_RAYS_OCCLUDED: one byte per ray, closest_hit's any-hit form (as shadow rays); else one CrtRayHit per ray.
//   Bound   B = !(tmax >= 99999) ? tmax : 99999 (NaN stays NaN: every ray a miss) is the distance the loop starts with.
//   Cull    beyond_cull_range's predicate (double, NaN included) per ray; a wave with any such lane traces its chunk as a launch
//           without the cull would: all-never bounds table, no instance tree, the chunked candidate loop (closest_hit's
//           chunkedOnly). Decided per chunk, so a batch may mix near and far origins and the near waves keep the cull.
// ctl: [0] the next chunk (reset before every launch), [1] chunks traced without the cull (crt_debug_rays_stats).
struct CrtRaysArgs {
    const float* __restrict__ origins; const float* __restrict__ dirs; const float* __restrict__ tmax;   // tmax: or null
    void* __restrict__ out;
    uint32_t* __restrict__ ctl;
    double cullOriginLimit;                      // (double)State::cullOriginLimit: converted on the host, compared from scalar registers
    const float4* __restrict__ noCullBounds;     // State::noCullBounds
    uint32_t originStride, dirStride;            // in floats; 0: one value for every ray (a wave-uniform load)
    uint32_t n, chunks;                          // n <= 2^30
};
template <bool ANYHIT, bool TLAS> __global__ void crt_rays_kernel(CrtDevScene S0, CrtRaysArgs A);
