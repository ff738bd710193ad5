// crt_query.h -- the queries on device buffers (crt_trace_rays, crt_trace_ao, crt_frame_ao, crt_shade_rays): the shape their kernels share, written once.
// Included by crt_rays.h, crt_ao.h and crt_shade.h; the host half is crt_query_host.h. The traversal is shared text too: closest_hit of crt_device.h.
#pragma once
#include "crt_device.h"

// ---- the shape of a query kernel ----------------------------------------------------------------------------------------------------
// No counters, the plain kernels' budget (64 VGPRs, 8 waves/SIMD), inputs and results stay on the device.
//   Grid    PERSISTENT: as many one-wave workgroups as are resident at once, whatever the number of items is, claim 64-item chunks
//           from a device counter (claim_chunk: one atomicAdd by lane 0, shared through readfirstlane) until they are gone -- explicit
//           rays are ragged work, and a statically dealt tail would idle behind one long ray. The overflow area is owned per
//           workgroup, so it is bounded by the grid too.
//   Regs    what derives from the lane number (stack addresses, the item's index) is recomputed where it is used -- opaque_lane per
//           chunk, and once more behind each traversal -- instead of being hoisted out of the chunk loop and kept in registers through
//           the traversal, which then spills.
//   Bound   query_bound: B = !(x >= 99999) ? x : 99999 (NaN stays NaN: every ray a miss) is the distance the loop starts with.
//   Cull    cull_decision: beyond_cull_range's predicate (double, NaN included) per lane on its ray origin; a wave with any such lane
//           traces its chunk as a launch without the cull would: all-never bounds table, no instance tree, the chunked candidate loop
//           (closest_hit's chunkedOnly). Decided per chunk, so a batch may mix near and far origins and the near waves keep the cull.
// ctl: [0] the next chunk, [1] chunks traced without the cull; both reset before every launch. Every family of queries has its own
// pair of words in the query context's ctl (QueryFamily::ctl0) and its own statistics.
struct CrtQueryArgs {
    uint32_t* __restrict__ ctl;
    double cullOriginLimit;                      // (double)State::cullOriginLimit: converted on the host, compared from scalar registers
    const float4* __restrict__ noCullBounds;     // State::noCullBounds
};

// element k of an array of 3-vectors: three dwords per lane at the given stride (in floats), or (stride 0) one scalar load for the wave
__device__ __forceinline__ v3 load_xyz(const float* __restrict__ p, uint32_t stride, uint32_t k)
{
    if (stride == 0) {
        typedef const float __attribute__((address_space(4)))* crt_const_f32_ptr;
        const crt_const_f32_ptr q = (crt_const_f32_ptr)p;
        return mk3(q[0], q[1], q[2]);
    }
    const float* e = p + (size_t)k * (size_t)stride;
    return mk3(e[0], e[1], e[2]);
}

// the wave's next chunk; true: none is left (the kernel's loop breaks on it -- handing out the negation inverts a compare / branch pair)
__device__ __forceinline__ bool claim_chunk(const CrtQueryArgs& Q, uint32_t chunks, uint32_t& chunk)
{
    chunk = 0;
    if ((threadIdx.x & 63) == 0) chunk = atomicAdd(&Q.ctl[0], 1u);
    chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk);
    return chunk >= chunks;
}

// the lane number, opaque to the compiler (Regs above)
__device__ __forceinline__ uint32_t opaque_lane()
{
    uint32_t lane = threadIdx.x & 63u;
    asm volatile("" : "+v"(lane));
    return lane;
}

// ... and once more behind a traversal, with the chunk (a scalar): what the item's index is recomputed from
__device__ __forceinline__ void chunk_lane_again(uint32_t& chunk, uint32_t& lane)
{
    lane = threadIdx.x & 63u;
    asm volatile("" : "+s"(chunk), "+v"(lane));
}

__device__ __forceinline__ float query_bound(float x) { return !(x >= 99999.0f) ? x : 99999.0f; }

// The chunk's cull decision on the lanes' ray origins `o` (the lanes that trace are the active ones): wave-uniform; when true, S -- the
// caller's copy of the launch's scene -- has become the scene of a launch without the cull and the chunk is counted in ctl[1]
__device__ __forceinline__ bool cull_decision(const CrtQueryArgs& Q, const v3& o, uint32_t lane, CrtDevScene& S)
{
    const bool beyond = !(sqrt((double)o.x * (double)o.x + (double)o.y * (double)o.y + (double)o.z * (double)o.z) <= Q.cullOriginLimit);
    const bool noCull = __ballot(beyond) != 0;
    if (noCull) {
        S.instBounds = Q.noCullBounds; S.tlas = nullptr; S.tlasNodes = 0; S.alwaysList = nullptr; S.numAlways = 0;
        if ((int)lane == __ffsll((long long)__ballot(1)) - 1) atomicAdd(&Q.ctl[1], 1u);      // one vector atomic per affected chunk
    }
    return noCull;
}
