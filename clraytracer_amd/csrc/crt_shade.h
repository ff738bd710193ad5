// crt_shade.h -- shaded ray queries on device buffers (crt_shade_rays): the kernel's arguments, its declaration and its text.
// The kernel is compiled in a translation unit of its own (crt_shade.hip, one of the Makefile's HIP_UNITS) and launched from crt_shade_host.h: the device
// code of the other units is the same with and without it. It is the chunk loop of crt_rays_body (crt_query.h: the persistent grid, the claim,
// the bound, the cull decision, ctl) around the bounce loop of trace_body (crt_kernels.h) -- the path starts from the batch's (o, d)
// instead of camera_path, everything behind the closest hit is shade_bounce (crt_device.h), the one text every frame shades with.
// The definition of every value: include/crt_api.h.
#pragma once
#include "crt_query.h"

// ---- crt_shade_kernel<WHAT, TLAS>: radiance and / or the first-hit surface record of explicit rays -------
// A lane owns one ray, chunk c = rays 64 c .. 64 c + 63.
//   WHAT    CRT_SHADE_RADIANCE: float4 per ray, both bounces, no sink. CRT_SHADE_SURFACE: one CrtSurfaceHit per ray, written by
//           shade_bounce's SINK at bounce 0; the path ends there and no colour is stored. CRT_SHADE_BOTH: both.
//   Bound   query_bound(tmax[k]), 99999 without a tmax array, for the given ray only; the bounce ray starts at 99999 as a frame's does.
//           Without a hit Closest::distance is the bound, not 99999, and shade_bounce's `c.distance > 99998` assumes the unbounded start:
//           a ray without a hit inside the bound (Closest::anyHit, a NaN bound included) continues as no_hit().
//   Cull    per chunk on the given origins; the scene of a chunk without the cull serves its bounce rays too (bounce origins lie within
//           bounceReach of the scene whatever the first origin was, but the tables of a launch without the cull are right for every origin).
//   Regs    nothing of the path but the ray waits in registers during a traversal. Its radiance so far and its energy -- (0, 0, 0; 1) at the
//           start, kernel_main.cl:179-185 -- wait in the ray's own element of `radiance` (the lane reads its own store; the element's last
//           store is (result, 1)); without that plane (SURFACE) the ray itself is read again behind its one traversal. The ray's index is
//           recomputed behind every traversal (chunk_lane_again), by the sink for itself. With that all six fit the plain kernels' budget.
// q.ctl: the query context's ctl[4], ctl[5] (crt_debug_shade_stats).
#define CRT_SHADE_RADIANCE 1
#define CRT_SHADE_SURFACE 2
#define CRT_SHADE_BOTH 3
struct CrtShadeArgs {
    const float* __restrict__ origins; const float* __restrict__ dirs; const float* __restrict__ tmax;   // tmax: or null
    float4* __restrict__ radiance;               // or null (CRT_SHADE_SURFACE)
    CrtSurfaceHit* __restrict__ surface;         // or null (CRT_SHADE_RADIANCE)
    CrtQueryArgs q;
    uint32_t originStride, dirStride;            // in floats; 0: one value for every ray (a wave-uniform load)
    uint32_t n, chunks;                          // n <= 2^30
    float lightY, lightZ;                        // (float)sin((double)sunAngle), (float)cos((double)sunAngle), computed on the host (as CrtFrame's)
};
template <int WHAT, bool TLAS> __global__ void crt_shade_kernel(CrtDevScene S0, CrtShadeArgs A);

// A constant row of a store, made where it is stored: as a loop invariant of the chunk loop the compiler builds the 128-bit tuple once
// in front of the loop and keeps it through every traversal -- in scratch (16 B per lane and row).
__device__ __forceinline__ float made_here(float x) { asm volatile("" : "+v"(x)); return x; }

// shade_bounce's SINK for a ray of a batch: record k = 64 chunk + lane, three 16-byte rows. Rows 0 and 1 and the albedo are what
// GBufferSink stores in the three planes; material, texU, texV: the surface overload of the sink call (crt_device.h, SinkTakesSurface).
// A miss is decided on Closest::anyHit (the bound); a hit that upstream shades as sky (t > InfMinusOne, kernel_main.cl:219) keeps its ids
// and t and has the rest of a miss.
struct SurfaceSink {
    CrtSurfaceHit* __restrict__ out; uint32_t chunk;
    __device__ __forceinline__ float4* record() const
    {
        uint32_t chunk2 = chunk, lane2;
        chunk_lane_again(chunk2, lane2);
        return reinterpret_cast<float4*>(out + (size_t)(chunk2 * CRT_BLOCK + lane2));
    }
    __device__ __forceinline__ void hit(const Closest& c, v3 normal, uint32_t albedo, uint32_t material, float texU, float texV) const
    {
        float4* r = record();
        r[0] = make_float4(normal.x, normal.y, normal.z, c.hit.t);
        r[1] = make_float4(__int_as_float(c.hitInstance), __uint_as_float(c.hit.tri), c.hit.u, c.hit.v);
        r[2] = make_float4(__uint_as_float(albedo), __uint_as_float(material), texU, texV);
    }
    __device__ __forceinline__ void miss(const Closest& c) const
    {
        float4* r = record();
        const float zero = made_here(0.0f);
        r[0] = make_float4(zero, zero, zero, c.distance);
        r[1] = c.anyHit ? make_float4(__int_as_float(c.hitInstance), __uint_as_float(c.hit.tri), c.hit.u, c.hit.v)
                        : make_float4(__int_as_float(-1), zero, zero, zero);
        r[2] = make_float4(zero, zero, zero, zero);
    }
};

// The kernel's text; the kernel (crt_shade.hip) owns the LDS stack and passes it in, as crt_rays_kernel does.
template <int WHAT, bool TLAS>
__device__ __forceinline__ void crt_shade_body(CrtDevScene S0, CrtShadeArgs A, crt_lds_u32_ptr s_stack)
{
    constexpr bool kRadiance = (WHAT & CRT_SHADE_RADIANCE) != 0, kSurface = (WHAT & CRT_SHADE_SURFACE) != 0;
    constexpr unsigned kRay = opt_if(TLAS, TR_TLAS) | opt_if(policy::kDeviceQueryDivides, TR_DIVIDE) | opt_if(policy::kShadeStagesCull, TR_STAGE)
                            | opt_if(policy::kDeviceQueryOffset32, TR_OFFSET32);
    constexpr unsigned kShade = opt_if(policy::kShadeSkyDouble, SB_SKY_DOUBLE) | opt_if(policy::kDeviceQueryOffset32, SB_OFFSET32);
    LaneCounters lc = {};                        // no TR_COUNT: never read
    for (;;) {
        uint32_t chunk;
        if (claim_chunk(A.q, A.chunks, chunk)) break;
        const uint32_t lane = opaque_lane();
        const CrtStackT<TLAS ? CRT_TLAS_PARK : 0> stack = { s_stack + lane, S0.stackOverflow };
        const uint32_t k = chunk * CRT_BLOCK + lane;
        if (k < A.n) {
            // the path of kernel_main.cl:179-185 with the batch's ray in the camera ray's place
            PathState ps;
            ps.o = load_xyz(A.origins, A.originStride, k);
            ps.d = load_xyz(A.dirs, A.dirStride, k);
            // ... whose radiance so far and energy (0, 0, 0; 1) wait in the ray's own element of `radiance` during a traversal, not in registers
            if constexpr (kRadiance) { const float zero = made_here(0.0f); A.radiance[k] = make_float4(zero, zero, zero, made_here(1.0f)); }
            float bound = 99999.0f;
            if (A.tmax) bound = query_bound(A.tmax[k]);
            CrtDevScene S = S0;
            const bool noCull = cull_decision(A.q, ps.o, lane, S);
            for (int bounce = 0;; ++bounce) {
                Closest c = closest_hit<kRay>(S, ps.o, ps.d, stack, lc, bound, noCull);
                bound = 99999.0f;                // the given ray's alone: the bounce ray is unbounded
                if (!c.anyHit) c = no_hit();
                // (the record's row of ids is put together behind the traversal: left to the compiler, <SURFACE, true> carries it through
                // the traversal as a 128-bit tuple that it updates in scratch)
                if constexpr (kSurface) asm volatile("" : "+v"(c.hitInstance), "+v"(c.hit.tri), "+v"(c.hit.u), "+v"(c.hit.v));
                uint32_t chunk2 = chunk, lane2;
                chunk_lane_again(chunk2, lane2);
                const size_t k2 = (size_t)(chunk2 * CRT_BLOCK + lane2);
                if constexpr (!kRadiance) {
                    // the one traversal of this form: the ray is read again behind it instead of staying in registers through it
                    ps.o = load_xyz(A.origins, A.originStride, (uint32_t)k2);
                    ps.d = load_xyz(A.dirs, A.dirStride, (uint32_t)k2);
                    ps.result = mk3(0.0f, 0.0f, 0.0f); ps.energy = 1.0f;      // (never stored)
                } else {
                    // kernel_main.cl:267 adds to it in the same order as if it had stayed in registers
                    const float4 partial = A.radiance[k2];
                    ps.result = mk3(partial.x, partial.y, partial.z); ps.energy = partial.w;
                }
                int cont;
                if constexpr (!kSurface) cont = shade_bounce<kShade>(S, c, ps, bounce, A.lightY, A.lightZ);
                else {
                    const SurfaceSink sink = { A.surface, chunk };
                    cont = shade_bounce<kShade>(S, c, ps, bounce, A.lightY, A.lightZ, nullptr, &sink);
                }
                if constexpr (!kRadiance) break;
                const bool last = !cont || bounce == 1;
                A.radiance[k2] = make_float4(ps.result.x, ps.result.y, ps.result.z, last ? 1.0f : ps.energy);
                if (last) break;
            }
        }
    }
}
