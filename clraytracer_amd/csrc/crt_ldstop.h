// crt_ldstop.h -- Trace with the HOT BVH TILES STAGED IN LDS (round 6; CRT_KERNEL=ldstop): north_star's "per-wavefront traversal stack and
// hot BVH tiles staged in LDS", on today's kernel. Opt-in, bit-identical to the default kernel, measured beside it.
//
// What is staged: the top levels of EVERY mesh's tree -- CRT_TOP_PAIRS = 252 sibling-pair records of 64 B (15.75 KiB), split evenly over the
// scene's meshes and filled breadth-first from each root (8 meshes: 31 records = 5 levels each; one mesh: 252 records = 7-8 levels) by
// crt_build_top_kernel whenever the BVH layout is rebuilt. Inside the table a child that is itself in the table is referenced as
// CRT_TOP_BIT | record; every other reference is the global one, so a traversal leaves the table exactly once per descent and never comes back
// (pops may return to it: pushed references keep their form). An instance record carries its root's table reference in r2.w.
// How it is used: a workgroup is FOUR waves (four 8x8 tiles next to each other in one XCD's tile row) that share one LDS copy of the table and
// keep 15 stack slots each in LDS (4 x 3.75 KiB + 15.75 KiB = 30.75 KiB: five workgroups = 20 waves per CU, against the default kernel's 32).
// Traversal::inner then has three fetch paths: every lane on the same record -> scalar load from the table's global copy (unchanged); every lane
// on SOME table record -> four ds_read_b128 per lane, no vector-memory instruction; anything else -> the four vector loads, table lanes reading
// the table's global copy. Per ray the sequence of visits, tests and stack contents is the default kernel's (a table record holds the same boxes
// and the same child order), so frames and work counters are bit-identical (tests/test_gpu_variants.py, test_gpu_fuzz.py).
// Loop served: kernel_main.cl:131-158.
#pragma once
#include "crt_kernels.h"

#ifndef CRT_TOP_PAIRS
#define CRT_TOP_PAIRS 252                    // (A/B builds override these three: profiles/r06_ldstop_ab.txt)
#endif
#ifndef CRT_TOP_WAVES
#define CRT_TOP_WAVES 4                      // waves (tiles) per workgroup
#endif
#define CRT_TOP_LDS_SLOTS 15                 // stack slots per wave in LDS; the other 17 of upstream's 32 in the overflow area (CRT_OVF_SLOTS_MAX)
static_assert(CRT_TOP_PAIRS <= 0xFFFF, "table references keep the record in 16 bits");

// One thread per mesh: breadth-first copy of the tree's top `perMesh` pair records into the mesh's range of the table, children that land in
// the table re-referenced. Runs once per BVH upload / device build (rebuild_bvh_layout); the trees are acyclic by then (crt_relayout_nodes).
__global__ void crt_build_top_kernel(const float4* __restrict__ pairs, const uint32_t* __restrict__ rootRefs, uint32_t numRoots, uint32_t perMesh,
                                     float4* __restrict__ topPairs, uint32_t* __restrict__ topRootRefs)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= CRT_MAX_MESHES) return;
    const uint32_t root = rootRefs[m];
    topRootRefs[m] = root;                                   // a leaf root, a mesh without a tree, no room: the global reference
    if (m >= numRoots || perMesh == 0 || (root & CRT_LEAF_BIT) || (m + 1) * perMesh > CRT_TOP_PAIRS) return;
    const uint32_t base = m * perMesh;
    uint32_t q[CRT_TOP_PAIRS];                               // global pair index of table record base + k (scratch: runs once per upload)
    uint32_t n = 1;
    q[0] = root;
    topRootRefs[m] = CRT_TOP_BIT | base;
    for (uint32_t h = 0; h < n; ++h) {
        const float4* p = pairs + (size_t)q[h] * 4;
        float4 lmin = p[0], lmax = p[1], rmin = p[2], rmax = p[3];
        uint32_t lref = __float_as_uint(lmin.w), rref = __float_as_uint(rmin.w);
        if (!(lref & CRT_LEAF_BIT) && n < perMesh) { q[n] = lref; lref = CRT_TOP_BIT | (base + n); ++n; }
        if (!(rref & CRT_LEAF_BIT) && n < perMesh) { q[n] = rref; rref = CRT_TOP_BIT | (base + n); ++n; }
        lmin.w = __uint_as_float(lref); rmin.w = __uint_as_float(rref);
        float4* o = topPairs + (size_t)(base + h) * 4;
        o[0] = lmin; o[1] = lmax; o[2] = rmin; o[3] = rmax;
    }
}

// The stack of one wave of a four-wave workgroup: CrtStackT's layout (slot s of lane l at lds[s * 64 + l]) with 15 slots in LDS, the
// overflow block per WAVE, indexed by the wave's virtual block number, and the workgroup's LDS copy of the tree tops.
typedef CrtStackT<0, CRT_TOP_LDS_SLOTS, true> CrtStackTop;

// RayGen + Trace, both bounces: trace_body as in crt_trace_kernel<COUNT> (plain instantiation: no shadow rays / refraction / instance tree /
// stamps / feedback lists), four tiles per workgroup. Workgroup g runs on XCD g % 8 and holds the tiles at positions (g / 8) * 4 + w of that XCD's plain list, so the
// tile-to-XCD mapping is the default kernel's (lane_pixel with the wave's virtual block number).
template <bool COUNT>
__global__ __launch_bounds__(CRT_BLOCK * CRT_TOP_WAVES) void crt_trace_ldstop_kernel(CrtDevScene S, CrtFrame F, float4* __restrict__ out, unsigned long long* __restrict__ counters)
{
    __shared__ crt_f32x4 s_top[CRT_TOP_PAIRS * 4];
    __shared__ uint32_t s_stack[CRT_TOP_WAVES * CRT_TOP_LDS_SLOTS * CRT_BLOCK];
    // stage the table: 1008 float4, four per thread (every wave of the workgroup takes part, also one whose tile lies outside the frame)
    {
        const crt_f32x4* __restrict__ src = reinterpret_cast<const crt_f32x4*>(S.topPairs);
        for (int k = (int)threadIdx.x; k < CRT_TOP_PAIRS * 4; k += CRT_BLOCK * CRT_TOP_WAVES) s_top[k] = src[k];
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);   // wave-uniform: the block number stays in SGPRs
    const int vb = (int)(((blockIdx.x >> 3) * CRT_TOP_WAVES + (uint32_t)wave) * 8u + (blockIdx.x & 7u));
    const CrtStackTop stack = { (crt_lds_u32_ptr)s_stack + wave * (CRT_TOP_LDS_SLOTS * CRT_BLOCK) + lane, S.stackOverflow, (crt_lds_f32x4_ptr)s_top, (uint32_t)vb };
    trace_body<COUNT, false, false, false, false, CRT_TRACE_PLAIN>(S, F, out, counters, stack, vb, lane);
}
