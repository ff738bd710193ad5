// crt_device.h -- device-side data layout and the per-ray traversal/shading code (gfx950).
//
// Reference semantics restated for CDNA4 (citations relative to upstream CLRayTracer/...):
//   kernels/kernel_main.cl:84-160   IntersectTriangle / IntersectAABB / IntersectBVH
//   kernels/kernel_main.cl:164-275  Trace          kernels/kernel_main.cl:277-287  RayGen
//   kernels/MathAndSTL.cl:100-119, 243-266  MatMul / Mat3Mul / reflect / colour / sampling
// Arithmetic contract (must match oracle/crt_oracle.h "Pinned builtin semantics"): fp32, no FMA
// contraction (-ffp-contract=off), IEEE divide/sqrt, per-ray operation order exactly upstream's.
//
// HBM layout (built by the kernels of crt_relayout.h from the reference-layout uploads):
//   pairs   : one 64-byte, 64-byte-aligned record per sibling pair {L.min,L.ref | L.max,- |
//             R.min,R.ref | R.max,-}; pair index = leftFirst >> 1 (siblings are adjacent upstream,
//             BVH.cpp:203-204). One inner-node visit = one aligned 64-byte fetch per lane.
//   ref     : 32-bit child descriptor. Inner: pair index. Leaf: bit31 | count<<24 | firstTri
//             (count 1..127; 0 = look up CrtDevScene::bigLeaf[firstTri]). A popped/descended node
//             needs no re-fetch to learn whether it is a leaf (upstream re-reads the 32-byte node).
//   triHot  : 36 bytes per triangle {v0, v1-v0, v2-v0} (edges precomputed with the same fp32
//             subtraction upstream performs per test -> bit-identical), read only by leaf tests.
//   triCold : the 32-byte attribute tail of the reference Tri (uv halfs, material, normal halfs),
//             read once per shaded hit.
//   texels  : RGBA8 (one dword per texel) expanded from the packed RGB8 pool.
//   instBounds : per instance, a conservative world-space bounding sphere of the mesh's root box
//             (computed in double on the host at upload time). Upstream has no TLAS: every ray
//             transforms into every instance and tests the root's two child boxes
//             (kernel_main.cl:198-217). A ray that misses the enlarged sphere cannot pass either
//             slab test, so the instance is skipped with identical results -- and the counters
//             record the one pop / one inner visit upstream would have spent on it.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <type_traits>
#include <utility>
#include "../../include/crt_types.h"
#include "crt_vec3.h"

#define CRT_LEAF_BIT 0x80000000u
// CRT_KERNEL=ldstop only: an INNER reference with this bit names record (ref & 0xFFFF) of the tree-top table (crt_ldstop.h) instead of
// a pair index; such references exist only inside that table and in CrtDevInstance::r2.w, which no other kernel form reads
#define CRT_TOP_BIT 0x40000000u
#define CRT_BLOCK 64      // one wave64 per workgroup: a finished wave frees its LDS and wave slot at once
#ifndef CRT_WAVES_PER_SIMD
#define CRT_WAVES_PER_SIMD 8   // 32 waves per CU: 64 VGPRs (the trace kernel fits them without scratch) and 5 KiB of LDS each = the CU's 160 KiB
#endif
#define CRT_WAVES_PER_SIMD_COUNT 6   // instrumented instantiations (work counters, stamps, queries) carry 14 more registers: 80 VGPRs, no heavy spills
// Traversal stack: upstream's `int nodesToVisit[32]` (kernel_main.cl:126), slot indices wrapping modulo 32 where
// upstream's array would overflow. Slots 0..CRT_LDS_SLOTS-1 live in LDS -- slot s of lane l at lds[s * 64 + l], so a
// wave's ds_read/ds_write_b32 is conflict-free; 20 slots = 5 KiB per wave, which is what lets 32 waves share a CU's
// 160 KiB. Slots 20..31 (no scene here has passed depth 15; hand-built deep trees in tests/test_gpu_deep_stack.py do)
// live in a global overflow block owned by the WORKGROUP (blockIdx.x): no two waves of a launch share an entry, every
// frame slot / query has its own area, and an entry is always written (push) before it is read (pop) within one
// traversal, so the area needs no initialisation and costs nothing until a stack passes 20 entries.
// (Round 1 indexed the area by the hardware wave slot from HW_ID; that is only unique while no wave is context-saved
// and restored elsewhere. Round 1 also had two flavours, 32 LDS slots at 5 waves/SIMD and 25 at 6: the SLP vectoriser's
// packed-math splats cost 20+ VGPRs and spilled; with -fno-slp-vectorize one flavour at 8 waves/SIMD wins everywhere:
// 5.9 -> 6.6 (no SLP, 6 waves) -> 7.0 (7 waves) -> 7.6 Gray/s (8 waves) on multi-1M with frames in flight.)
// (Explicit LDS pointer type: through a generic pointer the compiler read the stack with flat_load.)
typedef uint32_t __attribute__((address_space(3))) * crt_lds_u32_ptr;
// loads through a constant-address-space pointer become scalar loads (s_load_*, scalar cache) when the address is wave-uniform
typedef float crt_f32x4 __attribute__((ext_vector_type(4)));
typedef const crt_f32x4 __attribute__((address_space(4)))* crt_const_f32x4_ptr;
typedef const crt_f32x4 __attribute__((address_space(3)))* crt_lds_f32x4_ptr;
#ifndef CRT_LDS_SLOTS
#define CRT_LDS_SLOTS 20
#endif
// PARK: the last PARK of the wave's LDS slots do not hold stack entries but per-lane values "parked" across the traversals
// (values that are live through them but not used in them, which would otherwise be spilled to scratch by the instantiations
// that carry more state: the instance tree's candidate list, the shadow ray's n.l). The stack then has CRT_LDS_SLOTS - PARK
// slots in LDS and the rest in the overflow block; the block is sized for the largest PARK.
#define CRT_MAX_PARK 5
#define CRT_OVF_SLOTS_MAX (CRT_STACK_DEPTH - (CRT_LDS_SLOTS - CRT_MAX_PARK))
#define CRT_OVF_WORDS_PER_BLOCK ((size_t)CRT_OVF_SLOTS_MAX * CRT_BLOCK)
// SLOTS / TOP: CRT_KERNEL=ldstop's four-wave workgroups (crt_ldstop.h) keep fewer slots per wave in LDS, own their overflow block per WAVE
// (`vblock`, the wave's virtual block number, instead of blockIdx.x) and carry the workgroup's LDS copy of the tree tops (`top`); every
// other kernel leaves those two members unset and unused.
template <int PARK, int SLOTS = CRT_LDS_SLOTS, bool TOP = false>
struct CrtStackT {
    static constexpr bool kTop = TOP;        // LDS-resident tree tops: Traversal::inner's third fetch path
    static constexpr int kLds = SLOTS - PARK;
    static_assert(PARK >= 0 && PARK <= CRT_MAX_PARK && kLds >= 1 && kLds <= CRT_STACK_DEPTH && CRT_STACK_DEPTH - kLds <= CRT_OVF_SLOTS_MAX, "LDS slots");
    crt_lds_u32_ptr lds;     // this lane's slot 0
    uint32_t* ovf;           // base of the launch's overflow area (wave-uniform)
    crt_lds_f32x4_ptr top;   // TOP: the workgroup's copy of the tree-top table
    uint32_t vblock;         // TOP: the wave's virtual block number (wave-uniform)
    __device__ __forceinline__ uint32_t* overflow_slot(int k) const
    {
        uint32_t lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));      // keep the address arithmetic inside this (rarely taken) branch: hoisted out of the
                                            // traversal loop it costs two VGPRs for the whole kernel
        return ovf + ((size_t)(TOP ? vblock : blockIdx.x) * CRT_OVF_SLOTS_MAX + (size_t)k) * CRT_BLOCK + lane;
    }
    // The overflow test is made for the WAVE first (one compare + one scalar branch): no scene here passes kLds entries in the
    // common case, and the per-lane form costs every push and pop an exec-mask save / restore pair (the CU's scalar unit is
    // ~66 % busy with such bookkeeping).
    __device__ __forceinline__ void write(int slot, uint32_t v) const
    {
        const int s = slot & (CRT_STACK_DEPTH - 1);
        if (kLds >= CRT_STACK_DEPTH || __ballot(s >= kLds) == 0) { lds[s * 64] = v; return; }
        if (kLds >= CRT_STACK_DEPTH || s < kLds) lds[s * 64] = v;
        else *overflow_slot(s - kLds) = v;
    }
    __device__ __forceinline__ uint32_t read(int slot) const
    {
        const int s = slot & (CRT_STACK_DEPTH - 1);
        if (kLds >= CRT_STACK_DEPTH || __ballot(s >= kLds) == 0) return lds[s * 64];
        if (kLds >= CRT_STACK_DEPTH || s < kLds) return lds[s * 64];
        return *overflow_slot(s - kLds);
    }
    __device__ __forceinline__ crt_lds_f32x4_ptr top_record(uint32_t k) const { return top + k * 4; }
    // parked value k (0 <= k < PARK) of this lane
    __device__ __forceinline__ void park(int k, uint32_t v) const { lds[(kLds + k) * 64] = v; }
    __device__ __forceinline__ uint32_t parked(int k) const { return lds[(kLds + k) * 64]; }
};
typedef CrtStackT<0> CrtStack;
#ifndef CRT_SPLIT_BETA
#define CRT_SPLIT_BETA 1.2f
#endif
#ifndef CRT_SPLIT_BETA_ASYNC
#define CRT_SPLIT_BETA_ASYNC 2.0f
#endif
#define CRT_MAX_SPLIT 96   // per XCD and frame: heaviest tiles traced as four 4x4-pixel waves instead of one 8x8 wave
#ifndef CRT_MAX_SPLIT_PIPELINED
#define CRT_MAX_SPLIT_PIPELINED 8   // with frames in flight the tail is hidden by the next frame: split only the very heaviest
#endif
#define CRT_TILE 8        // 8x8 pixels per wave, Morton order inside

// Node of the instance tree (TLAS): a world-space bounding sphere and two children; child bit 31 set = leaf, low bits =
// instance index. Built on the host whenever instances are uploaded (crt_instances.h, rebuild_instance_master).
struct CrtTlasNode { float4 sphere; uint32_t left, right, pad0, pad1; };
#define CRT_TLAS_LEAF 0x80000000u
#define CRT_TLAS_MIN_INSTANCES 64      // with fewer instances the linear sphere loop of candidate_mask is cheaper
#define CRT_TLAS_LIST 8                // candidates a lane can hold; a wave with a lane that needs more uses the chunked loop

struct CrtDevScene {
    const float4* __restrict__ pairs;
    const float* __restrict__ triHot;
    const uint4* __restrict__ triCold;
    const uint32_t* __restrict__ bigLeaf;
    const uint32_t* __restrict__ rootRefs;
    uint32_t* stackOverflow;             // this launch's overflow area: CRT_OVF_WORDS_PER_BLOCK words per workgroup, see CrtStack
    const CrtMeshInstance* __restrict__ instances;
    const struct CrtDevInstance* __restrict__ devInstances;
    const float4* __restrict__ instBounds;   // world-space bounding sphere per instance (xyz, r); r < 0: never cull
    const CrtMaterial* __restrict__ materials;
    const CrtTexture* __restrict__ textures;
    const uint32_t* __restrict__ texels;
    int numTexels;
    uint32_t numInstances;
    const CrtTlasNode* __restrict__ tlas;    // bounding-sphere tree over the cullable instances (host-built), or null
    uint32_t tlasNodes;                      // 0: no tree (few instances, or none cullable)
    const uint32_t* __restrict__ alwaysList; // instances that are never culled (single-leaf meshes, unbounded), ascending
    uint32_t numAlways;
    const float4* __restrict__ topPairs;     // CRT_KERNEL=ldstop: the top levels of every mesh's tree, CRT_TOP_PAIRS records (crt_ldstop.h); else unused
};

struct CrtFrame {
    float invView[16];
    float invProj[16];
    float camPos[3];
    float lightY, lightZ;     // (float)sin((double)sunAngle), (float)cos((double)sunAngle), computed on the host
    int width, height;
    int tilesX;               // ceil(width / 16)
    int ownedTileRows;        // 16-row tile rows this rank renders
    int gridBlocks;           // ceil(ownedTileRows / 8) * 8 * tilesX
    int tileRowsPerBand;      // bandRows / 8
    int rank, nRanks;
    int slotsPerXcd;          // ceil(ownedTileRows / 8) * tilesX: tiles in each XCD's list
    const uint32_t* order;    // per-XCD dispatch list, heaviest first: slot | quadrant << 28 | split << 31; see crt_order_kernel
    const uint32_t* listLen;  // entries in each XCD's list (tiles + 3 extra entries per split tile)
    int listCap;              // capacity of one XCD's list = slotsPerXcd + 3 * CRT_MAX_SPLIT
    uint32_t* cost;           // per tile: shader cycles the wave spent on it this frame (feeds the next frame's order)
    uint32_t epilogue;        // crt_trace_kernel: per-pixel stages applied before the pixel is stored (CRT_EPILOGUE_*); 0 = the plain HDR value
    int ss;                   // crt_trace_ssaa_kernel: k of k x k supersampling (CRT_RENDER_SSAA2/4), 1 otherwise. It sits in the padding before
                              // packOut, so the struct's size -- and with it the offsets of every kernel argument behind F -- is unchanged
    uint32_t* packOut;        // with CRT_EPILOGUE_QUANTIZE: also store the pixel's RGBA8 bytes here (the frame a read-back delivers); or null
};

// The first-hit planes of a CRT_RENDER_GBUFFER frame (crt_trace_gbuffer_kernel's own argument: CrtFrame keeps its size, see `ss`),
// W x H each, row-major like the frame, back to back in one allocation (layouts in include/crt_api.h):
//   geometry  float4 {normal.xyz, t}                          at planes
//   ids       uint4 {instance, triIndex, u bits, v bits}      at planes + 16 W H
//   albedo    uint32 0xFF000000 | b << 16 | g << 8 | r        at planes + 32 W H
// One pointer, not three: the Trace kernels keep their arguments alive through both traversals and already spill SGPRs into the
// lanes of a VGPR; every further argument is two more lanes.
struct CrtGBuffer {
    char* __restrict__ planes;
    __host__ __device__ char* geometry() const { return planes; }
    __host__ __device__ char* ids(size_t pixels) const { return planes + 16 * pixels; }
    __host__ __device__ char* albedo(size_t pixels) const { return planes + 32 * pixels; }
};

// v3, mk3, add3, sub3, mul3, scale3, neg3, dot3: crt_vec3.h (included above)
__device__ __forceinline__ v3 cross3(v3 a, v3 b)
{
    return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ v3 normalize3(v3 v)
{
    float inv = 1.0f / sqrtf(dot3(v, v));
    return scale3(v, inv);
}
__device__ __forceinline__ v3 reflect3(v3 v, v3 n)
{
    float d = dot3(n, v);
    return sub3(v, scale3(scale3(n, d), 2.0f));
}
// (int) pinned: truncation, NaN -> 0, saturating
__device__ __forceinline__ int f2i(float x)
{
    if (!(x == x)) return 0;
    if (x >= 2147483648.0f) return 2147483647;
    if (x <= -2147483648.0f) return (-2147483647 - 1);
    return (int)x;
}
__device__ __forceinline__ float h2f(uint32_t bits16) { return __half2float(__ushort_as_half((unsigned short)bits16)); }

struct CrtDevInstance;
struct Triout { float t, u, v; uint32_t tri; };

struct LaneCounters {
    uint32_t rays, primary, secondary, hits, misses;
    uint32_t traversals, pops, innerVisits, triTests, capHits, stackOverflows, maxStack;
    uint32_t shadowRays, shadowHits;      // CRT_RENDER_SHADOWS only
    uint32_t culled;                      // instance visits the sphere cull answered (counted in traversals/pops/innerVisits as upstream's one pop + one root visit)
};
// n instance visits answered by the sphere cull: each is the one pop + one root visit upstream spends on it
__device__ __forceinline__ void count_culled(LaneCounters& lc, uint32_t n) { lc.traversals += n; lc.pops += n; lc.innerVisits += n; lc.culled += n; }

// kernel_main.cl:108-117
// INCLUSIVE (the device queries' opt-in rule, crt_api.h: CRT_RAYS_INCLUSIVE; never a frame): the same tnear / tfar, but a box the ray
// starts in, or of zero thickness, is entered -- at entry = max(tnear, 0). A compile-time constant: the plain form is what it was.
template <bool INCLUSIVE = false>
__device__ __forceinline__ float intersect_aabb(v3 o, v3 inv, float4 bmin, float4 bmax, float minSoFar)
{
    float tminx = (bmin.x - o.x) * inv.x, tminy = (bmin.y - o.y) * inv.y, tminz = (bmin.z - o.z) * inv.z;
    float tmaxx = (bmax.x - o.x) * inv.x, tmaxy = (bmax.y - o.y) * inv.y, tmaxz = (bmax.z - o.z) * inv.z;
    float tnear = fmaxf(fmaxf(fminf(tminx, tmaxx), fminf(tminy, tmaxy)), fminf(tminz, tmaxz));
    float tfar  = fminf(fminf(fmaxf(tminx, tmaxx), fmaxf(tminy, tmaxy)), fmaxf(tminz, tmaxz));
    if constexpr (INCLUSIVE) {
        const float entry = fmaxf(tnear, 0.0f);
        return (tnear <= tfar && tfar >= 0.0f && entry < minSoFar) ? entry : 1e30f;
    } else return (tnear < tfar && tnear > 0.0f && tnear < minSoFar) ? tnear : 1e30f;
}

// ------------------------------------------------------------------------------------------------
// `1.0f / x` of the traversal (native_recip pinned to IEEE: Traversal::enter's three 1 / md, intersect_triangle's 1 / a) in four
// instructions instead of the division's eleven: v_rcp_f32, one Newton step, v_div_fixup_f32. Over all 2^32 inputs the short
// sequence returns the bits of `1.0f / x` for every x with a biased exponent of 1 ... 252 and for every zero, infinity and NaN
// (payloads included); it differs only for denormal x and for finite |x| >= 2^126, whose quotient is denormal
// (tools/ubench/recip_exhaustive.hip; crt_debug_recip_sweep re-checks both facts on the device the library runs on).
// The guard: v_frexp_exp_i32_f32 is 0 for zeros, infinities and NaNs, <= -126 for denormals, >= 127 for finite |x| >= 2^126, and
// -125 ... 126 for everything the short sequence gets right -- so "outside -125 ... 126" is exactly the set that needs the division.
// The decision is taken for the WAVE (one compare mask against zero, a uniform branch the wave falls through): if any lane active at
// this step needs the division, every lane of the step takes the division's result, otherwise the division is a block no lane enters.
// DIVIDE (the traversal's TR_DIVIDE): the division as written, no guard -- the kernels of policy's "who keeps the division" below, and
// everything under -DCRT_IEEE_RECIP (A/B builds).
// ------------------------------------------------------------------------------------------------
#ifdef CRT_IEEE_RECIP
#define CRT_RECIP_DIVIDES(DIVIDE) true
#else
#define CRT_RECIP_DIVIDES(DIVIDE) (DIVIDE)
#endif
__device__ __forceinline__ float recip_short(float x)
{
    float r = __builtin_amdgcn_rcpf(x);
    const float e = __builtin_fmaf(-x, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
    return __builtin_amdgcn_div_fixupf(r, x, 1.0f);
}
// per lane: x is outside what recip_short gets right (x = m 2^e, 0.5 <= |m| < 1: e outside -125 ... 126; 0, inf, NaN give e = 0)
__device__ __forceinline__ bool recip_needs_division(int e) { return (uint32_t)(e + 125) > 251u; }
__device__ __forceinline__ bool recip_needs_division(float x) { return recip_needs_division(__builtin_amdgcn_frexp_expf(x)); }

template <bool DIVIDE = false>
__device__ __forceinline__ float recip(float x)
{
    if constexpr (CRT_RECIP_DIVIDES(DIVIDE)) return 1.0f / x;
    else {
        float r = recip_short(x);
        if (__builtin_expect(__ballot(recip_needs_division(x)) != 0, 0)) r = 1.0f / x;
        return r;
    }
}
// the three of an instance entry under one decision: the largest and the smallest exponent stand for all three
template <bool DIVIDE = false, bool ONE_COMPARE = false>
__device__ __forceinline__ v3 recip3(v3 d)
{
    if constexpr (CRT_RECIP_DIVIDES(DIVIDE)) return mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    else {
        const int ex = __builtin_amdgcn_frexp_expf(d.x), ey = __builtin_amdgcn_frexp_expf(d.y), ez = __builtin_amdgcn_frexp_expf(d.z);
        const int hi = max(max(ex, ey), ez), lo = min(min(ex, ey), ez);
        v3 r = mk3(recip_short(d.x), recip_short(d.y), recip_short(d.z));
        // ONE_COMPARE (root_pretest_misses): the same predicate as one compare against zero -- exponents are small integers, nothing wraps --
        // where the two compares' constants, kept in SGPRs from the top of the kernel, are registers the caller does not have
        if constexpr (ONE_COMPARE) { if (__builtin_expect(__ballot(max(hi - 126, -125 - lo) > 0) != 0, 0)) r = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z); }
        else if (__builtin_expect(__ballot(hi > 126 || lo < -125) != 0, 0)) r = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        return r;
    }
}

// kernel_main.cl:84-106; hot = {v0, edge1, edge2}
template <bool DIVIDE = false>
__device__ __forceinline__ int intersect_triangle(v3 o, v3 d, v3 x, v3 edge1, v3 edge2, Triout& out, uint32_t i)
{
    const v3 h = cross3(d, edge2);
    const float a = dot3(edge1, h);
    const float f = recip<DIVIDE>(a);
    const v3 s = sub3(o, x);
    const float u = f * dot3(s, h);
    const v3 q = cross3(s, edge1);
    const float v = f * dot3(d, q);
    const float t = f * dot3(edge2, q);
    int passed = (((int)(t > 0.0f) ^ (int)(t < out.t)) + (int)(u < 0.0f) + (int)(u > 1.0f) + (int)(v < 0.0f) + (int)(u + v > 1.0f)) == 0;
    int notPassed = 1 - passed;
    // arithmetic blend kept as upstream (NaN/inf propagate through the 0-weighted term)
    out.u = u * (float)passed + ((float)notPassed * out.u);
    out.v = v * (float)passed + ((float)notPassed * out.v);
    out.t = t * (float)passed + ((float)notPassed * out.t);
    out.tri = i * (uint32_t)passed + ((uint32_t)notPassed * out.tri);
    return passed;
}

// MathAndSTL.cl:100-102 with a row-major matrix in memory: ((m.x*v.x + m.y*v.y) + m.z*v.z) + m.w*v.w
__device__ __forceinline__ v3 matmul_xyz(const float* __restrict__ m, float vx, float vy, float vz, float vw)
{
    v3 r;
    r.x = ((m[0] * vx + m[4] * vy) + m[8] * vz) + m[12] * vw;
    r.y = ((m[1] * vx + m[5] * vy) + m[9] * vz) + m[13] * vw;
    r.z = ((m[2] * vx + m[6] * vy) + m[10] * vz) + m[14] * vw;
    return r;
}
__device__ __forceinline__ float matmul_w(const float* __restrict__ m, float vx, float vy, float vz, float vw)
{
    return ((m[3] * vx + m[7] * vy) + m[11] * vz) + m[15] * vw;
}
__device__ __forceinline__ v3 mat3mul(const float* __restrict__ m, v3 v)
{
    v3 r;
    r.x = (m[0] * v.x + m[4] * v.y) + m[8] * v.z;
    r.y = (m[1] * v.x + m[5] * v.y) + m[9] * v.z;
    r.z = (m[2] * v.x + m[6] * v.y) + m[10] * v.z;
    return r;
}

struct Closest { float distance; int hitInstance; int anyHit; Triout hit; };
// "no hit yet" (kernel_main.cl:189-190): what a ray without a candidate instance ends with, and shade_bounce's skybox case
__device__ __forceinline__ Closest no_hit(float distance = 99999.0f)
{
    Closest c;
    c.distance = distance; c.hitInstance = 0; c.anyHit = 0;
    c.hit.t = 0.0f; c.hit.u = 0.0f; c.hit.v = 0.0f; c.hit.tri = 0;
    return c;
}


// diagnostic (TR_ITERS instantiations only): true in exactly one active lane, so summing over lanes counts wave-level loop trips
__device__ __forceinline__ bool first_active_lane() { return (int)__lane_id() == __ffsll((long long)__ballot(1)) - 1; }

// Device-side instance record (64 B, built at upload): the 3 used columns of inverseTransform
// (MatMul(...).xyz and Mat3Mul never read column 3) with the root ref and materialStart in the
// spare lanes. One aligned 64-byte gather per lane when a lane enters an instance.
struct CrtDevInstance { float4 r0, r1, r2, r3; };   // rK = {m[K][0], m[K][1], m[K][2], extra}; r0.w = rootRef, r1.w = materialStart

__device__ __forceinline__ v3 xform_xyz(const CrtDevInstance& m, float vx, float vy, float vz, float vw)
{
    v3 r;   // MathAndSTL.cl:100-102: ((m.x*v.x + m.y*v.y) + m.z*v.z) + m.w*v.w
    r.x = ((m.r0.x * vx + m.r1.x * vy) + m.r2.x * vz) + m.r3.x * vw;
    r.y = ((m.r0.y * vx + m.r1.y * vy) + m.r2.y * vz) + m.r3.y * vw;
    r.z = ((m.r0.z * vx + m.r1.z * vy) + m.r2.z * vz) + m.r3.z * vw;
    return r;
}

__device__ __forceinline__ v3 mat3mul(const CrtDevInstance& m, v3 v)
{
    v3 r;   // MathAndSTL.cl:104-106 on ConvertToMatrix3(inverseTransform)
    r.x = (m.r0.x * v.x + m.r1.x * v.y) + m.r2.x * v.z;
    r.y = (m.r0.y * v.x + m.r1.y * v.y) + m.r2.y * v.z;
    r.z = (m.r0.z * v.x + m.r1.z * v.y) + m.r2.z * v.z;
    return r;
}

// ------------------------------------------------------------------------------------------------
// Record addresses of the per-lane fetches (TR_OFFSET32, policy's "who takes 32-bit record offsets"). A lane's record address is
// base + index * size with a wave-uniform base. Written with a 64-bit index it is built in a VGPR pair -- two moves from a VGPR that holds 0,
// a 64-bit shift, a 64-bit add -- and the loads go through that pair; written as base plus a 32-bit BYTE offset the base stays in its SGPR pair
// and one VGPR of offset is all the vector unit computes (global_load ... v, s[n:n+1]). Same loads, same bytes; fewer VALU instructions.
// Why 32 bits hold it: a reference that reaches a kernel is inside its pool. The pools have the fixed capacities below, whatever the scene
// (crt_upload.h: alloc_pools allocates with these constants); crt_relayout.h's make_ref admits a leaf only with firstTri + count <= the
// triangle pool's slots and an inner node only with both children below the node count, which an upload keeps below the node pool's slots
// (SPANCHK), and anything else sets the error word: the scene is invalid and no frame or query is launched on it (g.sceneValid). The empty
// reference names slot CRT_TRI_POOL_SLOTS itself with a count of zero: bigLeaf has that one entry more, and the triangle address is formed
// and never loaded from. An instance index is below numInstances <= CRT_MAX_INSTANCES. Each static_assert says that the largest offset its
// helper can form is below 2^32; tests/test_offset32_cpu.py says the same in a sentence when a capacity changes.
// OFFSET32 false: the 64-bit expressions as they were. -DCRT_NO_OFFSET32 (A/B builds): those everywhere.
// ------------------------------------------------------------------------------------------------
#define CRT_TRI_POOL_SLOTS ((size_t)CRT_MAX_TRIANGLES * 2)      // ResourceManager.cpp:158
#define CRT_NODE_POOL_SLOTS ((size_t)CRT_MAX_TRIANGLES * 2)     // ResourceManager.cpp:159 (MAX_BVHMEMORY * 2)
#define CRT_PAIR_POOL_RECORDS (CRT_NODE_POOL_SLOTS / 2 + 1)     // siblings are adjacent: pair index = leftFirst >> 1
#define CRT_PAIR_BYTES 64u
#define CRT_TRI_HOT_BYTES 36u
#define CRT_TRI_COLD_BYTES 32u
#ifdef CRT_NO_OFFSET32
#define CRT_OFFSETS32(OFFSET32) false
#else
#define CRT_OFFSETS32(OFFSET32) (OFFSET32)
#endif
// the pair record of inner reference `ref`
static_assert(CRT_PAIR_POOL_RECORDS * CRT_PAIR_BYTES < (1ull << 32) && CRT_PAIR_BYTES == 4 * sizeof(float4), "pair pool: 32-bit byte offsets");
template <bool OFFSET32>
__device__ __forceinline__ const float4* pair_record(const CrtDevScene& S, uint32_t ref)
{
    if constexpr (CRT_OFFSETS32(OFFSET32)) return reinterpret_cast<const float4*>(reinterpret_cast<const char*>(S.pairs) + ref * CRT_PAIR_BYTES);
    else return S.pairs + (size_t)ref * 4;
}
// the hot record of triangle `i` (i <= CRT_TRI_POOL_SLOTS: the empty reference's address is formed)
static_assert((CRT_TRI_POOL_SLOTS + 1) * CRT_TRI_HOT_BYTES < (1ull << 32) && CRT_TRI_HOT_BYTES == 9 * sizeof(float), "hot triangle pool: 32-bit byte offsets");
template <bool OFFSET32>
__device__ __forceinline__ const float* tri_hot_record(const CrtDevScene& S, uint32_t i)
{
    if constexpr (CRT_OFFSETS32(OFFSET32)) return reinterpret_cast<const float*>(reinterpret_cast<const char*>(S.triHot) + i * CRT_TRI_HOT_BYTES);
    else return S.triHot + (size_t)i * 9;
}
// the cold record of triangle `i` (a hit's triangle: i < CRT_TRI_POOL_SLOTS)
static_assert(CRT_TRI_POOL_SLOTS * CRT_TRI_COLD_BYTES < (1ull << 32) && CRT_TRI_COLD_BYTES == 2 * sizeof(uint4), "cold triangle pool: 32-bit byte offsets");
template <bool OFFSET32>
__device__ __forceinline__ const uint4* tri_cold_record(const CrtDevScene& S, uint32_t i)
{
    if constexpr (CRT_OFFSETS32(OFFSET32)) return reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(S.triCold) + i * CRT_TRI_COLD_BYTES);
    else return S.triCold + (size_t)i * 2;
}
// the triangle count of a leaf of 128 or more triangles (first <= CRT_TRI_POOL_SLOTS)
static_assert((CRT_TRI_POOL_SLOTS + 1) * sizeof(uint32_t) < (1ull << 32), "bigLeaf: 32-bit byte offsets");
template <bool OFFSET32>
__device__ __forceinline__ uint32_t big_leaf_count(const CrtDevScene& S, uint32_t first)
{
    if constexpr (CRT_OFFSETS32(OFFSET32)) return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(S.bigLeaf) + first * (uint32_t)sizeof(uint32_t));
    else return S.bigLeaf[first];
}
// the device record of instance `inst`
static_assert((size_t)CRT_MAX_INSTANCES * sizeof(CrtDevInstance) < (1ull << 32) && sizeof(CrtDevInstance) == 64, "instance table: 32-bit byte offsets");
template <bool OFFSET32>
__device__ __forceinline__ const CrtDevInstance* instance_record(const CrtDevInstance* __restrict__ table, uint32_t inst)
{
    if constexpr (CRT_OFFSETS32(OFFSET32)) return reinterpret_cast<const CrtDevInstance*>(reinterpret_cast<const char*>(table) + inst * (uint32_t)sizeof(CrtDevInstance));
    else return table + inst;
}

// The device record of instance `inst` (per lane). It comes through a SCALAR load (one s_load_dwordx16 through the scalar
// cache) when every lane that asks in this step asks for the same instance -- the common case for a coherent packet, whose
// lanes share their first candidates and mostly hit the same instance -- and through four per-lane vector loads otherwise:
// vector-memory instructions are what bounds the kernel, and unlike the node fetches (where the same test
// cost more than it saved, round 2) instance records are fetched rarely enough for one readfirstlane + compare + ballot
// per step to pay. (The table is written by crt_refresh_instances_kernel in an earlier launch, never by the reading kernel.)
// OFFSET32: the divergent path's record address (instance_record above); the uniform path addresses through SGPRs already.
template <bool OFFSET32 = false>
__device__ __forceinline__ CrtDevInstance load_instance(const CrtDevInstance* __restrict__ table, uint32_t inst)
{
    CrtDevInstance I;
    const uint32_t inst0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)inst);
    if (__ballot(inst != inst0) == 0) {
        const crt_const_f32x4_ptr p = (crt_const_f32x4_ptr)(table + inst0);
        const crt_f32x4 a = p[0], b = p[1], c = p[2], e = p[3];
        I.r0 = make_float4(a.x, a.y, a.z, a.w); I.r1 = make_float4(b.x, b.y, b.z, b.w);
        I.r2 = make_float4(c.x, c.y, c.z, c.w); I.r3 = make_float4(e.x, e.y, e.z, e.w);
    } else {
        const CrtDevInstance* ip = instance_record<OFFSET32>(table, inst);
        I.r0 = ip->r0; I.r1 = ip->r1; I.r2 = ip->r2; I.r3 = ip->r3;
    }
    return I;
}

// ------------------------------------------------------------------------------------------------
// Compile-time options of the traversal, the instance cull and the shading: one `unsigned` of named bits per function, spelled at the
// call site -- closest_hit<TR_ANYHIT | opt_if(TLAS, TR_TLAS)>(...). An option that is not named is off, and none follows from another.
// ------------------------------------------------------------------------------------------------
enum : unsigned {               // closest_hit, trip_steps, Traversal
    TR_COUNT = 1u << 0,         // per-ray work counters (LaneCounters)
    TR_ITERS = 1u << 1,         // stamped diagnostic launches: the counters record wave-level trips instead of per-ray work
    TR_ANYHIT = 1u << 2,        // shadow rays, occlusion: stop at the first triangle that passes
    TR_TLAS = 1u << 3,          // candidates from the instance tree
    TR_INCLUSIVE = 1u << 4,     // intersect_aabb's inclusive rule for every box test (the device queries only)
    TR_STAGE = 1u << 5,         // the camera bounce's cull terms once per wave (staged_candidate_mask)
    TR_DIVIDE = 1u << 6,        // the reciprocals as divisions (recip)
    TR_WAVE_CULL = 1u << 7,     // ... and one test per instance and wave against the tile's ray cone before the per-lane loop (cone_rejects)
    TR_ROOT_PRETEST = 1u << 8,  // ... and the exact root step per surviving instance and wave behind it (root_pretest_misses)
    TR_BOUNCE_PRETEST = 1u << 9,    // ... and the same step per instance and wave for the reflection bounce's candidates (bounce_pretest_mask)
    TR_PRETEST_ENTRY = 1u << 10,    // ... and the camera bounce's pre-test leaves a lane inside its first surviving instance (root_pretest_enters)
    TR_OFFSET32 = 1u << 11,         // the per-lane record fetches address as a scalar base plus a 32-bit byte offset (pair_record ... instance_record)
    TR_ALL = (1u << 12) - 1u
};
enum : unsigned { CM_COUNT = 1u << 0, CM_DEFER_COUNT = 1u << 1, CM_ALL = (1u << 2) - 1u };                        // candidate_mask
enum : unsigned { SB_DEFER_ENERGY = 1u << 0, SB_REFRACT = 1u << 1, SB_SKY_DOUBLE = 1u << 2, SB_OFFSET32 = 1u << 3, SB_ALL = (1u << 4) - 1u };   // shade_bounce
constexpr unsigned opt_if(bool on, unsigned bit) { return on ? bit : 0u; }
constexpr bool has_opt(unsigned opts, unsigned bit) { return (opts & bit) != 0u; }

// ------------------------------------------------------------------------------------------------
// Which kernel keeps the division (TR_DIVIDE), which the double-only skybox index (SB_SKY_DOUBLE), which stages the camera bounce's cull
// terms (TR_STAGE): decided here and nowhere else, by kernel family, and passed by name at the call sites. DESIGN.md 4a ("Who keeps the
// division", "Who keeps the double-only form", the staged cull) lists the same items in the same order. Every choice is pinned by a row
// of the kernel-resource ledger (tests/golden/kernel_resources.json): 64 VGPRs, no scratch, 8 waves/SIMD for the plain kernels.
// A counted launch (diagnostics, never the frame a user waits for) keeps the division and the double-only form in every family: it runs
// the same instructions whatever the uncounted ones do, and is the independent path the frame tests compare with.
// ------------------------------------------------------------------------------------------------
namespace policy {
// ---- who keeps the division ----
// trace_body (crt_trace_kernel, its SSAA, G-buffer and ldstop forms): the counted launches, and the one G-buffer kernel that sits at its 64 VGPRs
// so tightly that the short form's branch costs it 8 spilled registers (shadow rays + instance tree without refraction)
constexpr bool trace_divides(bool COUNT, bool GBUFFER, bool SHADOW, bool TLAS, bool REFRACT) { return COUNT || (GBUFFER && SHADOW && TLAS && !REFRACT); }
// crt_ao_body (crt_ao_kernel and its inclusive twin): the G-buffer source without an instance tree -- with the short form's branch in the
// triangle loop it spills one register
constexpr bool ao_divides(bool FRAME, bool TLAS) { return FRAME && !TLAS; }
// the wavefront form: crt_primary_kernel when counted; crt_bounce_kernel always -- this opt-in form's kernel is recorded register for
// register, and stays that
constexpr bool primary_divides(bool COUNT) { return COUNT; }
constexpr bool kBounceDivides = true;
// crt_trace_refill_kernel, crt_trace_block_kernel: when counted
constexpr bool refill_block_divides(bool COUNT) { return COUNT; }
// crt_query_kernel (hit-record parity on the host's rays): a counted kernel
constexpr bool kQueryDivides = true;
// the queries on device buffers (crt_rays_kernel and its inclusive twin, crt_shade_kernel): the short form at the plain budget
constexpr bool kDeviceQueryDivides = false;

// ---- who keeps the double-only skybox index ----
// trace_body: the counted launches, and every uncounted instantiation whose row of the ledger the second out-of-line function would move --
// the G-buffer kernels with shadow rays and an instance tree or refraction (<shadow, tree, no refraction> spills 8 registers to 32 B of
// scratch, the other two move an SGPR or an SGPR spill) and the shadow-ray kernels without tree and refraction, plain and supersampled
// (SGPR spills)
constexpr bool trace_sky_double(bool COUNT, bool GBUFFER, bool SHADOW, bool TLAS, bool REFRACT)
{
    return COUNT || (GBUFFER && SHADOW && (TLAS || REFRACT)) || (!GBUFFER && SHADOW && !TLAS && !REFRACT);
}
// the wavefront form (crt_primary_kernel, crt_bounce_kernel) and crt_trace_refill_kernel: when counted
constexpr bool wavefront_sky_double(bool COUNT) { return COUNT; }
constexpr bool refill_sky_double(bool COUNT) { return COUNT; }
// crt_trace_block_kernel: always -- the guarded form moves the uncounted kernel's SGPR spills (61 -> 63)
constexpr bool kBlockSkyDouble = true;
// crt_shade_kernel: the guarded form
constexpr bool kShadeSkyDouble = false;

// ---- who stages the camera bounce's cull terms ----
// trace_body alone: uncounted, unstamped, without an instance tree, on a one-wave workgroup's stack (not ldstop's) -- at the camera bounce
// every ray of the wave starts at F.camPos, so the cull's origin-only terms are computed once per wave (closest_hit's sharedOrigin says
// which bounce that is). Every other kernel compiles to what it compiled to before the staged form existed.
constexpr bool trace_stages_cull(bool COUNT, bool STAMP, bool TLAS, bool TOP) { return !COUNT && !STAMP && !TLAS && !TOP; }
// crt_shade_kernel: the origins of a batch are not shared
constexpr bool kShadeStagesCull = false;

// ---- who rejects instances per wave against the tile's ray cone (cone_rejects, before the staged per-lane loop) ----
// trace_body: the kernels of trace_stages_cull, except the two whose row of the ledger the wave test would move -- the G-buffer kernel with shadow
// rays and refraction (one more SGPR: 77 -> 78) and the plain kernel with shadow rays and without refraction (SGPR spills 53 -> 47). They keep
// the staged loop over all instances.
constexpr bool trace_wave_culls(bool STAGES, bool PLAIN, bool GBUFFER, bool SHADOW, bool REFRACT)
{
    return STAGES && !(GBUFFER && SHADOW && REFRACT) && !(PLAIN && SHADOW && !REFRACT);
}

// ---- who takes the exact root step per wave for the camera bounce's surviving instances (root_pretest_misses, behind the staged per-lane loop) ----
// trace_body: the kernels of trace_wave_culls (the pre-test runs over the wave test's survivors, in the waves that take the wave test), except the four
// whose row of the ledger it would move -- the plain and the supersampled kernel with shadow rays and refraction (SGPR spills 53 -> 55 and 54 -> 56)
// and the two G-buffer kernels without shadow rays (SGPR spills 50 -> 53). They keep the wave test alone.
constexpr bool trace_root_pretests(bool WAVE_CULLS, bool GBUFFER, bool SHADOW, bool REFRACT)
{
    return WAVE_CULLS && !(SHADOW && REFRACT) && !(GBUFFER && !SHADOW);
}

// ---- who takes the same root step per wave for the reflection bounce's candidates (bounce_pretest_mask, behind candidate_mask at bounce 1) ----
// trace_body: the kernels of trace_root_pretests, all six -- no row of the ledger moves with it (the shape of bounce_pretest_mask is what holds them).
// Every other kernel keeps candidate_mask alone at bounce 1 and compiles to what it compiled to before.
constexpr bool trace_bounce_pretests(bool ROOT_PRETESTS) { return ROOT_PRETESTS; }

// ---- whose camera-bounce pre-test enters a lane's first surviving instance (root_pretest_enters, in place of root_pretest_misses there) ----
// trace_body: the kernels of trace_root_pretests, except the two with shadow rays, whose row of the ledger it would move -- the supersampled kernel
// (SGPR spills 52 -> 48) and the G-buffer kernel (59 -> 57). The four without shadow rays -- plain and supersampled, with and without refraction --
// hold every row. Every other kernel keeps root_pretest_misses and compiles to what it compiled to before.
constexpr bool trace_pretest_enters(bool ROOT_PRETESTS, bool SHADOW) { return ROOT_PRETESTS && !SHADOW; }

// ---- who takes 32-bit record offsets (TR_OFFSET32 in the traversal: pair_record, tri_hot_record, big_leaf_count, instance_record;
//      SB_OFFSET32 in the shading: tri_cold_record, instance_record) ----
// A counted or stamped launch keeps the 64-bit form in every family (the independent path, above). Of the others, a kernel takes the option
// unless a row of the ledger would move with it; five would, each downwards, and keep the 64-bit form:
//   crt_trace_gbuffer_kernel<true, true, true>   VGPRs 68 -> 67
//   crt_trace_ldstop_kernel<false>               VGPRs 65 -> 64 (its vector path selects between two bases per lane: little to gain)
//   crt_primary_kernel<false>                    VGPRs 59 -> 58
//   crt_bounce_kernel<false>                     VGPRs 64 -> 63
//   crt_trace_block_kernel<false, false>         ScratchSize 32 -> 16, VGPRs Spill 6 -> 2
// trace_body: the plain, supersampled and G-buffer kernels, the benchmark's among them -- all but the one G-buffer kernel above and the ldstop form (TOP)
constexpr bool trace_offset32(bool COUNT, bool STAMP, bool TOP, bool GBUFFER, bool SHADOW, bool TLAS, bool REFRACT)
{
    return !COUNT && !STAMP && !TOP && !(GBUFFER && SHADOW && TLAS && REFRACT);
}
// the wavefront form (crt_primary_kernel, crt_bounce_kernel) and crt_trace_block_kernel: never; crt_trace_refill_kernel: uncounted and unstamped
constexpr bool kWavefrontOffset32 = false;
constexpr bool kBlockOffset32 = false;
constexpr bool refill_offset32(bool COUNT, bool STAMP) { return !COUNT && !STAMP; }
// crt_query_kernel: a counted kernel
constexpr bool kQueryOffset32 = false;
// the queries on device buffers (crt_rays_kernel, crt_ao_kernel, their inclusive twins, crt_shade_kernel): all of them, no row moves
constexpr bool kDeviceQueryOffset32 = true;
}

// ------------------------------------------------------------------------------------------------
// Per-lane traversal state machine: the instance loop + IntersectBVH of kernel_main.cl:124-160,198-217.
//
// Upstream (and a literal port) runs `for instance { while pop { descend } }` in lock-step: a wave pays, for
// every instance, the slowest lane's traversal, and every lane waits for its neighbours' whole descents. Here
// every lane owns a `Traversal`: its own ascending list of candidate instances and its own position in the tree,
// advanced by three step kinds -- enter(next candidate), inner(one child pair), leaf(its triangles, then pop).
// Per ray the sequence of instances, node visits, triangle tests and the running best t is exactly upstream's,
// so results are bit-identical; only the interleaving between lanes differs.
// The stack lives in LDS/scratch (CRT_STACK_*); slot indices wrap modulo 32 where upstream's array would overflow.
// ------------------------------------------------------------------------------------------------
// OPTS: the TR_* options of the closest_hit (or the kernel's own loop, crt_refill.h) that owns it, carried in the type: trip_steps reads them
// back from it. The members read TR_COUNT, TR_DIVIDE and TR_OFFSET32; inner and leaf take the box rule and any-hit from the options of the trip that calls them.
template <unsigned OPTS>
struct Traversal {
    static_assert((OPTS & ~TR_ALL) == 0u, "unknown traversal option");
    static constexpr bool COUNT = has_opt(OPTS, TR_COUNT), DIVIDE = has_opt(OPTS, TR_DIVIDE), OFFSET32 = has_opt(OPTS, TR_OFFSET32);
    v3 mo, md, inv;               // ray in the current instance's object space (direction not renormalised, hazard H6)
    Triout tr;                    // running best of the current instance (kernel_main.cl:200-202)
    int sp, prot, inters;         // stack pointer, pop counter (kernel_main.cl:131), OR of the `passed` flags
    uint32_t ref, curInst;
    bool active;                  // inside an instance

    __device__ __forceinline__ void reset()
    {
        mo = mk3(0.f, 0.f, 0.f); md = mo; inv = mo;
        tr.t = 0.f; tr.u = 0.f; tr.v = 0.f; tr.tri = 0;
        sp = 0; prot = 0; inters = 0; ref = 0; curInst = 0; active = false;
    }
    __device__ __forceinline__ bool at_inner() const { return active && !(ref & CRT_LEAF_BIT); }
    __device__ __forceinline__ bool at_leaf() const { return active && (ref & CRT_LEAF_BIT); }

    // ends the current instance: keep the hit if any triangle passed (kernel_main.cl:210-216)
    __device__ __forceinline__ void finish(Closest& c)
    {
        if (inters) { c.hitInstance = (int)curInst; c.hit = tr; c.distance = tr.t; c.anyHit = 1; }
        active = false;
    }
    // `while (currentNodeIndex > 0 && protection++ < 250) node = stack[--currentNodeIndex]` (kernel_main.cl:131-133)
    template <class STK>
    __device__ __forceinline__ void pop_next(const STK& stack, Closest& c, LaneCounters& lc)
    {
        // one level of branching: `protection++` happens exactly when the stack is not empty
        const bool nonEmpty = sp > 0, canPop = nonEmpty && prot < CRT_MAX_POPS;
        prot += nonEmpty ? 1 : 0;
        if (COUNT) { if (nonEmpty && !canPop) lc.capHits++; if (canPop) lc.pops++; }
        if (canPop) { --sp; ref = stack.read(sp); }
        else {
            const bool keep = inters != 0;                       // finish(): selects instead of a nested branch
            c.hitInstance = keep ? (int)curInst : c.hitInstance; c.distance = keep ? tr.t : c.distance; c.anyHit = keep ? 1 : c.anyHit;
            c.hit.t = keep ? tr.t : c.hit.t; c.hit.u = keep ? tr.u : c.hit.u; c.hit.v = keep ? tr.v : c.hit.v; c.hit.tri = keep ? tr.tri : c.hit.tri;
            active = false;
        }
    }
    // kernel_main.cl:200-210: transform the ray into instance `inst` and start at its root (record fetch: load_instance above)
    // TOP (crt_ldstop.h): start at the root's record in the tree-top table (CrtDevInstance::r2.w) instead of the global pair
    template <bool TOP = false>
    __device__ __forceinline__ void enter(const CrtDevScene& S, uint32_t inst, v3 o, v3 d, float bestSoFar, LaneCounters& lc)
    {
        curInst = inst;
        const CrtDevInstance I = load_instance<OFFSET32>(S.devInstances, inst);
        mo = xform_xyz(I, o.x, o.y, o.z, 1.0f);
        md = xform_xyz(I, d.x, d.y, d.z, 0.0f);
        inv = recip3<DIVIDE>(md);                                   // native_recip pinned to IEEE: the bits of 1.0f / x
        tr.t = bestSoFar; tr.tri = 0; tr.u = 0.0f; tr.v = 0.0f;
        ref = __float_as_uint(TOP ? I.r2.w : I.r0.w);            // the root is popped at once: sp 1 -> 0, protection 0 -> 1
        sp = 0; prot = 1; inters = 0; active = true;
        if (COUNT) { lc.traversals++; lc.pops++; }
    }
    // kernel_main.cl:142-157: fetch the child pair, two slab tests, near child first, far child pushed
    // (TR_INCLUSIVE of the trip's options: intersect_aabb's; two boxes that both hold the origin return 0 and 0, `dist1 > dist2` is false: left first)
    template <unsigned TRIP, class STK>
    __device__ __forceinline__ void inner(const CrtDevScene& S, const STK& stack, Closest& c, LaneCounters& lc)
    {
        constexpr bool INCLUSIVE = has_opt(TRIP, TR_INCLUSIVE);
        // every lane of this step on the same node (the top of a tree under a coherent packet): one scalar load instead of four
        // vector loads, the boxes as scalar operands. (Round 2 measured the same idea as a wash -- the uniformity test costs every
        // step -- but with the instance bounds and records on the scalar path the node fetches are 3/4 of the vector-memory
        // instructions that bound the kernel: sponza-sibenik +6 %, multi-1M-dense +2 %, multi-1M and nanosuit-demo +-0, synchronous
        // frames +0...5 %. The same for leaves -- a uniform triangle through scalar loads -- lost 18 %: the 9 scalar operands push the
        // kernel into scratch, and small triangles are never shared by a whole packet.)
        // (Round 5: the two slab tests are written out in each branch, so that the scalar branch uses the record's SGPRs as operands
        // directly instead of copying 14 of them into VGPRs first.)
        float dist1, dist2;
        uint32_t nearRef, farRef;
        const uint32_t ref0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)ref);
        if (__ballot(ref != ref0) == 0) {
            // (STK::kTop: a wave-uniform step on a tree-top record reads the table's GLOBAL copy through the scalar cache, as before)
            const crt_const_f32x4_ptr q = (STK::kTop && (ref0 & CRT_TOP_BIT)) ? (crt_const_f32x4_ptr)(S.topPairs + (size_t)(ref0 & 0xFFFFu) * 4)
                                                                             : (crt_const_f32x4_ptr)(S.pairs + (size_t)ref0 * 4);
            const crt_f32x4 a = q[0], b = q[1], c4 = q[2], e = q[3];
            dist1 = intersect_aabb<INCLUSIVE>(mo, inv, make_float4(a.x, a.y, a.z, a.w), make_float4(b.x, b.y, b.z, b.w), tr.t);
            dist2 = intersect_aabb<INCLUSIVE>(mo, inv, make_float4(c4.x, c4.y, c4.z, c4.w), make_float4(e.x, e.y, e.z, e.w), tr.t);
            nearRef = __float_as_uint(a.w); farRef = __float_as_uint(c4.w);
#ifndef CRT_TOP_NO_LDS_PATH
#define CRT_TOP_NO_LDS_PATH 0                // A/B builds: 1 = the four-wave form without its LDS reads (what the workgroup shape alone costs)
#endif
        } else if (STK::kTop && !CRT_TOP_NO_LDS_PATH && __ballot(!(ref & CRT_TOP_BIT)) == 0) {
            // crt_ldstop.h: EVERY lane of this step wants a record of the LDS-resident tree tops, and they differ: four ds_read_b128 per
            // lane instead of four vector-memory instructions for the wave (north_star's "hot BVH tiles staged in LDS")
            const auto q = stack.top_record(ref & 0xFFFFu);
            const crt_f32x4 a = q[0], b = q[1], c4 = q[2], e = q[3];
            dist1 = intersect_aabb<INCLUSIVE>(mo, inv, make_float4(a.x, a.y, a.z, a.w), make_float4(b.x, b.y, b.z, b.w), tr.t);
            dist2 = intersect_aabb<INCLUSIVE>(mo, inv, make_float4(c4.x, c4.y, c4.z, c4.w), make_float4(e.x, e.y, e.z, e.w), tr.t);
            nearRef = __float_as_uint(a.w); farRef = __float_as_uint(c4.w);
        } else {
            // one aligned 64-byte record (a step that mixes tree-top and other records takes the top ones from the table's global copy:
            // the four vector loads are issued for the wave either way)
            const float4* p = (STK::kTop && (ref & CRT_TOP_BIT)) ? S.topPairs + (size_t)(ref & 0xFFFFu) * 4 : pair_record<OFFSET32>(S, ref);
            const float4 lmin = p[0], lmax = p[1], rmin = p[2], rmax = p[3];
            dist1 = intersect_aabb<INCLUSIVE>(mo, inv, lmin, lmax, tr.t);
            dist2 = intersect_aabb<INCLUSIVE>(mo, inv, rmin, rmax, tr.t);
            nearRef = __float_as_uint(lmin.w); farRef = __float_as_uint(rmin.w);
        }
        if (COUNT) lc.innerVisits++;
        {   // kernel_main.cl:148-151 as four selects on one compare (the branchy form costs an exec-mask save / restore)
            const bool sw = dist1 > dist2;
            const float d1 = sw ? dist2 : dist1, d2 = sw ? dist1 : dist2;
            const uint32_t r1 = sw ? farRef : nearRef, r2 = sw ? nearRef : farRef;
            dist1 = d1; dist2 = d2; nearRef = r1; farRef = r2;
        }
        if (dist2 != 1e30f) {                                   // both children hit (dist1 <= dist2): push the far one
            if (COUNT) { if (sp >= CRT_STACK_DEPTH) lc.stackOverflows++; }
            stack.write(sp, farRef);
            sp++;
            if (COUNT) { if ((uint32_t)sp > lc.maxStack) lc.maxStack = (uint32_t)sp; }
        }
        if (dist1 == 1e30f) pop_next(stack, c, lc);
        else ref = nearRef;
    }
    // kernel_main.cl:135-140: every triangle of the leaf, then the next pop.
    // TR_ANYHIT of the trip's options (shadow rays): the traversal ends at the first triangle that passes.
    template <unsigned TRIP, class STK>
    __device__ __forceinline__ void leaf(const CrtDevScene& S, const STK& stack, Closest& c, LaneCounters& lc)
    {
        constexpr bool ANYHIT = has_opt(TRIP, TR_ANYHIT);
        const uint32_t first = ref & 0x00FFFFFFu;
        uint32_t n = (ref >> 24) & 0x7Fu;
        if (n == 0) n = big_leaf_count<OFFSET32>(S, first);
        for (uint32_t i = first, end = first + n; i < end; ++i) {
            if (COUNT) lc.triTests++;
            const float* __restrict__ hot = tri_hot_record<OFFSET32>(S, i);
            inters |= intersect_triangle<DIVIDE>(mo, md, mk3(hot[0], hot[1], hot[2]), mk3(hot[3], hot[4], hot[5]), mk3(hot[6], hot[7], hot[8]), tr, i);
            if (ANYHIT) { if (inters) break; }
        }
        if (ANYHIT && inters) finish(c);
        else pop_next(stack, c, lc);
    }
};

// ------------------------------------------------------------------------------------------------
// The conservative instance cull, and why its slack is enough.
//
// Claim: if the predicate below rejects instance i for a ray (o, d), the ray fails BOTH child slab tests of that instance's
// root as the traversal would compute them in fp32 (kernel_main.cl:203-207 transform + kernel_main.cl:108-117), so skipping the
// instance changes no hit record; the counters add the one pop + one inner visit upstream spends on it.
//
// Notation. u = 2^-24, g3 = 3u/(1-3u), g4 = 4u/(1-4u). M3 / T: the 3x3 part / the translation row of the instance's fp32
// inverseTransform, F3 = M3^-1 (double, host). kappa = |M3|_F |F3|_F (Frobenius condition number, >= 3; 3 for rigid +
// uniform scale), tau = |T|_2 |F3|_F. (c, r): exact centre / radius of the sphere around the world image of the union of the
// root's two child boxes; the table holds (fl(c), w) with w >= r (1 + 1e-4) + |c - fl(c)|, so its sphere contains the exact
// one. x = |c - o|, O = |o|.
//
// (1) What an fp32 pass means in world space. xform_xyz sums four products left to right:
//     |mo - o M|_2 <= g4 (|o| |M3|_F + |T|),  |md - d M3|_2 <= g3 |d| |M3|_F.
// In a slab test every t is (b - mo_k) * (1 / md_k): three roundings, t_computed = t_exact (1 + theta), |theta| <= g3. If the
// test passes (tnear < tfar, tnear > 0), the point p = mo + tnear md of the COMPUTED ray lies in the box grown along each
// axis by g3 max(|bmin_k - mo_k|, |bmax_k - mo_k|) (from lo_k (1 + theta) <= tnear < hi_k (1 + theta')); a zero / overflowing
// 1 / md_k or a 0 * inf NaN can only turn a pass into a miss or leave p inside the closed slab. Carried back to world space
// (a factor |F3|; t is the same parameter on both sides because directions are not renormalised, H6; |d| t <= x + r there), the
// exact world ray o + t d, t > 0, comes within
//     Delta(O, x) = g4 (kappa O + tau) + (1 + sqrt 3) g3 kappa (x + w)
// of the exact world image of the box, hence of the sphere (c, r): a pass implies dist(ray, c) <= r + Delta.
// (2) What a rejection means. With fp32 inputs (fl(c), w, o, d), oc = fl(c) - o is exact to u per component, oc2, dd and b =
// oc.d carry <= 5u, 3u (relative) and 4u |oc| |d| (absolute); `oc2 dd - b b > r2 dd` computed implies, in exact arithmetic,
//     dist(line, fl(c))^2 > 1.0201 (1 - 12u) w^2 + (4e-6 (1 - 12u) - 19u) x^2  >=  1.02 w^2 + 2.8e-6 x^2
// -- the 4e-6 |oc|^2 term is what outweighs the cancellation in oc2 dd - b b -- and the second clause (centre behind the origin,
// origin outside the grown sphere) gives the same bound for every t > 0 (b < 0 computed allows b <= 4u |oc| |d| exactly, which
// moves the closest approach by a factor 1 - 16u^2). Any NaN makes both comparisons false: not culled.
// (3) The slack dominates when sqrt(1.02 w^2 + 2.8e-6 x^2) >= w + Delta(O, x) for all x >= 0. The left side is convex in x, the
// right side affine; with c1 = (1 + sqrt 3) g3 kappa (4.9e-7 kappa) the minimum of the difference is at
// 2.8e-6 x = c1 sqrt(1.02 w^2 + 2.8e-6 x^2) and equals  w (sqrt(1.02 (1 - c1^2 / 2.8e-6)) - 1 - c1) - g4 (kappa O + tau), so
//     the cull is exact for ray origins with  |o| <= O_i = (w (sqrt(1.02 (1 - c1^2 / 2.8e-6)) - 1 - c1) - g4 tau) / (g4 kappa).
// Rigid + uniform scale, instance centre p: kappa = 3, tau = sqrt 3 |p|: O_i ~ 13,800 w - 0.58 |p| -- a 1-unit instance may be
// viewed from 13,800 units, a 1000-unit one from 1.4e7; kappa above ~470 (c1 > 2.3e-4) leaves no range at all.
// (4) Outside the range the host turns the cull off (crt_instances.h rebuild_instance_master / crt_frame.h crt1_render): an instance whose O_i is
// below the reach of bounce-ray origins (object-space hit points used as world origins, H6) is stored with r = -1 = never
// culled; a frame whose camera, or a query whose farthest origin, lies beyond the smallest O_i of the remaining instances runs
// with an all-never table (and the linear candidate loop). tests/test_gpu_cull_bound.py: instance scales 1e-3 ... 1e3,
// condition numbers to 300, origins out to 1e6 and to 0.95 O_i with grazing rays, hit records against the oracle.
// (5) Nodes of the instance tree (sphere_culls on CrtTlasNode::sphere, radius R around >= 2 instance spheres, so R >= sqrt 3 w_i
// and |C - c_i| + w_i <= R): a rejected node has dist(ray, c_i) >= dist(ray, C) - (R - w_i) > w_i + sqrt(1.02 R^2 + 2.8e-6 X^2) - R,
// and with x_i <= X + R the same minimisation gives R (0.00995 - 2 c1) - g4 (kappa O + tau) >= the instance's own margin
// w_i (0.00995 - c1) - ... for every c1 in the admitted range: a subtree is never rejected for a ray one of its instances admits.
// Inclusive pass (intersect_aabb<true>: tnear <= tfar, tfar >= 0, entry = max(tnear, 0)). (1) holds with t* = max(tnear, 0) >= 0 in
// place of tnear: for tnear > 0 it is the same point, now of the closed grown box (lo_k (1 + theta) <= tnear <= hi_k (1 + theta'));
// for tnear <= 0 <= tfar every slab holds t = 0, so p = mo -- the computed origin -- lies in the closed box exactly, and |d| t* <= x + r
// as before. (2) both rejection clauses already bound the distance for EVERY t >= 0, t = 0 included: the first bounds the whole line, the
// second needs oc2 > r2 -- the origin itself outside the grown sphere -- besides b < 0. (3), (4) and (5) use only (1) and (2): unchanged.
// So the cull, the instance tree and the cull range serve inclusive queries as they are; an origin INSIDE an instance's sphere fails
// both clauses and the instance is a candidate.
// ------------------------------------------------------------------------------------------------
// The ray/sphere rejection of candidate_mask for the instance tree (same arithmetic; any NaN -> not culled).
__device__ __forceinline__ bool sphere_culls(const float4 bs, v3 o, v3 d, float dd)
{
    const v3 oc = mk3(bs.x - o.x, bs.y - o.y, bs.z - o.z);
    const float oc2 = dot3(oc, oc), b = dot3(oc, d);
    const float r2 = bs.w * bs.w * 1.0201f + 4e-6f * oc2;           // 1 % on the radius + slack growing with distance
    return (bs.w >= 0.0f) & ((oc2 * dd - b * b > r2 * dd) | ((b < 0.0f) & (oc2 > r2)));
}

// Conservative candidate mask for instances [base, base + cnt): bit k is cleared only when the ray provably misses
// instance base+k's bounding sphere (any NaN -> candidate). A culled instance costs upstream exactly one pop and one
// inner visit and changes nothing, which is what the counters record for it. Wave-uniform loop, scalar loads.
// The bounding spheres are read through a constant-address-space pointer: the index is wave-uniform, and only for that
// address space does the compiler turn a uniform load into a SCALAR load (s_load_dwordx4, scalar cache). Through the plain
// pointer -- a member of a by-value kernel argument carries no noalias/readonly information -- rounds 1-2 issued one VECTOR
// load per instance, bounce and wave here: 12 % of the trace kernel's vector-memory instructions, on the pipeline that
// bounds it. The table is written by the host before the launch and never by a kernel.
// OPTS: CM_COUNT: the culled instances are counted; CM_DEFER_COUNT: ... by the caller (closest_hit's any-hit form), not here.
template <unsigned OPTS = 0u>
__device__ __forceinline__ unsigned long long candidate_mask(const CrtDevScene& S, v3 o, v3 d, uint32_t base, uint32_t cnt, LaneCounters& lc)
{
    static_assert((OPTS & ~CM_ALL) == 0u, "unknown cull option");
    constexpr bool COUNT = has_opt(OPTS, CM_COUNT), DEFER_COUNT = has_opt(OPTS, CM_DEFER_COUNT);
    const float dd = dot3(d, d);
    unsigned long long cand = 0;
    const crt_const_f32x4_ptr bounds = (crt_const_f32x4_ptr)S.instBounds;
    for (uint32_t k = 0; k < cnt; ++k) {
        const crt_f32x4 bs = bounds[base + k];
        const v3 oc = mk3(bs.x - o.x, bs.y - o.y, bs.z - o.z);
        const float oc2 = dot3(oc, oc), b = dot3(oc, d);
        const float r2 = bs.w * bs.w * 1.0201f + 4e-6f * oc2;       // 1 % on the radius + slack growing with distance
        const bool cull = (bs.w >= 0.0f) && ((oc2 * dd - b * b > r2 * dd) || (b < 0.0f && oc2 > r2));
        if (!cull) cand |= 1ull << k;
    }
    if (COUNT && !DEFER_COUNT) { const uint32_t culled = cnt - (uint32_t)__popcll(cand); count_culled(lc, culled); }
    return cand;
}

// candidate_mask for a wave whose rays share their origin (the camera bounce of the uncounted Trace kernels: whole tiles, the quadrant
// waves of split tiles, the SSAA virtual frame). Of candidate_mask's 27 VALU instructions per instance 16 depend on the origin and the
// instance alone -- oc, oc2, r2, `w >= 0`, `oc2 > r2` -- and every lane of every wave computed them again. Here the wave's r-th active
// lane computes them for instances base + r, base + r + (active lanes), ... with candidate_mask's expressions in candidate_mask's order
// (-ffp-contract=off: the same roundings) and stores them in the wave's stack rows, which are dead until the first push (the ownership
// rule of tlas_candidates; rows 0..5 of the kLds >= 15 stack rows, no parked slot):
//     words [4k, 4k + 4)              {oc.x, oc.y, oc.z, oc2}
//     words [256 + 2k, 256 + 2k + 2)  {r2', thr}:  r2' = r2, or +inf when !(w >= 0);  thr = 0 when w >= 0 && oc2 > r2, else -inf
// and every lane runs the per-instance loop on broadcast reads (one ds_read_b128 + one ds_read_b64, a wave-uniform address):
//     b = oc.d,  cull = (oc2 dd - b b > r2' dd) | (b < thr).
// The two uniform predicates are folded into values without changing a bit of the mask: `x > r2' dd` with r2' = +inf is `x > inf` or
// `x > NaN` (dd = 0 or NaN) -- false, like `w >= 0` false (w < 0: never cull, or a NaN w); `b < -inf` is false for every b, NaN
// included, like `oc2 > r2` false; `b < 0.0f` is the original clause. A NaN or overflowing oc2 / r2 takes the original operations.
// A lane's own stack entries lie in these rows, so every lane of the wave has finished reading before any lane pushes: the loop below
// is wave-uniform and the trip loop starts behind it; the next 64-chunk restages after the trip loop has ended for the whole wave
// (every lane's stack empty).
// ------------------------------------------------------------------------------------------------
// The wave test (TR_WAVE_CULL, policy::trace_wave_culls): one test per instance and WAVE in front of the per-lane loop. The 64 primary rays
// of a tile share their origin o and lie in a narrow cone; an instance whose grown sphere lies outside that cone is rejected for every lane
// at once, and the per-lane loop runs over the survivors only (multi-1M, 1920x1080: 2.06 of 16 per tile, profiles/wave_cull_counts.txt).
// This clears bits candidate_mask would keep, which is legitimate through the lemma below -- it continues the derivation above sphere_culls.
//
// (6) Lemma. If cone_rejects returns true for instance k, then for EVERY lane of the wave, with its fp32 d and the shared o, in exact arithmetic
//         |o + t d - fl(c)|^2 > 1.02 w^2 + 2.8e-6 x^2   for all t > 0        (x = |fl(c) - o|)
//     -- the conclusion of (2). (3)-(5) use nothing else of the predicate, so the cull range O_i, the all-never table and the never-culled
//     instances (w < 0: not rejected here either) hold as they stand: a rejected instance is one the traversal would have left at its root.
// (6a) Geometry. N^2 = 1.02 w^2 + 2.8e-6 x^2, oc = fl(c) - o, a = the direction of lane 0, and the exact angles theta >= angle(d, a) for every lane,
//     phi = angle(oc, a), psi = asin(N / x) (N < x below). If phi > theta + psi then angle(d, oc) >= phi - angle(d, a) > psi for every lane (the
//     triangle inequality on the sphere; theta + psi < pi because theta < pi/3, psi <= pi/2). For angle(d, oc) < pi/2 the distance from fl(c)
//     to the line is x sin(angle(d, oc)) > x sin psi = N; for angle(d, oc) >= pi/2 the closest point of the ray t > 0 is its origin, at x > N.
// (6b) The computed test implies phi > theta + psi. The test is  cphi < ct cpsi - st spsi - m2  with ct, st, spsi, cpsi >= 0. The right side
//     is decreasing in st and spsi and increasing in ct and cpsi, so it is enough that each computed value errs to its safe side (or by
//     an amount m2 absorbs); cos is decreasing on [0, pi]. u = 2^-24; v_rsq_f32 and v_sqrt_f32 are good to 1 ulp (<= 2u relative).
//       ct   = min over the lanes of fl(d.a) rsq(dd), times rsq(aa), minus m0. fl(d.a): 3u |d||a|; dd, aa: 3u relative, each rsq then 3.5u;
//              two products and the subtraction 3u: ct + m0 is within 13u = 7.7e-7 of cos theta, so with m0 = 4e-6 (5 x that), ct <= cos theta - 3.2e-6.
//              The guard admits the wave only when every lane has 0.999 <= dd <= 1.001 and d.a > 0 as computed (a NaN fails each compare; a lane that
//              fails contributes 0 to the minimum) and ct >= 0.5: the unsigned minimum of the bit patterns is the minimum of non-negative floats.
//       st   = sqrt(max(0, 1 - ct ct)): 1 - ct^2 >= sin^2 theta + 2 ct 3.2e-6 >= sin^2 theta + 3.2e-6 (ct >= 0.5); the roundings of the square, the
//              subtraction and the root take at most 3.6e-7 of that (9 x to spare): st >= sin theta.
//       spsi = sqrt(R2) rsq(oc2), R2 = r2 (1 + m1), r2 candidate_mask's: r2 >= N^2 (1 + 9e-5) by (2)'s own bounds (1.0201 against 1.02, 4e-6 against
//              2.8e-6), which is NOT counted here. Root 2u, rsq 3.5u, oc against x 1u, the product and R2's 1.5u: 8u, against sqrt(1 + m1) = 1 + 66u for
//              m1 = 8e-6 (8 x): spsi >= N / x = sin psi. The test requires oc2 > R2 as computed, hence x^2 (1 + 5u) > N^2 (1 + 9e-5): x > N; and
//              1e-30 < oc2 < 1e30 keeps both special functions away from denormals and overflow.
//       cpsi = sqrt(max(0, 1 - spsi spsi)) <= cos psi + 2.6u: for spsi^2 >= 0.01 the surplus of spsi outweighs the roundings (cpsi <= cos psi outright up
//              to the root's 2u), below that cpsi > 0.99 and the roundings move it by 0.6u + 2u.
//       cphi = (fl(oc.a) rsq(oc2)) rsq(aa): 3u for the dot product, 2u for oc's own rounding, 3.5u for each rsq, 2u for the products: 14u.
//       The right side's own products and subtractions: 4u. Together 14u + 2.6u + 4u = 21u = 1.25e-6 against m2 = 8e-6 (6 x).
//     So every margin has more than a factor of 4 to spare. Any NaN (a NaN w, camera or centre) makes a compare false: the instance survives.
// ------------------------------------------------------------------------------------------------
#ifdef CRT_NO_WAVE_CULL
#define CRT_WAVE_CULLS(WAVE) false        // A/B builds: the staged loop over all instances everywhere
#else
#define CRT_WAVE_CULLS(WAVE) (WAVE)
#endif
#define CRT_WAVE_CULL_MIN 8u              // fewest instances of a scene whose full waves take the wave test (staged_candidate_mask says why)
#define CRT_CONE_M0 4e-6f
#define CRT_CONE_M1 8e-6f
#define CRT_CONE_M2 8e-6f
// wave-uniform: the axis (lane 0's direction), rsq(a.a), cos and sin of the half-angle. ct >= 0.5 is the guard.
struct WaveCone { v3 a; float ra, ct, st; };
__device__ __forceinline__ bool cone_admits(const WaveCone& c) { return c.ct >= 0.5f; }
// min(v, v of another lane of the row of 16) as DPP moves: CTRL = quad_perm [1,0,3,2] 0xB1, [2,3,0,1] 0x4E, row_half_mirror 0x141, row_mirror 0x140
template <int CTRL> __device__ __forceinline__ uint32_t row_min_step(uint32_t v)
{
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
    return o < v ? o : v;
}
// The cone of a FULL wave (every lane active: a DPP move never reads an inactive lane's register); d, dd = d.d per lane
__device__ __forceinline__ WaveCone wave_cone(v3 d, float dd)
{
    WaveCone c;
    c.a = mk3(__uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(d.x))),
              __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(d.y))),
              __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(d.z))));
    c.ra = __builtin_amdgcn_rsqf(__uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(dd))));
    const float q = dot3(d, c.a);
    const bool admitted = (dd >= 0.999f) & (dd <= 1.001f) & (q > 0.0f);
    uint32_t m = admitted ? __float_as_uint(q * __builtin_amdgcn_rsqf(dd)) : 0u;
    m = row_min_step<0xB1>(m); m = row_min_step<0x4E>(m); m = row_min_step<0x141>(m); m = row_min_step<0x140>(m);
    const uint32_t m0 = (uint32_t)__builtin_amdgcn_readlane((int)m, 0), m1 = (uint32_t)__builtin_amdgcn_readlane((int)m, 16),
                   m2 = (uint32_t)__builtin_amdgcn_readlane((int)m, 32), m3 = (uint32_t)__builtin_amdgcn_readlane((int)m, 48);
    const uint32_t m01 = m0 < m1 ? m0 : m1, m23 = m2 < m3 ? m2 : m3;
    c.ct = __uint_as_float(m01 < m23 ? m01 : m23) * c.ra - CRT_CONE_M0;
    c.st = __builtin_amdgcn_sqrtf(fmaxf(0.0f, 1.0f - c.ct * c.ct));
    return c;
}
// The wave test of one instance, from the terms its staging lane holds (oc, oc2, r2, `w >= 0`): (6) above
__device__ __forceinline__ bool cone_rejects(const WaveCone& c, v3 oc, float oc2, float r2, bool cullable)
{
    const float R2 = r2 * (1.0f + CRT_CONE_M1);
    const float rs = __builtin_amdgcn_rsqf(oc2);
    const float cphi = (dot3(oc, c.a) * rs) * c.ra;
    const float spsi = __builtin_amdgcn_sqrtf(R2) * rs;
    const float cpsi = __builtin_amdgcn_sqrtf(fmaxf(0.0f, 1.0f - spsi * spsi));
    const float rhs = (c.ct * cpsi - c.st * spsi) - CRT_CONE_M2;
    return cullable & (oc2 > R2) & (oc2 > 1e-30f) & (oc2 < 1e30f) & (cphi < rhs);
}

// ------------------------------------------------------------------------------------------------
// The root pre-test (TR_ROOT_PRETEST, policy::trace_root_pretests): behind the per-lane loop, once per instance the wave test left and WAVE,
// the lanes whose mask still holds the instance compute the step the traversal would start it with -- Traversal::enter and the root's inner
// step -- and clear the bit when both child boxes are missed. Half of the primary rays' entries end that way (multi-1M, 1920x1080: 2.03 M of
// 4.02 M, profiles/camera_cull_counts.txt), each of them as a part-occupied enter block and root step somewhere in the wave's trip loop; here the
// instance index is wave-uniform, so the instance record and the root's pair record come through the scalar cache and every lane of the tile works.
// This clears bits the sphere cull keeps, which is legitimate through (7) -- it continues the numbering of the cull's derivation.
//
// (7) Claim. If root_pretest_misses returns true for a lane's ray (o, d) and instance k, then entering k changes nothing for that ray: the
//     Closest every later instance sees, and the one closest_hit returns, are bit for bit what they are when k is skipped.
// (7a) Same bits. The values are the traversal's own, from the traversal's own functions: load_instance's uniform path, xform_xyz for mo (w = 1) and
//     md (w = 0), recip3<DIVIDE> with the kernel's DIVIDE, the pair record S.pairs[4 root ..] as the scalar path of Traversal::inner reads it, and
//     intersect_aabb<false> on both children -- the same operations in the same order under -ffp-contract=off. recip3 decides division or short form
//     for whichever lanes run it together, and both forms return the bits of 1.0f / x wherever the short one is taken (crt_recip.h: crt_debug_recip_sweep
//     checks exactly that, on the division and the short sequence), so the company of lanes, which differs from the trip loop's, does not matter.
//     The guard here is recip3's ONE_COMPARE form, `max(hi - 126, -125 - lo) > 0`: for integers it is `hi > 126 || lo < -125` (the maximum is positive
//     iff one of its operands is; exponents lie in -149 ... 128, nothing wraps). The sweep instantiates the two-compare form only; the one-compare form
//     is covered by this argument and by the frames of tests/test_gpu_root_pretest.py, not by the sweep. Only the bound differs: closest_hit's best0
//     here, tr.t = c.distance there.
// (7b) Monotone. The plain slab test passes only if tnear < minSoFar besides conditions that do not read the bound. closest_hit starts at
//     c.distance = best0 (99999 in trace_body, the only caller of the staged form; the pre-test takes the caller's value, whatever it is) and
//     c.distance only decreases: it is assigned tr.t of an instance with a passing triangle, and intersect_triangle requires t < out.t. So the
//     bound the traversal holds when it reaches k is <= best0, and a box missed at best0 is missed at that bound: `tnear < bound` false at the
//     larger bound is false at the smaller. A NaN tnear, tfar or best0 fails a compare whatever the bound.
// (7c) No state leaves a wasted entry. enter sets curInst, mo, md, inv, tr, ref, sp = 0, prot = 1, inters = 0 -- all of it set again by the next
//     enter before it is read. The root's inner step with both distances 1e30 pushes nothing (dist2 == 1e30) and calls pop_next with sp == 0:
//     no pop, prot unchanged, and `keep = inters != 0` is false, so every field of c stays as it was and the lane is inactive again. Nothing else
//     is written: the stack rows are untouched, the uncounted kernels keep no counters.
// (7d) Single-leaf meshes (hazard H3). A root ref with CRT_LEAF_BIT names triangles, not a pair record: there is no box to test, the traversal tests
//     the triangles at once, and the bit stays.
// (7e) Who does not take it. Counted and stamped launches, the instance tree and the ldstop form never reach
//     staged_candidate_mask and compile to what they compiled to before; the counters of the wasted visits belong to the counted launch, which still
//     makes them, and stay exact. Of the staged kernels, the waves that take no wave test (partial tiles, quadrant waves, scenes outside
//     CRT_WAVE_CULL_MIN ... 64 instances) keep the path they had; a kernel the policy leaves out, and every kernel
//     under -DCRT_NO_ROOT_PRETEST, compiles to the instructions of the wave test alone (the unit's assembly compared: no difference).
// (7f) The reflection bounce (TR_BOUNCE_PRETEST, policy::trace_bounce_pretests, bounce_pretest_mask below: sharedOrigin false). The same function behind
//     candidate_mask, every lane with its OWN origin o and direction d -- root_pretest_misses takes both per lane and never assumed o uniform; only
//     `inst` must be wave-uniform, and it is the scalar loop's k. (7) holds lane by lane, and nothing in it asks where the origin lies:
//     the origins of bounce 1 sit in the hit mesh's object space (hazard H6), and that does not enter the argument.
//     (7a) Same bits: mo is xform_xyz of the lane's o exactly as Traversal::enter computes it from the o closest_hit was called with -- the same `o`
//          and `d` are handed to both. The wave at bounce 1 holds only the lanes whose path continued (the others left the bounce loop and wait at
//          its end): __ballot is over those lanes, and so is recip3's wave-level choice between division and short form -- any company of lanes
//          gives the bits of 1.0f / x, as in (7a) above.
//     (7b) Monotone: closest_hit starts every call, bounce 1's included, at c.distance = best0 (a fresh no_hit(best0)); the bound only falls from there.
//     (7c) No state leaves a wasted entry: the argument is about one lane's Traversal and Closest and reads neither the origin nor the other lanes.
//     (7d) Single-leaf roots: the leaf bit is read from the instance record before the origin is touched; the bit stays.
//     A lane whose mask does not hold the instance computes along and clears nothing (`lo & ~bit` of a clear bit); a lane that is not live computes nothing.
//     Who takes it: the kernels of the camera bounce's pre-test, in scenes of CRT_WAVE_CULL_MIN ... 64 instances, full waves or not (rank == lane is not
//     used). Every other kernel, and every kernel under -DCRT_NO_BOUNCE_PRETEST, compiles to the instructions it had (the unit's assembly compared:
//     no difference in any function).
// (7g) The pre-test enters (TR_PRETEST_ENTRY, policy::trace_pretest_enters, root_pretest_enters below). A lane that survives the pre-test of its first
//     instance would repeat, in the trip loop, the step the pre-test has just made: enter, then the root's inner step, in blocks the wave runs for
//     however few lanes are at that step. The camera bounce's pre-test, which walks the wave's survivors in ascending k, keeps the step instead. A lane
//     commits to k when (i) its mask holds bit k, (ii) it is inside no instance (T.active false: every lane starts so, T.reset in closest_hit, and a lane
//     that has committed is inside), (iii) its mask holds no bit below k, (iv) the nearer child is hit. Its bit k is cleared and the trip loop starts
//     with the lane at level 1 of k; every later instance is entered by `enter`, as before.
//     1. Same state. The lane's first `enter` in the trip loop would be for the lowest bit of its mask -- k, by (i) and (iii) -- with
//        bestSoFar = c.distance = best0: c is a fresh no_hit(best0) and nothing has touched it. The pre-test's bound is best0 (an opaque copy of the same
//        bits). enter would set curInst = k, mo, md, inv (7a: the same functions on the same o and d; recip3 here in enter's own two-compare form),
//        tr = {best0, 0, 0, 0}, ref = root, sp = 0, prot = 1, inters = 0, active = true. The trip's inner step on that root would compute dist1, dist2
//        at tr.t = best0 -- the pre-test's two distances, (7a) -- and select on `dist1 > dist2`: n1 <= n2 afterwards, nearRef / farRef as here. It
//        would push farRef at sp = 0 and set sp = 1 when n2 != 1e30, and otherwise leave sp = 0; then, n1 == 1e30: pop_next -- not taken here, by
//        (iv), whatever n2 is; else ref = nearRef. inner touches no other field, and neither does the commit: curInst, mo, md, inv, tr, prot, inters,
//        active, sp, stack row 0 under the same condition, ref -- bit for bit what the two steps leave. When both distances are 1e30 the bit is cleared
//        as in (7); when n1 == 1e30 != n2 (possible only for a bound above 1e30, never for a frame's 99999) nothing is committed and the bit stays.
//        The counted kernels make these steps themselves and count them: they do not take the pre-test (7e). The stamps (TR_ITERS) are not here either.
//     2. Order. Per ray the instances are visited in ascending index (upstream's loop), and that order decides ties: `t < out.t` is strict, so of two
//        instances hit at the same t the lower index keeps the hit. (iii) keeps the order: a lane may be inside k before the trip loop only if the
//        trip loop would have entered k first. Bits below k that the pre-test cleared are instances the ray leaves at the root (7); a bit it left is
//        either an inner root whose step passed for a lane that was not `first` -- then the lane is inside a lower instance already, (ii) -- or a
//        single-leaf root (7d), whose bit is never cleared here and which is never committed to (root_pretest_enters returns before it reads the
//        lane). A lane that holds the bit of a lower single-leaf instance therefore fails (iii) for every k above it and enters that instance first,
//        through the trip loop. The test is `(lo & (bit | (bit - 1))) == bit` on the low half and, on the high half, the same with `lo == 0` besides.
//        After the commit the lane's mask holds only bits above k (k cleared, none below), and `cand == 0` / find-first-set go on from there.
//     3. Stack row 0. The staged cull terms lie in the wave's rows 0-5, and a lane's slot 0 is a word of row 0. The push is a store to the lane's own
//        slot 0, written in the pre-test's loop: behind both `culls(k)` loops and behind the wave test's rowA[lane] read in the source. Two things
//        keep it there. The compiler: the store and those loads go through pointers into the same LDS array (lds, rowA, rowB: s_stack) whose
//        addresses it cannot tell apart -- they do alias -- so it may not move the store above a load, fence or no fence; and the store is
//        control-dependent on the lane's mask, which is computed from the low half's loads. The hardware: LDS operations of one wave complete in the
//        order they are issued, and in a one-wave workgroup nobody else reads these rows. Nothing reads rows 0-5 as cull terms after the pre-test: the scene has one 64-chunk (the guard on
//        numInstances), so no restaging follows. The fence and wave barrier at the end of staged_candidate_mask stood between the last read and the
//        first push of the trip loop; they still stand behind every read, and the pushes that now precede them are ordered behind the reads by the
//        rule above. The first pop of a committed lane reads slot 0 in the trip loop, behind the barrier and behind the lane's own store.
//     4. Who does not take it: the list of (7e) -- counted and stamped launches, the instance tree, ldstop, the refill, block, wavefront and query
//        kernels never reach staged_candidate_mask; waves that take no wave test keep the path they had -- and, of the six kernels of the pre-test,
//        the two with shadow rays (policy). The reflection bounce's pre-test (7f) commits nothing: bounce_pretest_mask is as it was. A kernel the
//        policy leaves out, and every kernel under -DCRT_NO_PRETEST_ENTRY, compiles to the instructions it had (the unit's assembly compared
//        function by function: no difference).
// ------------------------------------------------------------------------------------------------
#ifdef CRT_NO_ROOT_PRETEST
#define CRT_ROOT_PRETESTS(PRETEST) false  // A/B builds: the instructions of the wave test alone, everywhere
#else
#define CRT_ROOT_PRETESTS(PRETEST) (PRETEST)
#endif
// `inst`: wave-uniform. Every lane of the wave runs it with the shared origin o; the lanes whose mask holds the instance use the answer.
// The shape is what the ledger's rows allow (the benchmark kernel's: 64 VGPRs, 43 spilled SGPRs); each item below moved rows when left out:
//  - recip3 takes its guard as one compare against zero (ONE_COMPARE): the two compares' constants 126 and -125 otherwise sit in SGPRs from the top
//    of the kernel through both traversals (four more spilled SGPRs in every kernel that takes the pre-test);
//  - the bound (best0: 99999 once inlined) is an opaque VGPR copy for the same reason (a v_mov per call instead of an SGPR per kernel).
// (Asking for the records 16 bytes at a time, each piece consumed before the next, held the same rows and no more, and measured no better.)
template <bool DIVIDE>
__device__ __forceinline__ bool root_pretest_misses(const CrtDevScene& S, v3 o, v3 d, uint32_t inst, float best0)
{
    const crt_const_f32x4_ptr p = (crt_const_f32x4_ptr)(S.devInstances + inst);         // load_instance's uniform path
    const crt_f32x4 r0 = p[0];
    const uint32_t root = __float_as_uint(r0.w);
    if (root & CRT_LEAF_BIT) return false;
    const crt_f32x4 r1 = p[1], r2 = p[2], r3 = p[3];
    CrtDevInstance I;
    I.r0 = make_float4(r0.x, r0.y, r0.z, r0.w); I.r1 = make_float4(r1.x, r1.y, r1.z, r1.w);
    I.r2 = make_float4(r2.x, r2.y, r2.z, r2.w); I.r3 = make_float4(r3.x, r3.y, r3.z, r3.w);
    float bound = best0;
    asm volatile("" : "+v"(bound));
    const v3 mo = xform_xyz(I, o.x, o.y, o.z, 1.0f);
    const v3 md = xform_xyz(I, d.x, d.y, d.z, 0.0f);
    const v3 inv = recip3<DIVIDE, true>(md);
    const crt_const_f32x4_ptr q = (crt_const_f32x4_ptr)(S.pairs + (size_t)root * 4);            // the scalar path of Traversal::inner
    const crt_f32x4 a = q[0], b = q[1], c4 = q[2], e = q[3];
    const float dist1 = intersect_aabb<false>(mo, inv, make_float4(a.x, a.y, a.z, a.w), make_float4(b.x, b.y, b.z, b.w), bound);
    const float dist2 = intersect_aabb<false>(mo, inv, make_float4(c4.x, c4.y, c4.z, c4.w), make_float4(e.x, e.y, e.z, e.w), bound);
    return (dist1 == 1e30f) & (dist2 == 1e30f);
}

#ifdef CRT_NO_PRETEST_ENTRY
#define CRT_PRETEST_ENTERS(ENTER) false   // A/B builds: root_pretest_misses alone, everywhere
#else
#define CRT_PRETEST_ENTERS(ENTER) (ENTER)
#endif
// The committing form, (7g): root_pretest_misses' step, and a lane for which `first` holds (its mask holds `inst`, no lower instance, and it is
// inside none yet) and whose root step goes on to a child keeps the step as its traversal state instead of throwing it away. Returns whether the
// lane's bit is to be cleared: both children missed, or the lane is now inside the instance.
// The shape is again what the ledger's rows allow. With root_pretest_misses' one-compare recip3 the benchmark kernel's spilled SGPRs moved with every
// form of the commit tried: one branch 43 -> 42, all selects and an exec-masked ds_write 39, the branch without the stores of zeros 41, opaque VGPR
// copies of `first`, of the take-flag or of the instance index 39 ... 42, the bound not opaque 42 (and a spilled VGPR with the selects). With recip3 in
// enter's own two-compare form (the same bits, (7a)) the branch form, and the select form, hold every row
// of the four kernels without shadow rays; the two with shadow rays move in every form (SGPR spills 59 -> 57, 52 -> 48) and are left out by the policy.
template <bool DIVIDE, unsigned OWNER, class STK>
__device__ __forceinline__ bool root_pretest_enters(const CrtDevScene& S, v3 o, v3 d, uint32_t inst, float best0, bool first, Traversal<OWNER>& T, const STK& stack)
{
    const crt_const_f32x4_ptr p = (crt_const_f32x4_ptr)(S.devInstances + inst);         // load_instance's uniform path
    const crt_f32x4 r0 = p[0];
    const uint32_t root = __float_as_uint(r0.w);
    if (root & CRT_LEAF_BIT) return false;
    const crt_f32x4 r1 = p[1], r2 = p[2], r3 = p[3];
    CrtDevInstance I;
    I.r0 = make_float4(r0.x, r0.y, r0.z, r0.w); I.r1 = make_float4(r1.x, r1.y, r1.z, r1.w);
    I.r2 = make_float4(r2.x, r2.y, r2.z, r2.w); I.r3 = make_float4(r3.x, r3.y, r3.z, r3.w);
    float bound = best0;
    asm volatile("" : "+v"(bound));
    const v3 mo = xform_xyz(I, o.x, o.y, o.z, 1.0f);
    const v3 md = xform_xyz(I, d.x, d.y, d.z, 0.0f);
    const v3 inv = recip3<DIVIDE>(md);                                                  // enter's own form: two compares
    const crt_const_f32x4_ptr q = (crt_const_f32x4_ptr)(S.pairs + (size_t)root * 4);            // the scalar path of Traversal::inner
    const crt_f32x4 a = q[0], b = q[1], c4 = q[2], e = q[3];
    const float dist1 = intersect_aabb<false>(mo, inv, make_float4(a.x, a.y, a.z, a.w), make_float4(b.x, b.y, b.z, b.w), bound);
    const float dist2 = intersect_aabb<false>(mo, inv, make_float4(c4.x, c4.y, c4.z, c4.w), make_float4(e.x, e.y, e.z, e.w), bound);
    const bool miss = (dist1 == 1e30f) & (dist2 == 1e30f);
    // Traversal::inner's select and its two conditions: the far child is pushed when it is hit, the lane goes on at the nearer child when that is hit
    const bool sw = dist1 > dist2;
    const float n1 = sw ? dist2 : dist1, n2 = sw ? dist1 : dist2;
    const uint32_t nearRef = sw ? __float_as_uint(c4.w) : __float_as_uint(a.w), farRef = sw ? __float_as_uint(a.w) : __float_as_uint(c4.w);
    const bool take = first & (n1 != 1e30f);
    if (take) {
        T.curInst = inst; T.mo = mo; T.md = md; T.inv = inv;
        T.tr.t = bound; T.tr.u = 0.0f; T.tr.v = 0.0f; T.tr.tri = 0;
        T.prot = 1; T.inters = 0; T.active = true;
        T.sp = 0;
        if (n2 != 1e30f) { stack.write(0, farRef); T.sp = 1; }
        T.ref = nearRef;
    }
    return miss | take;
}

typedef uint32_t crt_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t crt_u32x2 __attribute__((ext_vector_type(2)));
typedef crt_u32x4 __attribute__((address_space(3)))* crt_lds_u32x4_ptr;
typedef crt_u32x2 __attribute__((address_space(3)))* crt_lds_u32x2_ptr;
#define CRT_STAGE_ROWS 6
template <bool WAVE, bool PRETEST, bool DIVIDE, bool ENTER, unsigned OWNER, class STK>
__device__ __forceinline__ unsigned long long staged_candidate_mask(const CrtDevScene& S, v3 o, v3 d, uint32_t base, uint32_t cnt, const STK& stack, float best0,
                                                                    [[maybe_unused]] Traversal<OWNER>& T)
{
    static_assert(STK::kLds >= CRT_STAGE_ROWS && CRT_BLOCK == 64, "the staged cull terms take six stack rows of a one-wave workgroup");
    // the wave's row 0. One-wave workgroups: lds = s_stack + threadIdx.x, so this folds to the array's address (the kernel's only LDS
    // object: offset 0, which is what the 16- and 8-byte records below rely on) -- a constant, where `lds - lane` was a VGPR hoisted out
    // of the bounce loop and kept alive through both traversals (16 B of scratch)
    const crt_lds_u32_ptr wave = stack.lds - threadIdx.x;
    const crt_lds_u32x4_ptr rowA = (crt_lds_u32x4_ptr)wave;
    const crt_lds_u32x2_ptr rowB = (crt_lds_u32x2_ptr)(wave + 4 * 64);
    const unsigned long long act = __ballot(1);
    const uint32_t nAct = (uint32_t)__popcll(act);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
    for (uint32_t k0 = 0; k0 < cnt; k0 += nAct) {
        const uint32_t k = k0 + rank;
        if (k < cnt) {
            const float4 bs = S.instBounds[base + k];
            const v3 oc = mk3(bs.x - o.x, bs.y - o.y, bs.z - o.z);
            const float oc2 = dot3(oc, oc);
            const float r2 = bs.w * bs.w * 1.0201f + 4e-6f * oc2;   // candidate_mask's r2
            const bool cullable = bs.w >= 0.0f;
            crt_u32x4 a; crt_u32x2 t;
            a.x = __float_as_uint(oc.x); a.y = __float_as_uint(oc.y); a.z = __float_as_uint(oc.z); a.w = __float_as_uint(oc2);
            t.x = cullable ? __float_as_uint(r2) : 0x7F800000u;
            t.y = (cullable && oc2 > r2) ? 0u : 0xFF800000u;
            rowA[k] = a; rowB[k] = t;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float dd = dot3(d, d);
    const auto culls = [&](uint32_t k) {
        const crt_u32x4 a = rowA[k]; const crt_u32x2 t = rowB[k];
        const v3 oc = mk3(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z));
        const float oc2 = __uint_as_float(a.w), r2 = __uint_as_float(t.x), thr = __uint_as_float(t.y);
        const float b = dot3(oc, d);
        return (oc2 * dd - b * b > r2 * dd) | (b < thr);
    };
    // the mask in two 32-bit halves: one select and one OR per instance instead of two of each
    uint32_t lo = 0, hi = 0;
    if constexpr (CRT_WAVE_CULLS(WAVE)) {
        // The wave test: in a full wave (rank == lane, one staging pass) lane k tests instance k on the record it staged -- `thr == 0` is
        // `w >= 0 && oc2 > r2`, and r2' = +inf fails `oc2 > R2`. Every other wave -- a partial tile, a quadrant wave -- rejects nothing.
        // (Behind the barrier, not inside the staging loop: there its operands cost a VGPR spill in every kernel.)
        // (Opaque copies of the direction: the cone does not change from one 64-chunk of instances to the next, and hoisted out of closest_hit's
        // chunk loop it lives through the traversal -- a spilled VGPR and two more spilled SGPRs in every kernel.)
        // Scenes of CRT_WAVE_CULL_MIN ... 64 instances only. Below: the cone and the test cost about 80 VALU instructions per wave
        // (profiles/wave_cull_summary.md: 144 saved with 14 of 16 rejected at 16 each), what five rejected instances save -- a scene of two
        // instances lost 1 % with the test. Above: the scene reaches this loop only as the fallback of the instance tree (CRT_TLAS=0, a lane whose
        // candidates do not fit its list); it takes no wave test and its loops below run over all `cnt` bits. (An opaque copy: the compare's
        // result, hoisted out of the bounce loop, is two more spilled SGPRs in every kernel.)
        bool reject = false;
        // `pre` (kernels that take the root pre-test only; without it no instruction differs from the wave test alone): all ones in a wave that takes
        // the wave test -- the pre-test's loops run in those. An opaque scalar below: as a bool it is a 64-bit lane mask that lives through both cull loops.
        [[maybe_unused]] uint32_t pre = 0u;
        const uint32_t n = cnt;
        uint32_t all = S.numInstances;
        asm volatile("" : "+s"(all));
        if (act == ~0ull && all - CRT_WAVE_CULL_MIN <= 64u - CRT_WAVE_CULL_MIN) {
            if constexpr (CRT_ROOT_PRETESTS(PRETEST)) pre = ~0u;
            v3 dc = d; float ddc = dd; uint32_t lane = rank;
            asm volatile("" : "+v"(dc.x), "+v"(dc.y), "+v"(dc.z), "+v"(ddc), "+v"(lane));
            const WaveCone cone = wave_cone(dc, ddc);
            if (cone_admits(cone) && lane < n) {
                const crt_u32x4 a = rowA[lane]; const crt_u32x2 t = rowB[lane];
                reject = cone_rejects(cone, mk3(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z)), __uint_as_float(a.w), __uint_as_float(t.x), t.y == 0u);
            }
        }
        // `touch`: the instances the wave test leaves. The loops run over its set bits only (a scalar find-first-set per survivor); a bit
        // outside it stays clear in every lane's mask
        const unsigned long long touch = (n == 64u ? ~0ull : (1ull << n) - 1ull) & ~__ballot(reject);
        // (the halves as opaque scalars: `(touch >> 32) != 0` is otherwise compiled as a 64-bit compare, which only the vector unit has -- against
        // a constant in a VGPR pair that then lives through the whole kernel)
        uint32_t touchLo = (uint32_t)touch, touchHi = (uint32_t)(touch >> 32);
        asm volatile("" : "+s"(touchLo), "+s"(touchHi));
        if constexpr (CRT_ROOT_PRETESTS(PRETEST)) asm volatile("" : "+s"(pre));
        for (uint32_t m = touchLo; m != 0u; m &= m - 1u) { const uint32_t k = (uint32_t)__builtin_ctz(m); lo |= culls(k) ? 0u : 1u << k; }
        for (uint32_t m = touchHi; m != 0u; m &= m - 1u) { const uint32_t k = (uint32_t)__builtin_ctz(m); hi |= culls(k + 32u) ? 0u : 1u << k; }
        if constexpr (CRT_ROOT_PRETESTS(PRETEST)) {
            // The root pre-test, (7) above: over the same survivors, in the waves that took the wave test (`pre`; the others have all `cnt` bits in
            // `touch` and keep the path they had). A survivor no lane kept is skipped. The branch is the wave's, not the lanes': every lane computes
            // and a lane without the bit clears nothing -- one compare and a scalar branch instead of a saved and restored exec mask.
            if constexpr (CRT_PRETEST_ENTERS(ENTER)) {
                // (7g): the lane whose lowest remaining bit is `bit`, and which is inside no instance yet, may stay inside this one
                for (uint32_t m = touchLo & pre; m != 0u; m &= m - 1u) {
                    const uint32_t k = (uint32_t)__builtin_ctz(m), bit = 1u << k;
                    if (__ballot((lo & bit) != 0u) != 0) {
                        const bool first = ((lo & (bit | (bit - 1u))) == bit) & !T.active;
                        lo &= root_pretest_enters<DIVIDE>(S, o, d, base + k, best0, first, T, stack) ? ~bit : ~0u;
                    }
                }
                for (uint32_t m = touchHi & pre; m != 0u; m &= m - 1u) {
                    const uint32_t k = (uint32_t)__builtin_ctz(m), bit = 1u << k;
                    if (__ballot((hi & bit) != 0u) != 0) {
                        const bool first = (lo == 0u) & ((hi & (bit | (bit - 1u))) == bit) & !T.active;
                        hi &= root_pretest_enters<DIVIDE>(S, o, d, base + k + 32u, best0, first, T, stack) ? ~bit : ~0u;
                    }
                }
            } else {
            for (uint32_t m = touchLo & pre; m != 0u; m &= m - 1u) {
                const uint32_t k = (uint32_t)__builtin_ctz(m), bit = 1u << k;
                if (__ballot((lo & bit) != 0u) != 0) lo &= root_pretest_misses<DIVIDE>(S, o, d, base + k, best0) ? ~bit : ~0u;
            }
            for (uint32_t m = touchHi & pre; m != 0u; m &= m - 1u) {
                const uint32_t k = (uint32_t)__builtin_ctz(m), bit = 1u << k;
                if (__ballot((hi & bit) != 0u) != 0) hi &= root_pretest_misses<DIVIDE>(S, o, d, base + k + 32u, best0) ? ~bit : ~0u;
            }
            }
        }
    } else {
        const uint32_t nLo = cnt < 32u ? cnt : 32u;
        for (uint32_t k = 0; k < nLo; ++k) lo |= culls(k) ? 0u : 1u << k;
        for (uint32_t k = 32; k < cnt; ++k) hi |= culls(k) ? 0u : 1u << (k - 32u);
    }
    const unsigned long long cand = ((unsigned long long)hi << 32) | lo;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return cand;
}

#ifdef CRT_NO_BOUNCE_PRETEST
#define CRT_BOUNCE_PRETESTS(PRETEST) false  // A/B builds: candidate_mask alone at bounce 1, everywhere
#else
#define CRT_BOUNCE_PRETESTS(PRETEST) (PRETEST)
#endif
// The root pre-test of the reflection bounce (TR_BOUNCE_PRETEST, policy::trace_bounce_pretests; (7) above root_pretest_misses): behind candidate_mask,
// once per instance that some live lane's mask `cand` still holds, every live lane runs root_pretest_misses on its OWN origin and direction and
// clears the bit where it returns true. No cone and no staging: the instance index is wave-uniform, so both records come through the scalar cache,
// and rank == lane is not used, so a wave of any occupancy takes it. Scenes of CRT_WAVE_CULL_MIN ... 64 instances, like the wave test (one chunk:
// base == 0): below, a pre-test costs more than the entries of so few instances save; above, the instance tree serves the scene.
// The shape is staged_candidate_mask's, whose items each moved rows of the ledger when left out: the mask in 32-bit halves, the instance count as an
// opaque scalar in a one-compare guard, the bound as root_pretest_misses' opaque VGPR copy. With it no row moved in any of the six kernels
// (the benchmark kernel: 64 VGPRs, no scratch, 78 SGPRs, 43 spilled, as recorded).
template <bool DIVIDE>
__device__ __forceinline__ unsigned long long bounce_pretest_mask(const CrtDevScene& S, v3 o, v3 d, uint32_t base, uint32_t cnt, unsigned long long cand, float best0)
{
    uint32_t lo = (uint32_t)cand, hi = (uint32_t)(cand >> 32);
    uint32_t all = S.numInstances;
    asm volatile("" : "+s"(all));
    if (all - CRT_WAVE_CULL_MIN <= 64u - CRT_WAVE_CULL_MIN) {
        const uint32_t nLo = cnt < 32u ? cnt : 32u;
        for (uint32_t k = 0; k < nLo; ++k) {
            const uint32_t bit = 1u << k;
            if (__ballot((lo & bit) != 0u) != 0) lo &= root_pretest_misses<DIVIDE>(S, o, d, base + k, best0) ? ~bit : ~0u;
        }
        for (uint32_t k = 32; k < cnt; ++k) {
            const uint32_t bit = 1u << (k - 32u);
            if (__ballot((hi & bit) != 0u) != 0) hi &= root_pretest_misses<DIVIDE>(S, o, d, base + k, best0) ? ~bit : ~0u;
        }
    }
    return ((unsigned long long)hi << 32) | lo;
}

// Candidate instances of one ray from the instance tree: up to CRT_TLAS_LIST indices (16 bits each, unordered, 0xFFFF =
// empty) in four words; returns false when the lane would need more. The traversal stack is idle at this point
// and serves as the tree stack. Scenes with hundreds of instances (upstream allows 401 and loops over all of them for
// every ray, kernel_main.cl:198) spend their time here otherwise: 401 instances, 1920x1080: 1.12 ms -> see DESIGN.md.
// The four words live in the stack's parked LDS slots 0..3 (CrtStackT<PARK >= 4>), not in registers: they are read once per
// instance entry, and as registers they were what the TLAS instantiations spilled to scratch (rounds 1-2: 48 B per lane).
#define CRT_TLAS_PARK (CRT_TLAS_LIST / 2)
template <class STK>
__device__ __forceinline__ bool candidate_list_add(const STK& stack, uint32_t& n, uint32_t idx)
{
    if (n >= (uint32_t)CRT_TLAS_LIST) return false;
    const uint32_t sh = (n & 1u) * 16u, m = ~(0xFFFFu << sh), v = idx << sh;
    const int k = (int)(n >> 1);
    stack.park(k, (stack.parked(k) & m) | v);
    n++;
    return true;
}
// smallest candidate index greater than `after` (after = -1 for the first), or 0xFFFF
template <class STK>
__device__ __forceinline__ uint32_t candidate_list_next(const STK& stack, int after)
{
    uint32_t best = 0xFFFFu;
#pragma unroll
    for (int k = 0; k < CRT_TLAS_PARK; ++k) {
        const uint32_t w = stack.parked(k);
        const uint32_t lo = w & 0xFFFFu, hi = w >> 16;
        if ((int)lo > after && lo < best) best = lo;
        if ((int)hi > after && hi < best) best = hi;
    }
    return best;
}
// fills the parked list; `n` receives the number of candidates
template <class STK>
__device__ __forceinline__ bool tlas_candidates(const CrtDevScene& S, v3 o, v3 d, const STK& stack, uint32_t& n)
{
#pragma unroll
    for (int k = 0; k < CRT_TLAS_PARK; ++k) stack.park(k, 0xFFFFFFFFu);
    n = 0;
    bool ok = true;
    for (uint32_t k = 0; k < S.numAlways; ++k) { const uint32_t i = S.alwaysList[k]; if (i < S.numInstances) ok = candidate_list_add(stack, n, i) && ok; }
    if (S.tlasNodes == 0) return ok;
    const float dd = dot3(d, d);
    uint32_t node = 0; int sp = 0;
    for (;;) {
        const CrtTlasNode nd = S.tlas[node];
        bool descend = false;
        if (!sphere_culls(nd.sphere, o, d, dd)) {
            // children: a leaf child is tested through its own sphere when it is popped as a one-node subtree
            if (nd.left & CRT_TLAS_LEAF) {
                const uint32_t i = nd.left & 0xFFFFu;             // a leaf NODE: left = leaf | instance, right unused
                if (i < S.numInstances) ok = candidate_list_add(stack, n, i) && ok;
            } else { stack.write(sp, nd.right); sp++; node = nd.left; descend = true; }
        }
        if (!descend) { if (sp == 0) break; --sp; node = stack.read(sp); }
    }
    return ok;
}

// Closest hit of one ray per lane over all instances (kernel_main.cl:198-217), driven in flat trips: every lane owns a
// Traversal and a trip of the wave's loop is  enter -> inner -> leaf -> inner  for whichever lanes are at that step (a lane
// may enter an instance, visit a node and test a leaf in the same trip; a lane that popped an inner node out of a leaf or a
// miss goes on at once). One ballot per trip decides when the wave is done. (Rounds 1-2 voted for ONE step kind per trip in
// packets with many working lanes -- three ballots, popcounts and the majority logic; at 8 waves/SIMD that lost 6 % and
// the second inner step gained another 10 %; the voted form was retired in round 3.)
// ANYHIT (shadow rays, CRT_RENDER_SHADOWS): a lane stops at the first triangle that passes -- inside the leaf, and
// for all later instances. `anyHit` is the same boolean the full closest-hit loop would return, because until the
// first passing triangle both visit the same nodes in the same order; only the work (and the counters) shrink.
// ITERS (stamped diagnostic launches): the counters record wave-level trips instead of per-ray work.
// OPTS (TR_*): the trip's options -- its traversal's, except that a trip may leave the stamps out (closest_hit's instance-tree path).
template <unsigned OPTS, unsigned OWNER, class STK>
__device__ __forceinline__ void trip_steps(const CrtDevScene& S, const STK& stack, Traversal<OWNER>& T, Closest& c, LaneCounters& lc, bool done)
{
    static_assert((OPTS & ~TR_ALL) == 0u && ((OPTS ^ OWNER) & ~TR_ITERS) == 0u, "a trip runs under its traversal's options");
    constexpr bool ITERS = has_opt(OPTS, TR_ITERS);
    if (!done && T.at_inner()) {
        if (ITERS) { lc.rays++; if (first_active_lane()) lc.innerVisits++; }
        T.template inner<OPTS>(S, stack, c, lc);
    }
    if (!done && T.at_leaf()) {
        if (ITERS) {
            if (first_active_lane()) lc.triTests++;
            // wave-level triangle iterations of this leaf step = the largest count among the lanes taking it (3 vector loads each)
            uint32_t n = (T.ref >> 24) & 0x7Fu; if (n == 0) n = S.bigLeaf[T.ref & 0x00FFFFFFu];
            for (int off = 32; off > 0; off >>= 1) { const uint32_t o2 = (uint32_t)__shfl_xor((int)n, off, 64); n = o2 > n ? o2 : n; }
            if (first_active_lane()) lc.misses += n;
        }
        T.template leaf<OPTS>(S, stack, c, lc);
    }
    if (!done && T.at_inner()) {
        if (ITERS) { if (first_active_lane()) lc.hits++; }
        T.template inner<OPTS>(S, stack, c, lc);           // lanes that just popped an inner node go on at once
    }
}

// best0 (ray queries with a distance bound, crt_rays_kernel): the "closest so far" the loop starts with instead of upstream's 99999 --
// nothing else changes, `t < out.t` and `tnear < minSoFar` do the rest (a NaN bound fails both: every ray a miss).
// chunkedOnly (TLAS only, wave-uniform): take the chunked candidate loop although an instance tree exists -- what a wave of the TLAS
// instantiation does anyway when a lane's candidates do not fit its list; crt_rays_kernel forces it for a wave with an origin beyond
// the cull's proven range, whose scene then has the all-never bounds table. Both are defaulted and constant for every other caller.
// OPTS: the TR_* options, by name (COUNT ... DIVIDE below are their bits).
// INCLUSIVE (the device queries only): intersect_aabb's rule for every box test, threaded down through trip_steps and Traversal::inner in the
// trip's options -- no run-time branch in a step; the instance cull stays on (sphere_culls' derivation, "Inclusive pass").
// STAGE (policy::trace_stages_cull) + sharedOrigin (wave-uniform, run time: the camera bounce): the
// chunk's mask comes from staged_candidate_mask -- the same mask, bit for bit. A run-time value, not a second instantiation: the trip
// loop below exists once per kernel. With TR_BOUNCE_PRETEST the other bounce (sharedOrigin false) passes candidate_mask's mask through
// bounce_pretest_mask, which clears the instances the lane's ray would leave at their root.
template <unsigned OPTS, class STK>
__device__ __forceinline__ Closest closest_hit(const CrtDevScene& S, v3 o, v3 d, const STK& stack, LaneCounters& lc, float best0 = 99999.0f,
                                               bool chunkedOnly = false, bool sharedOrigin = false)
{
    constexpr bool COUNT = has_opt(OPTS, TR_COUNT), ITERS = has_opt(OPTS, TR_ITERS), ANYHIT = has_opt(OPTS, TR_ANYHIT), TLAS = has_opt(OPTS, TR_TLAS),
                   STAGE = has_opt(OPTS, TR_STAGE);
    static_assert((OPTS & ~TR_ALL) == 0u, "unknown traversal option");
    static_assert(!STAGE || (!COUNT && !ITERS && !ANYHIT && !TLAS && !STK::kTop), "staged cull terms: uncounted closest-hit traversals of one-wave workgroups");
    static_assert(STAGE || !has_opt(OPTS, TR_WAVE_CULL), "the wave test lives in the staged cull");
    static_assert(has_opt(OPTS, TR_WAVE_CULL) || !has_opt(OPTS, TR_ROOT_PRETEST), "the root pre-test runs over the wave test's survivors");
    static_assert(has_opt(OPTS, TR_ROOT_PRETEST) || !has_opt(OPTS, TR_BOUNCE_PRETEST), "the reflection bounce's pre-test: kernels that take the camera bounce's");
    static_assert(has_opt(OPTS, TR_ROOT_PRETEST) || !has_opt(OPTS, TR_PRETEST_ENTRY), "the entry is made by the camera bounce's pre-test");
    Closest c = no_hit(best0);
    Traversal<OPTS> T; T.reset();

    if constexpr (TLAS) {
        // Many instances: every lane collects its (few) candidates from the instance tree and walks them in ascending
        // order -- the same instances, in the same order, as the chunked loop below would. A wave in which some lane
        // has more than CRT_TLAS_LIST candidates takes the chunked loop instead.
        static_assert(!TLAS || STK::kLds <= CRT_LDS_SLOTS - CRT_TLAS_PARK, "the candidate list needs CRT_TLAS_PARK parked slots");
        uint32_t listed = 0;
        const bool fits = !chunkedOnly && tlas_candidates(S, o, d, stack, listed);    // (chunkedOnly: no lane "fits", the wave takes the loop below)
        if (__ballot(!fits) == 0) {
            int prev = -1;                                        // last instance entered (ANYHIT + COUNT: culled ones in between)
            if (COUNT && !ANYHIT) { const uint32_t culled = S.numInstances - listed; count_culled(lc, culled); }
            bool done = false;
            for (;;) {
                const bool wEnter = !done && !T.active;
                const bool wInner = !done && T.at_inner();
                const bool wLeaf = !done && T.at_leaf();
                if (__ballot(wEnter || wInner || wLeaf) == 0) break;      // (this exact form: `__ballot(!done)` makes the register allocator spill 30 VGPRs)
                if (wEnter) {
                    const uint32_t k = (ANYHIT && c.anyHit) ? 0xFFFFu : candidate_list_next(stack, prev);
                    if (k == 0xFFFFu) {
                        done = true;
                        if (COUNT && ANYHIT && !c.anyHit) { const uint32_t n = S.numInstances - (uint32_t)(prev + 1); count_culled(lc, n); }
                    } else {
                        if (COUNT && ANYHIT) { const uint32_t n = k - (uint32_t)(prev + 1); count_culled(lc, n); }
                        prev = (int)k;
                        T.template enter<STK::kTop>(S, k, o, d, c.distance, lc);
                    }
                }
                trip_steps<OPTS & ~TR_ITERS>(S, stack, T, c, lc, done);      // (this path records no wave-level trips)
            }
            return c;
        }
    }

    for (uint32_t base = 0; base < S.numInstances; base += 64) {
        const uint32_t cnt = (S.numInstances - base) < 64u ? (S.numInstances - base) : 64u;
        unsigned long long cand;
        if constexpr (STAGE && CRT_BOUNCE_PRETESTS(has_opt(OPTS, TR_BOUNCE_PRETEST))) {
            if (sharedOrigin) cand = staged_candidate_mask<has_opt(OPTS, TR_WAVE_CULL), has_opt(OPTS, TR_ROOT_PRETEST), has_opt(OPTS, TR_DIVIDE), has_opt(OPTS, TR_PRETEST_ENTRY)>(S, o, d, base, cnt, stack, best0, T);
            else cand = bounce_pretest_mask<has_opt(OPTS, TR_DIVIDE)>(S, o, d, base, cnt, candidate_mask(S, o, d, base, cnt, lc), best0);
        } else if constexpr (STAGE) cand = sharedOrigin ? staged_candidate_mask<has_opt(OPTS, TR_WAVE_CULL), has_opt(OPTS, TR_ROOT_PRETEST), has_opt(OPTS, TR_DIVIDE), has_opt(OPTS, TR_PRETEST_ENTRY)>(S, o, d, base, cnt, stack, best0, T)
                                                 : candidate_mask(S, o, d, base, cnt, lc);
        else cand = candidate_mask<opt_if(COUNT, CM_COUNT) | opt_if(ANYHIT, CM_DEFER_COUNT)>(S, o, d, base, cnt, lc);
        // ANYHIT + COUNT: a culled instance is only "visited" (one pop, one inner visit upstream) if the ray gets that
        // far, so culled instances are counted when a later candidate is entered or the chunk ends without a hit
        unsigned long long culledLeft = (COUNT && ANYHIT) ? (~cand & (cnt == 64u ? ~0ull : ((1ull << cnt) - 1ull))) : 0ull;
        bool done = ANYHIT && c.anyHit;
        for (;;) {
            const bool wEnter = !done && !T.active;
            const bool wInner = !done && T.at_inner();
            const bool wLeaf = !done && T.at_leaf();
            if (__ballot(wEnter || wInner || wLeaf) == 0) break;
            if (ITERS) { if (first_active_lane()) lc.pops++; }
            if (wEnter) {
                if (ANYHIT && c.anyHit) done = true;           // occluded: later instances are never visited
                else if (cand == 0) {                          // this lane is finished with the chunk
                    done = true;
                    if (COUNT && ANYHIT) { const uint32_t n = (uint32_t)__popcll(culledLeft); count_culled(lc, n); culledLeft = 0; }
                } else {
                    if (ITERS) { if (first_active_lane()) lc.traversals++; }
                    const uint32_t k = (uint32_t)__ffsll((long long)cand) - 1u;
                    cand &= cand - 1;
                    if (COUNT && ANYHIT) {
                        const unsigned long long below = culledLeft & ((1ull << k) - 1ull);
                        const uint32_t n = (uint32_t)__popcll(below);
                        count_culled(lc, n); culledLeft &= ~below;
                    }
                    T.template enter<STK::kTop>(S, base + k, o, d, c.distance, lc);
                }
            }
            trip_steps<OPTS>(S, stack, T, c, lc, done);
        }
    }
    return c;
}

__device__ __forceinline__ int clamp_texel(int idx, int n) { return idx < 0 ? 0 : (idx >= n ? n - 1 : idx); }

// MathAndSTL.cl:253-258 (hard-wired to textures[2] and pool offset 2 upstream, hazard H9)
// Out of line on purpose: the double-precision atan2/acos expansion needs ~60 VGPRs of temporaries; inlined
// into the persistent kernel it forced the per-lane traversal state into scratch inside the hot loop.
__device__ __noinline__ int sample_skybox(v3 d, int texW, int texH)
{
    const double PI = 3.14159265358979323846;
    float at = (float)(atan2((double)d.x, (double)(-d.z)) / PI);
    float ac = (float)(acos((double)d.y) / PI);
    int theta = f2i((at * 0.5f) * (float)texW);
    int phi = f2i(ac * (float)texH);
    return (int)((uint32_t)phi * (uint32_t)texW + (uint32_t)(theta + 2));
}

// ------------------------------------------------------------------------------------------------
// The same index decided in single precision where that is provably safe (sample_skybox_guarded); sample_skybox above stays the
// definition and serves every lane the float decision leaves open. No claim that a float function equals the double one: the float
// values only have to land in the same texel, and a lane whose value comes near a texel edge is not decided by them.
//  1. at~ (sky_index_float): q = min(|x|, |z|) / max(|x|, |z|), p = q * A(q * q) with A of degree 8 fitted to atan(q) / (pi q) on [0, 1],
//     then the octant fix-ups 0.5 - p (|x| > |z|), 1 - a (-z < 0), -a (x < 0). ac~: c = sqrt(1 - |y|) * C(|y|) with C of degree 7 fitted to
//     acos(t) / (pi sqrt(1 - t)) on [0, 1], then 1 - c (y < 0). Only IEEE single-precision + - * / sqrt, compares and selects, each written
//     as one operation (the library is built with -ffp-contract=off): tests/sky_fast_ref.py (numpy) and tools/sky_index_bounds.c (C)
//     restate the sequence and get the device's bits.
//  2. E_c = max |ac~ - acos(y) / pi| over ALL float y with CRT_SKY_MIN_COMPONENT <= |y| < 1 (every other pattern is never decided, 5.),
//     E_p = max |p - atan(q) / pi| over EVERY float q in [0, 1], both against glibc's double functions: tools/sky_index_bounds.c,
//     recorded in profiles/sky_index_bounds.txt (E_p = 5.08e-8, E_c = 9.85e-8). p is taken at the rounded q: the true quotient is within
//     2^-25 of it (q <= 1) and atan' <= 1, so 2^-24 / pi covers the division generously; each of the two fix-up subtractions rounds by at
//     most 2^-25 (results <= 1). E_a = E_p + 2^-24 / pi + 2 * 2^-25.
//  3. The definition's own roundings: (float) of the double quotient moves at, ac by at most 2^-25 (|at|, |ac| <= 1); two correct double
//     libraries differ by a few 1e-16 before that (1e-15 taken). at * 0.5f is exact; the product with (float)texW rounds by at most half
//     an ulp of a value of magnitude <= texW / 2, that is (texW / 2) 2^-24 -- once in the definition, once in the float form; the same with
//     texH for phi.
//  4. So with T the real-number value atan2(x, -z) / pi * texW / 2: |s_def - T| <= (texW / 2)(2^-25 + 1e-15 + 2^-24) and
//     |s - T| <= (texW / 2)(E_a + 2^-24). If no integer lies within mW = (texW / 2) K_a of s, K_a = E_a + 2^-25 + 2^-23 + 1e-15, s and s_def
//     lie strictly between the same two integers, and truncation towards zero -- whose only steps are at integers -- gives the same theta.
//     Likewise mH = texH K_c, K_c = E_c + 2^-25 + 2^-23 + 1e-15, for phi (K_a = 2.784e-7, K_c = 2.475e-7). CRT_SKY_KA and CRT_SKY_KC are K_a and K_c times the
//     safety factor 1.25, rounded up (the factor also covers the rounding of the float products that form mW and mH); a larger factor only sends more
//     lanes to the double form.
//  5. A lane is decided iff |s - rint(s)| > mW and |sv - rint(sv)| > mH, |s| and sv are below CRT_SKY_MAX_SCALED (2^22: rint, the difference
//     and (int) are exact there), min(|x|, |z|) and |y| are at least CRT_SKY_MIN_COMPONENT (the smallest normal: zeros and denormals out),
//     max(|x|, |z|) is at most CRT_SKY_MAX_COMPONENT (infinities out) and |y| < 1. Every compare is written so that a NaN fails it.
//     Never decided, then: NaN, infinite, zero and denormal components, d.y in {0, +-1}, |d.y| > 1, texW or texH = 0 -- the arguments at
//     which the definition returns special values -- and every value within the margin of a texel edge.
//  6. The decision is taken for the wave, like recip's: if any lane of the call is undecided, those lanes, and only those, run the double
//     form; otherwise it is a block the wave jumps over with one not-taken branch.
// SKY_DOUBLE (shade_bounce's SB_SKY_DOUBLE): the double form alone, no float decision -- the kernels of policy's "who keeps the double-only
// skybox index" above, and everything under -DCRT_SKY_DOUBLE (A/B builds). tools/ubench/sky_index checks all of this on the device.
// ------------------------------------------------------------------------------------------------
#ifdef CRT_SKY_DOUBLE
#define CRT_SKY_IS_DOUBLE(SKY_DOUBLE) true
#else
#define CRT_SKY_IS_DOUBLE(SKY_DOUBLE) (SKY_DOUBLE)
#endif
#define CRT_SKY_A0 3.183098733e-01f
#define CRT_SKY_A1 -1.061023548e-01f
#define CRT_SKY_A2 6.363610178e-02f
#define CRT_SKY_A3 -4.519299418e-02f
#define CRT_SKY_A4 3.379932418e-02f
#define CRT_SKY_A5 -2.373590693e-02f
#define CRT_SKY_A6 1.341282204e-02f
#define CRT_SKY_A7 -5.007412285e-03f
#define CRT_SKY_A8 8.805354009e-04f
#define CRT_SKY_C0 5.000000000e-01f
#define CRT_SKY_C1 -6.830871105e-02f
#define CRT_SKY_C2 2.831966616e-02f
#define CRT_SKY_C3 -1.595187746e-02f
#define CRT_SKY_C4 9.779155254e-03f
#define CRT_SKY_C5 -5.360673647e-03f
#define CRT_SKY_C6 2.066315385e-03f
#define CRT_SKY_C7 -3.857081174e-04f
#define CRT_SKY_KA 3.48e-07f
#define CRT_SKY_KC 3.10e-07f
#define CRT_SKY_MIN_COMPONENT 1.17549435e-38f
#define CRT_SKY_MAX_COMPONENT 3.40282347e+38f
#define CRT_SKY_MAX_SCALED 4194304.0f
// the float decision of one lane: theta and phi are the definition's iff it returns true (1.-5. above)
__device__ __forceinline__ bool sky_index_float(v3 d, int texW, int texH, int& theta, int& phi)
{
    const float fW = (float)texW, fH = (float)texH;
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    const bool steep = ax > az;
    const float mn = steep ? az : ax, mx = steep ? ax : az;
    const float q = mn / mx;
    const float u = q * q;
    float p = CRT_SKY_A8;
    p = p * u; p = p + CRT_SKY_A7;
    p = p * u; p = p + CRT_SKY_A6;
    p = p * u; p = p + CRT_SKY_A5;
    p = p * u; p = p + CRT_SKY_A4;
    p = p * u; p = p + CRT_SKY_A3;
    p = p * u; p = p + CRT_SKY_A2;
    p = p * u; p = p + CRT_SKY_A1;
    p = p * u; p = p + CRT_SKY_A0;
    p = p * q;
    float a = steep ? 0.5f - p : p;
    a = d.z > 0.0f ? 1.0f - a : a;
    a = d.x < 0.0f ? -a : a;
    const float r = __builtin_sqrtf(1.0f - ay);
    float c = CRT_SKY_C7;
    c = c * ay; c = c + CRT_SKY_C6;
    c = c * ay; c = c + CRT_SKY_C5;
    c = c * ay; c = c + CRT_SKY_C4;
    c = c * ay; c = c + CRT_SKY_C3;
    c = c * ay; c = c + CRT_SKY_C2;
    c = c * ay; c = c + CRT_SKY_C1;
    c = c * ay; c = c + CRT_SKY_C0;
    c = c * r;
    c = d.y < 0.0f ? 1.0f - c : c;
    const float s = (a * 0.5f) * fW, sv = c * fH;
    const float es = fabsf(s - __builtin_rintf(s)), ev = fabsf(sv - __builtin_rintf(sv));
    const float mW = CRT_SKY_KA * fabsf(0.5f * fW), mH = CRT_SKY_KC * fabsf(fH);      // |texW|, |texH|: 4. holds for either sign
    theta = (int)s;
    phi = (int)sv;
    return es > mW && ev > mH && fabsf(s) < CRT_SKY_MAX_SCALED && sv < CRT_SKY_MAX_SCALED
        && mn >= CRT_SKY_MIN_COMPONENT && mx <= CRT_SKY_MAX_COMPONENT && ay >= CRT_SKY_MIN_COMPONENT && ay < 1.0f;
}
// Out of line like sample_skybox, whose body it holds a second time behind the wave's decision (a call from here would make this a
// function with a frame of its own).
__device__ __noinline__ int sample_skybox_guarded(v3 d, int texW, int texH)
{
    int theta, phi;
    const bool decided = sky_index_float(d, texW, texH, theta, phi);
    int idx = (int)((uint32_t)phi * (uint32_t)texW + (uint32_t)(theta + 2));
    if (__builtin_expect(__ballot(!decided) != 0, 0)) {
        if (!decided) {
            const double PI = 3.14159265358979323846;
            float at = (float)(atan2((double)d.x, (double)(-d.z)) / PI);
            float ac = (float)(acos((double)d.y) / PI);
            idx = (int)((uint32_t)f2i(ac * (float)texH) * (uint32_t)texW + (uint32_t)(f2i((at * 0.5f) * (float)texW) + 2));
        }
    }
    return idx;
}
template <bool SKY_DOUBLE>
__device__ __forceinline__ int sky_index(v3 d, int texW, int texH)
{
    if constexpr (CRT_SKY_IS_DOUBLE(SKY_DOUBLE)) return sample_skybox(d, texW, texH);
    else return sample_skybox_guarded(d, texW, texH);
}

// MathAndSTL.cl:260-266
__device__ __forceinline__ int sample_texture(const CrtTexture& tex, float u, float v)
{
    u = u - floorf(u);
    v = v - floorf(v);
    int uS = f2i((float)tex.width * u);
    int vS = f2i((float)tex.height * v);
    return (int)((uint32_t)vS * (uint32_t)tex.width + (uint32_t)tex.offset + (uint32_t)uS);
}

// kernel_main.cl:277-287
__device__ __forceinline__ v3 raygen_dir(const CrtFrame& F, int i, int j, int width, int height)
{
    float cx = (float)i / (float)width, cy = (float)j / (float)height;
    cx = cx * 2.0f - 1.0f;
    cy = cy * 2.0f - 1.0f;
    v3 t = matmul_xyz(F.invProj, cx, cy, 1.0f, 1.0f);
    float w = matmul_w(F.invProj, cx, cy, 1.0f, 1.0f);
    float tx = t.x / w, ty = t.y / w, tz = t.z / w, tw = w / w;
    v3 wv = matmul_xyz(F.invView, tx, ty, tz, tw);
    return normalize3(wv);
}

__device__ __forceinline__ v3 raygen_dir(const CrtFrame& F, int i, int j) { return raygen_dir(F, i, j, F.width, F.height); }

// One bounce of kernel_main.cl:187-272 after the closest hit is known. Returns false when the
// path terminated (miss -> skybox). On a hit, updates ray/energy/atmospheric/lightDir in place.
// Per-path state carried across the two bounces (kernel_main.cl:179-187). Upstream also carries
//   energy (float3): starts (1,1,1) and is only ever multiplied by a splat (kernel_main.cl:264,268) -> one float;
//   atmosphericLight: (0.255,0.25,0.27)*1 at bounce 0, that * 0.4 at bounce 1 (kernel_main.cl:185,269) -> from `bounce`;
//   lightDir: the sun at bounce 0, the bounce ray's direction at bounce 1 (kernel_main.cl:181,271) -> from `bounce`.
struct PathState { v3 o, d, result; float energy; };
// a path at the camera (kernel_main.cl:179-185), direction `d` (raygen_dir of its pixel)
__device__ __forceinline__ PathState camera_path(const CrtFrame& F, v3 d)
{
    PathState ps;
    ps.o = mk3(F.camPos[0], F.camPos[1], F.camPos[2]);
    ps.d = d;
    ps.result = mk3(0.0f, 0.0f, 0.0f);
    ps.energy = 1.0f;
    return ps;
}

// kernel_main.cl:264: specular = ((1 - roughness) * ndl * shadow) * specularColor * ndl, x component (a splat)
__device__ __forceinline__ float specular_x(float ndl, float shadow)
{
    const float sp = ((1.0f - 0.5f) * ndl) * shadow;
    return (sp * 0.2f) * ndl;
}

// DEFER_ENERGY (CRT_RENDER_SHADOWS): leave `energy *= specular` to the caller, which first traces the shadow ray
// from the new ray origin; `ndlOut` receives the clamped n.l that decides whether the shadow factor is observable.
// REFRACT (CRT_RENDER_REFRACTION, an extension defined by the oracle, oracle/crt_oracle.h): at the first hit of a material
// whose opacity (MTL `d`, kept in Material::roughness) is below 1 the continuing ray is the refracted one (Snell, index
// 1.5; total internal reflection keeps the reflection), 0.01 behind the surface, with (1 - opacity) of the energy.
// Returns 0: path ended (miss -> skybox); 1: continues with the reflected ray; 2: continues with the transmitted ray
// (energy already applied, no shadow ray wanted).
// SINK (CRT_RENDER_GBUFFER: GBufferSink, crt_kernels.h; NoSink: nothing): at bounce 0 `sink` is handed what the primary ray found
// where it is in registers anyway -- sink->miss(c) before the skybox lookup, sink->hit(c, record.normal, the bytes of record.color)
// (kernel_main.cl:236,245) behind the texture fetch -- so that nothing of it has to stay alive through the second traversal.
// A sink that also wants what only this function knows of the hit -- the material index as clamped below (kernel_main.cl:229) and the
// interpolated uv before SampleTexture's fract (kernel_main.cl:238-240) -- provides hit(c, normal, albedo, material, texU, texV) as well
// (SurfaceSink, crt_shade.h); GBufferSink does not and is called as before.
struct NoSink { };
template <class SINK, class = void> struct SinkTakesSurface : std::false_type { };
template <class SINK>
struct SinkTakesSurface<SINK, std::void_t<decltype(std::declval<const SINK&>().hit(std::declval<const Closest&>(), v3(), 0u, 0u, 0.0f, 0.0f))>> : std::true_type { };
// SKY_DOUBLE: the skybox index in its double form alone (sample_skybox; see sample_skybox_guarded)
// OPTS: the SB_* options, by name (DEFER_ENERGY, REFRACT, SKY_DOUBLE are their bits); SINK is deduced from `sink`.
template <unsigned OPTS = 0u, class SINK = NoSink>
__device__ __forceinline__ int shade_bounce(const CrtDevScene& S, const Closest& c, PathState& ps, int bounce, float lightY, float lightZ,
                                            float* ndlOut = nullptr, const SINK* sink = nullptr)
{
    static_assert((OPTS & ~SB_ALL) == 0u, "unknown shading option");
    constexpr bool DEFER_ENERGY = has_opt(OPTS, SB_DEFER_ENERGY), REFRACT = has_opt(OPTS, SB_REFRACT), SKY_DOUBLE = has_opt(OPTS, SB_SKY_DOUBLE),
                   OFFSET32 = has_opt(OPTS, SB_OFFSET32);
    constexpr bool kSink = !std::is_same<SINK, NoSink>::value;
    const float UcharToFloat01 = 1.0f / 255.0f;
    if (c.distance > 99998.0f) {
        if constexpr (kSink) { if (bounce == 0) sink->miss(c); }
        // textures[2] for every lane: a scalar load (constant address space, see crt_const_f32x4_ptr)
        const crt_f32x4 skyHdr = ((crt_const_f32x4_ptr)S.textures)[2];
        int idx = clamp_texel(sky_index<SKY_DOUBLE>(ps.d, __float_as_int(skyHdr.x), __float_as_int(skyHdr.y)), S.numTexels);
        uint32_t px = S.texels[idx];
        v3 skyc = scale3(mk3((float)(px & 0xffu), (float)((px >> 8) & 0xffu), (float)((px >> 16) & 0xffu)), UcharToFloat01);
        ps.result = add3(ps.result, scale3(skyc, ps.energy));
        return 0;
    }
    const v3 light = bounce == 0 ? mk3(0.0f, lightY, lightZ) : ps.d;     // lightDir = ray.direction after the first bounce
    const v3 atm0 = scale3(mk3(0.255f, 0.25f, 0.27f), 1.0f);
    const v3 atm = bounce == 0 ? atm0 : scale3(atm0, 0.4f);
    const CrtDevInstance I = load_instance<OFFSET32>(S.devInstances, (uint32_t)c.hitInstance);
    // meshRay of the winning instance, recomputed with the same arithmetic as in the loop
    const v3 mo = xform_xyz(I, ps.o.x, ps.o.y, ps.o.z, 1.0f);
    const v3 md = xform_xyz(I, ps.d.x, ps.d.y, ps.d.z, 0.0f);

    const uint4* cold = tri_cold_record<OFFSET32>(S, c.hit.tri);
    const uint4 c0 = cold[0], c1 = cold[1];
    // c0 = {uv0x|uv0y, uv1x|uv1y, uv2x|uv2y, mat|n0x}; c1 = {n0y|n0z, n1x|n1y, n1z|n2x, n2y|n2z}
    const uint32_t matIndex = c0.w & 0xffffu;
    uint32_t mi = __float_as_uint(I.r1.w) + matIndex;
    mi = mi < (uint32_t)CRT_MAX_MATERIALS ? mi : (uint32_t)CRT_MAX_MATERIALS - 1;
    const CrtMaterial mat = S.materials[mi];
    const float bx = (1.0f - c.hit.u) - c.hit.v, by = c.hit.u, bz = c.hit.v;

    const v3 n0 = mat3mul(I, mk3(h2f(c0.w >> 16), h2f(c1.x & 0xffffu), h2f(c1.x >> 16)));
    const v3 n1 = mat3mul(I, mk3(h2f(c1.y & 0xffffu), h2f(c1.y >> 16), h2f(c1.z & 0xffffu)));
    const v3 n2 = mat3mul(I, mk3(h2f(c1.z >> 16), h2f(c1.w & 0xffffu), h2f(c1.w >> 16)));
    const v3 normal = normalize3(add3(add3(scale3(n0, bx), scale3(n1, by)), scale3(n2, bz)));

    const float uvx = (h2f(c0.x & 0xffffu) * bx + h2f(c0.y & 0xffffu) * by) + h2f(c0.z & 0xffffu) * bz;
    const float uvy = (h2f(c0.x >> 16) * bx + h2f(c0.y >> 16) * by) + h2f(c0.z >> 16) * bz;

    uint32_t ti = mat.albedoTextureIndex;
    ti = ti < (uint32_t)CRT_MAX_TEXTURES ? ti : (uint32_t)CRT_MAX_TEXTURES - 1;
    const CrtTexture tex = S.textures[ti];
    const uint32_t px = S.texels[clamp_texel(sample_texture(tex, uvx, uvy), S.numTexels)];
    // the specular texel (kernel_main.cl:243) is fetched upstream but never used: not fetched here
    const uint32_t a = mat.color;
    const uint32_t cr = (((a & 0xffu) * (px & 0xffu)) >> 8) & 0xffu;
    const uint32_t cg = ((((a >> 8) & 0xffu) * ((px >> 8) & 0xffu)) >> 8) & 0xffu;
    const uint32_t cb = ((((a >> 16) & 0xffu) * ((px >> 16) & 0xffu)) >> 8) & 0xffu;
    const v3 color = scale3(mk3((float)cr, (float)cg, (float)cb), UcharToFloat01);
    if constexpr (kSink) {
        if (bounce == 0) {
            if constexpr (SinkTakesSurface<SINK>::value) sink->hit(c, normal, 0xFF000000u | (cb << 16) | (cg << 8) | cr, mi, uvx, uvy);
            else sink->hit(c, normal, 0xFF000000u | (cb << 16) | (cg << 8) | cr);
        }
    }
    const v3 point = add3(mo, scale3(md, c.hit.t));


    bool transmitted = false;
    float opacity = 1.0f;
    if (REFRACT) {
        if (bounce == 0) {
            opacity = h2f(mat.roughness);
            if (opacity < 1.0f) {
                const float dn = dot3(normal, ps.d);
                const bool entering = dn < 0.0f;
                const v3 nf = entering ? normal : neg3(normal);
                const float cosi = entering ? (0.0f - dn) : dn;
                const float eta = entering ? 0.6666667f : 1.5f;
                const float k = 1.0f - (eta * eta) * (1.0f - cosi * cosi);
                if (k >= 0.0f) {
                    const float w = eta * cosi - sqrtf(k);
                    const v3 refr = add3(scale3(ps.d, eta), scale3(nf, w));
                    ps.o = sub3(point, scale3(nf, 0.01f));
                    ps.d = refr;
                    transmitted = true;
                }
            }
        }
    }
    if (!transmitted) {
        ps.o = add3(point, scale3(normal, 0.01f));
        ps.d = reflect3(ps.d, normal);
    }

    float ndl = dot3(normal, neg3(light));
    const v3 ambient = mul3(scale3(atm, fmaxf(0.0f - ndl, 0.1f)), color);
    ndl = fmaxf(ndl, 0.0f);
    // pow(x, shininess) with shininess == 1.0f (kernel_main.cl:250) is exactly x
    const float sl = (ndl * fmaxf(dot3(reflect3(neg3(light), normal), md), 0.0f)) * 0.2f;

    ps.result = add3(ps.result, add3(add3(scale3(scale3(color, ndl), ps.energy), ambient), mk3(sl, sl, sl)));
    if (REFRACT && transmitted) { ps.energy = ps.energy * (1.0f - opacity); return 2; }
    if (DEFER_ENERGY) *ndlOut = ndl;
    else ps.energy = ps.energy * specular_x(ndl, 1.0f);      // shadow = 1.0f (kernel_main.cl:258: no shadow ray upstream)
    return 1;
}
