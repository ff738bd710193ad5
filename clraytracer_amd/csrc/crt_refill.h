// crt_refill.h -- Trace with IN-TILE LANE REFILL (round 5; CRT_KERNEL=refill): north_star's "wavefront ballot / compaction used to
// keep ray packets coherent", applied inside the wave instead of across waves.
//
// The default megakernel (crt_kernels.h) gives a wave one 8x8 tile and one pixel per lane: a lane whose path ends early (sky after
// the instance cull, a short traversal, a bounce ray that leaves the scene) idles until the slowest lane of the tile is done --
// 28 of 64 lanes work per vector-memory instruction on multi-1M (profiles/r04_summary.md, valu.lane_utilisation 0.442). The two
// compaction forms measured before both lost coherence: `persistent` (r1) refilled lanes from OTHER tiles, `wavefront` regroups
// rays across waves through memory (two tails, atomics, arrival order). Here a wave owns a BLOCK of CRT_REFILL_TILES 8x8 tiles
// side by side (16x8 pixels by default, Morton order inside each tile) and a lane whose path has ended takes the block's next
// pixel: one ballot of the lanes that want a pixel, their rank from mbcnt, a cursor in an SGPR. No memory traffic, no
// synchronisation between waves, and every ray of the wave stays within 16 pixels of the others.
//
// Per ray nothing changes -- the same RayGen, instance order, node visits, triangle tests, shading arithmetic as the megakernel
// (kernel_main.cl:164-287), so frames and work counters are bit-identical; what changes is which rays share a wave-level
// instruction. Shading (kernel_main.cl:219-272) moves INTO the traversal loop as a "service step": lanes whose ray is finished
// wait until CRT_REFILL_BATCH of them have gathered (or until they outnumber half the lanes still traversing), then shade
// together, start their bounce ray or store their pixel and draw the next one. The pixel index (and the bounce number in bit 31)
// and the path's energy wait in parked LDS slots (CrtStackT<2>), so the kernel carries no more registers across the traversal than the megakernel does.
//
// Limits: up to 64 instances (one candidate mask), no shadow rays / refraction / instance tree: those frames take the megakernel.
#pragma once
#include "crt_kernels.h"

#ifndef CRT_REFILL_TILES
#define CRT_REFILL_TILES 2        // 8x8 tiles per block, side by side
#endif
#ifndef CRT_REFILL_BATCH
#define CRT_REFILL_BATCH 32       // finished rays that gather before a service step is run for them
#endif
#ifndef CRT_REFILL_RATIO
#define CRT_REFILL_RATIO 1         // ... or when RATIO x (finished lanes) outnumber the lanes still traversing
#endif
#define CRT_REFILL_PIXELS (64 * CRT_REFILL_TILES)

// Block of workgroup `b`: the launch's CrtFrame counts BLOCKS where the megakernel's counts tiles (tilesX = blocks per tile row,
// slotsPerXcd, gridBlocks, the launch lists and the per-slot costs), so deal_tile -- block b on XCD b % 8, XCD x owning
// the tile rows k with k % 8 == x, heaviest first when a feedback list exists -- carries over unchanged. Wave-uniform.
__device__ __forceinline__ bool refill_block(const CrtFrame& F, int b, int& tx0, int& tileRow, int& costSlot, int tiles = CRT_REFILL_TILES)
{
    int bx = 0, quadrant;
    const bool dealt = deal_tile(F, b, bx, tileRow, quadrant, &costSlot);
    tx0 = bx * tiles;
    return dealt;
}

// pixel p of the block: tile p / 64, Morton position p % 64 inside it
__device__ __forceinline__ void refill_pixel(int tx0, int tileRow, uint32_t p, int& px, int& py) { tile_pixel(tx0 + (int)(p >> 6), tileRow, (int)(p & 63u), px, py); }

// STAMP (diagnostic, CRT_RENDER_STAMPS): per-wave time stamps and wave-level step counts in the megakernel's record layout
// (tools/wave_timeline.py), plus the number of service steps in the upper half of word 6.
template <bool COUNT, bool STAMP = false>
__global__ __launch_bounds__(CRT_BLOCK, (COUNT || STAMP) ? CRT_WAVES_PER_SIMD_COUNT : CRT_WAVES_PER_SIMD)
void crt_trace_refill_kernel(CrtDevScene S, CrtFrame F, float4* __restrict__ out, unsigned long long* __restrict__ counters)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    typedef CrtStackT<2> Stack;                              // parked slots: [0] pixel index within the block | bounce << 31, [1] the path's energy
    const Stack stack = { (crt_lds_u32_ptr)s_stack + threadIdx.x, S.stackOverflow };
    LaneCounters lc; zero_counters(lc);
    WaveStampStart t0 = { 0, 0 };
    if (STAMP) t0 = wave_stamp_start();
    const unsigned long long tc0 = tile_cost_start(F);
    int tx0 = 0, tileRow = 0, costSlot = -1;
    const bool valid = refill_block(F, blockIdx.x, tx0, tileRow, costSlot);
    if (valid) {
        uint32_t cursor = 0;                                 // next pixel of the block nobody has taken yet (wave-uniform)
        PathState ps = camera_path(F, mk3(0.f, 0.f, 0.f));
        Closest c = no_hit();
        constexpr unsigned kTrip = opt_if(COUNT, TR_COUNT) | opt_if(STAMP, TR_ITERS) | opt_if(policy::refill_block_divides(COUNT), TR_DIVIDE)
                                 | opt_if(policy::refill_offset32(COUNT, STAMP), TR_OFFSET32);
        Traversal<kTrip> T; T.reset();
        unsigned long long cand = 0;
        bool havePath = false;
        const uint32_t cnt = S.numInstances < 64u ? S.numInstances : 64u;
        for (;;) {
            // a lane's ray is finished when it is inside no instance and has no candidate left (kernel_main.cl:198-217 ran out)
            const bool rayDone = havePath && !T.active && cand == 0;
            const unsigned long long mDone = __ballot(rayDone);
            const unsigned long long mBusy = __ballot(havePath && !rayDone);
            if ((mDone | mBusy) == 0 && cursor >= (uint32_t)CRT_REFILL_PIXELS) break;       // every pixel of the block is stored
            const uint32_t nDone = (uint32_t)__popcll(mDone), nBusy = (uint32_t)__popcll(mBusy);
            if (STAMP) { if (first_active_lane()) lc.pops++; }
            // Service step: shade the finished rays, start bounce rays, store finished pixels, hand out new pixels. Run when enough
            // finished lanes have gathered to pay for the step's instruction stream, when they outnumber half of the lanes still
            // traversing (waiting would idle more lanes than it saves steps), or when nobody is traversing at all.
            if (nDone >= (uint32_t)CRT_REFILL_BATCH || (uint32_t)CRT_REFILL_RATIO * nDone > nBusy || nBusy == 0) {
                bool newRay = false;
                if (STAMP) { if (first_active_lane()) lc.capHits++; }
                if (rayDone) {
                    T.reset();                                // (the traversal is idle: nothing of it needs to survive the shading code)
                    const uint32_t st = stack.parked(0);
                    const int bounce = (int)(st >> 31);
                    ps.energy = __uint_as_float(stack.parked(1));      // (waits in LDS through the traversals, as in the megakernel's SHADOW instantiations)
                    const int cont = shade_bounce<opt_if(policy::refill_sky_double(COUNT), SB_SKY_DOUBLE) | opt_if(policy::refill_offset32(COUNT, STAMP), SB_OFFSET32)>(S, c, ps, bounce, F.lightY, F.lightZ);
                    c = no_hit();
                    if (COUNT) { if (cont) lc.hits++; else lc.misses++; }
                    if (cont != 0 && bounce == 0) {           // kernel_main.cl:187: the second iteration of the bounce loop
                        stack.park(0, st | 0x80000000u);
                        stack.park(1, __float_as_uint(ps.energy));
                        newRay = true;
                        if (COUNT) { lc.rays++; lc.secondary++; }
                    } else {
                        // the plain HDR value; upstream's per-pixel stages behind Trace are applied by the pass below the loop
                        int qx, qy;
                        refill_pixel(tx0, tileRow, st & 0x7FFFFFFFu, qx, qy);
                        out[(size_t)qy * (size_t)F.width + (size_t)qx] = make_float4(ps.result.x, ps.result.y, ps.result.z, 1.0f);
                        havePath = false;
                    }
                }
                // refill: the lanes without a path take the block's next pixels in lane order
                const unsigned long long mWant = __ballot(!havePath);
                if (mWant != 0 && cursor < (uint32_t)CRT_REFILL_PIXELS) {
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mWant >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mWant, 0u));
                    const uint32_t p = cursor + rank;
                    cursor += (uint32_t)__popcll(mWant);
                    if (!havePath && p < (uint32_t)CRT_REFILL_PIXELS) {
                        int px, py;
                        refill_pixel(tx0, tileRow, p, px, py);
                        if (px < F.width && py < F.height) {
                            havePath = true;
                            stack.park(0, p);
                            // opaque copies: otherwise (float)width / (float)height are hoisted out of the loop and kept alive (spilled) through it
                            int w2 = F.width, h2 = F.height;
                            asm volatile("" : "+s"(w2), "+s"(h2));
                            ps = camera_path(F, raygen_dir(F, px, py, w2, h2));
                            stack.park(1, __float_as_uint(ps.energy));
                            newRay = true;
                            if (COUNT) { lc.rays++; lc.primary++; }
                        }
                    }
                }
                if (newRay) cand = candidate_mask<opt_if(COUNT, CM_COUNT)>(S, ps.o, ps.d, 0u, cnt, lc);
            }
            // one traversal trip (closest_hit's: enter -> inner -> leaf -> inner) for the lanes that have something to traverse
            if (havePath && !T.active && cand != 0) {
                if (STAMP) { if (first_active_lane()) lc.traversals++; }
                const uint32_t k = (uint32_t)__ffsll((long long)cand) - 1u;
                cand &= cand - 1;
                T.enter(S, k, ps.o, ps.d, c.distance, lc);
            }
            trip_steps<kTrip>(S, stack, T, c, lc, false);
        }
    }
    if (valid) finish_block_pixels(F, tx0, tileRow, CRT_REFILL_PIXELS, out);   // upstream's per-pixel stages behind Trace
    add_tile_cost(F, costSlot, tc0);
    if (COUNT) flush_counters(lc, counters);
    if (STAMP) write_wave_stamp(counters, lc, t0, wave_sum(lc.capHits));      // + the service steps
}

// ------------------------------------------------------------------------------------------------------------------------------
// crt_trace_block_kernel (CRT_KERNEL=block) -- PHASE-SEPARATED compaction inside the wave.
//
// What the refill form above taught (profiles/r05_in_wave_compaction_timeline.txt, r05refill_summary.md): a wave that mixes rays at different stages executes every step kind
// (enter / inner / leaf) on every trip, so the wave-level instruction count falls far less than the lane utilisation rises, and
// the service steps cost what the packing saves. Here the rays of a block are regrouped BETWEEN the stages instead, so every
// traversal still runs as a packet of rays that start together:
//   phase 0  classify the block's pixels: RayGen + the instance cull for 64 pixels at a time. A primary ray without a candidate
//            instance is a sky pixel and is finished on the spot (all such lanes shade together); the others' pixel indices are
//            appended to a list in the wave's parked LDS slots (ballot + mbcnt: no atomics, the list is the wave's own).
//   phase 1  the listed primary rays, 64 per pass, as DENSE packets: closest hit, shading; a path that continues stores its
//            partial radiance in the frame and appends its bounce ray {origin, energy, direction, pixel} to the block's queue
//            (a 32-byte record in global memory that only this wave touches: written and read back through its own L2).
//   phase 2  the queued bounce rays, 64 per pass, again dense.
// Per ray nothing changes (the same closest_hit / shade_bounce as the megakernel; result = partial + bounce-1 terms in the order of
// kernel_main.cl:267), so frames and work counters are bit-identical. The cull of phase 0 is not counted; closest_hit counts it
// when the ray is traced (a culled instance is upstream's one pop + one root visit either way, so the totals are the same).
// ------------------------------------------------------------------------------------------------------------------------------
#ifndef CRT_BLOCK_TILES
#define CRT_BLOCK_TILES 2
#endif
#define CRT_BLOCK_PIXELS (64 * CRT_BLOCK_TILES)

template <bool COUNT, bool STAMP = false>
__global__ __launch_bounds__(CRT_BLOCK, (COUNT || STAMP) ? CRT_WAVES_PER_SIMD_COUNT : CRT_WAVES_PER_SIMD)
void crt_trace_block_kernel(CrtDevScene S, CrtFrame F, float4* __restrict__ out, unsigned long long* __restrict__ counters, CrtBounceRay* __restrict__ queue)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    typedef CrtStackT<CRT_BLOCK_TILES> Stack;                // parked slots: the list of primary rays that have a candidate instance
    const Stack stack = { (crt_lds_u32_ptr)s_stack + threadIdx.x, S.stackOverflow };
    const crt_lds_u32_ptr list = (crt_lds_u32_ptr)s_stack + Stack::kLds * 64;
    const uint32_t lane = threadIdx.x & 63u;
    LaneCounters lc; zero_counters(lc);
    WaveStampStart t0 = { 0, 0 };
    if (STAMP) t0 = wave_stamp_start();
    const unsigned long long tc0 = tile_cost_start(F);
    int tx0 = 0, tileRow = 0, costSlot = -1;
    const bool valid = refill_block(F, blockIdx.x, tx0, tileRow, costSlot, CRT_BLOCK_TILES);
    constexpr unsigned kRay = opt_if(COUNT, TR_COUNT) | opt_if(STAMP, TR_ITERS) | opt_if(policy::refill_block_divides(COUNT), TR_DIVIDE)
                                 | opt_if(policy::kBlockOffset32, TR_OFFSET32);
    constexpr unsigned kShade = opt_if(policy::kBlockSkyDouble, SB_SKY_DOUBLE);
    if (valid) {
        const uint32_t cnt = S.numInstances < 64u ? S.numInstances : 64u;
        CrtBounceRay* __restrict__ q = queue + (size_t)costSlot * CRT_BLOCK_PIXELS;
        uint32_t nList = 0, nQueue = 0;                      // wave-uniform
        // ---- phase 0: classify ----
        for (uint32_t t = 0; t < (uint32_t)CRT_BLOCK_TILES; ++t) {
            const uint32_t p = t * 64u + lane;
            int px, py;
            refill_pixel(tx0, tileRow, p, px, py);
            const bool inFrame = px < F.width && py < F.height;
            bool listed = false;
            if (inFrame) {
                PathState ps = camera_path(F, raygen_dir(F, px, py));
                LaneCounters none;
                const unsigned long long cand = candidate_mask(S, ps.o, ps.d, 0u, cnt, none);
                if (cand == 0 && S.numInstances <= 64u) {
                    // no instance can be hit: closest_hit would return the initial miss (kernel_main.cl:219-224: skybox, break)
                    if (COUNT) { lc.rays++; lc.primary++; lc.misses++; count_culled(lc, cnt); }
                    (void)shade_bounce<kShade>(S, no_hit(), ps, 0, F.lightY, F.lightZ);
                    out[(size_t)py * (size_t)F.width + (size_t)px] = make_float4(ps.result.x, ps.result.y, ps.result.z, 1.0f);
                } else listed = true;
            }
            const unsigned long long m = __ballot(listed);
            if (listed) list[nList + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = p;
            nList += (uint32_t)__popcll(m);
        }
        // ---- phase 1: the primary rays that may hit something, as dense packets ----
        // (what is not used inside the traversal is recomputed behind it rather than kept alive through it: the pixel index, as in
        // the megakernel; the opaque asm keeps the two computations apart)
        for (uint32_t base = 0; base < nList; base += 64u) {
            bool cont = false;
            PathState ps = camera_path(F, mk3(0.f, 0.f, 0.f));
            if (base + lane < nList) {
                {
                    int px, py;
                    refill_pixel(tx0, tileRow, list[base + lane], px, py);
                    ps.d = raygen_dir(F, px, py);
                }
                if (COUNT) { lc.rays++; lc.primary++; }
                const Closest c = closest_hit<kRay>(S, ps.o, ps.d, stack, lc);
                cont = shade_bounce<kShade>(S, c, ps, 0, F.lightY, F.lightZ) != 0;
                if (COUNT) { if (cont) lc.hits++; else lc.misses++; }
            }
            uint32_t base2 = base, lane2 = lane;
            asm volatile("" : "+s"(base2), "+v"(lane2));
            uint32_t pixel = 0;
            if (base2 + lane2 < nList) {
                int px, py;
                refill_pixel(tx0, tileRow, list[base2 + lane2], px, py);
                pixel = (uint32_t)py * (uint32_t)F.width + (uint32_t)px;
                out[pixel] = make_float4(ps.result.x, ps.result.y, ps.result.z, 1.0f);
            }
            const unsigned long long m = __ballot(cont);
            if (cont) {
                q[nQueue + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = pack_bounce(ps, pixel);
            }
            nQueue += (uint32_t)__popcll(m);
        }
        // ---- phase 2: the bounce rays, as dense packets (the wave reads its own stores: workgroup-scope release / acquire) ----
        if (nQueue != 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        for (uint32_t base = 0; base < nQueue; base += 64u) {
            if (base + lane < nQueue) {
                PathState ps = unpack_bounce(q[base + lane]);
                if (COUNT) { lc.rays++; lc.secondary++; }
                const Closest c = closest_hit<kRay>(S, ps.o, ps.d, stack, lc);
                // the partial radiance and the pixel index are fetched behind the traversal (nothing kept alive through it)
                uint32_t base2 = base, lane2 = lane;
                asm volatile("" : "+s"(base2), "+v"(lane2));
                const uint32_t pixel = q[base2 + lane2].pixel;
                const float4 partial = out[pixel];
                ps.result = mk3(partial.x, partial.y, partial.z);
                const bool cont = shade_bounce<kShade>(S, c, ps, 1, F.lightY, F.lightZ) != 0;
                if (COUNT) { if (cont) lc.hits++; else lc.misses++; }
                out[pixel] = make_float4(ps.result.x, ps.result.y, ps.result.z, 1.0f);
            }
        }
    }
    if (valid) finish_block_pixels(F, tx0, tileRow, CRT_BLOCK_PIXELS, out);   // upstream's per-pixel stages behind Trace
    add_tile_cost(F, costSlot, tc0);
    if (COUNT) flush_counters(lc, counters);
    if (STAMP) write_wave_stamp(counters, lc, t0);
}
