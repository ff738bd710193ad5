// crt_kernels.h -- the per-frame kernels of the MI355X ray-trace path (gfx950).
//
//   crt_trace_kernel        RayGen + Trace megakernel (kernel_main.cl:164-287), the default and dominant launch
//   crt_trace_ssaa_kernel   the same body (trace_body) over a k x k supersampled frame, resolved in registers (CRT_RENDER_SSAA2 / SSAA4)
//   crt_trace_gbuffer_kernel  the same body, also storing the first hit's normal, distance, ids and albedo planes (CRT_RENDER_GBUFFER)
//   crt_primary_kernel /    wavefront form: one launch per bounce with ballot compaction (CRT_KERNEL=wavefront)
//   crt_bounce_kernel
//   crt_raygen_kernel       RayGen alone (kernel_main.cl:277-287), only for CRT_RENDER_WRITE_RAYS
//   crt_postprocess_kernel  PostProcess (kernel_main.cl:342-359)
//   crt_query_kernel        closest-hit records for explicit rays on the host (parity tests, counted)
//   crt_rays_kernel         closest hit / occlusion for batches of rays on the device (crt_trace_rays): declared in crt_rays.h, compiled in crt_rays.hip
//   crt_shade_kernel        radiance / first-hit surface records for batches of rays on the device (crt_shade_rays): declared in crt_shade.h, compiled in crt_shade.hip
//   crt_order_kernel        feedback launch lists: per-XCD counting sort of the tiles by last frame's cost
// Device-side traversal/shading code lives in crt_device.h. (Two further kernel structures of round 1 -- resident waves
// pulling tiles from per-XCD queues, and 768-thread workgroups with the hot BVH tiles staged in LDS -- were measured
// at 1.67 and 2.25 Gray/s against 4.55 for this one and retired in round 2; docs/DESIGN_HISTORY.md 4f keeps the numbers.)
#pragma once
#include "crt_device.h"
#include "crt_post.h"

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int off = 32; off > 0; off >>= 1) { uint32_t o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}

__device__ __forceinline__ void flush_counters(const LaneCounters& lc, unsigned long long* g)
{
    // every lane of the wave must call this (inactive pixels contribute zeros)
    uint32_t s[14] = { lc.rays, lc.primary, lc.secondary, lc.hits, lc.misses, lc.traversals, lc.pops,
                       lc.innerVisits, lc.triTests, lc.capHits, lc.stackOverflows, lc.shadowRays, lc.shadowHits, lc.culled };
    uint32_t mx = wave_max(lc.maxStack);
#pragma unroll
    for (int k = 0; k < 14; ++k) {
        uint32_t t = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(&g[k < 11 ? k : k + 1], (unsigned long long)t);   // [11] is maxStack
    }
    if ((threadIdx.x & 63) == 0) atomicMax(&g[11], (unsigned long long)mx);
}

__device__ __forceinline__ void zero_counters(LaneCounters& lc)
{
    lc.rays = lc.primary = lc.secondary = lc.hits = lc.misses = 0;
    lc.traversals = lc.pops = lc.innerVisits = lc.triTests = lc.capHits = lc.stackOverflows = lc.maxStack = 0;
    lc.shadowRays = lc.shadowHits = 0; lc.culled = 0;
}


// Pixel of this lane. One wave64 per workgroup owns an 8x8 pixel tile, lanes in Morton order
// (coherent ray packets). Workgroups are dealt round-robin over the 8 XCDs (block b runs on XCD
// b % 8), so block b takes tile row (b/8 / tilesX) * 8 + b % 8: every XCD (own 4 MiB L2) walks whole
// tile rows left to right -- neighbouring tiles share BVH subtrees in its L2 -- while the eight XCDs
// interleave row by row, which keeps them equally loaded when geometry is concentrated in one part
// of the frame (a contiguous slab per XCD left most XCDs idle: ~1.2 resident waves/SIMD measured).
// deal_tile is the wave-uniform part: workgroup b's list entry -- `slotOut` receives its index into the per-tile cost array (or -1),
// `quadrant` the quadrant a quadrant wave traces (or -1) -- and its tile (column tx, tile row of the rank's band); false when the
// workgroup has no tile.
__device__ __forceinline__ bool deal_tile(const CrtFrame& F, int b, int& tx, int& tileRow, int& quadrant, int* slotOut)
{
    const int xcd = b & 7;
    int slot = b >> 3;
    quadrant = -1;
    // Feedback scheduling (crt_order_kernel): each XCD's tiles are launched heaviest-first, by the cycles the same
    // tile cost in the previous frame, and the very heaviest are traced by four waves of one 4x4 quadrant each, so
    // that no single wave's serial chain outlasts the rest of the frame. Nothing is cached or skipped -- only the
    // launch order and the wave shape change. (Before: 0.45 ms with the machine full + 0.45 ms of tail.)
    if (F.order) {
        if ((uint32_t)slot >= F.listLen[xcd]) { if (slotOut) *slotOut = -1; return false; }
        const uint32_t e = __builtin_amdgcn_readfirstlane(F.order[xcd * F.listCap + slot]);   // wave-uniform: keep it (and what follows from it) in SGPRs
        slot = (int)(e & 0x0FFFFFFFu);
        if (e & 0x80000000u) quadrant = (int)((e >> 28) & 3u);
    } else if (slot >= F.slotsPerXcd) { if (slotOut) *slotOut = -1; return false; }
    if (slotOut) *slotOut = xcd * F.slotsPerXcd + slot;
    const int round = slot / F.tilesX;
    tx = slot - round * F.tilesX;
    const int k = round * 8 + xcd;                     // index among the tile rows this rank owns
    if (k >= F.ownedTileRows) return false;
    const int bandK = k / F.tileRowsPerBand;
    tileRow = (F.rank + bandK * F.nRanks) * F.tileRowsPerBand + (k - bandK * F.tileRowsPerBand);
    return true;
}
// pixel (tx * 8 + lx, tileRow * 8 + ly) of Morton position m (0..63) in tile (tx, tileRow)
__device__ __forceinline__ void tile_pixel(int tx, int tileRow, int m, int& px, int& py)
{
    px = tx * CRT_TILE + ((m & 1) | ((m >> 1) & 2) | ((m >> 2) & 4));
    py = tileRow * CRT_TILE + (((m >> 1) & 1) | ((m >> 2) & 2) | ((m >> 3) & 4));
}
__device__ __forceinline__ bool lane_pixel(const CrtFrame& F, int& px, int& py, int* slotOut = nullptr, bool* quadrantOut = nullptr, int b = blockIdx.x,
                                           int lane = (int)(threadIdx.x & 63))
{
    int tx, tileRow, quadrant;
    const bool dealt = deal_tile(F, b, tx, tileRow, quadrant, slotOut);
    if (quadrantOut) *quadrantOut = quadrant >= 0;
    if (!dealt) return false;
    if (quadrant >= 0 && (lane >> 4) != quadrant) return false;   // Morton order: lanes 16q..16q+15 are one 4x4 quadrant
    tile_pixel(tx, tileRow, lane, px, py);
    return px < F.width && py < F.height;
}

// Builds the next frame's launch lists: one workgroup per XCD, counting sort of that XCD's tiles by this frame's
// cost, descending (1024 linear bins up to the list's maximum). A tile is traced by four quadrant waves instead of one
// when its wave alone would run longer than `splitFactor` x (the XCD's total cost): with splitFactor = beta / (wave slots
// of the XCD) that is "longer than beta times the time the XCD needs for the whole frame" -- only then does its serial
// chain, not the throughput, decide when the frame ends. (A fixed "more than half the maximum, at most 96" rule
// over-split large frames: 1920x1080 ran 16 % slower with 96 than with 4 splits per XCD, while one rank's eighth of
// a 3840x2160 frame wanted them.) At most maxSplit tiles per XCD; they come first in the list.
// Sort key of a tile = its own cost or `spread` x the heaviest of its eight neighbours' costs, whichever is larger: when the
// camera moves, the heavy tiles of the next frame are the heavy tiles of this one or the tiles next to them.
__global__ void crt_cost_spread_kernel(const uint32_t* __restrict__ cost, uint32_t* __restrict__ key, int slotsPerXcd, int tilesX, float spread)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 8 * slotsPerXcd) return;
    const int x = g / slotsPerXcd, i = g - x * slotsPerXcd;
    const int round = i / tilesX, tx = i - round * tilesX;
    const int k = round * 8 + x, rows = (slotsPerXcd / tilesX) * 8;
    uint32_t nb = 0;
    for (int dk = -1; dk <= 1; ++dk)
        for (int dx = -1; dx <= 1; ++dx) {
            const int kk = k + dk, xx = tx + dx;
            if ((dk | dx) == 0 || kk < 0 || kk >= rows || xx < 0 || xx >= tilesX) continue;
            const uint32_t c = cost[(size_t)(kk & 7) * slotsPerXcd + (size_t)(kk >> 3) * tilesX + xx];
            nb = c > nb ? c : nb;
        }
    const uint32_t own = cost[g], lifted = (uint32_t)((float)nb * spread);
    key[g] = own > lifted ? own : lifted;
}

// `key`: what the tiles are sorted and split by (crt_cost_spread_kernel's output, or the costs themselves)
__global__ __launch_bounds__(1024) void crt_order_kernel(uint32_t* __restrict__ cost, const uint32_t* __restrict__ key, uint32_t* __restrict__ order,
                                                       uint32_t* __restrict__ listLen, int slotsPerXcd, int listCap, uint32_t maxSplit,
                                                       float splitFactor)
{
    __shared__ uint32_t s_bins[1024];
    __shared__ uint32_t s_max, s_nSplit;
    __shared__ float s_sum;
    const int x = blockIdx.x, tid = threadIdx.x;
    const uint32_t* c = key + (size_t)x * slotsPerXcd;
    const uint32_t* own = cost + (size_t)x * slotsPerXcd;
    uint32_t* o = order + (size_t)x * listCap;
    s_bins[tid] = 0;
    if (tid == 0) { s_max = 1; s_sum = 0.0f; }
    __syncthreads();
    uint32_t m = 0; float sum = 0.0f;
    for (int i = tid; i < slotsPerXcd; i += 1024) { m = c[i] > m ? c[i] : m; sum += (float)own[i]; }
    atomicMax(&s_max, m);
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((tid & 63) == 0) atomicAdd(&s_sum, sum);
    __syncthreads();
    const float scale = 1023.0f / (float)s_max;
    for (int i = tid; i < slotsPerXcd; i += 1024) {
        int bin = 1023 - (int)((float)c[i] * scale);     // heaviest -> bin 0
        bin = bin < 0 ? 0 : (bin > 1023 ? 1023 : bin);
        atomicAdd(&s_bins[bin], 1u);
    }
    __syncthreads();
    // exclusive scan of the 1024 bins: one bin per thread, wave scans + a scan of the 16 wave totals
    {
        const uint32_t n = s_bins[tid];
        uint32_t incl = n;
        for (int off = 1; off < 64; off <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64); if ((tid & 63) >= off) incl += v; }
        __shared__ uint32_t s_wave[16];
        if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
        __syncthreads();
        uint32_t wbase = 0;
        for (int w = 0; w < (tid >> 6); ++w) wbase += s_wave[w];
        s_bins[tid] = wbase + incl - n;
    }
    __syncthreads();
    if (tid == 0) {
        // tiles in the bins above the threshold: s_bins[b] = number of tiles in bins 0..b-1 (heavier than bin b)
        const float thr = splitFactor * s_sum;
        int b = 1023 - (int)(thr * scale);
        b = b < 0 ? 0 : (b > 1023 ? 1023 : b);
        const uint32_t heavy = s_bins[b];
        s_nSplit = heavy < maxSplit ? heavy : maxSplit;
        listLen[x] = (uint32_t)slotsPerXcd + 3u * s_nSplit;
    }
    __syncthreads();
    const uint32_t nSplit = s_nSplit;
    for (int i = tid; i < slotsPerXcd; i += 1024) {
        int bin = 1023 - (int)((float)c[i] * scale);
        bin = bin < 0 ? 0 : (bin > 1023 ? 1023 : bin);
        const uint32_t pos = atomicAdd(&s_bins[bin], 1u);
        if (pos < nSplit) { for (uint32_t q = 0; q < 4; ++q) o[4 * pos + q] = (uint32_t)i | (q << 28) | 0x80000000u; }
        else o[3 * nSplit + pos] = (uint32_t)i;
    }
    __syncthreads();
    for (int i = tid; i < slotsPerXcd; i += 1024) cost[(size_t)x * slotsPerXcd + i] = 0;    // this frame's waves add their cycles
}

__global__ void crt_identity_order_kernel(uint32_t* __restrict__ order, uint32_t* __restrict__ listLen, int slotsPerXcd, int listCap)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 8) listLen[i] = (uint32_t)slotsPerXcd;
    if (i < 8 * slotsPerXcd) order[(i / slotsPerXcd) * listCap + (i % slotsPerXcd)] = (uint32_t)(i % slotsPerXcd);
}

// ---- per-pixel stages behind Trace, shared by their own launches and by the Trace kernel's epilogue ---------------------------
// post_pixel, unorm8, quantize1, quantize3, pack_rgba8 and the FXAA filter (fxaa_pixel): crt_post.h, which libcrt_present.so compiles too
#define CRT_EPILOGUE_QUANTIZE 1   // CrtFrame::epilogue bits
#define CRT_EPILOGUE_POST 2

// The per-pixel stages that follow Trace upstream (its RGBA8 render target, PostProcess) applied to a value in registers, and the
// store of pixel (x, y) of a width x height frame: no second and third pass over the frame (wave-uniform branches). With
// F.packOut also the bytes of upstream's RGBA8 texture, for a read-back (what crt_pack_unorm8_kernel would make of the value
// just stored). `always` = false: the float frame already holds the plain value (the post-pass of the refill / block forms).
__device__ __forceinline__ void finish_pixel(const CrtFrame& F, v3 rgb, int x, int y, int width, int height, float4* __restrict__ out, bool always = true)
{
    if (F.epilogue & CRT_EPILOGUE_QUANTIZE) rgb = quantize3(rgb);
    if (F.epilogue & CRT_EPILOGUE_POST) {
        rgb = post_pixel(rgb, x, y, width, height);
        if (F.epilogue & CRT_EPILOGUE_QUANTIZE) rgb = quantize3(rgb);
    }
    const size_t idx = (size_t)y * (size_t)width + (size_t)x;
    if (always || F.epilogue != 0) out[idx] = make_float4(rgb.x, rgb.y, rgb.z, 1.0f);
    if (F.packOut) F.packOut[idx] = pack_rgba8(rgb);
}
// ... as one pass over the `pixels` pixels of a block of tiles starting at tile (tx0, tileRow), at full lane occupancy, on the
// plain values this wave stored before (workgroup-scope release / acquire: the wave reads its own stores). The refill and block
// forms keep the stages out of their loops: seven powf per pixel inside cost the traversal its registers.
__device__ __forceinline__ void finish_block_pixels(const CrtFrame& F, int tx0, int tileRow, uint32_t pixels, float4* __restrict__ out)
{
    if (F.epilogue == 0 && F.packOut == nullptr) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    for (uint32_t p = threadIdx.x & 63u; p < pixels; p += 64u) {
        int qx, qy;
        tile_pixel(tx0 + (int)(p >> 6), tileRow, (int)(p & 63u), qx, qy);
        if (qx >= F.width || qy >= F.height) continue;
        const float4 v = out[(size_t)qy * (size_t)F.width + (size_t)qx];
        finish_pixel(F, mk3(v.x, v.y, v.z), qx, qy, F.width, F.height, out, false);
    }
}

// Per-tile cost of this frame (wave-uniform value, one atomic): the cycles since `tc0` = tile_cost_start(F).
// `halve`: the four quadrant waves of a split tile each add half their cycles: about what the tile would take as one wave
// (a quadrant wave runs ~0.6x as long as the whole tile's), so a split tile neither sticks nor flips every frame
__device__ __forceinline__ unsigned long long tile_cost_start(const CrtFrame& F) { return F.cost ? __builtin_amdgcn_s_memtime() : 0ull; }
__device__ __forceinline__ void add_tile_cost(const CrtFrame& F, int costSlot, unsigned long long tc0, bool halve = false)
{
    if (F.cost && costSlot >= 0) {
        unsigned long long dt = __builtin_amdgcn_s_memtime() - tc0;
        if (halve) dt >>= 1;
        if ((threadIdx.x & 63) == 0) atomicAdd(&F.cost[costSlot], dt > 0x0FFFFFFFull ? 0x0FFFFFFFu : (uint32_t)dt);
    }
}

// STAMP (diagnostic build only, CRT_RENDER_STAMPS): every wave records start/end s_memrealtime (100 MHz), its s_memtime cycle
// count, XCC/HW ids and its wave-level step counts (closest_hit's TR_ITERS) into 8 words of a buffer nothing else reads
// (tools/wave_timeline.py). Every lane of the wave must call write_wave_stamp.
struct WaveStampStart { unsigned long long rt, c; };
__device__ __forceinline__ WaveStampStart wave_stamp_start() { return { __builtin_amdgcn_s_memrealtime(), __builtin_amdgcn_s_memtime() }; }
__device__ __forceinline__ void write_wave_stamp(unsigned long long* __restrict__ counters, const LaneCounters& lc, WaveStampStart t0, uint32_t wService = 0)
{
    const unsigned long long t1c = __builtin_amdgcn_s_memtime(), t1rt = __builtin_amdgcn_s_memrealtime();
    const uint32_t wOuter = wave_sum(lc.pops), wEnter = wave_sum(lc.traversals), wDescent = wave_sum(lc.innerVisits),
                   wLeaf = wave_sum(lc.triTests), laneVisits = wave_sum(lc.rays), wInner2 = wave_sum(lc.hits), wLeafIters = wave_sum(lc.misses);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* st = counters + 16 + (size_t)blockIdx.x * 8;
        st[4] = wOuter | ((unsigned long long)wInner2 << 32); st[5] = wEnter | ((unsigned long long)wLeafIters << 32);
        st[6] = wDescent | ((unsigned long long)wService << 32); st[7] = ((unsigned long long)wLeaf << 32) | laneVisits;
        st[0] = t0.rt; st[1] = t1rt; st[2] = t1c - t0.c;
        st[3] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 32);
    }
}

// (v + v of lane ^ M) per channel, for the SSAA resolve: ds_swizzle in bit mode, and_mask 0x1F, or_mask 0, xor_mask M (M < 32)
template <int M> __device__ __forceinline__ float xor_add(float v) { return v + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1F | (M << 10))); }
template <int M> __device__ __forceinline__ v3 xor_add3(v3 v) { return mk3(xor_add<M>(v.x), xor_add<M>(v.y), xor_add<M>(v.z)); }

// The pixel of lane `lane` of workgroup `b` once more, behind the traversals: the pixel coordinates are recomputed rather than
// kept alive through both traversals (4 VGPRs that were spilled to scratch at 8 waves/SIMD): the block index goes through an
// opaque asm so the two computations are not merged
__device__ __forceinline__ void lane_pixel_again(const CrtFrame& F, int b, int lane, int& qx, int& qy)
{
    asm volatile("" : "+s"(b), "+v"(lane));
    (void)lane_pixel(F, qx, qy, nullptr, nullptr, b, lane);
}

// kernel Trace (kernel_main.cl:164-275) with RayGen (kernel_main.cl:277-287) fused: the ray
// direction is computed with the same arithmetic RayGen stores, so the 24.9 MB ray buffer
// round-trip disappears. One thread per pixel, both bounces. The body of crt_trace_kernel, crt_trace_ssaa_kernel and
// crt_trace_ldstop_kernel: `stack` is the wave's stack (parked slots: the instance tree's candidate list [0, 4) and the shadow
// ray's n.l behind it), `b` its (virtual) block number, `lane` the lane.
// STAMP: see write_wave_stamp.
// SHADOW (CRT_RENDER_SHADOWS, an extension: upstream only threads the factor through, kernel_main.cl:256-258,264):
// after the first hit a shadow ray (new ray origin, -lightDir) decides `shadow` in `energy *= specular`. Traced only
// where it is observable: at bounce 0 (the energy after bounce 1 is never read) and when n.l > 0 (otherwise the
// product is 0 whatever the shadow factor).
// TLAS: candidates come from the instance tree instead of the linear sphere loop (scenes with many instances).
// REFRACT (CRT_RENDER_REFRACTION, the other README TODO of upstream, oracle-defined): translucent materials transmit.
// SSAA (CRT_RENDER_SSAA2 / SSAA4, k = F.ss): F describes the VIRTUAL frame kW x kH -- its tile grid, raygen_dir's width and
// height -- and every lane traces virtual pixel (k x + sx, k y + sy) exactly as a pixel of a kW x kH frame. The k x k subsamples
// of output pixel (x, y) are Morton lanes 4p..4p+3 (k = 2) or 16q..16q+15 (k = 4) of one wave, all active or all inactive (kW, kH
// are multiples of k, k divides the 8x8 tile). The epilogue resolves them in registers in a fixed order -- lane ^ 1 (sx bit 0),
// ^ 2 (sy bit 0), ^ 4 (sx bit 1), ^ 8 (sy bit 1), then x 1/k^2 (exact) -- and the lane of sub-index 0 applies the stages behind
// Trace at OUTPUT coordinates and stores the W x H pixel.
// GBUFFER (CRT_RENDER_GBUFFER): the lane also stores its pixel of the three first-hit planes `gb` (include/crt_api.h) from inside the
// bounce-0 shading (shade_bounce's SINK), where normal, albedo and the hit record are in registers anyway: nothing is carried
// through the second traversal, and the pixel's coordinates are recomputed as in the epilogue. ids and t are what crt_query_kernel
// stores for the ray; a hit that upstream shades as sky (t > InfMinusOne, kernel_main.cl:219) has the normal and albedo of a miss.
struct GBufferSink {
    const CrtGBuffer* gb; const CrtFrame* F; int b, lane;
    // byte offset of the lane's pixel in the albedo plane (x 4 in the other two): 32 bits (a frame of fewer than 2^28 pixels,
    // refuse_gbuffer), so each store is a scalar plane base plus one VGPR of offset -- no 64-bit address per plane in registers
    __device__ __forceinline__ uint32_t pixel_offset() const
    {
        int gx, gy;
        lane_pixel_again(*F, b, lane, gx, gy);
        return ((uint32_t)gy * (uint32_t)F->width + (uint32_t)gx) << 2;
    }
    template <class T> static __device__ __forceinline__ void store(char* plane, uint32_t byteOffset, T v) { *reinterpret_cast<T*>(plane + byteOffset) = v; }
    __device__ __forceinline__ size_t pixels() const { return (size_t)((uint32_t)F->width * (uint32_t)F->height); }   // wave-uniform
    __device__ __forceinline__ void hit(const Closest& c, v3 normal, uint32_t albedo) const
    {
        const uint32_t off = pixel_offset();
        store(gb->geometry(), off << 2, make_float4(normal.x, normal.y, normal.z, c.hit.t));
        store(gb->ids(pixels()), off << 2, make_uint4((uint32_t)c.hitInstance, c.hit.tri, __float_as_uint(c.hit.u), __float_as_uint(c.hit.v)));
        store(gb->albedo(pixels()), off, albedo);
    }
    __device__ __forceinline__ void miss(const Closest& c) const
    {
        const uint32_t off = pixel_offset();
        // Closest::anyHit without keeping that register alive through the traversal: a hit's t is below the distance the ray
        // started with (intersect_triangle: t < out.t), and Closest::distance is that t
        const bool anyHit = c.distance < no_hit().distance;
        store(gb->geometry(), off << 2, make_float4(0.0f, 0.0f, 0.0f, c.distance));
        store(gb->ids(pixels()), off << 2, anyHit ? make_uint4((uint32_t)c.hitInstance, c.hit.tri, __float_as_uint(c.hit.u), __float_as_uint(c.hit.v)) : make_uint4(0xFFFFFFFFu, 0u, 0u, 0u));
        store(gb->albedo(pixels()), off, 0u);
    }
};
#define CRT_TRACE_PLAIN 0     // trace_body's CASE
#define CRT_TRACE_SSAA 1
#define CRT_TRACE_GBUFFER 2
template <bool SHADOW, bool TLAS> using CrtTraceStack = CrtStackT<(TLAS ? CRT_TLAS_PARK : 0) + (SHADOW ? 1 : 0)>;
template <bool COUNT, bool STAMP, bool SHADOW, bool TLAS, bool REFRACT, int CASE, class STK>
__device__ __forceinline__ void trace_body(const CrtDevScene& S, const CrtFrame& F, float4* __restrict__ out, unsigned long long* __restrict__ counters,
                                           const STK& stack, int b, int lane, const CrtGBuffer* gb = nullptr)
{
    constexpr bool SSAA = CASE == CRT_TRACE_SSAA, GBUFFER = CASE == CRT_TRACE_GBUFFER;
    constexpr int kParkNdl = TLAS ? CRT_TLAS_PARK : 0;
    // what both traversals share, the primary one's own options, and the shading's (division, double-only sky index, staged cull: crt_device.h, policy)
    constexpr unsigned kRay = opt_if(COUNT, TR_COUNT) | opt_if(TLAS, TR_TLAS) | opt_if(policy::trace_divides(COUNT, GBUFFER, SHADOW, TLAS, REFRACT), TR_DIVIDE)
                            | opt_if(policy::trace_offset32(COUNT, STAMP, STK::kTop, GBUFFER, SHADOW, TLAS, REFRACT), TR_OFFSET32);
    constexpr bool kStages = policy::trace_stages_cull(COUNT, STAMP, TLAS, STK::kTop);
    constexpr bool kWaveCulls = policy::trace_wave_culls(kStages, CASE == CRT_TRACE_PLAIN, GBUFFER, SHADOW, REFRACT);
    constexpr bool kRootPretests = policy::trace_root_pretests(kWaveCulls, GBUFFER, SHADOW, REFRACT);
    constexpr unsigned kPrimary = kRay | opt_if(STAMP, TR_ITERS) | opt_if(kStages, TR_STAGE) | opt_if(kWaveCulls, TR_WAVE_CULL) | opt_if(kRootPretests, TR_ROOT_PRETEST)
                                | opt_if(policy::trace_bounce_pretests(kRootPretests), TR_BOUNCE_PRETEST)
                                | opt_if(policy::trace_pretest_enters(kRootPretests, SHADOW), TR_PRETEST_ENTRY);
    constexpr unsigned kShade = opt_if(SHADOW, SB_DEFER_ENERGY) | opt_if(REFRACT, SB_REFRACT)
                              | opt_if(policy::trace_sky_double(COUNT, GBUFFER, SHADOW, TLAS, REFRACT), SB_SKY_DOUBLE)
                              | opt_if(has_opt(kRay, TR_OFFSET32), SB_OFFSET32);
    LaneCounters lc; zero_counters(lc);
    WaveStampStart t0 = { 0, 0 };
    if (STAMP) t0 = wave_stamp_start();
    int px, py, costSlot = -1;
    bool isQuadrant = false;
    const unsigned long long tc0 = tile_cost_start(F);
    const bool active = lane_pixel(F, px, py, &costSlot, &isQuadrant, b, lane);
    if (active) {
        PathState ps = camera_path(F, raygen_dir(F, px, py));
        for (int bounce = 0; bounce < 2; ++bounce) {
            if (COUNT) { lc.rays++; if (bounce == 0) lc.primary++; else lc.secondary++; }
            // SHADOW: the path's energy waits in the parked LDS slot while the ray is traced (the one value these instantiations
            // would otherwise spill to scratch); the shadow ray's n.l uses the same slot later, when the energy is dead
            // (GBUFFER: the same -- the plane stores' addresses take the register the plain kernel keeps the energy in)
            if (SHADOW || GBUFFER) stack.park(kParkNdl, __float_as_uint(ps.energy));
            Closest c = closest_hit<kPrimary>(S, ps.o, ps.d, stack, lc, 99999.0f, false, bounce == 0);
            if (SHADOW || GBUFFER) ps.energy = __uint_as_float(stack.parked(kParkNdl));
            float ndl = 0.0f;
            int cont;
            if constexpr (!GBUFFER) cont = shade_bounce<kShade>(S, c, ps, bounce, F.lightY, F.lightZ, &ndl);
            else {
                const GBufferSink sink = { gb, &F, b, lane };
                cont = shade_bounce<kShade>(S, c, ps, bounce, F.lightY, F.lightZ, &ndl, &sink);
            }
            if (COUNT) { if (cont) lc.hits++; else lc.misses++; }
            if (!cont) break;
            if (SHADOW && cont == 1) {
                if (bounce == 0) {
                    // the energy is still its initial 1.0f here (only a transmitted ray, cont == 2, changes it before), so it
                    // need not stay in a register across the any-hit traversal: 1.0f * x == x bit for bit
                    // ... and n.l waits in a parked LDS slot meanwhile
                    float shadow = 1.0f;
                    if (ndl > 0.0f) {
                        if (COUNT) { lc.rays++; lc.shadowRays++; }
                        stack.park(kParkNdl, __float_as_uint(ndl));
                        const Closest sc = closest_hit<kRay | TR_ANYHIT>(S, ps.o, neg3(mk3(0.0f, F.lightY, F.lightZ)), stack, lc);
                        if (sc.anyHit) { shadow = 0.0f; if (COUNT) lc.shadowHits++; }
                        ndl = __uint_as_float(stack.parked(kParkNdl));
                    }
                    ps.energy = specular_x(ndl, shadow);
                } else ps.energy = ps.energy * specular_x(ndl, 1.0f);
            }
        }
        int qx, qy;
        if constexpr (SSAA) {
            // resolve: every lane of the k x k group is active here (see above), so each swizzle reads a partner of the same pixel
            const int k = F.ss;                                   // wave-uniform: 2 or 4
            v3 rgb = xor_add3<2>(xor_add3<1>(ps.result));
            if (k == 4) rgb = xor_add3<8>(xor_add3<4>(rgb));
            rgb = scale3(rgb, k == 4 ? 1.0f / 16.0f : 0.25f);
            lane_pixel_again(F, b, lane, qx, qy);
            if ((lane & (k * k - 1)) == 0) {                      // Morton sub-index 0: virtual pixel (k x, k y)
                const int sh = k == 4 ? 2 : 1;
                int w2 = F.width >> sh, h2 = F.height >> sh;       // the output frame W x H
                asm volatile("" : "+s"(w2), "+s"(h2));
                finish_pixel(F, rgb, qx >> sh, qy >> sh, w2, h2, out);
            }
        } else {
            lane_pixel_again(F, b, lane, qx, qy);
            // opaque copies: otherwise (float)width / (float)height of RayGen are kept alive (spilled) through both traversals
            int w2 = F.width, h2 = F.height;
            asm volatile("" : "+s"(w2), "+s"(h2));
            finish_pixel(F, ps.result, qx, qy, w2, h2, out);
        }
    }
    add_tile_cost(F, costSlot, tc0, isQuadrant);
    if (COUNT) flush_counters(lc, counters);
    if (STAMP) write_wave_stamp(counters, lc, t0);
}

template <bool COUNT, bool STAMP = false, bool SHADOW = false, bool TLAS = false, bool REFRACT = false>
__global__ __launch_bounds__(CRT_BLOCK, (COUNT || STAMP) ? CRT_WAVES_PER_SIMD_COUNT : CRT_WAVES_PER_SIMD)
void crt_trace_kernel(CrtDevScene S, CrtFrame F, float4* __restrict__ out, unsigned long long* __restrict__ counters)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    const CrtTraceStack<SHADOW, TLAS> stack = { (crt_lds_u32_ptr)s_stack + threadIdx.x, S.stackOverflow };
    trace_body<COUNT, STAMP, SHADOW, TLAS, REFRACT, CRT_TRACE_PLAIN>(S, F, out, counters, stack, blockIdx.x, (int)(threadIdx.x & 63));
}

// Supersampled Trace: trace_body's SSAA case. No stamps (refused).
// Counted instantiations are bounded at 5 waves/SIMD (96 VGPRs), not 6: at 80 VGPRs the counted instance-tree traversal spills
// 32-48 B per lane (as crt_trace_kernel's counted TLAS instantiations do); the others still fit 80 and run at 6.
template <bool COUNT, bool SHADOW, bool TLAS, bool REFRACT>
__global__ __launch_bounds__(CRT_BLOCK, COUNT ? CRT_WAVES_PER_SIMD_COUNT - 1 : CRT_WAVES_PER_SIMD)
void crt_trace_ssaa_kernel(CrtDevScene S, CrtFrame F, float4* __restrict__ out, unsigned long long* __restrict__ counters)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    const CrtTraceStack<SHADOW, TLAS> stack = { (crt_lds_u32_ptr)s_stack + threadIdx.x, S.stackOverflow };
    trace_body<COUNT, false, SHADOW, TLAS, REFRACT, CRT_TRACE_SSAA>(S, F, out, counters, stack, blockIdx.x, (int)(threadIdx.x & 63));
}

// Trace with the first-hit planes: trace_body's GBUFFER case. No counters, no stamps (refused): eight instantiations. Every one has
// the parked LDS slot of the SHADOW stack (the path's energy waits there during a traversal). Seven fit the plain kernel's budget
// (64 VGPRs, 8 waves/SIMD, no scratch). <1,1,1> -- shadow rays, instance tree and refraction at once -- spills 69 SGPRs where its
// crt_trace_kernel twin spills 60: a second VGPR of spill lanes, which at 64 VGPRs pushes the pixel's radiance into scratch (16 B
// per lane around the first traversal). It is bounded at 7 waves/SIMD instead and takes 68 VGPRs without scratch.
template <bool SHADOW, bool TLAS, bool REFRACT>
__global__ __launch_bounds__(CRT_BLOCK, (SHADOW && TLAS && REFRACT) ? CRT_WAVES_PER_SIMD - 1 : CRT_WAVES_PER_SIMD)
void crt_trace_gbuffer_kernel(CrtDevScene S, CrtFrame F, float4* __restrict__ out, CrtGBuffer gb)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    const CrtTraceStack<true, TLAS> stack = { (crt_lds_u32_ptr)s_stack + threadIdx.x, S.stackOverflow };
    trace_body<false, false, SHADOW, TLAS, REFRACT, CRT_TRACE_GBUFFER>(S, F, out, nullptr, stack, blockIdx.x, (int)(threadIdx.x & 63), &gb);
}

// ---- wavefront form of Trace: one launch per bounce with ballot compaction in between ----------------
// The megakernel above runs bounce 1 inside the same wave as bounce 0, at the lane density of the pixels
// that hit something (31 % on multi-1M) and on top of the wave's bounce-0 latency. Here bounce 0 writes the
// pixel's partial result and hands {origin, direction, energy, pixel} of every continuing path to a queue:
// the lanes of a wave that continue are found with one ballot and every lane stores its 32-byte record at
// (the wave's own 64-record range) + (its rank among the continuing lanes); the wave also stores how many
// there were. A scan launch (one workgroup per XCD) turns the counts into offsets, and bounce 1 is traced by
// dense 64-ray packets that look their records up through the offsets. Per-path arithmetic is unchanged:
// result = (partial) + (bounce-1 terms) in the same order as kernel_main.cl:267, so pixels are bit-identical
// to the megakernel.
// (Round 5, VERDICT r4 #3: rounds 1-4 reserved the queue range with one atomicAdd per wave on a global counter,
// so a bounce packet mixed whichever waves' rays ARRIVED together; now the order is deterministic -- XCD x's
// bounce packets hold the rays of XCD x's tiles in launch order, tile rows left to right, so neighbouring
// tiles' bounce rays share a packet and an L2 -- and nothing is shared between frames: queue, counts and
// offsets belong to the frame slot, so the wavefront form may keep frames in flight like the default kernel.)
struct CrtBounceRay { float ox, oy, oz, energy, dx, dy, dz; uint32_t pixel; };   // 32 B
__device__ __forceinline__ CrtBounceRay pack_bounce(const PathState& ps, uint32_t pixel)
{
    CrtBounceRay r;
    r.ox = ps.o.x; r.oy = ps.o.y; r.oz = ps.o.z; r.energy = ps.energy;
    r.dx = ps.d.x; r.dy = ps.d.y; r.dz = ps.d.z; r.pixel = pixel;
    return r;
}
// the path a queued record continues; `result`: the pixel's partial radiance (whoever reads it first stores it in ps.result)
__device__ __forceinline__ PathState unpack_bounce(const CrtBounceRay& r, v3 result = mk3(0.0f, 0.0f, 0.0f))
{
    PathState ps;
    ps.o = mk3(r.ox, r.oy, r.oz); ps.d = mk3(r.dx, r.dy, r.dz); ps.result = result; ps.energy = r.energy;
    return ps;
}

template <bool COUNT>
__global__ __launch_bounds__(CRT_BLOCK, COUNT ? CRT_WAVES_PER_SIMD_COUNT : CRT_WAVES_PER_SIMD) void crt_primary_kernel(CrtDevScene S, CrtFrame F, float4* __restrict__ out,
                                                                unsigned long long* __restrict__ counters,
                                                                CrtBounceRay* __restrict__ queue, uint32_t* __restrict__ waveCount)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    const CrtStack stack = { (crt_lds_u32_ptr)s_stack + threadIdx.x, S.stackOverflow };
    LaneCounters lc; zero_counters(lc);
    int px, py;
    const bool active = lane_pixel(F, px, py);
    bool cont = false;
    PathState ps = camera_path(F, mk3(0.f, 0.f, 0.f));
    if (active) {
        ps.d = raygen_dir(F, px, py);
        if (COUNT) { lc.rays++; lc.primary++; }
        Closest c = closest_hit<opt_if(COUNT, TR_COUNT) | opt_if(policy::primary_divides(COUNT), TR_DIVIDE) | opt_if(policy::kWavefrontOffset32, TR_OFFSET32)>(S, ps.o, ps.d, stack, lc);
        cont = shade_bounce<opt_if(policy::wavefront_sky_double(COUNT), SB_SKY_DOUBLE)>(S, c, ps, 0, F.lightY, F.lightZ) != 0;
        if (COUNT) { if (cont) lc.hits++; else lc.misses++; }
        out[(size_t)py * (size_t)F.width + (size_t)px] = make_float4(ps.result.x, ps.result.y, ps.result.z, 1.0f);
    }
    // wave-level compaction of the continuing paths into the wave's own range; entry = this wave's place in its XCD's launch order
    const uint32_t entry = (blockIdx.x & 7u) * (uint32_t)F.slotsPerXcd + (blockIdx.x >> 3);
    const unsigned long long m = __ballot(cont);
    if (cont) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        queue[(size_t)entry * 64 + rank] = pack_bounce(ps, (uint32_t)py * (uint32_t)F.width + (uint32_t)px);
    }
    if ((threadIdx.x & 63) == 0) waveCount[entry] = (uint32_t)__popcll(m);
    if (COUNT) flush_counters(lc, counters);
}

// Exclusive scan of each XCD's wave counts (one 1024-thread workgroup per XCD): offs[x * slots + i] = continuing rays of XCD x's
// waves before wave i, total[x] = all of them.
__global__ __launch_bounds__(1024) void crt_wavefront_scan_kernel(const uint32_t* __restrict__ waveCount, uint32_t* __restrict__ offs, uint32_t* __restrict__ total, int slotsPerXcd)
{
    __shared__ uint32_t s_wave[16];
    const int x = blockIdx.x, tid = threadIdx.x;
    const uint32_t* c = waveCount + (size_t)x * slotsPerXcd;
    uint32_t* o = offs + (size_t)x * slotsPerXcd;
    const int per = (slotsPerXcd + 1023) / 1024, i0 = tid * per, i1 = (i0 + per < slotsPerXcd) ? i0 + per : slotsPerXcd;
    uint32_t sum = 0;
    for (int i = i0; i < i1; ++i) sum += c[i];
    uint32_t incl = sum;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64); if ((tid & 63) >= off) incl += v; }
    if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
    __syncthreads();
    uint32_t base = incl - sum;
    for (int w = 0; w < (tid >> 6); ++w) base += s_wave[w];
    for (int i = i0; i < i1; ++i) { o[i] = base; base += c[i]; }
    if (tid == 1023) total[x] = base;
}

template <bool COUNT>
__global__ __launch_bounds__(CRT_BLOCK, COUNT ? CRT_WAVES_PER_SIMD_COUNT : CRT_WAVES_PER_SIMD) void crt_bounce_kernel(CrtDevScene S, CrtFrame F, float4* __restrict__ out,
                                                               unsigned long long* __restrict__ counters,
                                                               const CrtBounceRay* __restrict__ queue, const uint32_t* __restrict__ offs,
                                                               const uint32_t* __restrict__ total)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    const CrtStack stack = { (crt_lds_u32_ptr)s_stack + threadIdx.x, S.stackOverflow };
    LaneCounters lc; zero_counters(lc);
    const uint32_t xcd = blockIdx.x & 7u;
    const uint32_t n = total[xcd];
    const uint32_t k = (blockIdx.x >> 3) * CRT_BLOCK + threadIdx.x;      // k-th continuing ray of this XCD's tiles, in launch order
    if (k < n) {
        // the wave that queued it: the last entry whose offset is <= k (waves without a continuing ray share their successor's offset)
        const uint32_t* o = offs + (size_t)xcd * (uint32_t)F.slotsPerXcd;
        uint32_t lo = 0, hi = (uint32_t)F.slotsPerXcd;
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (o[mid] <= k) lo = mid; else hi = mid; }
        const CrtBounceRay r = queue[((size_t)xcd * (uint32_t)F.slotsPerXcd + lo) * 64 + (k - o[lo])];
        const float4 partial = out[r.pixel];
        PathState ps = unpack_bounce(r, mk3(partial.x, partial.y, partial.z));
        if (COUNT) { lc.rays++; lc.secondary++; }
        Closest c = closest_hit<opt_if(COUNT, TR_COUNT) | opt_if(policy::kBounceDivides, TR_DIVIDE) | opt_if(policy::kWavefrontOffset32, TR_OFFSET32)>(S, ps.o, ps.d, stack, lc);
        const bool cont = shade_bounce<opt_if(policy::wavefront_sky_double(COUNT), SB_SKY_DOUBLE)>(S, c, ps, 1, F.lightY, F.lightZ) != 0;
        if (COUNT) { if (cont) lc.hits++; else lc.misses++; }
        out[r.pixel] = make_float4(ps.result.x, ps.result.y, ps.result.z, 1.0f);
    }
    if (COUNT) flush_counters(lc, counters);
}

// kernel RayGen as its own launch (only for CRT_RENDER_WRITE_RAYS)
__global__ __launch_bounds__(CRT_BLOCK) void crt_raygen_kernel(CrtFrame F, float* __restrict__ rays)
{
    int px, py;
    if (!lane_pixel(F, px, py)) return;
    v3 d = raygen_dir(F, px, py);
    float* o = rays + 3 * ((size_t)px + (size_t)py * (size_t)F.width);
    o[0] = d.x; o[1] = d.y; o[2] = d.z;
}

// kernel PostProcess (kernel_main.cl:342-359, MathAndSTL.cl:132-169) on the float frame, as its own launch (the default Trace
// kernel applies post_pixel in its epilogue instead; this launch serves FXAA frames and the kernel variants)
__global__ __launch_bounds__(CRT_BLOCK) void crt_postprocess_kernel(CrtFrame F, float4* __restrict__ img)
{
    int px, py;
    if (!lane_pixel(F, px, py)) return;
    const size_t idx = (size_t)py * (size_t)F.width + (size_t)px;
    const float4 p = img[idx];
    const v3 rgb = post_pixel(mk3(p.x, p.y, p.z), px, py, F.width, F.height);
    img[idx] = make_float4(rgb.x, rgb.y, rgb.z, 1.0f);
}

// FXAA (crt_post.h: fxaa_pixel) over the float frame `src`, and the stages behind it
__global__ __launch_bounds__(CRT_BLOCK) void crt_fxaa_kernel(CrtFrame F, const float4* __restrict__ src, float4* __restrict__ dst)
{
    int px, py;
    if (!lane_pixel(F, px, py)) return;
    const int W = F.width, H = F.height;
    v3 o = fxaa_pixel(src, W, H, px, py);
    // the stages behind the filter, on the value in registers: PostProcess, then the store into upstream's RGBA8 target
    if (F.epilogue & CRT_EPILOGUE_POST) o = post_pixel(o, px, py, W, H);
    if (F.epilogue & CRT_EPILOGUE_QUANTIZE) o = quantize3(o);
    dst[(size_t)py * (size_t)W + (size_t)px] = make_float4(o.x, o.y, o.z, 1.0f);
    if (F.packOut) F.packOut[(size_t)py * (size_t)W + (size_t)px] = pack_rgba8(o);
}

// Hazard H8: the store + load through upstream's RGBA8-UNORM render target (write_imagef / read_imagef):
// convert_uchar_sat_rte(x * 255) / 255 per channel, in place (CRT_RENDER_UNORM8), and the packed bytes.
__global__ __launch_bounds__(CRT_BLOCK) void crt_quantize_kernel(CrtFrame F, float4* __restrict__ img)
{
    int px, py;
    if (!lane_pixel(F, px, py)) return;
    const size_t idx = (size_t)py * (size_t)F.width + (size_t)px;
    const float4 p = img[idx];
    img[idx] = make_float4(quantize1(p.x), quantize1(p.y), quantize1(p.z), quantize1(p.w));
}
__global__ void crt_pack_unorm8_kernel(const float4* __restrict__ img, uint32_t* __restrict__ out, size_t pixels)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= pixels) return;
    out[k] = pack_rgba8(img[k]);
}

// ... of the pixels this launch owns only (a device's share of a banded frame: the other rows of `out` belong to other devices' copies)
__global__ __launch_bounds__(CRT_BLOCK) void crt_pack_owned_kernel(CrtFrame F, const float4* __restrict__ img, uint32_t* __restrict__ out)
{
    int px, py;
    if (!lane_pixel(F, px, py)) return;
    const size_t k = (size_t)py * (size_t)F.width + (size_t)px;
    out[k] = pack_rgba8(img[k]);
}
// the float frame back from the bytes of the RGBA8 target: x = byte / 255 -- bit for bit what quantize1 stored (multi-device RGBA8 gather)
__global__ void crt_unpack_unorm8_kernel(const uint32_t* __restrict__ in, float4* __restrict__ img, size_t pixels)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= pixels) return;
    const uint32_t b = in[k];
    img[k] = make_float4((float)(b & 255u) / 255.0f, (float)((b >> 8) & 255u) / 255.0f, (float)((b >> 16) & 255u) / 255.0f, (float)(b >> 24) / 255.0f);
}

// closest-hit query over explicit rays (hit-record parity)
template <bool TLAS>
__global__ __launch_bounds__(CRT_BLOCK, CRT_WAVES_PER_SIMD_COUNT) void crt_query_kernel(CrtDevScene S, const float* __restrict__ origins,
                                                              const float* __restrict__ dirs, int n,
                                                              CrtRayHit* __restrict__ out, unsigned long long* __restrict__ counters)
{
    __shared__ uint32_t s_stack[CRT_LDS_SLOTS * CRT_BLOCK];
    const CrtStackT<TLAS ? CRT_TLAS_PARK : 0> stack = { (crt_lds_u32_ptr)s_stack + threadIdx.x, S.stackOverflow };
    LaneCounters lc; zero_counters(lc);
    const int k = blockIdx.x * CRT_BLOCK + threadIdx.x;
    if (k < n) {
        v3 o = mk3(origins[3 * k], origins[3 * k + 1], origins[3 * k + 2]);
        v3 d = mk3(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]);
        lc.rays++;
        Closest c = closest_hit<TR_COUNT | opt_if(TLAS, TR_TLAS) | opt_if(policy::kQueryDivides, TR_DIVIDE) | opt_if(policy::kQueryOffset32, TR_OFFSET32)>(S, o, d, stack, lc);
        CrtRayHit h;
        if (c.anyHit) { h.t = c.hit.t; h.u = c.hit.u; h.v = c.hit.v; h.triIndex = c.hit.tri; h.instance = c.hitInstance; lc.hits++; }
        else { h.t = c.distance; h.u = 0.0f; h.v = 0.0f; h.triIndex = 0; h.instance = -1; lc.misses++; }
        out[k] = h;
    }
    flush_counters(lc, counters);
}

