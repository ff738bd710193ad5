// crt_frame.h -- one frame: feedback launch lists, the Trace launch by kernel structure, frame slots and events (Renderer.cpp:305-375), the host-memory query (crt_query_hits), reads, statistics
// Part of the one translation unit crt_shim.hip (included there, in this order: crt_own.h, crt_state.h, crt_instances.h, crt_upload.h,
// crt_bvh_driver.h, crt_frame.h, crt_query_host.h, crt_ao_host.h, crt_multidev.h); everything here has internal linkage.
#pragma once
namespace {

// the device counters of the last counted launch -> g.lastCounters, g.lastCulled
static void unpack_counters(const unsigned long long c[CRT_NUM_COUNTERS])
{
    CrtCounters& o = g.lastCounters;
    o.rays = c[0]; o.primary = c[1]; o.secondary = c[2]; o.hits = c[3]; o.misses = c[4]; o.traversals = c[5];
    o.pops = c[6]; o.innerVisits = c[7]; o.triTests = c[8]; o.capHits = c[9]; o.stackOverflows = c[10]; o.maxStack = c[11];
    o.shadowRays = c[12]; o.shadowHits = c[13]; g.lastCulled = c[14];
}

// Event timing is read back lazily: when the slot is about to be reused (which also bounds the frames in flight to
// one per slot), or when somebody asks. Synchronous frames are complete by then, so this never blocks them.
int collect_set(EventSet& es)
{
    if (!es.pending) return CRT_OK;
    const Event* ev = es.ev;
    hipEvent_t traceStart = es.evRaygen ? ev[1] : ev[0], frameEnd = es.evPost ? ev[3] : ev[2];
    HIPCHK(hipEventSynchronize(frameEnd));
    float ms[4] = { 0, 0, 0, 0 };
    HIPCHK(hipEventElapsedTime(&ms[0], ev[0], frameEnd));
    if (es.evRaygen) HIPCHK(hipEventElapsedTime(&ms[1], ev[0], ev[1]));
    HIPCHK(hipEventElapsedTime(&ms[2], traceStart, ev[2]));
    if (es.evPost) HIPCHK(hipEventElapsedTime(&ms[3], ev[2], ev[3]));
    for (int k = 0; k < 4; ++k) g.msSum[k] += (double)ms[k];
    g.framesTimed++;
    if (g.statStartValid && es.seq >= g.statStartSeq) {
        float ext = 0;
        HIPCHK(hipEventElapsedTime(&ext, g.statStart, frameEnd));
        if ((double)ext > g.statExtent) g.statExtent = (double)ext;
        if (es.seq == g.statStartSeq) g.statFirstMs = (double)ext;      // the first frame of the extent: fill time of the pipeline
        if (g.frameLogN < 256) {
            float st = 0;
            if (hipEventElapsedTime(&st, g.statStart, ev[0]) == hipSuccess) { g.frameLog[2 * g.frameLogN] = (double)st; g.frameLog[2 * g.frameLogN + 1] = (double)ext; g.frameLogN++; }
        }
    }
    if (es.seq >= g.msSeq) { memcpy(g.ms, ms, sizeof ms); g.msSeq = es.seq; }
    if ((es.flags & CRT_RENDER_ASYNC) && !(es.flags & (CRT_RENDER_COUNTERS | CRT_RENDER_STAMPS | CRT_RENDER_WRITE_RAYS))) g.pipelinedLatencyMs = ms[0];
    if (es.flags & CRT_RENDER_COUNTERS) {
        unsigned long long c[CRT_NUM_COUNTERS];
        HIPCHK(hipMemcpy(c, g.counters, sizeof c, hipMemcpyDeviceToHost));
        unpack_counters(c);
    }
    es.pending = false;
    return CRT_OK;
}

int collect_timing()
{
    for (int i = 0; i < g.nSlots; ++i) {
        FrameSlot& fs = g.slot[i];
        const int older = fs.es[0].seq <= fs.es[1].seq ? 0 : 1;
        RCCHK(collect_set(fs.es[older]));
        RCCHK(collect_set(fs.es[older ^ 1]));
    }
    return CRT_OK;
}

// Whether a frame with these flags rotates over the frame slots (crt1_render and the multi-device dispatcher). Everything
// else -- synchronous frames, the diagnostic flags (they share the counters, the stamp and ray buffers) -- runs on slot 0.
static bool frame_is_pipelined(int flags) { return (flags & CRT_RENDER_ASYNC) && !(flags & (CRT_RENDER_WRITE_RAYS | CRT_RENDER_COUNTERS | CRT_RENDER_STAMPS)); }

// Feedback launch lists for the megakernel (lane_pixel / crt_order_kernel). Buffers follow the frame geometry; a
// change of geometry resets to the identity order. The previous frame's per-tile costs are turned into this frame's
// lists (and the costs zeroed) by a sort that is queued right AFTER the previous frame's last kernel and its end
// event (sort_for_next_frame), so it runs while the host is between two crt1_render calls and is off the frame's
// critical path.
// One allocation per slot (FrameSlot::lists), for n = 8 x listCap entries: order[n] | per-tile costs[n] | sort keys[n] | the 8 list lengths.
// The sort's launches on a `lists` allocation (a slot's, or crt_debug_launch_lists' scratch copy): spread > 0 ranks by the neighbours too
static void launch_list_kernels(uint32_t* lists, int slotsPerXcd, int listCap, int tilesX, float spread, uint32_t maxSplit, float splitFactor, hipStream_t stream)
{
    const size_t n = (size_t)8 * (size_t)listCap;
    uint32_t* cost = lists + n; uint32_t* key = cost;
    if (spread > 0.0f) {
        key = cost + n;
        crt_cost_spread_kernel<<<(8 * slotsPerXcd + 255) / 256, 256, 0, stream>>>(cost, key, slotsPerXcd, tilesX, spread);
    }
    crt_order_kernel<<<8, 1024, 0, stream>>>(cost, key, lists, lists + 3 * n, slotsPerXcd, listCap, maxSplit, splitFactor);
}
static void launch_identity_lists(uint32_t* lists, int slotsPerXcd, int listCap, hipStream_t stream)
{
    crt_identity_order_kernel<<<(8 * slotsPerXcd + 255) / 256, 256, 0, stream>>>(lists, lists + 3 * (size_t)8 * (size_t)listCap, slotsPerXcd, listCap);
}

// this frame's per-tile costs -> the next frame's lists; with g.costSpread > 0 a tile is ranked by its neighbours' costs too
static void launch_order_kernel(const CrtFrame& F, FrameSlot& fs, bool pipelined, bool noSplit)
{
    launch_list_kernels(fs.lists, F.slotsPerXcd, F.listCap, F.tilesX, g.viewMoved ? g.costSpread : 0.0f, noSplit ? 0u : (uint32_t)(pipelined ? g.maxSplitPipelined : g.maxSplit),
                        (pipelined ? g.splitBetaAsync : g.splitBeta) / (float)((g.numCUs / 8) * 4 * CRT_WAVES_PER_SIMD), fs.stream);
}

// noSplit: the lists of the refill / block forms, whose entries are blocks of tiles, are never split
static int prepare_launch_lists(CrtFrame& F, unsigned& grid, FrameSlot& fs, bool pipelined, bool noSplit = false)
{
    const int key[7] = { g.width, g.height, g.bandRows, g.rank, g.nRanks, F.slotsPerXcd, F.ss };   // ss: another factor is another tile grid
    F.listCap = F.slotsPerXcd + 3 * CRT_MAX_SPLIT;
    const size_t n = (size_t)8 * (size_t)F.listCap;
    if (3 * n + 8 > fs.lists.capacity()) fs.orderSlots = -1;     // new memory: start from the identity order
    RCCHK(fs.lists.grow(3 * n + 8, fs.stream));
    if (fs.orderSlots != F.slotsPerXcd || memcmp(key, fs.orderKey, sizeof key) != 0) {
        HIPCHK(hipMemsetAsync(fs.lists + n, 0, sizeof(uint32_t) * n, fs.stream));
        launch_identity_lists(fs.lists, F.slotsPerXcd, F.listCap, fs.stream);
        fs.orderSlots = F.slotsPerXcd; memcpy(fs.orderKey, key, sizeof key);
    } else if (!fs.listsReady) {
        launch_order_kernel(F, fs, pipelined, noSplit);
    }
    fs.listsReady = false;
    HIPCHK(hipGetLastError());
    F.order = fs.lists; F.cost = fs.lists + n; F.listLen = fs.lists + 3 * n;
    grid = 8u * (unsigned)F.listCap;
    return CRT_OK;
}

// Queued behind a frame's last kernel: this frame's costs -> the next frame's lists (same geometry assumed; a change is
// caught by the key in prepare_launch_lists, which then starts from the identity order again).
static int sort_for_next_frame(const CrtFrame& F, FrameSlot& fs, bool pipelined, bool noSplit)
{
    launch_order_kernel(F, fs, pipelined, noSplit);
    HIPCHK(hipGetLastError());
    fs.listsReady = true;
    return CRT_OK;
}

// CRT_RENDER_DIAG_MIX3: three copies of the plain row-interleaved order, copy j starting a third of the XCD's list later:
// entry 3 i + j = tile (i + j S / 3) mod S. One allocation: the 8 lists, then their 8 lengths.
static int prepare_mix3_lists(CrtFrame& F, unsigned& grid, FrameSlot& fs)
{
    const int S = F.slotsPerXcd, S3 = 3 * S;
    const size_t entries = (size_t)8 * S3;
    if (entries + 8 > fs.mixOrder.capacity()) fs.mixSlots = -1;       // new memory: write the lists
    RCCHK(fs.mixOrder.grow(entries + 8, fs.stream));
    if (fs.mixSlots != S) {
        std::vector<uint32_t> h(entries + 8, (uint32_t)S3);
        for (int x = 0; x < 8; ++x)
            for (int i = 0; i < S; ++i)
                for (int j = 0; j < 3; ++j) h[(size_t)x * S3 + 3 * i + j] = (uint32_t)((i + j * (S / 3)) % S);
        HIPCHK(hipMemcpyAsync(fs.mixOrder, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, fs.stream));
        HIPCHK(hipStreamSynchronize(fs.stream));      // the host vector goes out of scope
        fs.mixSlots = S;
    }
    F.order = fs.mixOrder; F.listLen = fs.mixOrder + entries; F.listCap = S3; F.cost = nullptr;
    grid = 8u * (unsigned)S3;
    return CRT_OK;
}

// CRT_KERNEL=ldstop: one workgroup per CRT_TOP_WAVES tiles of each XCD's list
static unsigned ldstop_grid(const CrtFrame& F) { return (unsigned)((F.slotsPerXcd + CRT_TOP_WAVES - 1) / CRT_TOP_WAVES) * 8u; }

// TLAS: more than CRT_TLAS_MIN_INSTANCES instances and an instance tree to walk (CRT_TLAS=0/1 forces). S.tlasNodes = 0: no
// tree, or a launch without the cull.
static bool use_tlas(const CrtDevScene& S) { return S.tlasNodes > 0 && S.numInstances <= g.instHigh && (g.forceTlas >= 0 ? g.forceTlas != 0 : S.numInstances > CRT_TLAS_MIN_INSTANCES); }

// F in plain row-interleaved order (no launch lists); `whole`: every tile row of the frame, as if one rank rendered it all.
// Of an SSAA frame: the output frame W x H (the per-pixel stages behind Trace run on the resolved pixels).
static CrtFrame plain_frame(const CrtFrame& F, bool whole)
{
    CrtFrame P = F;
    P.order = nullptr; P.cost = nullptr; P.listLen = nullptr;
    if (F.ss > 1) {
        P.ss = 1; P.width = g.width; P.height = g.height; P.tileRowsPerBand = g.bandRows / CRT_TILE;
        set_tile_grid(P, owned_tile_rows(g.height, g.bandRows), (g.width + CRT_TILE - 1) / CRT_TILE);
    }
    if (whole) { P.rank = 0; P.nRanks = 1; set_tile_grid(P, (g.height + CRT_TILE - 1) / CRT_TILE, P.tilesX); }
    return P;
}

static bool is_primary() { return g.groupSize > 1 && g.primary == G; }
static bool is_secondary() { return g.groupSize > 1 && g.primary != G; }

// In a multi-device session the dispatcher (crt_render) decides once per frame what every device must agree on and hands it
// to each device's crt1_render: the frame slot (so a device that owned no rows of some frame, or failed one, cannot fall out
// of step with the primary's slot rotation) and whether the call may return before the device has finished (secondaries
// never wait on the host: the primary's end-of-frame event waits for their partDone events, which is what gives a
// synchronous N-device frame the duration of the longest share instead of the sum of two).
struct RenderPlan { int slot; bool noHostWait; };

// What the stages of one crt1_render share
struct FrameCtx {
    int flags = 0; const RenderPlan* plan = nullptr; bool pipelined = false;
    int slot = 0; FrameSlot* fs = nullptr; EventSet* es = nullptr;
    CrtFrame F; unsigned grid = 0;       // the frame in tiles (RayGen, the per-pixel stages); its workgroups: one per tile or list entry
    CrtFrame T; unsigned gridT = 0;      // the Trace launch: F, or for refill / block the same frame in blocks of tiles
    CrtDevScene S;
    // fused: the Trace launch applied F.epilogue itself; gather8: frame_gathers_rgba8; packInKernel: the kernel that stores a
    // final pixel stores its RGBA8 bytes too
    bool fused = false, gather8 = false, packInKernel = false;
};

// CRT_RENDER_GBUFFER: bytes per pixel of plane `plane` (CRT_GBUFFER_*; 0: no such plane), and the planes of a slot that holds them
#define CRT_GBUFFER_PIXEL_BYTES 36
static size_t gbuffer_plane_pixel_bytes(int plane) { return plane == CRT_GBUFFER_GEOMETRY || plane == CRT_GBUFFER_IDS ? 16 : plane == CRT_GBUFFER_ALBEDO ? 4 : 0; }
static CrtGBuffer slot_gbuffer(const FrameSlot& fs) { CrtGBuffer gb; gb.planes = fs.gbuf; return gb; }

// Run-time bools -> template arguments: with_bools(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...), so a
// generic lambda can name the kernel instantiation: K<decltype(A)::value, ...>.
template <class Fn> static void with_bools(Fn&& f) { f(); }
template <class Fn, class... Rest> static void with_bools(Fn&& f, bool b, Rest... rest)
{
    if (b) with_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else with_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

// The Trace launch(es) of one frame, by kernel form, on c.T and c.gridT. `out`: the frame the launch writes (the slot's frame,
// or its unfiltered copy when FXAA follows). Sets c.fused: every form but wavefront applies T.epilogue (RGBA8 target /
// PostProcess) in the Trace kernel.
static int launch_trace(FrameCtx& c, float4* out)
{
    const CrtDevScene& S = c.S; const CrtFrame& T = c.T; const unsigned grid = c.gridT; FrameSlot& fs = *c.fs;
    const bool count = (c.flags & CRT_RENDER_COUNTERS) != 0;
    if (count) HIPCHK(hipMemsetAsync(g.counters, 0, CRT_NUM_COUNTERS * sizeof(unsigned long long), fs.stream));
    c.fused = true;
    if (c.flags & CRT_RENDER_STAMPS) {   // diagnostic launch with per-wave stamps (megakernel, refill, block): the stamped instantiation applies T.epilogue too
        const size_t words = 16 + (size_t)grid * 8;
        RCCHK(g.stamps.grow(words, fs.stream));
        g.stampWaves = grid;
        HIPCHK(hipMemsetAsync(g.stamps, 0, words * sizeof(unsigned long long), fs.stream));
        if (g.form == Form::Block) crt_trace_block_kernel<false, true><<<grid, CRT_BLOCK, 0, fs.stream>>>(S, T, out, g.stamps, fs.blockQueue);
        else if (g.form == Form::Refill) crt_trace_refill_kernel<false, true><<<grid, CRT_BLOCK, 0, fs.stream>>>(S, T, out, g.stamps);
        else crt_trace_kernel<false, true><<<grid, CRT_BLOCK, 0, fs.stream>>>(S, T, out, g.stamps);
        snprintf(g.lastKernel, sizeof g.lastKernel, "%s", g.form == Form::Block ? "crt_trace_block_kernel<0,1>" : g.form == Form::Refill ? "crt_trace_refill_kernel<0,1>" : "crt_trace_kernel<0,1,0,0,0>");
        HIPCHK(hipGetLastError());
        return CRT_OK;
    }
    // crt_debug_last_kernel: the Trace launch(es) of this frame under the names rocprofv3 prints for them
    switch (g.form) {
    case Form::Refill:                   // in-tile lane refill / block compaction (crt_refill.h); T counts blocks, not tiles
        snprintf(g.lastKernel, sizeof g.lastKernel, "crt_trace_refill_kernel<%d,0>", (int)count);
        with_bools([&](auto C) { crt_trace_refill_kernel<decltype(C)::value><<<grid, CRT_BLOCK, 0, fs.stream>>>(S, T, out, g.counters); }, count);
        break;
    case Form::Block:
        snprintf(g.lastKernel, sizeof g.lastKernel, "crt_trace_block_kernel<%d,0>", (int)count);
        with_bools([&](auto C) { crt_trace_block_kernel<decltype(C)::value><<<grid, CRT_BLOCK, 0, fs.stream>>>(S, T, out, g.counters, fs.blockQueue); }, count);
        break;
    case Form::LdsTop:                   // four tiles per workgroup sharing an LDS copy of the tree tops (crt_ldstop.h)
        snprintf(g.lastKernel, sizeof g.lastKernel, "crt_trace_ldstop_kernel<%d>", (int)count);
        with_bools([&](auto C) { crt_trace_ldstop_kernel<decltype(C)::value><<<ldstop_grid(T), CRT_BLOCK * CRT_TOP_WAVES, 0, fs.stream>>>(S, T, out, g.counters); }, count);
        break;
    case Form::Wavefront: {              // bounce 0, ballot compaction, bounce 1
        c.fused = false;
        snprintf(g.lastKernel, sizeof g.lastKernel, "crt_primary_kernel<%d>+crt_wavefront_scan_kernel+crt_bounce_kernel<%d>", (int)count, (int)count);
        // per-slot state (prepare_lists sized it): queue = one 64-record range per primary wave; counts, offsets, per-XCD totals
        uint32_t* cnt = fs.wfCount; uint32_t* offs = cnt + grid; uint32_t* total = offs + grid;
        with_bools([&](auto C) {
            crt_primary_kernel<decltype(C)::value><<<grid, CRT_BLOCK, 0, fs.stream>>>(S, T, out, g.counters, fs.blockQueue, cnt);
            crt_wavefront_scan_kernel<<<8, 1024, 0, fs.stream>>>(cnt, offs, total, T.slotsPerXcd);
            // an XCD's tiles can all continue: the bounce launch has the primary launch's shape (waves past their XCD's total leave at once)
            crt_bounce_kernel<decltype(C)::value><<<grid, CRT_BLOCK, 0, fs.stream>>>(S, T, out, g.counters, fs.blockQueue, offs, total);
        }, count);
        break;
    }
    case Form::Mega: {                   // <COUNT, STAMP, SHADOW, TLAS, REFRACT>; a supersampled frame (CRT_RENDER_SSAA2 / SSAA4; c.T is the virtual frame): <COUNT, SHADOW, TLAS, REFRACT>
        const bool shadow = (c.flags & CRT_RENDER_SHADOWS) != 0, refract = (c.flags & CRT_RENDER_REFRACTION) != 0, tlas = use_tlas(S);
        if (c.flags & CRT_RENDER_GBUFFER) {   // <SHADOW, TLAS, REFRACT> (never counted or supersampled: refuse_gbuffer), the slot's planes as its own argument
            const CrtGBuffer gb = slot_gbuffer(fs);
            snprintf(g.lastKernel, sizeof g.lastKernel, "crt_trace_gbuffer_kernel<%d,%d,%d>", (int)shadow, (int)tlas, (int)refract);
            with_bools([&](auto Sh, auto Tl, auto R) {
                crt_trace_gbuffer_kernel<decltype(Sh)::value, decltype(Tl)::value, decltype(R)::value><<<grid, CRT_BLOCK, 0, fs.stream>>>(S, T, out, gb);
            }, shadow, tlas, refract);
            break;
        }
        if (T.ss > 1) snprintf(g.lastKernel, sizeof g.lastKernel, "crt_trace_ssaa_kernel<%d,%d,%d,%d>", (int)count, (int)shadow, (int)tlas, (int)refract);
        else snprintf(g.lastKernel, sizeof g.lastKernel, "crt_trace_kernel<%d,0,%d,%d,%d>", (int)count, (int)shadow, (int)tlas, (int)refract);
        with_bools([&](auto C, auto Sh, auto Tl, auto R) {
            constexpr bool kC = decltype(C)::value, kSh = decltype(Sh)::value, kTl = decltype(Tl)::value, kR = decltype(R)::value;
            if (T.ss > 1) crt_trace_ssaa_kernel<kC, kSh, kTl, kR><<<grid, CRT_BLOCK, 0, fs.stream>>>(S, T, out, g.counters);
            else crt_trace_kernel<kC, false, kSh, kTl, kR><<<grid, CRT_BLOCK, 0, fs.stream>>>(S, T, out, g.counters);
        }, count, shadow, tlas, refract);
        break;
    }
    }
    HIPCHK(hipGetLastError());
    return CRT_OK;
}

// The frame's launch lists, then what its kernel form's Trace launch needs: its frame and grid (c.T, c.gridT), its queues,
// and the slot's traversal-stack overflow area. Feedback launch lists serve synchronous frames, whose end is decided by their
// slowest waves. With frames in flight the tail is hidden by the next frame and the lists only cost (cost atomics, the sort
// launch, quadrant waves at a quarter of the lane utilisation): 7.58 with, 7.72 Gray/s without on multi-1M -> pipelined
// frames use the plain row-interleaved order.
static int prepare_lists(FrameCtx& c)
{
    FrameSlot& fs = *c.fs;
    const bool feedback = g.feedback && (!c.pipelined || g.feedbackAsync);
    c.grid = (unsigned)c.F.gridBlocks;
    if (c.flags & CRT_RENDER_DIAG_MIX3) RCCHK(prepare_mix3_lists(c.F, c.grid, fs));
    else if (feedback && g.form == Form::Mega) RCCHK(prepare_launch_lists(c.F, c.grid, fs, c.pipelined));
    c.T = c.F; c.gridT = c.grid;
    size_t ovfBlocks = c.grid;           // one overflow block per workgroup of the largest launch of this frame
    switch (g.form) {
    case Form::Mega: break;
    case Form::Refill:
    case Form::Block: {                  // the Trace launch (and its feedback lists) count blocks of tiles where F counts tiles
        const int tiles = g.form == Form::Block ? CRT_BLOCK_TILES : CRT_REFILL_TILES;
        set_tile_grid(c.T, c.F.ownedTileRows, (c.F.tilesX + tiles - 1) / tiles);
        c.gridT = (unsigned)c.T.gridBlocks;
        if (feedback) RCCHK(prepare_launch_lists(c.T, c.gridT, fs, c.pipelined, true));
        if (g.form == Form::Block) RCCHK(fs.blockQueue.grow((size_t)c.T.gridBlocks * CRT_BLOCK_PIXELS, fs.stream));
        break;
    }
    case Form::Wavefront:                // this slot's queue (64 records per primary wave), counts + offsets + per-XCD totals
        RCCHK(fs.blockQueue.grow((size_t)c.grid * 64, fs.stream));
        RCCHK(fs.wfCount.grow((size_t)c.grid * 2 + 8, fs.stream));
        break;
    case Form::LdsTop: ovfBlocks = (size_t)ldstop_grid(c.F) * CRT_TOP_WAVES; break;   // one block per WAVE of the four-wave workgroups
    }
    return ensure_overflow(fs, ovfBlocks);
}

// Multi-device session: does a frame with these flags travel to the primary as RGBA8 bytes (4 B per pixel) instead of float4 (16 B)?
// Upstream's render target IS RGBA8 (Renderer.cpp:63,192), CRT_RENDER_UNORM8 quantises every pixel in the Trace epilogue anyway, so the
// bytes carry the whole frame: at 8 GPUs 7 x 4.1 MB instead of 7 x 16.6 MB per 3840x2160 frame converge on the primary's links. FXAA
// frames keep the float gather (the filter runs on the primary over the gathered Trace result).
static bool frame_gathers_rgba8(int flags) { return g.groupSize > 1 && g.gather8 && (flags & CRT_RENDER_UNORM8) && !(flags & CRT_RENDER_FXAA); }
// every slot's byte frame allocated (the dispatcher calls this on every device BEFORE the secondaries submit: they copy into the primary's)
int crt1_prepare_gather8(void)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    for (int i = 0; i < g.nSlots; ++i) RCCHK(g.slot[i].packBuf.grow((size_t)g.width * (size_t)g.height, g.slot[i].stream));
    return CRT_OK;
}
// the float frame of slot `fs` from its byte frame, if the last frame on it was gathered as RGBA8 (the caller has drained the streams)
static int expand_rgba8_frame(FrameSlot& fs)
{
    if (!fs.frameIs8) return CRT_OK;
    const size_t pixels = (size_t)g.width * (size_t)g.height;
    crt_unpack_unorm8_kernel<<<(unsigned)((pixels + 255) / 256), 256, 0, fs.stream>>>(fs.packBuf, fs.out, pixels);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(fs.stream));
    fs.frameIs8 = false;
    return CRT_OK;
}

// one wave that occupies its stream for `ticks` periods of the 100 MHz real-time counter (start-up stagger, see State::burstFrames)
__global__ void crt_delay_kernel(unsigned long long ticks)
{
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long guard = 0;
    while (__builtin_amdgcn_s_memrealtime() - r0 < ticks && guard < (1ull << 22)) { __builtin_amdgcn_s_sleep(16); ++guard; }
}

// A device that owns no rows of this frame still takes part in the frame's hand-shake: its "bands have arrived" event is
// recorded on the planned slot, so the primary's wait refers to this frame, not to an older one.
static int record_empty_share(const RenderPlan* plan)
{
    if (plan && is_secondary() && plan->slot >= 0 && plan->slot < g.nSlots) {
        FrameSlot& fs = g.slot[plan->slot];
        if (plan->slot != 0) g.othersBusy = true;
        HIPCHK(hipEventRecord(fs.partDone, fs.stream));
    }
    return CRT_OK;
}

// k of a frame's k x k supersampling (CRT_RENDER_SSAA2 / SSAA4; both at once is refused by crt1_render before this is asked)
static int ssaa_factor(int flags) { return (flags & CRT_RENDER_SSAA4) ? 4 : (flags & CRT_RENDER_SSAA2) ? 2 : 1; }
#define CRT_SSAA_MAX_PIXELS (7680ull * 4320ull)

// The frame's supersampling rules (CRT_E_UNSUPPORTED): the default kernel form only; no per-wave stamps, no ray buffer (it is W x H),
// no three-frame mix; a virtual frame of at most 7680 x 4320 pixels (the traversal-stack overflow area is sized per workgroup of the
// virtual grid: 2.3 GB per slot at that size). The multi-device dispatcher asks too, before it advances the slot rotation.
static int refuse_ssaa(int flags)
{
    const int ss = ssaa_factor(flags);
    if (ss == 1) return CRT_OK;
    if (g.form != Form::Mega || (flags & (CRT_RENDER_STAMPS | CRT_RENDER_WRITE_RAYS | CRT_RENDER_DIAG_MIX3))) return CRT_E_UNSUPPORTED;
    if ((unsigned long long)g.width * (unsigned long long)g.height * (unsigned long long)(ss * ss) > CRT_SSAA_MAX_PIXELS) return CRT_E_UNSUPPORTED;
    return CRT_OK;
}

// The rules of a frame with the first-hit planes (CRT_RENDER_GBUFFER, CRT_E_UNSUPPORTED): the default kernel form on one device; no
// supersampling (the planes hold one primary ray per pixel), no per-wave stamps, no three-frame mix, no counters (which keeps the
// kernel at 8 instantiations instead of 16); fewer than 2^28 pixels (GBufferSink addresses a plane with 32-bit byte offsets).
static int refuse_gbuffer(int flags)
{
    if (!(flags & CRT_RENDER_GBUFFER)) return CRT_OK;
    if ((unsigned long long)g.width * (unsigned long long)g.height >= (1ull << 28)) return CRT_E_UNSUPPORTED;
    if (g.form != Form::Mega || g.groupSize > 1) return CRT_E_UNSUPPORTED;
    if (flags & (CRT_RENDER_SSAA2 | CRT_RENDER_SSAA4 | CRT_RENDER_STAMPS | CRT_RENDER_DIAG_MIX3 | CRT_RENDER_COUNTERS)) return CRT_E_UNSUPPORTED;
    return CRT_OK;
}

// Every CRT_E_UNSUPPORTED rule of a frame, checked before the frame changes any state. A frame the session's kernel form
// cannot render is refused, never rendered by another kernel behind the caller's back.
static int refuse_unsupported(int flags, uint32_t numMeshes)
{
    const bool stamped = (flags & CRT_RENDER_STAMPS) != 0;
    if ((flags & (CRT_RENDER_SHADOWS | CRT_RENDER_REFRACTION)) && stamped) return CRT_E_UNSUPPORTED;   // the stamped instantiation is the plain one
    // The opt-in forms lack shadow rays, refraction, the three-frame diagnostic mix and the instance tree (CRT_TLAS=1);
    // wavefront and ldstop the stamped launch; refill and block more than 64 instances (one 64-bit candidate mask per lane).
    if (g.form != Form::Mega) {
        if (flags & (CRT_RENDER_SHADOWS | CRT_RENDER_REFRACTION | CRT_RENDER_DIAG_MIX3)) return CRT_E_UNSUPPORTED;
        if (g.forceTlas == 1) return CRT_E_UNSUPPORTED;
        if ((g.form == Form::Wavefront || g.form == Form::LdsTop) && stamped) return CRT_E_UNSUPPORTED;
        if ((g.form == Form::Refill || g.form == Form::Block) && numMeshes > 64u) return CRT_E_UNSUPPORTED;
    }
    if ((flags & CRT_RENDER_FXAA) && g.groupSize <= 1 && g.nRanks > 1) return CRT_E_UNSUPPORTED;   // the filter reads across band edges
    RCCHK(refuse_ssaa(flags));
    RCCHK(refuse_gbuffer(flags));
    // the three-frame mix: a synchronous frame of one device, without the other diagnostics or FXAA
    if ((flags & CRT_RENDER_DIAG_MIX3) && (frame_is_pipelined(flags) || g.groupSize > 1 || (flags & (CRT_RENDER_STAMPS | CRT_RENDER_WRITE_RAYS | CRT_RENDER_FXAA))))
        return CRT_E_UNSUPPORTED;
    return CRT_OK;
}

// Slot choice: pipelined frames rotate over the frame slots so consecutive frames overlap (each slot has its own stream,
// output buffer, launch lists and queues); every other frame runs on slot 0 once the other slots have drained.
static int choose_slot(FrameCtx& c)
{
    c.pipelined = frame_is_pipelined(c.flags);
    c.slot = 0;
    if (c.pipelined) c.slot = c.plan ? c.plan->slot : (int)(g.asyncSeq++ % (unsigned)g.nSlots);   // a session's dispatcher chose it for every device
    if (c.slot < 0 || c.slot >= g.nSlots) return CRT_E_BAD_ARGUMENT;
    if (!c.pipelined) RCCHK(quiesce());
    c.fs = &g.slot[c.slot];
    c.es = &c.fs->es[c.fs->frames & 1u];
    RCCHK(collect_set(*c.es));               // waits for the frame two back on this slot: at most two queued per slot
    if (c.flags & CRT_RENDER_COUNTERS) RCCHK(collect_timing());
    if (c.slot != 0) g.othersBusy = true;
    return ensure_slot_instances(*c.fs);     // this slot's instance tables, refreshed on its stream if an upload happened since
}

// The scene as this frame sees it, the start of the statistics extent, the start-up stagger, the frame's first event and RayGen.
// events: [0] frame start, [1] Trace start, [2] Trace end, [3] end of PostProcess = frame end.
// A plain frame records only two (RayGen is fused, PostProcess off): [0] == [1], [2] == [3].
static int begin_frame(FrameCtx& c, const CrtTraceArgs* args)
{
    FrameSlot& fs = *c.fs; EventSet& es = *c.es;
    fill_scene(c.S, args->numMeshes, fs, beyond_cull_range(sqrt((double)args->cameraPos[0] * args->cameraPos[0] + (double)args->cameraPos[1] * args->cameraPos[1] + (double)args->cameraPos[2] * args->cameraPos[2])));
    if (g.statStartArmed) {                  // first frame since the statistics were reset: start of the extent
        HIPCHK(hipEventRecord(g.statStart, fs.stream));
        g.statStartArmed = false; g.statStartValid = true; g.statStartSeq = g.frameSeq + 1; g.statExtent = 0; g.statFirstMs = 0; g.frameLogN = 0;
    }
    if (c.pipelined) {
        // first frame of this slot in a burst that starts from an idle device: hold it back so the slots do not run in lockstep
        const unsigned k = g.burstFrames++;
        // (automatic only with up to three slots: with eight -- a rank's small share of a tiled frame, where one frame cannot fill the
        // GPU and the slots exist to run many at once -- the ramp costs more than the coinciding tails: 83.2 -> 74.6 Gray/s predicted at N = 8)
        if (k > 0 && k < (unsigned)g.nSlots && g.staggerUs != 0 && (g.staggerUs > 0 || (g.nSlots <= 3 && g.prevBurstFrames > (unsigned)g.nSlots))) {
            double step = g.staggerUs > 0 ? (double)g.staggerUs : (double)g.pipelinedLatencyMs * 1e3 / (double)g.nSlots;
            if (step > 500.0) step = 500.0;                      // a stale or foreign latency must not stall a burst
            const double us = step * k;
            if (us >= 5.0) { crt_delay_kernel<<<1, 64, 0, fs.stream>>>((unsigned long long)(us * 100.0)); HIPCHK(hipGetLastError()); g.staggeredFrames++; }
        }
    } else { if (g.burstFrames) g.prevBurstFrames = g.burstFrames; g.burstFrames = 0; }
    es.evRaygen = (c.flags & CRT_RENDER_WRITE_RAYS) != 0;
    es.evPost = (c.flags & (CRT_RENDER_POSTPROCESS | CRT_RENDER_UNORM8 | CRT_RENDER_FXAA)) != 0;
    HIPCHK(hipEventRecord(es.ev[0], fs.stream));
    if (es.evRaygen) {
        crt_raygen_kernel<<<c.grid, CRT_BLOCK, 0, fs.stream>>>(c.F, g.rays);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(es.ev[1], fs.stream));
    }
    return CRT_OK;
}

// In-process multi-GPU, primary device: the frame is complete when every secondary's bands have arrived -- its last event is
// recorded behind waits for their partDone events (recorded before this call: the dispatcher submits the secondaries first).
static int wait_for_parts(const FrameCtx& c)
{
    for (int d = 1; d < g.groupSize; ++d) HIPCHK(hipStreamWaitEvent(c.fs->stream, g.group[d]->slot[c.slot].partDone, 0));
    return CRT_OK;
}

// The Trace launch and the per-pixel stages behind it, up to the frame's end event. Upstream's stages behind Trace (its RGBA8
// render target, PostProcess) ride in the Trace kernel's epilogue unless the kernel form has none. FXAA sits between them and
// reads neighbours: on one device Trace then writes the slot's second buffer (its pixels already through the RGBA8 target) and
// the filter writes the frame, applying PostProcess and the final RGBA8 store in ITS epilogue -- two launches, no copy.
static int launch_passes(FrameCtx& c)
{
    FrameSlot& fs = *c.fs; EventSet& es = *c.es; CrtFrame& F = c.F;
    const bool unorm = (c.flags & CRT_RENDER_UNORM8) != 0, post = (c.flags & CRT_RENDER_POSTPROCESS) != 0, fxaa = (c.flags & CRT_RENDER_FXAA) != 0;
    const bool fxaaLocal = fxaa && g.groupSize <= 1;
    const size_t framePixels = (size_t)g.width * (size_t)g.height;
    if (fxaa && !is_secondary()) RCCHK(fs.aux.grow(framePixels, fs.stream));
    if (c.flags & CRT_RENDER_GBUFFER) {
        RCCHK(fs.gbuf.grow(framePixels * CRT_GBUFFER_PIXEL_BYTES, fs.stream));
        // an AO query may still read this slot's planes (crt_frame_ao): the frame waits for it on the device, the host does not
        if (fs.aoPending && g.rayQuery.inFlight) HIPCHK(hipStreamWaitEvent(fs.stream, g.rayQuery.raysDone, 0));
        fs.aoPending = false;
    }
    if (!fxaa) F.epilogue = (unorm ? CRT_EPILOGUE_QUANTIZE : 0u) | (post ? CRT_EPILOGUE_POST : 0u);
    else if (fxaaLocal) F.epilogue = unorm ? CRT_EPILOGUE_QUANTIZE : 0u;
    // the kernel that stores the final pixel stores its four bytes too: for a read-back of the RGBA8 frame on one device (a
    // multi-device session packs the gathered frame on its first device), and on every device of a session whose RGBA8 frames
    // are gathered as bytes
    c.gather8 = frame_gathers_rgba8(c.flags);
    c.packInKernel = unorm && (((c.flags & CRT_RENDER_READBACK) && g.groupSize <= 1) || c.gather8);
    if (c.packInKernel) RCCHK(fs.packBuf.grow(framePixels, fs.stream));
    if (c.packInKernel && !fxaa) F.packOut = fs.packBuf;
    c.T.epilogue = F.epilogue; c.T.packOut = F.packOut;
    RCCHK(launch_trace(c, fxaaLocal ? fs.aux : fs.out));
    if (is_primary() && !es.evPost) RCCHK(wait_for_parts(c));
    HIPCHK(hipEventRecord(es.ev[2], fs.stream));
    if (!es.evPost) return CRT_OK;
    if (!fxaa) {
        // upstream: Trace write_imagef's into an RGBA8 texture, PostProcess read_imagef's it back and write_imagef's again
        if (!c.fused) {
            if (unorm) crt_quantize_kernel<<<c.grid, CRT_BLOCK, 0, fs.stream>>>(F, fs.out);
            if (post) crt_postprocess_kernel<<<c.grid, CRT_BLOCK, 0, fs.stream>>>(F, fs.out);
            if (unorm && post) crt_quantize_kernel<<<c.grid, CRT_BLOCK, 0, fs.stream>>>(F, fs.out);
            // RGBA8 gather behind a kernel form without the epilogue (wavefront): the bytes as a launch of their own (rows of other
            // devices are not touched: on the primary their bytes may already have arrived)
            if (c.gather8) crt_pack_owned_kernel<<<(unsigned)F.gridBlocks, CRT_BLOCK, 0, fs.stream>>>(plain_frame(F, false), fs.out, fs.packBuf);
            HIPCHK(hipGetLastError());
        }
        if (is_primary()) RCCHK(wait_for_parts(c));
    } else if (!is_secondary()) {
        // FXAA reads up to 5 pixels around its own in the Trace result, so it runs on the whole frame: a multi-device session
        // gathers the raw bands first (the secondaries skip their per-pixel stages) and its first device filters
        if (is_primary()) RCCHK(wait_for_parts(c));
        CrtFrame FF = plain_frame(F, true);
        const unsigned gridAll = (unsigned)FF.gridBlocks;
        if (fxaaLocal) {
            if (unorm && !c.fused) crt_quantize_kernel<<<gridAll, CRT_BLOCK, 0, fs.stream>>>(FF, fs.aux);
        } else {
            if (unorm) crt_quantize_kernel<<<gridAll, CRT_BLOCK, 0, fs.stream>>>(FF, fs.out);
            HIPCHK(hipMemcpyAsync(fs.aux, fs.out, framePixels * sizeof(float4), hipMemcpyDeviceToDevice, fs.stream));
        }
        FF.epilogue = (unorm ? CRT_EPILOGUE_QUANTIZE : 0u) | (post ? CRT_EPILOGUE_POST : 0u);
        FF.packOut = c.packInKernel ? fs.packBuf : nullptr;
        crt_fxaa_kernel<<<gridAll, CRT_BLOCK, 0, fs.stream>>>(FF, fs.aux, fs.out);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(es.ev[3], fs.stream));
    return CRT_OK;
}

// Secondary device: this device's bands go into the primary's frame of the same slot (peer copy over xGMI), once the primary
// is done with whatever the slot's previous frame still had queued (its read-back).
static int gather_to_primary(const FrameCtx& c)
{
    FrameSlot& fs = *c.fs; FrameSlot& pfs = g.primary->slot[c.slot];
    HIPCHK(hipStreamWaitEvent(fs.stream, pfs.slotDone, 0));
    if (c.gather8) RCCHK(copy_owned_rows_async(pfs.packBuf, fs.packBuf, 4, hipMemcpyDeviceToDevice, fs.stream));
    else RCCHK(copy_owned_rows_async(pfs.out, fs.out, 16, hipMemcpyDeviceToDevice, fs.stream));
    HIPCHK(hipEventRecord(fs.partDone, fs.stream));
    return CRT_OK;
}

// The frame is queued: its bookkeeping, the sort for the next frame, the read-back (CRT_RENDER_READBACK), and for a
// synchronous frame the reference's clFinish (Renderer.cpp:367).
static int finish_frame(const FrameCtx& c)
{
    FrameSlot& fs = *c.fs; EventSet& es = *c.es;
    fs.frameIs8 = c.gather8;
    g.cur = c.slot;
    if (c.flags & CRT_RENDER_GBUFFER) {         // what crt_frame_ao needs of this frame: its camera, and an event behind its kernels
        g.gbufSlot = c.slot;
        memcpy(fs.gbufInvView, c.F.invView, 64); memcpy(fs.gbufInvProj, c.F.invProj, 64);
        memcpy(fs.gbufArgs.cameraPos, c.F.camPos, 12); fs.gbufArgs.numMeshes = c.S.numInstances;
        if (!fs.gbufDone) RCCHK(fs.gbufDone.create(hipEventDisableTiming));
        HIPCHK(hipEventRecord(fs.gbufDone, fs.stream));
    }
    es.pending = true; es.flags = c.flags; es.seq = ++g.frameSeq; fs.frames++;
    if (c.T.order != nullptr && !(c.flags & CRT_RENDER_DIAG_MIX3)) {
        // did the view change since the last sorted frame? (camera matrices and position, instance tables)
        float view[35];
        memcpy(view, c.F.invView, 64); memcpy(view + 16, c.F.invProj, 64); memcpy(view + 32, c.F.camPos, 12);
        g.viewMoved = memcmp(view, g.lastView, sizeof view) != 0 || g.lastViewInst != g.instVersion;
        memcpy(g.lastView, view, sizeof view); g.lastViewInst = g.instVersion;
        RCCHK(sort_for_next_frame(c.T, fs, c.pipelined, g.form != Form::Mega));
    }
    if (c.flags & CRT_RENDER_READBACK) {
        // the frame travels to pinned host memory behind its own kernels; the other slots' frames keep the GPU busy meanwhile
        const size_t pixels = (size_t)g.width * (size_t)g.height;
        const bool bytes8 = (c.flags & CRT_RENDER_UNORM8) != 0;
        const size_t bytes = pixels * (bytes8 ? 4 : 16);
        RCCHK(fs.hostBuf.grow(bytes, hipHostMallocDefault));
        if (!fs.copied) RCCHK(fs.copied.create(hipEventDisableTiming));
        const void* src = fs.out;
        if (bytes8) {
            RCCHK(fs.packBuf.grow(pixels, fs.stream));
            // the Trace (or FXAA) kernel stored the bytes already / the byte frame was gathered
            const bool packed = (c.packInKernel && ((c.flags & CRT_RENDER_FXAA) || c.fused)) || c.gather8;
            if (!packed) crt_pack_unorm8_kernel<<<(unsigned)((pixels + 255) / 256), 256, 0, fs.stream>>>(fs.out, fs.packBuf, pixels);
            HIPCHK(hipGetLastError());
            src = fs.packBuf;
        }
        // only the rows this rank renders travel (the host buffer keeps the full-frame layout)
        RCCHK(copy_owned_rows_async(fs.hostBuf, src, bytes8 ? 4 : 16, hipMemcpyDeviceToHost, fs.stream, is_primary()));
        HIPCHK(hipEventRecord(fs.copied, fs.stream));
        fs.hostBytes = bytes; g.readbackRing[g.readbackCount++ % CRT_MAX_FRAMES_IN_FLIGHT] = c.slot;
    }
    if (is_primary()) HIPCHK(hipEventRecord(fs.slotDone, fs.stream));
    // wait for the frame's end event -- the sort for the next frame that is queued behind it needs no waiting for
    if (!(c.flags & CRT_RENDER_ASYNC) && !(c.plan && c.plan->noHostWait)) HIPCHK(hipEventSynchronize(es.evPost ? es.ev[3] : es.ev[2]));
    return CRT_OK;
}

int crt1_render(const CrtTraceArgs* args, const float invView[16], const float invProj[16], int flags, const RenderPlan* plan = nullptr)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!args || !invView || !invProj) return CRT_E_BAD_ARGUMENT;
    if (args->numMeshes > CRT_MAX_INSTANCES) return CRT_E_OUT_OF_RANGE;
    if (!g.sceneValid) return CRT_E_BAD_ARGUMENT;
    if ((flags & CRT_RENDER_SSAA2) && (flags & CRT_RENDER_SSAA4)) return CRT_E_BAD_ARGUMENT;
    FrameCtx c;
    c.flags = flags; c.plan = plan;
    fill_frame(c.F, args, invView, invProj, ssaa_factor(flags));
    if (c.F.gridBlocks == 0) return record_empty_share(plan);
    RCCHK(refuse_unsupported(flags, args->numMeshes));
    RCCHK(choose_slot(c));
    RCCHK(prepare_lists(c));
    RCCHK(begin_frame(c, args));
    RCCHK(launch_passes(c));
    if (is_secondary()) RCCHK(gather_to_primary(c));
    return finish_frame(c);
}

// Diagnostic: the shader clock under whatever load the device carries right now. One wave per XCD spins for `micros`
// microseconds of the 100 MHz real-time counter and reports delta s_memtime / delta s_memrealtime (MI355X_MICROARCH.md, DVFS
// item 6); runs on a stream of its own, next to the frames in flight.
__global__ void crt_clock_probe_kernel(unsigned long long ticks, double* __restrict__ out)
{
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime();
    unsigned long long r1 = r0, guard = 0;
    while (r1 - r0 < ticks && guard < (1ull << 24)) { __builtin_amdgcn_s_sleep(8); r1 = __builtin_amdgcn_s_memrealtime(); ++guard; }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) out[blockIdx.x] = r1 > r0 ? (double)(c1 - c0) / (double)(r1 - r0) * 0.1 : 0.0;
}

int crt1_debug_measure_clock(int micros, double* ghz)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!ghz || micros < 1 || micros > 100000) return CRT_E_BAD_ARGUMENT;
    DevBuf<double> d; Stream st;
    RCCHK(d.alloc(8));
    RCCHK(st.create(hipStreamNonBlocking));
    double h[8] = { 0 };
    crt_clock_probe_kernel<<<8, 64, 0, st>>>((unsigned long long)micros * 100ull, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double sum = 0; int n = 0;
    for (double v : h) if (v > 0.0) { sum += v; ++n; }
    *ghz = n ? sum / n : 0.0;
    return CRT_OK;
}

// Diagnostic: crt_recip_sweep_kernel (crt_recip.h) over `count` bit patterns from `first`; one launch on a stream of its own.
int crt1_debug_recip_sweep(uint32_t first, uint64_t count, uint64_t out[4])
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!out || count > (1ull << 32)) return CRT_E_BAD_ARGUMENT;
    DevBuf<unsigned long long> d; Stream st;
    RCCHK(d.alloc(4));
    RCCHK(st.create(hipStreamNonBlocking));
    unsigned long long h[4] = { 0, 0, 0, ~0ull };
    HIPCHK(hipMemcpyAsync(d, h, sizeof h, hipMemcpyHostToDevice, st));
    if (count) {
        const unsigned long long blocks = (count + 255) / 256;
        crt_recip_sweep_kernel<<<(unsigned)(blocks < 4096 ? blocks : 4096), 256, 0, st>>>(first, (unsigned long long)count, d);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    out[0] = h[0]; out[1] = h[1]; out[2] = h[2];
    out[3] = h[3] == ~0ull ? ~0ull : (uint64_t)(uint32_t)(first + (uint32_t)h[3]);
    return CRT_OK;
}

int crt1_sync(void)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    return sync_all();
}

int crt1_query_hits(const float* origins, const float* dirs, int n, uint32_t numInstances, CrtRayHit* out)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (n <= 0) return CRT_OK;
    if (!origins || !dirs || !out || numInstances > CRT_MAX_INSTANCES) return CRT_E_BAD_ARGUMENT;
    if (!g.sceneValid) return CRT_E_BAD_ARGUMENT;
    RCCHK(collect_timing());
    RCCHK(quiesce());
    const size_t rayBytes = sizeof(float) * 3 * (size_t)n, need = rayBytes * 2 + sizeof(CrtRayHit) * (size_t)n;
    RCCHK(g.queryBuf.grow(need, g.stream));
    float* dO = reinterpret_cast<float*>(static_cast<char*>(g.queryBuf));
    float* dD = dO + 3 * (size_t)n;
    CrtRayHit* dH = reinterpret_cast<CrtRayHit*>(dD + 3 * (size_t)n);
    HIPCHK(hipMemcpyAsync(dO, origins, rayBytes, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(dD, dirs, rayBytes, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemsetAsync(g.counters, 0, CRT_NUM_COUNTERS * sizeof(unsigned long long), g.stream));
    FrameSlot& fs = g.slot[0];
    RCCHK(ensure_slot_instances(fs));
    RCCHK(ensure_overflow(fs, (size_t)((n + CRT_BLOCK - 1) / CRT_BLOCK)));
    double farthest2 = 0.0;      // the cull is proven for origins up to State::cullOriginLimit from the world origin
    for (int k = 0; k < n; ++k) {
        const double x = origins[3 * k], y = origins[3 * k + 1], z = origins[3 * k + 2], d2 = x * x + y * y + z * z;
        if (!(d2 <= farthest2)) farthest2 = d2;      // (NaN sticks)
    }
    CrtDevScene S; fill_scene(S, numInstances, fs, beyond_cull_range(sqrt(farthest2)));
    with_bools([&](auto Tl) { crt_query_kernel<decltype(Tl)::value><<<(unsigned)((n + CRT_BLOCK - 1) / CRT_BLOCK), CRT_BLOCK, 0, g.stream>>>(S, dO, dD, n, dH, g.counters); }, use_tlas(S));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dH, sizeof(CrtRayHit) * (size_t)n, hipMemcpyDeviceToHost, g.stream));
    unsigned long long c[CRT_NUM_COUNTERS];
    HIPCHK(hipMemcpyAsync(c, g.counters, sizeof c, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    unpack_counters(c);
    return CRT_OK;
}

int crt1_read_output(float* dst, size_t floats)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!dst || floats != (size_t)g.width * (size_t)g.height * 4) return CRT_E_BAD_ARGUMENT;
    RCCHK(sync_all());
    RCCHK(expand_rgba8_frame(g.slot[g.cur]));
    HIPCHK(hipMemcpy(dst, g.slot[g.cur].out, floats * sizeof(float), hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt1_read_output_rows(float* dst, int row0, int rows)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!dst || row0 < 0 || rows < 0 || row0 + rows > g.height) return CRT_E_BAD_ARGUMENT;
    RCCHK(sync_all());
    RCCHK(expand_rgba8_frame(g.slot[g.cur]));
    HIPCHK(hipMemcpy(dst, g.slot[g.cur].out + (size_t)row0 * (size_t)g.width, (size_t)rows * (size_t)g.width * sizeof(float4), hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt1_read_output_rgba8(uint8_t* dst, size_t bytes)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    const size_t pixels = (size_t)g.width * (size_t)g.height;
    if (!dst || bytes != pixels * 4) return CRT_E_BAD_ARGUMENT;
    RCCHK(sync_all());
    if (g.slot[g.cur].frameIs8) {                          // a multi-device session's RGBA8 frame: the gathered bytes ARE the frame
        HIPCHK(hipMemcpy(dst, g.slot[g.cur].packBuf, pixels * 4, hipMemcpyDeviceToHost));
        return CRT_OK;
    }
    RCCHK(g.queryBuf.grow(pixels * 4, g.stream));   // shares the query scratch buffer
    crt_pack_unorm8_kernel<<<(unsigned)((pixels + 255) / 256), 256, 0, g.stream>>>(g.slot[g.cur].out, reinterpret_cast<uint32_t*>(static_cast<char*>(g.queryBuf)), pixels);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dst, g.queryBuf, pixels * 4, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return CRT_OK;
}

int crt1_map_host_frame_back(int framesBack, const void** ptr, size_t* bytes)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    // a pipelined frame's copy lives in its slot until the slot is reused: the last nSlots READBACK frames are reachable
    if (!ptr || framesBack < 0 || (unsigned)framesBack >= g.readbackCount || framesBack >= g.nSlots) return CRT_E_BAD_ARGUMENT;
    const int slot = g.readbackRing[(g.readbackCount - 1u - (unsigned)framesBack) % CRT_MAX_FRAMES_IN_FLIGHT];
    for (int k = 0; k < framesBack; ++k)      // a later frame on the same slot (synchronous frames all use slot 0) has replaced it
        if (g.readbackRing[(g.readbackCount - 1u - (unsigned)k) % CRT_MAX_FRAMES_IN_FLIGHT] == slot) return CRT_E_BAD_ARGUMENT;
    FrameSlot& fs = g.slot[slot];
    HIPCHK(hipEventSynchronize(fs.copied));
    *ptr = fs.hostBuf;
    if (bytes) *bytes = fs.hostBytes;
    return CRT_OK;
}

int crt1_map_host_frame(const void** ptr, size_t* bytes) { return crt1_map_host_frame_back(0, ptr, bytes); }

int crt1_read_rays(float* dst, size_t floats)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!dst || floats != (size_t)g.width * (size_t)g.height * 3) return CRT_E_BAD_ARGUMENT;
    RCCHK(sync_all());
    HIPCHK(hipMemcpy(dst, g.rays, floats * sizeof(float), hipMemcpyDeviceToHost));
    return CRT_OK;
}

// The planes of the most recently submitted CRT_RENDER_GBUFFER frame (its slot keeps them until its next G-buffer frame, a resize or
// the shutdown; frames without the flag leave them alone).
static char* gbuffer_plane(int plane)
{
    if (g.gbufSlot < 0 || !g.slot[g.gbufSlot].gbuf || gbuffer_plane_pixel_bytes(plane) == 0) return nullptr;
    const CrtGBuffer gb = slot_gbuffer(g.slot[g.gbufSlot]);
    const size_t pixels = (size_t)g.width * (size_t)g.height;
    return plane == CRT_GBUFFER_GEOMETRY ? gb.geometry() : plane == CRT_GBUFFER_IDS ? gb.ids(pixels) : gb.albedo(pixels);
}

int crt1_read_gbuffer(int plane, void* dst, size_t bytes)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    const char* src = gbuffer_plane(plane);
    if (!dst || !src || bytes != (size_t)g.width * (size_t)g.height * gbuffer_plane_pixel_bytes(plane)) return CRT_E_BAD_ARGUMENT;
    RCCHK(sync_all());
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return CRT_OK;
}

void* crt1_gbuffer_device_ptr(int plane) { return g.initialized ? (void*)gbuffer_plane(plane) : nullptr; }

// one pixel of the three planes: three small copies (16 + 16 + 4 B), no frame read
int crt1_pick_pixel(int x, int y, CrtGBufferPixel* out)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!out || !gbuffer_plane(CRT_GBUFFER_GEOMETRY)) return CRT_E_BAD_ARGUMENT;
    if (x < 0 || y < 0 || x >= g.width || y >= g.height) return CRT_E_OUT_OF_RANGE;
    RCCHK(sync_all());
    const size_t idx = (size_t)y * (size_t)g.width + (size_t)x;
    HIPCHK(hipMemcpy(out->normal, gbuffer_plane(CRT_GBUFFER_GEOMETRY) + idx * 16, 16, hipMemcpyDeviceToHost));   // normal[3], t
    HIPCHK(hipMemcpy(&out->instance, gbuffer_plane(CRT_GBUFFER_IDS) + idx * 16, 16, hipMemcpyDeviceToHost));      // instance, triIndex, u, v
    HIPCHK(hipMemcpy(&out->albedo, gbuffer_plane(CRT_GBUFFER_ALBEDO) + idx * 4, 4, hipMemcpyDeviceToHost));
    return CRT_OK;
}

// (a frame gathered as RGBA8 is expanded into the float frame first: waits for the frames in flight)
void* crt1_output_device_ptr(void)
{
    if (!g.initialized) return nullptr;
    if (g.slot[g.cur].frameIs8 && (sync_all() != CRT_OK || expand_rgba8_frame(g.slot[g.cur]) != CRT_OK)) return nullptr;
    return (void*)g.slot[g.cur].out;
}

float crt1_last_kernel_ms(int which)
{
    if (!g.initialized || which < 0 || which > 3) return -1.0f;
    if (collect_timing() != CRT_OK) return -1.0f;
    return g.ms[which];
}

int crt1_frame_time_stats(CrtFrameStats* out, int reset)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    RCCHK(collect_timing());
    if (out) {
        out->frames = g.framesTimed;
        for (int k = 0; k < 4; ++k) out->sumMs[k] = g.msSum[k];
        out->extentMs = g.statExtent;
        out->firstFrameMs = g.statFirstMs;
    }
    if (reset) {
        for (int k = 0; k < 4; ++k) g.msSum[k] = 0.0;
        g.framesTimed = 0; g.statExtent = 0; g.statFirstMs = 0; g.statStartArmed = true; g.statStartValid = false;
    }
    return CRT_OK;
}

int crt1_debug_read_frame_times(double* dst, size_t maxFrames, size_t* numFrames)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!numFrames) return CRT_E_BAD_ARGUMENT;
    RCCHK(collect_timing());
    *numFrames = g.frameLogN;
    if (dst) memcpy(dst, g.frameLog, sizeof(double) * 2 * (maxFrames < g.frameLogN ? maxFrames : g.frameLogN));
    return CRT_OK;
}

int crt1_debug_read_stamps(uint64_t* dst, size_t maxWaves, size_t* numWaves)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!numWaves) return CRT_E_BAD_ARGUMENT;
    *numWaves = g.stampWaves;
    if (!dst || !g.stamps) return CRT_OK;
    const size_t n = maxWaves < g.stampWaves ? maxWaves : g.stampWaves;
    RCCHK(sync_all());
    HIPCHK(hipMemcpy(dst, g.stamps + 16, n * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return CRT_OK;
}

// Diagnostic: the sort of launch_order_kernel (or, slotsPerXcd < 0, the identity order) on costs the caller chose, in scratch memory and
// on a stream of its own; the session's slots are not touched. Everything that could index outside a buffer, or take a float beyond an
// int in the sort (splitFactor x the cost sum x 1023 / the maximum key <= slotsPerXcd x 1023 < 2^31), is refused before any launch.
int crt1_debug_launch_lists(const uint32_t* cost, int slotsPerXcd, int tilesX, int maxSplit, float splitFactor, float spread,
                            uint32_t* order, uint32_t* listLen, uint32_t* costAfter)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    const bool identity = slotsPerXcd < 0;
    const long long S = identity ? -(long long)slotsPerXcd : (long long)slotsPerXcd;
    if (!order || !listLen || S < 1 || S > (1 << 20)) return CRT_E_BAD_ARGUMENT;
    if (!identity) {
        if (!cost || !costAfter || tilesX < 1 || S % tilesX != 0 || maxSplit < 0 || maxSplit > CRT_MAX_SPLIT) return CRT_E_BAD_ARGUMENT;
        if (!(splitFactor >= 0.0f && splitFactor <= 1.0f) || !(spread >= 0.0f && spread <= 1.0f)) return CRT_E_BAD_ARGUMENT;   // NaN fails both
        // a cost no frame produces (four quadrant waves of at most 0x0FFFFFFF each, add_tile_cost); near 2^32 the lifted key would not fit
        for (long long i = 0; i < 8 * S; ++i) if (cost[i] > 0x3FFFFFFCu) return CRT_E_BAD_ARGUMENT;
    }
    const int slots = (int)S, listCap = slots + 3 * CRT_MAX_SPLIT;
    const size_t n = (size_t)8 * (size_t)listCap, costs = (size_t)8 * (size_t)slots;
    DevBuf<uint32_t> lists; Stream st;
    RCCHK(lists.alloc(3 * n + 8));
    RCCHK(st.create(hipStreamNonBlocking));
    if (identity) launch_identity_lists(lists, slots, listCap, st);
    else {
        HIPCHK(hipMemcpyAsync(lists + n, cost, costs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        launch_list_kernels(lists, slots, listCap, tilesX, spread, (uint32_t)maxSplit, splitFactor, st);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(order, lists, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(listLen, lists + 3 * n, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (!identity) HIPCHK(hipMemcpyAsync(costAfter, lists + n, costs * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return CRT_OK;
}

// Diagnostic: the lists slot 0's next frame of the same geometry would run on (the sort queued behind its last frame has built them)
int crt1_debug_read_launch_lists(uint32_t* order, size_t cap, uint32_t listLen[8], int* slotsPerXcd, int* listCap)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!listLen || !slotsPerXcd || !listCap) return CRT_E_BAD_ARGUMENT;
    const FrameSlot& fs = g.slot[0];
    if (!fs.lists || fs.orderSlots < 1 || !fs.listsReady) return CRT_E_UNSUPPORTED;
    const int cap1 = fs.orderSlots + 3 * CRT_MAX_SPLIT;
    const size_t n = (size_t)8 * (size_t)cap1;
    *slotsPerXcd = fs.orderSlots; *listCap = cap1;
    if (order && cap < n) return CRT_E_BAD_ARGUMENT;
    HIPCHK(hipStreamSynchronize(fs.stream));
    if (order) HIPCHK(hipMemcpy(order, fs.lists, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(listLen, fs.lists + 3 * n, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CRT_OK;
}

int crt1_get_culled_visits(uint64_t* out)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!out) return CRT_E_BAD_ARGUMENT;
    RCCHK(collect_timing());
    *out = g.lastCulled;
    return CRT_OK;
}

// Diagnostic: the range of ray origins the instance cull is proven for. limits[i] = O_i of instance i (0: never culled),
// *sceneLimit = the smallest over the cullable instances (a frame whose camera is farther out runs without the cull),
// *bounceReach = how far from the world origin bounce-ray origins can lie, *noCullFrames = launches that ran without it so far.
int crt1_get_cull_range(float* limits, int n, float* sceneLimit, float* bounceReach, uint64_t* noCullFrames)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (n < 0 || n > CRT_MAX_INSTANCES || (n > 0 && !limits)) return CRT_E_BAD_ARGUMENT;
    for (int i = 0; i < n; ++i) limits[i] = g.hCullOriginLimit[i];
    if (sceneLimit) *sceneLimit = g.cullOriginLimit;
    if (bounceReach) *bounceReach = g.bounceOriginReach;
    if (noCullFrames) *noCullFrames = g.noCullFrames;
    return CRT_OK;
}

int crt1_get_counters(CrtCounters* out)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!out) return CRT_E_BAD_ARGUMENT;
    RCCHK(collect_timing());
    *out = g.lastCounters;
    return CRT_OK;
}

} // namespace
