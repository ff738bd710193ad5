// crt_state.h -- host state of one device session: frame slots, pools, the helpers every other part uses
// Part of the one translation unit crt_shim.hip (included there, in this order: crt_own.h, crt_state.h, crt_instances.h, crt_upload.h,
// crt_bvh_driver.h, crt_frame.h, crt_query_host.h, crt_ao_host.h, crt_multidev.h); everything here has internal linkage.
#pragma once
// ------------------------------------------------------------------------------------------------
// host state
// ------------------------------------------------------------------------------------------------
namespace {

#define CRT_MAX_FRAMES_IN_FLIGHT 8
#define CRT_MAX_DEVICES 16

// The Trace kernel structure of a session (CRT_KERNEL). Mega: the megakernel with feedback launch lists (the default).
// The opt-in forms: Wavefront, one launch per bounce with ordered ballot compaction in between (crt_kernels.h); Refill, in-tile
// lane refill, and Block, phase-separated block compaction (crt_refill.h); LdsTop, four-wave workgroups sharing an LDS copy of
// the tree tops (crt_ldstop.h).
enum class Form { Mega, Wavefront, Refill, Block, LdsTop };

struct EventSet {
    Event ev[4];
    bool pending = false; int flags = 0; bool evRaygen = false, evPost = false;   // timing not yet read back
    unsigned long long seq = 0;
};

// A stream with its own copy of the instance tables and its traversal-stack overflow area: what every frame slot has, and all the ray
// queries' context borrows of one (create_slot_tables, ensure_slot_instances, fill_scene, ensure_overflow).
struct SlotTables {
    Stream stream;
    // This slot's copy of the instance tables (reference-layout records, device records, bounding spheres, instance tree,
    // never-culled list), refreshed on the slot's own stream from the host master when it is stale (ensure_slot_instances):
    // an instance upload never has to wait for the frames in flight, and those frames never see it.
    DevBuf<char> instBlock;                    // one device allocation; the four pointers below point into it
    CrtMeshInstance* instances = nullptr; float4* instBounds = nullptr; CrtTlasNode* tlas = nullptr; uint32_t* alwaysList = nullptr;
    DevBuf<CrtDevInstance> devInstances;
    uint32_t tlasNodes = 0, numAlways = 0;
    unsigned long long instVersion = 0;        // 0 = never filled (the master starts at 1)
    PinnedBuf<char> staging; Event staged;     // pinned staging block and "its copies have been issued and done" event
    char* stagingDev = nullptr;                // the staging block as the device sees it
    DevBuf<uint32_t> ovf;                      // traversal-stack overflow area of this slot's launches (CrtStack), one block per workgroup
};

struct FrameSlot : SlotTables {
    EventSet es[2];                            // two sets, so the host may queue a slot's next frame before reading the last one's timing
    unsigned frames = 0;
    DevBuf<float4> out;
    DevBuf<float4> aux;                        // CRT_RENDER_FXAA: the unfiltered frame the filter reads (allocated on first use)
    DevBuf<CrtBounceRay> blockQueue;           // CRT_KERNEL=block / wavefront: bounce-ray queue, one 64- or 128-record range per workgroup of the primary launch
    DevBuf<uint32_t> wfCount;                  // CRT_KERNEL=wavefront: per primary wave {continuing rays}, {offset within its XCD}, then the 8 per-XCD totals
    // CRT_RENDER_GBUFFER: this slot's first-hit planes, one allocation of 36 B per pixel (geometry, ids, albedo back to back), made on
    // the slot's first G-buffer frame (slot_gbuffer)
    DevBuf<char> gbuf;
    // crt_frame_ao: what the slot's last G-buffer frame was rendered with (the matrices and camera its pixels' rays are regenerated from,
    // its instance count), the event recorded behind it (an AO query's stream waits for it on the device), and the slot's AO plane --
    // W x H floats, allocated by the slot's first crt_frame_ao; `aoRaw`: the unfiltered plane CRT_AO_FILTER reads. aoPending: an AO query
    // that reads the planes may still run -- the slot's next G-buffer frame waits for it on the device.
    float gbufInvView[16] = { 0 }, gbufInvProj[16] = { 0 }; CrtTraceArgs gbufArgs = {}; Event gbufDone;
    DevBuf<float> ao, aoRaw; bool aoPending = false;
    DevBuf<uint32_t> lists;                    // feedback launch lists: order, costs, sort keys, lengths (prepare_launch_lists)
    int orderSlots = -1; int orderKey[7] = { 0, 0, 0, 0, 0, 0, 0 };
    bool listsReady = false;                   // the lists for the next frame were already sorted at the end of the last one
    // CRT_RENDER_READBACK: pinned host copy of this slot's frame (hostBytes of it), queued behind the frame on the slot's stream;
    // packBuf: the frame's RGBA8 bytes, one word per pixel
    PinnedBuf<char> hostBuf; size_t hostBytes = 0; DevBuf<uint32_t> packBuf; Event copied;
    DevBuf<uint32_t> mixOrder; int mixSlots = -1;   // CRT_RENDER_DIAG_MIX3 launch lists, then their 8 lengths
    // in-process multi-GPU (crt_init_devices): a secondary device records `partDone` behind the copy of its bands into the
    // primary's frame; the primary records `slotDone` behind everything a frame queues on this slot (incl. a read-back)
    Event partDone, slotDone;
    // RGBA8 gather (a multi-device session's CRT_RENDER_UNORM8 frames without FXAA): the WHOLE frame is in packBuf (every device's Trace
    // epilogue stores its pixels' four bytes, the secondaries copy 4 B per pixel into the primary's packBuf); `out` holds only this
    // device's bands until somebody asks for the float frame (expand_rgba8_frame: x = byte / 255, exactly what the epilogue stored)
    bool frameIs8 = false;
};

// One family of queries on the context below (crt_trace_rays; crt_trace_ao / crt_frame_ao; crt_shade_rays): its pair of control words, what its last launch
// was, and how many workgroups of each of its kernel's instantiations -- four per box rule, or the shaded queries' six -- a CU holds. Families share everything else of the context.
struct QueryFamily {
    uint32_t ctl0;                             // its words in QueryContext::ctl: [ctl0] chunk counter, [ctl0 + 1] chunks traced without the cull (CrtQueryArgs::ctl)
    unsigned long long chunks = 0, grid = 0;   // of the family's last query (crt_debug_rays_stats, crt_debug_ao_stats)
    int residentPerCU[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };   // hipOccupancyMaxActiveBlocksPerMultiprocessor of the kernel<X, TLAS>, [4 * inclusive + 2 * X + TLAS] (crt_shade_kernel<WHAT, TLAS>: [2 * (WHAT - 1) + TLAS]); 0 = not asked yet
};

// The context of the queries on device buffers (crt_query_host.h): queries never touch a frame slot, so they neither wait for the frames
// in flight nor make them wait. `tables`: the context's own stream (the instance-table refresh runs there), its copy of the instance
// tables with the staging block and `staged` event (ensure_slot_instances), and its overflow area, one block per workgroup of the
// persistent grid. One query at a time: every launch makes the caller's stream wait for `raysDone` of the one before (no host wait), and
// whatever edits shared device state waits for it on the host (quiesce).
struct QueryContext {
    SlotTables tables;
    bool ready = false;                        // allocated (by the first query)
    DevBuf<uint32_t> ctl;                      // device: six words, a pair per family
    Event raysDone; bool inFlight = false;     // recorded behind the last query on the caller's stream; inFlight: not yet known to be over
    bool refreshPending = false;               // a table refresh was queued on tables.stream and no raysDone covers it yet (a query that failed behind it): quiesce waits for tables.staged
    QueryFamily rays = { 0 }, ao = { 2 }, shade = { 4 };      // crt_rays_kernel<ANYHIT, TLAS>, crt_ao_kernel<SOURCE, TLAS>, crt_shade_kernel<WHAT, TLAS>
};

// Whatever a State holds is released when it is deleted, with its device current: destroy_group (crt_multidev.h) is the only place.
struct State {
    bool initialized = false;
    int device = -1;
    char deviceName[256] = { 0 };
    // Frame slots: a synchronous frame always uses slot 0; CRT_RENDER_ASYNC frames rotate over the first nSlots slots
    // (own stream, output buffer, launch lists and events each), so the tail of one frame overlaps the next.
    FrameSlot slot[CRT_MAX_FRAMES_IN_FLIGHT]; int nSlots = 3;
    hipStream_t stream = nullptr;              // == slot[0].stream: uploads, queries, diagnostics
    int cur = 0;                               // slot of the most recently submitted frame
    int gbufSlot = -1;                         // ... of the most recently submitted CRT_RENDER_GBUFFER frame; -1: none since crt_init / the last resize
    int aoSlot = -1;                           // ... of the most recent crt_frame_ao (its AO plane); -1: none since crt_init / the last resize
    int readbackRing[CRT_MAX_FRAMES_IN_FLIGHT] = { -1, -1, -1, -1, -1, -1, -1, -1 }; unsigned readbackCount = 0;   // slots of the latest CRT_RENDER_READBACK frames
    unsigned asyncSeq = 0; bool othersBusy = false;   // frames possibly running on slots > 0
    // Start-up stagger of a burst of frames in flight: frames submitted to an idle device start together, run in lockstep and have
    // their long-ray tails at the same time -- exactly what frames in flight are there to avoid -- until the slots drift apart (three
    // frames take 1.17 ms to fill the pipeline where steady state delivers 4.3). The first frame a slot runs after the session was
    // idle is therefore held back on its stream by slot x (last frame latency / slots) by a one-wave timer kernel.
    float pipelinedLatencyMs = 0.0f;     // latency of the newest plain frame-in-flight timed so far (what the stagger is derived from; 0 = none yet)
    unsigned burstFrames = 0; int staggerUs = -1;   // frames submitted since the device was last known idle; CRT_STAGGER_US: -1 = automatic, 0 = off, n = n us per slot
    // Automatic = only for a caller that is known to stream: the burst before this one ran longer than the slot count. A caller that
    // submits two or three frames and then reads never reaches steady state and would only pay the hold-back as latency.
    unsigned prevBurstFrames = 0; unsigned long long staggeredFrames = 0;
    int width = 0, height = 0;
    int bandRows = 16, rank = 0, nRanks = 1;
    // raw (reference-layout) device copies
    DevBuf<CrtTri> rawTris; DevBuf<CrtBVHNode> rawNodes; DevBuf<uint32_t> roots; DevBuf<uint8_t> rawTexels;
    // CDNA4 layouts
    DevBuf<float4> pairs; DevBuf<float> triHot; DevBuf<uint4> triCold; DevBuf<uint32_t> bigLeaf;
    DevBuf<uint32_t> rootRefs; DevBuf<uint32_t> texels;
    DevBuf<CrtMaterial> materials; DevBuf<CrtTexture> textures;
    // host master of everything derived from the instance table (rebuild_instance_master); slots copy it when stale
    float4 hBounds[CRT_MAX_INSTANCES]; CrtTlasNode hTlas[2 * CRT_MAX_INSTANCES]; uint32_t hAlways[CRT_MAX_INSTANCES];
    uint32_t hTlasNodes = 0, hNumAlways = 0; unsigned long long instVersion = 1;
    // incremental rebuild_instance_master (r6): the reach the limits were checked against, and what the instance tree was last BUILT for (it is refitted while
    // the set of cullable instances stays the same)
    double hReach = 0.0; bool hTlasBuilt = false; uint32_t hTlasBuiltHigh = 0, hTlasRefits = 0; double hTlasBuiltRadii = 0.0; uint8_t hTlasMember[CRT_MAX_INSTANCES] = { 0 };
    unsigned long long hTlasBuilds = 0;        // median-split builds so far (crt_debug_tlas_stats)
    CrtBVHNode hRootNodes[CRT_MAX_MESHES]; bool hHaveRoot[CRT_MAX_MESHES];   // root node of every mesh, cached at BVH upload
    CrtBVHNode hRootKids[CRT_MAX_MESHES][2]; bool hHaveKids[CRT_MAX_MESHES];  // ... and the root's two children: their boxes are what an entering ray is tested against
    // Range of ray origins for which the instance cull is provably exact (derivation: crt_device.h above sphere_culls):
    // per instance and the smallest over the cullable ones; a frame / query whose origins lie beyond it runs with `noCullBounds`.
    float hCullOriginLimit[CRT_MAX_INSTANCES]; float cullOriginLimit = 0.0f; float bounceOriginReach = 0.0f;
    double triReach2 = 0.0;                    // largest squared distance of a vertex in the triangle pool from its object-space origin (crt1_upload_triangles)
    DevBuf<uint32_t> triReachBits;             // device: that maximum as float bits (crt_tri_reach_kernel)
    DevBuf<float4> noCullBounds;               // device: CRT_MAX_INSTANCES x (0, 0, 0, -1) = "never cull"
    unsigned long long noCullFrames = 0;       // frames and queries that ran without the cull for that reason
    CrtMeshInstance hInstances[CRT_MAX_INSTANCES]; uint32_t hRoots[CRT_MAX_MESHES]; uint32_t instHigh = 0;
    DevBuf<float> rays;
    DevBuf<unsigned long long> counters; DevBuf<int> err;
    DevBuf<unsigned long long> stamps; size_t stampWaves = 0;
    int numCUs = 0;
    int forceTlas = -1;   // CRT_TLAS=0/1: force the linear / tree candidate search (tests); default: by instance count
    int feedbackAsync = 0; int feedback = 1; int maxSplit = CRT_MAX_SPLIT, maxSplitPipelined = CRT_MAX_SPLIT_PIPELINED;
    // feedback lists while the view changes: rank a tile by max(own cost, costSpread x heaviest of its 8 neighbours) -- next
    // frame's heavy tiles are this frame's or the ones next to them. A view that stood still for a frame is ranked by own cost.
    float costSpread = 0.8f;
    float lastView[35] = { 0 }; unsigned long long lastViewInst = 0; bool viewMoved = false;   // camera matrices + position / instance version of the last sorted frame
    float splitBeta = CRT_SPLIT_BETA, splitBetaAsync = CRT_SPLIT_BETA_ASYNC;   // split a tile whose wave would run longer than beta x the XCD's time for the frame
    Form form = Form::Mega;                    // CRT_KERNEL: the Trace kernel structure of every frame (one the form cannot render is refused)
    DevBuf<float4> topPairs; DevBuf<uint32_t> topRootRefs;   // the tree-top table (CRT_TOP_PAIRS records) and every mesh's entry into it, rebuilt with the BVH layout
    char lastKernel[128] = { 0 };              // crt_debug_last_kernel: the Trace launch(es) of the most recently submitted frame
    DevBuf<char> queryBuf;                     // scratch of crt_query_hits and crt_read_output_rgba8
    QueryContext rayQuery;                     // crt_trace_rays, crt_trace_ao, crt_frame_ao, crt_shade_rays
    int raysGridCap = 0;                       // CRT_RAYS_GRID=n: at most n workgroups per query (tests: few waves walking many chunks); 0 = as many as are resident
    DevBuf<char> buildBuf;                                    // crt_build_bvh scratch
    std::vector<CrtBuildCtl> buildReplay; unsigned long long buildReplayKey = 0;   // CRT_DEBUG_BVH_REPLAY (crt_bvh_driver.h): the level records of the last build
    unsigned buildLaunches = 0, buildLevels = 0;   // crt_debug_build_stats: kernel launches and levels of the last crt_build_bvh (before the re-layout)
    bool buildNoSpin = false;                                   // the spin on buildCtlHost timed out once: synchronise the stream per level instead
    PinnedBuf<CrtBuildCtlHost> buildCtlHost; uint32_t buildSeq = 0;   // pinned: the per-level control record the builder publishes (crt_bvh_publish)
    DevBuf<CrtTri> buildTris;                                  // crt_build_bvh: second triangle pool (same indexing as rawTris)
    size_t triCap = 0, nodeCap = 0, texelByteCap = 0;
    uint32_t nodeCount = 0, numRoots = 0; size_t texelBytesHigh = 0; size_t trisHigh = 0;
    bool sceneValid = true;
    double msSum[4] = { 0, 0, 0, 0 }; unsigned long long framesTimed = 0;   // crt_frame_time_stats
    float ms[4] = { 0, 0, 0, 0 }; unsigned long long msSeq = 0, frameSeq = 0;   // timing of the newest frame read back so far
    Event statStart; bool statStartArmed = true, statStartValid = false; unsigned long long statStartSeq = 0; double statExtent = 0, statFirstMs = 0;
    CrtCounters lastCounters; unsigned long long lastCulled = 0;
    double frameLog[512]; unsigned frameLogN = 0;      // crt_debug_read_frame_times: {start, end} ms after statStart of the frames since the last reset
    // in-process multi-GPU: this device renders band `rank` of `nRanks`; `primary` (rank 0) owns the frame that is read
    State* primary = nullptr; State* group[CRT_MAX_DEVICES] = { nullptr }; int groupSize = 1;
    int gather8 = 1;                           // CRT_GATHER_RGBA8=0: gather float4 bands even for CRT_RENDER_UNORM8 frames (A/B, tests)
};
// One State per device (crt_init: one; crt_init_devices: one per GPU). Every function below works on "the current
// device's state" through `g`; the dispatch layer at the end of the file selects it (and the HIP device) per call, on the
// calling thread or on a per-device worker thread.
thread_local State* G = nullptr;
#define g (*G)

// a spinning host thread's pause (the level read-back of crt_build_bvh, the per-device workers): x86 `pause`, otherwise a compiler barrier
static inline void crt_cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    __asm__ __volatile__("" ::: "memory");
#endif
}

#define CRT_NUM_COUNTERS 15

// Wait for frames still running on the second slot, and for the ray query in flight (it runs on the caller's stream), before anything
// touches shared device state.
int quiesce()
{
    if (g.rayQuery.inFlight) { HIPCHK(hipEventSynchronize(g.rayQuery.raysDone)); g.rayQuery.inFlight = false; }
    if (g.rayQuery.refreshPending) { HIPCHK(hipEventSynchronize(g.rayQuery.tables.staged)); g.rayQuery.refreshPending = false; }   // it reads g.rootRefs
    if (g.othersBusy) {
        for (int i = 1; i < g.nSlots; ++i) HIPCHK(hipStreamSynchronize(g.slot[i].stream));
        g.othersBusy = false;
    }
    return CRT_OK;
}

int sync_all()
{
    HIPCHK(hipStreamSynchronize(g.slot[0].stream));
    RCCHK(quiesce());
    if (g.burstFrames) g.prevBurstFrames = g.burstFrames;
    g.burstFrames = 0;                          // every slot is idle: the next pipelined frames start a burst
    return CRT_OK;
}

// ... of a frame `height` rows tall whose bands are `bandRows` rows (an SSAA frame: the virtual frame, k x the output's bands)
int owned_tile_rows(int height, int bandRows)
{
    const int totalTileRows = (height + CRT_TILE - 1) / CRT_TILE;
    const int tpb = bandRows / CRT_TILE;
    int n = 0;
    for (int r = 0; r < totalTileRows; ++r) if (((r / tpb) % g.nRanks) == g.rank) ++n;
    return n;
}

// F's launch geometry for `tileRows` x `tilesX` tiles: the tile rows rounded up to a multiple of 8, dealt over the 8 XCDs
void set_tile_grid(CrtFrame& F, int tileRows, int tilesX)
{
    F.tilesX = tilesX;
    F.ownedTileRows = tileRows;
    F.gridBlocks = ((tileRows + 7) / 8) * 8 * tilesX;
    F.slotsPerXcd = F.gridBlocks / 8;
    F.listCap = F.slotsPerXcd;
}

// ss: k of k x k supersampling -- F is then the virtual frame kW x kH, an output band of bandRows rows is k x bandRows virtual rows
void fill_frame(CrtFrame& F, const CrtTraceArgs* args, const float* invView, const float* invProj, int ss = 1)
{
    memset(&F, 0, sizeof F);
    if (invView) memcpy(F.invView, invView, 64);
    if (invProj) memcpy(F.invProj, invProj, 64);
    if (args) {
        memcpy(F.camPos, args->cameraPos, 12);
        F.lightY = (float)sin((double)args->sunAngle);
        F.lightZ = (float)cos((double)args->sunAngle);
    }
    F.width = ss * g.width; F.height = ss * g.height; F.ss = ss;
    set_tile_grid(F, owned_tile_rows(F.height, ss * g.bandRows), (F.width + CRT_TILE - 1) / CRT_TILE);
    F.tileRowsPerBand = ss * g.bandRows / CRT_TILE;
    F.rank = g.rank; F.nRanks = g.nRanks;
}

// noCull: the rays of this launch may start beyond the range the instance cull is proven for (State::cullOriginLimit): every
// instance is a candidate for every ray (all-never bounds table, no instance tree)
void fill_scene(CrtDevScene& S, uint32_t numInstances, const SlotTables& fs, bool noCull = false)
{
    S.pairs = g.pairs; S.triHot = g.triHot; S.triCold = g.triCold; S.bigLeaf = g.bigLeaf; S.rootRefs = g.rootRefs; S.stackOverflow = fs.ovf;
    S.instances = fs.instances; S.devInstances = fs.devInstances; S.instBounds = fs.instBounds; S.materials = g.materials; S.textures = g.textures; S.texels = g.texels;
    S.numTexels = (int)((g.texelBytesHigh + 2) / 3);
    if (S.numTexels < 1) S.numTexels = 1;
    S.numInstances = numInstances;
    S.tlas = fs.tlas; S.tlasNodes = fs.tlasNodes; S.alwaysList = fs.alwaysList; S.numAlways = fs.numAlways;
    S.topPairs = g.topPairs;
    if (noCull) { S.instBounds = g.noCullBounds; S.tlas = nullptr; S.tlasNodes = 0; S.alwaysList = nullptr; S.numAlways = 0; g.noCullFrames++; }
}
// true when a ray origin this far from the world origin is outside the proven range (NaN counts as outside)
bool beyond_cull_range(double originNorm) { return !(originNorm <= (double)g.cullOriginLimit); }

// The traversal-stack overflow area of a slot must hold one block per workgroup of its largest launch. It is never
// initialised: entries are written before they are read.
int ensure_overflow(SlotTables& fs, size_t blocks) { return fs.ovf.grow(blocks * CRT_OVF_WORDS_PER_BLOCK, fs.stream); }

// New frame buffers are allocated first and moved in only when every allocation succeeded: a failed resize leaves
// the old frame size fully usable (crt_resize returns the error; the new buffers free themselves).
int alloc_frame_buffers(int w, int h)
{
    const size_t pixels = (size_t)w * (size_t)h;
    DevBuf<float> rays; DevBuf<float4> outs[CRT_MAX_FRAMES_IN_FLIGHT];
    RCCHK(rays.alloc(3 * pixels));
    for (int i = 0; i < g.nSlots; ++i) {   // slots past nSlots are never rendered into
        RCCHK(outs[i].alloc(pixels));
        HIPCHK(hipMemsetAsync(outs[i], 0, sizeof(float4) * pixels, g.stream));
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    g.rays = std::move(rays);
    for (int i = 0; i < CRT_MAX_FRAMES_IN_FLIGHT; ++i) {
        FrameSlot& fs = g.slot[i];
        fs.out = std::move(outs[i]);
        fs.aux = DevBuf<float4>(); fs.gbuf = DevBuf<char>(); fs.ao = DevBuf<float>(); fs.aoRaw = DevBuf<float>(); fs.aoPending = false;
    }
    g.width = w; g.height = h; g.readbackCount = 0; g.pipelinedLatencyMs = 0.0f; g.gbufSlot = -1; g.aoSlot = -1;
    return CRT_OK;
}

// Copies the pixel rows this rank owns (16-row bands dealt round-robin, crt_set_row_bands) from one frame-shaped buffer to
// the same place in another: one strided 2-D copy (a band is contiguous, bands repeat every nRanks * bandRows rows) plus at
// most one partial band at the bottom. Used for band-only read-backs and for the in-process multi-GPU gather.
// The rows rank `rank` of `nRanks` owns, as one strided block list: `fullBands` bands of `bandRows` rows starting at row
// `firstRow` and repeating every bandRows * nRanks rows, plus `tailRows` rows of a last, partial band at row `tailRow`.
struct BandPlan { int firstRow, fullBands, tailRow, tailRows; };
// what every caller of band_plan has to hold: bands of whole tile rows, and `rank` one of `nRanks`
bool valid_bands(int bandRows, int rank, int nRanks) { return bandRows >= CRT_TILE && bandRows % CRT_TILE == 0 && nRanks >= 1 && rank >= 0 && rank < nRanks; }
BandPlan band_plan(int height, int bandRows, int rank, int nRanks)
{
    BandPlan p = { rank * bandRows, 0, 0, 0 };
    const int period = bandRows * nRanks;
    if (p.firstRow >= height) { p.tailRow = height; return p; }
    const int x = height - p.firstRow;
    p.fullBands = x / period + ((x % period) >= bandRows ? 1 : 0);
    p.tailRow = p.firstRow + p.fullBands * period;
    p.tailRows = p.tailRow < height ? height - p.tailRow : 0;
    return p;
}

int copy_owned_rows_async(void* dstFrame, const void* srcFrame, size_t bytesPerPixel, hipMemcpyKind kind, hipStream_t stream, bool allRows = false)
{
    const size_t rowBytes = (size_t)g.width * bytesPerPixel;
    if (g.nRanks == 1 || allRows) return (int)hipMemcpyAsync(dstFrame, srcFrame, rowBytes * (size_t)g.height, kind, stream);
    const BandPlan p = band_plan(g.height, g.bandRows, g.rank, g.nRanks);
    const size_t bandBytes = rowBytes * (size_t)g.bandRows, pitch = bandBytes * (size_t)g.nRanks;
    char* d = static_cast<char*>(dstFrame) + (size_t)p.firstRow * rowBytes; const char* sp = static_cast<const char*>(srcFrame) + (size_t)p.firstRow * rowBytes;
    if (p.fullBands > 0) HIPCHK(hipMemcpy2DAsync(d, pitch, sp, pitch, bandBytes, (size_t)p.fullBands, kind, stream));
    if (p.tailRows > 0) {
        const size_t off = (size_t)p.fullBands * pitch;
        HIPCHK(hipMemcpyAsync(d + off, sp + off, rowBytes * (size_t)p.tailRows, kind, stream));
    }
    return CRT_OK;
}

} // namespace
