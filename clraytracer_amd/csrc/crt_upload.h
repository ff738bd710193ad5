// crt_upload.h -- session set-up / tear-down, uploads in the reference layouts (Renderer.cpp:122-193, ResourceManager.cpp:145-300) and read-backs of the pools
// Part of the one translation unit crt_shim.hip (included there, in this order: crt_own.h, crt_state.h, crt_instances.h, crt_upload.h,
// crt_bvh_driver.h, crt_frame.h, crt_query_host.h, crt_ao_host.h, crt_multidev.h); everything here has internal linkage.
#pragma once
namespace {
// ---- per-device implementation of the C-ABI entry points (current state = g) ----


const char* crt1_device_name(void) { return g.deviceName; }

int crt1_upload_texels(const void* rgb8, size_t byteOffset, size_t bytes);

// an integer / a float / an on-off switch (0 = off, any other number = on) from the environment; `dflt` when the variable is not set
int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
float env_float(const char* name, float dflt) { const char* e = getenv(name); return e ? (float)atof(e) : dflt; }
bool env_on(const char* name, bool dflt) { const char* e = getenv(name); return e ? atoi(e) != 0 : dflt; }

// the values of CRT_KERNEL ("default" first: the error text lists them in this order)
const struct { const char* name; Form form; } kKernelForms[] = {
    { "default", Form::Mega }, { "wavefront", Form::Wavefront }, { "refill", Form::Refill }, { "block", Form::Block }, { "ldstop", Form::LdsTop } };

// ---- the steps of init_impl; a failure leaves a half-built State for the caller's destroy_group ----

int open_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return CRT_E_NO_DEVICE;
    if (device < 0 || device >= n) return CRT_E_BAD_ARGUMENT;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    snprintf(g.deviceName, sizeof g.deviceName, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    g.device = device;
    g.numCUs = prop.multiProcessorCount;
    return CRT_OK;
}

// a slot's copy of the instance tables, its staging block and `staged` event, on the slot's stream (a frame slot, or the ray queries' context)
int create_slot_tables(SlotTables& fs)
{
    RCCHK(fs.instBlock.alloc(kStageBytes));                // the slot's instance tables in the staging block's layout (crt_instances.h)
    fs.instances = reinterpret_cast<CrtMeshInstance*>(fs.instBlock + kStageInst); fs.instBounds = reinterpret_cast<float4*>(fs.instBlock + kStageBounds);
    fs.alwaysList = reinterpret_cast<uint32_t*>(fs.instBlock + kStageAlways); fs.tlas = reinterpret_cast<CrtTlasNode*>(fs.instBlock + kStageTlas);
    RCCHK(fs.devInstances.alloc(CRT_MAX_INSTANCES));
    RCCHK(fs.staging.alloc(kStageBytes, hipHostMallocDefault));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&fs.stagingDev), fs.staging, 0));     // the refresh kernel reads the pinned block itself
    RCCHK(fs.staged.create(hipEventDisableTiming));
    HIPCHK(hipEventRecord(fs.staged, fs.stream));
    fs.instVersion = 0;
    return CRT_OK;
}

// frames in flight: 3 by default; more pays when a frame is small against its slowest tile (a rank's 1/8 share of a
// frame: DESIGN.md 6). Each slot has its own stream; past four the runtime needs GPU_MAX_HW_QUEUES raised before
// its first call, or it folds the streams onto four hardware queues (crt_init_devices does that when it still can).
int create_frame_slots()
{
    g.nSlots = std::min(std::max(env_int("CRT_FRAMES_IN_FLIGHT", 3), 1), CRT_MAX_FRAMES_IN_FLIGHT);
    for (int si = 0; si < g.nSlots; ++si) {
        FrameSlot& fs = g.slot[si];
        RCCHK(fs.stream.create(hipStreamNonBlocking));
        RCCHK(fs.partDone.create(hipEventDisableTiming));
        RCCHK(fs.slotDone.create(hipEventDisableTiming));
        for (EventSet& es : fs.es) for (Event& ev : es.ev) RCCHK(ev.create());
        RCCHK(create_slot_tables(fs));
    }
    RCCHK(g.statStart.create());
    g.stream = g.slot[0].stream; g.cur = 0; g.asyncSeq = 0; g.othersBusy = false;
    return CRT_OK;
}

int alloc_pools()
{
    // (the constants crt_device.h's record-address helpers prove their 32-bit offsets with)
    g.triCap = CRT_TRI_POOL_SLOTS;                      // ResourceManager.cpp:158
    g.nodeCap = CRT_NODE_POOL_SLOTS;                    // ResourceManager.cpp:159 (MAX_BVHMEMORY * 2)
    static_assert(CRT_PAIR_POOL_RECORDS == CRT_NODE_POOL_SLOTS / 2 + 1, "the pair pool below");
    g.texelByteCap = CRT_MAX_TEXTURE_BYTES * 2;         // ResourceManager.cpp:163
    RCCHK(g.rawTris.alloc(g.triCap));
    HIPCHK(hipMemsetAsync(g.rawTris, 0, g.triCap * sizeof(CrtTri), g.stream));   // crt_tri_reach_kernel may scan slots nobody has uploaded yet (an upload that leaves a gap)
    RCCHK(g.rawNodes.alloc(g.nodeCap));
    RCCHK(g.roots.alloc(CRT_MAX_MESHES));
    RCCHK(g.rawTexels.alloc(g.texelByteCap + 16));
    RCCHK(g.pairs.alloc((g.nodeCap / 2 + 1) * 4));
    RCCHK(g.triHot.alloc(g.triCap * 9));
    RCCHK(g.triCold.alloc(g.triCap * 2));
    RCCHK(g.bigLeaf.alloc(g.triCap + 1));
    HIPCHK(hipMemset(g.bigLeaf + g.triCap, 0, sizeof(uint32_t)));      // crt_empty_ref: a leaf of zero triangles
    RCCHK(g.rootRefs.alloc(CRT_MAX_MESHES));
    RCCHK(g.topRootRefs.alloc(CRT_MAX_MESHES));
    RCCHK(g.topPairs.alloc(CRT_TOP_PAIRS * 4));
    HIPCHK(hipMemset(g.topPairs, 0, CRT_TOP_PAIRS * 4 * sizeof(float4)));
    RCCHK(g.texels.alloc(g.texelByteCap / 3 + 2));
    RCCHK(g.materials.alloc(CRT_MAX_MATERIALS));
    RCCHK(g.textures.alloc(CRT_MAX_TEXTURES));
    RCCHK(g.counters.alloc(CRT_NUM_COUNTERS));
    RCCHK(g.err.alloc(1));
    RCCHK(g.triReachBits.alloc(1));
    HIPCHK(hipMemset(g.triReachBits, 0, sizeof(uint32_t)));
    // the "never cull" bounds table of frames whose rays start beyond the cull's proven range
    static float4 never[CRT_MAX_INSTANCES];
    for (float4& b : never) b = make_float4(0.f, 0.f, 0.f, -1.0f);
    RCCHK(g.noCullBounds.alloc(CRT_MAX_INSTANCES));
    HIPCHK(hipMemcpy(g.noCullBounds, never, sizeof never, hipMemcpyHostToDevice));
    return CRT_OK;
}

int read_environment()
{
    // CRT_KERNEL: the Trace kernel structure of this session. Unset / "" / "default": the megakernel (faster);
    // "wavefront", "refill", "block": the opt-in compaction forms, "ldstop": tree tops staged in LDS. Anything else is a typo, not a wish for
    // the default: the session refuses to start, so a form's test cannot pass on the megakernel because the name stopped matching.
    const char* e = getenv("CRT_KERNEL");
    const auto* form = std::begin(kKernelForms);
    while (e && *e && form != std::end(kKernelForms) && strcmp(e, form->name) != 0) ++form;
    if (form == std::end(kKernelForms)) {
        fprintf(stderr, "crt_init: CRT_KERNEL=%s is not one of ", e);
        for (const auto& k : kKernelForms) fprintf(stderr, "%s%s", k.name, &k + 1 == std::end(kKernelForms) ? "\n" : ", ");
        return CRT_E_BAD_ARGUMENT;
    }
    g.form = form->form;
    g.splitBeta = env_float("CRT_SPLIT_BETA", CRT_SPLIT_BETA);
    g.splitBetaAsync = env_float("CRT_SPLIT_BETA_ASYNC", CRT_SPLIT_BETA_ASYNC);
    g.costSpread = env_float("CRT_COST_SPREAD", 0.8f);
    const char* split = getenv("CRT_SPLIT");            // tuning knob: cap on quadrant-split tiles per XCD (both modes)
    g.maxSplit = split ? std::min(std::max(atoi(split), 0), CRT_MAX_SPLIT) : CRT_MAX_SPLIT; g.maxSplitPipelined = split ? g.maxSplit : CRT_MAX_SPLIT_PIPELINED;
    g.gather8 = env_on("CRT_GATHER_RGBA8", true);
    { const char* e = getenv("CRT_TLAS"); g.forceTlas = e ? (atoi(e) != 0 ? 1 : 0) : -1; }
    g.staggerUs = env_int("CRT_STAGGER_US", -1);
    g.feedback = env_on("CRT_FEEDBACK", true);
    g.feedbackAsync = env_on("CRT_FEEDBACK_ASYNC", false);
    g.raysGridCap = std::max(env_int("CRT_RAYS_GRID", 0), 0);      // crt_trace_rays: cap on the persistent grid (0 = none)
    return CRT_OK;
}

// the empty scene: no nodes, roots, instances or texels, every mesh's root reference an empty leaf
int reset_scene()
{
    HIPCHK(hipMemset(g.roots, 0, CRT_MAX_MESHES * sizeof(uint32_t)));
    { std::vector<uint32_t> e(CRT_MAX_MESHES, crt_empty_ref((uint32_t)g.triCap)); HIPCHK(hipMemcpy(g.rootRefs, e.data(), e.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(g.topRootRefs, e.data(), e.size() * sizeof(uint32_t), hipMemcpyHostToDevice)); }
    HIPCHK(hipMemset(g.materials, 0, CRT_MAX_MATERIALS * sizeof(CrtMaterial)));
    HIPCHK(hipMemset(g.textures, 0, CRT_MAX_TEXTURES * sizeof(CrtTexture)));
    HIPCHK(hipMemset(g.texels, 0, 64));
    g.nodeCount = 0; g.numRoots = 0; g.texelBytesHigh = 0; g.trisHigh = 0; g.sceneValid = true; g.instHigh = 0;
    memset(g.hInstances, 0, sizeof g.hInstances); memset(g.hRoots, 0, sizeof g.hRoots);
    memset(g.hHaveRoot, 0, sizeof g.hHaveRoot); g.instVersion = 1;
    rebuild_instance_master();
    return CRT_OK;
}

static int init_impl(int device, int width, int height)
{
    if (g.initialized) return CRT_E_BAD_ARGUMENT;
    if (width < 16 || height < 16) return CRT_E_BAD_ARGUMENT;
    RCCHK(open_device(device));
    RCCHK(create_frame_slots());
    RCCHK(alloc_pools());
    RCCHK(read_environment());
    RCCHK(reset_scene());
    g.bandRows = 16; g.rank = 0; g.nRanks = 1;
    RCCHK(alloc_frame_buffers(width, height));
    g.initialized = true;
    // default white / black texels (ResourceManager.cpp:168-177)
    const unsigned char def[6] = { 0xFF, 0xFF, 0xFF, 0, 0, 0 };
    return crt1_upload_texels(def, 0, 6);
}

// Waits for everything the session may still have running, also after an init that failed half way. Freeing is not done here: the
// owners in State release what they hold when destroy_group deletes it.
static void release_all()
{
    for (FrameSlot& fs : g.slot) if (fs.stream) (void)hipStreamSynchronize(fs.stream);
    if (g.rayQuery.raysDone) (void)hipEventSynchronize(g.rayQuery.raysDone);      // the last ray query runs on its caller's stream
    if (g.rayQuery.tables.stream) (void)hipStreamSynchronize(g.rayQuery.tables.stream);
}

int crt1_resize(int width, int height)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (width < 16 || height < 16) return CRT_OK; // Renderer.cpp:200
    RCCHK(sync_all());
    return alloc_frame_buffers(width, height);
}

int crt1_set_row_bands(int bandRows, int rank, int nRanks)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!valid_bands(bandRows, rank, nRanks)) return CRT_E_BAD_ARGUMENT;
    RCCHK(sync_all());
    g.bandRows = bandRows; g.rank = rank; g.nRanks = nRanks;
    return CRT_OK;
}

int crt1_owned_rows(void)
{
    if (!g.initialized) return 0;
    const BandPlan p = band_plan(g.height, g.bandRows, g.rank, g.nRanks);
    return p.fullBands * g.bandRows + p.tailRows;
}

// The prologue of every upload and read-back of a pool, in this order: no session; nothing to do (CRT_OK); no buffer, or `first` / `count` not whole
// multiples of `unit`; beyond the pool's `cap` (first, count and cap in the same units: bytes where unit is a record's size, else elements).
#define SPANCHK(p, first, count, unit, cap) do { \
    if (!g.initialized) return CRT_E_NOT_INITIALIZED; \
    if ((count) == 0) return CRT_OK; \
    if (!(p) || (first) % (unit) || (count) % (unit)) return CRT_E_BAD_ARGUMENT; \
    if ((first) + (count) > (cap)) return CRT_E_OUT_OF_RANGE; } while (0)

int crt1_upload_triangles(const void* tris, size_t byteOffset, size_t bytes)
{
    SPANCHK(tris, byteOffset, bytes, sizeof(CrtTri), g.triCap * sizeof(CrtTri));
    RCCHK(quiesce());
    HIPCHK(hipMemcpyAsync(g.rawTris + byteOffset / sizeof(CrtTri), tris, bytes, hipMemcpyHostToDevice, g.stream));
    const size_t first = byteOffset / sizeof(CrtTri), count = bytes / sizeof(CrtTri);
    crt_relayout_tris<<<(unsigned)((count + 255) / 256), 256, 0, g.stream>>>(g.rawTris, first, count, g.triHot, g.triCold);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g.stream));
    // How far from the object-space origin a vertex (hence a hit point, hence a bounce-ray origin, hazard H6) can lie: the cull's proven range is
    // checked against this as well as against the root boxes, so that nodes uploaded through crt_upload_bvh_nodes whose boxes do not bound their
    // triangles cannot take bounce origins beyond it. Reduced on the device from the pool itself (r6, ADVICE r5: it used to be a serial host
    // scan per upload and per device state, and could only grow): an upload that appends folds its own range in; one that overwrites triangles
    // uploaded before recomputes over the whole pool, so a far vertex that has been replaced stops counting.
    const bool overwrites = first < g.trisHigh;
    if (first + count > g.trisHigh) g.trisHigh = first + count;
    if (overwrites) HIPCHK(hipMemsetAsync(g.triReachBits, 0, sizeof(uint32_t), g.stream));
    {
        const size_t f0 = overwrites ? 0 : first, n0 = overwrites ? g.trisHigh : count;
        crt_tri_reach_kernel<<<(unsigned)((n0 + 255) / 256), 256, 0, g.stream>>>(g.rawTris, f0, n0, g.triReachBits);
        HIPCHK(hipGetLastError());
    }
    uint32_t bitsHost = 0;
    HIPCHK(hipMemcpyAsync(&bitsHost, g.triReachBits, sizeof bitsHost, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    {
        float f; memcpy(&f, &bitsHost, sizeof f);
        const double far2 = (f == f && f < 3.0e38f) ? (double)f * (1.0 + 1e-6) : 1e300;     // (fp32 sum of three squares: 3 roundings; inf / NaN: unbounded)
        if (far2 != g.triReach2) { g.triReach2 = far2; rebuild_instance_master(); }
    }
    return CRT_OK;
}

int crt1_upload_bvh_nodes(const void* nodes, size_t byteOffset, size_t bytes)
{
    SPANCHK(nodes, byteOffset, bytes, sizeof(CrtBVHNode), g.nodeCap * sizeof(CrtBVHNode));
    RCCHK(quiesce());
    HIPCHK(hipMemcpyAsync(g.rawNodes + byteOffset / sizeof(CrtBVHNode), nodes, bytes, hipMemcpyHostToDevice, g.stream));
    const uint32_t high = (uint32_t)((byteOffset + bytes) / sizeof(CrtBVHNode));
    if (high > g.nodeCount) g.nodeCount = high;
    return rebuild_bvh_layout();
}

int crt1_upload_bvh_roots(const uint32_t* roots, size_t firstMesh, size_t count)
{
    SPANCHK(roots, firstMesh, count, 1, CRT_MAX_MESHES);
    RCCHK(quiesce());
    HIPCHK(hipMemcpyAsync(g.roots + firstMesh, roots, count * sizeof(uint32_t), hipMemcpyHostToDevice, g.stream));
    memcpy(g.hRoots + firstMesh, roots, count * sizeof(uint32_t));
    if (firstMesh + count > g.numRoots) g.numRoots = (uint32_t)(firstMesh + count);
    return rebuild_bvh_layout();
}

// a range of a fixed table of `elem`-byte records, `cap` of them
int upload_table(void* table, size_t elem, size_t cap, const void* src, size_t first, size_t count)
{
    SPANCHK(src, first, count, 1, cap);
    RCCHK(quiesce());
    HIPCHK(hipMemcpyAsync(static_cast<char*>(table) + first * elem, src, count * elem, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return CRT_OK;
}
int crt1_upload_materials(const void* materials, size_t first, size_t count) { return upload_table(g.materials, sizeof(CrtMaterial), CRT_MAX_MATERIALS, materials, first, count); }
int crt1_upload_texture_table(const void* textures, size_t count) { return upload_table(g.textures, sizeof(CrtTexture), CRT_MAX_TEXTURES, textures, 0, count); }

int crt1_upload_texels(const void* rgb8, size_t byteOffset, size_t bytes)
{
    SPANCHK(rgb8, byteOffset, bytes, 1, g.texelByteCap);
    RCCHK(quiesce());
    HIPCHK(hipMemcpyAsync(g.rawTexels + byteOffset, rgb8, bytes, hipMemcpyHostToDevice, g.stream));
    if (byteOffset + bytes > g.texelBytesHigh) g.texelBytesHigh = byteOffset + bytes;
    const size_t firstTexel = byteOffset / 3;
    // Every texel the span touches whose three bytes are in the pool. At the pool's end that is whole texels only (a trailing partial texel waits for
    // its bytes); a span that ends inside a texel uploaded before must redo that texel as well, or its word keeps the bytes it was made from.
    const size_t endTexel = std::min((byteOffset + bytes + 2) / 3, g.texelBytesHigh / 3);
    if (endTexel > firstTexel) {
        const size_t count = endTexel - firstTexel;
        crt_relayout_texels<<<(unsigned)((count + 255) / 256), 256, 0, g.stream>>>(g.rawTexels, firstTexel, count, g.texels);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    return CRT_OK;
}

int crt1_upload_instances(const void* instances, size_t first, size_t count)
{
    SPANCHK(instances, first, count, 1, CRT_MAX_INSTANCES);
    const CrtMeshInstance* in = static_cast<const CrtMeshInstance*>(instances);
    for (size_t i = 0; i < count; ++i) if (in[i].meshIndex >= CRT_MAX_MESHES) return CRT_E_BAD_ARGUMENT;
    // host only: frames already submitted keep the tables they were submitted with, every later frame (on whichever
    // slot) refreshes its slot's copy on its own stream first -- an animated scene stays pipelined
    memcpy(g.hInstances + first, instances, count * sizeof(CrtMeshInstance));
    if (first + count > g.instHigh) g.instHigh = (uint32_t)(first + count);
    rebuild_instance_master((uint32_t)first, (uint32_t)count, false);      // only the records that were replaced (+ a refit of the instance tree)
    return CRT_OK;
}

// Read back the reference-layout pools (after crt1_build_bvh: the reordered triangles with their centroids, the nodes,
// the roots), e.g. to keep host arenas in step with the device.
int download_pool(void* dst, const void* pool, size_t unit, size_t cap, size_t byteOffset, size_t bytes)
{
    SPANCHK(dst, byteOffset, bytes, unit, cap * unit);
    RCCHK(sync_all());
    HIPCHK(hipMemcpy(dst, static_cast<const char*>(pool) + byteOffset, bytes, hipMemcpyDeviceToHost));
    return CRT_OK;
}
int crt1_download_triangles(void* dst, size_t byteOffset, size_t bytes) { return download_pool(dst, g.rawTris, sizeof(CrtTri), g.triCap, byteOffset, bytes); }
int crt1_download_bvh_nodes(void* dst, size_t byteOffset, size_t bytes) { return download_pool(dst, g.rawNodes, sizeof(CrtBVHNode), g.nodeCap, byteOffset, bytes); }

int crt1_download_bvh_roots(uint32_t* dst, size_t firstMesh, size_t count)
{
    SPANCHK(dst, firstMesh, count, 1, CRT_MAX_MESHES);
    RCCHK(sync_all());
    HIPCHK(hipMemcpy(dst, g.roots + firstMesh, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CRT_OK;
}

} // namespace
