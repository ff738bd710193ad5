// crt_bvh_driver.h -- host driver of the device BuildBVH (kernels: crt_bvh_build.h; reference: BVH.cpp:218-255)
// Part of the one translation unit crt_shim.hip (included there, in this order: crt_own.h, crt_state.h, crt_instances.h, crt_upload.h,
// crt_bvh_driver.h, crt_frame.h, crt_query_host.h, crt_ao_host.h, crt_multidev.h); everything here has internal linkage.
#pragma once
namespace {

const int kBuildCtlLevels = 256;   // one zeroed control record per level up to here (one memset); deeper levels reuse the last one

// What the stages of one crt1_build_bvh share
struct BuildCtx {
    size_t firstTri = 0, firstNode = 0, firstMesh = 0; const uint32_t* meshTriCounts = nullptr; int numMeshes = 0;
    size_t total = 0;                                          // triangles of all meshes
    size_t maxNodes = 0, maxBig = 0, maxChunks = 0;            // capacities of the scratch arrays
    hipStream_t st = nullptr;
    CrtTri* src = nullptr; CrtTri* dst = nullptr;              // the two triangle pools: the level reads src and writes dst
    // the scratch (carve_scratch)
    CrtBuildNode* bn = nullptr;
    uint32_t* rank = nullptr; uint32_t* holes = nullptr; uint32_t* backL = nullptr;
    CrtBuildLists lists[2]; CrtBigScratch* bigs[2]; uint32_t* chunkNode[2];   // of the current level [cur] and the next one [cur ^ 1]
    uint32_t* chunkL = nullptr; uint32_t* chunkFR = nullptr; uint32_t* chunkBL = nullptr;
    uint32_t* dCounts = nullptr; uint32_t* dRoots = nullptr;
    uint32_t* dScal = nullptr;                                 // [0] nodes used, [1] "a node number fell outside the node array"
    CrtBuildCtl* dCtls = nullptr;                              // per level: next level's list sizes and chunk count (crt_bvh_build.h)
    // the level loop
    int cur = 0, level = 0;
    uint32_t cnt[3] = { 0, 0, 0 }, chunks = 0;                 // the current level's BIG / MID / TINY nodes and the chunks of the BIG ones
    uint32_t end = 0;                                          // build nodes so far; the current level's are the last cnt[0] + cnt[1] + cnt[2]
    CrtBuildCtl* dCtl = nullptr; CrtBuildCtl ctl = { 0, 0, 0 };   // the current level's control record, on the device and read back
    bool replaying = false, recording = false;                 // CRT_DEBUG_BVH_REPLAY (arm_replay)
};

// every kernel launch of a build, counted for crt_debug_build_stats
#define BVH_LAUNCH(kernel, grid, block, ...) do { kernel<<<(grid), (block), 0, c.st>>>(__VA_ARGS__); ++g.buildLaunches; } while (0)

// nothing stays queued behind a refused build
static int refuse(const BuildCtx& c) { (void)hipStreamSynchronize(c.st); return CRT_E_OUT_OF_RANGE; }

static int validate(BuildCtx& c)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!c.meshTriCounts || c.numMeshes < 1) return CRT_E_BAD_ARGUMENT;
    if (c.firstMesh + (size_t)c.numMeshes > CRT_MAX_MESHES) return CRT_E_OUT_OF_RANGE;
    for (int m = 0; m < c.numMeshes; ++m) { if (c.meshTriCounts[m] == 0) return CRT_E_BAD_ARGUMENT; c.total += c.meshTriCounts[m]; }
    if (c.firstTri + c.total > g.trisHigh) return CRT_E_BAD_ARGUMENT;              // triangles must have been uploaded
    if (c.firstTri + c.total > 0x00FFFFFFu) return CRT_E_OUT_OF_RANGE;             // leaf references carry 24-bit triangle indices
    if (c.firstNode + 2 * c.total > g.nodeCap) return CRT_E_OUT_OF_RANGE;          // a mesh of n triangles needs at most 2n-1 nodes
    if (c.total / CRT_BVH_SMALL >= (1u << 20) || c.total / CRT_BVH_TINY >= (1u << 20)) return CRT_E_OUT_OF_RANGE;   // field widths of the packed per-level counter (crt_bvh_build.h)
    // test hook (CRT_DEBUG_HOOKS=1 only): refuse, so that the caller's fall-back to the host BuildBVH can be exercised
    const char* h = getenv("CRT_DEBUG_HOOKS"); const char* f = getenv("CRT_DEBUG_FAIL_BVH_BUILD");
    // CRT_DEBUG_FAIL_BVH_BUILD: 1 = CRT_E_OUT_OF_RANGE; any other non-zero value is returned as it is -- 2 (hipErrorOutOfMemory: the builder's
    // scratch could not be allocated), -2 (CRT_E_BAD_ARGUMENT), 719 (hipErrorLaunchFailure: a sticky fault, the one kind the caller must not paper over)
    if (h && atoi(h) != 0 && f && atoi(f) != 0) return atoi(f) == 1 ? (int)CRT_E_OUT_OF_RANGE : atoi(f);
    return CRT_OK;
}

// second triangle pool (allocated on first use, indexed like rawTris) and scratch:
// build nodes | rank, holes, backL | 2 x 3 id lists | 2 x BIG-node scratch | 2 x chunk->node + 3 per-chunk counts | mesh counts, roots, scalars, control records
static int carve_scratch(BuildCtx& c)
{
    if (!g.buildTris) RCCHK(g.buildTris.alloc(g.triCap));
    if (!g.buildCtlHost) { RCCHK(g.buildCtlHost.alloc(1, hipHostMallocMapped | hipHostMallocCoherent)); g.buildCtlHost->seq = 0; g.buildSeq = 0; }
    const size_t total = c.total, nm = (size_t)c.numMeshes;
    c.maxNodes = 2 * total + nm;
    const size_t listCap = total + nm;                         // a level never has more nodes than triangles
    c.maxBig = total / CRT_BVH_SMALL + nm + 1;                 // BIG nodes of one level (each has more than CRT_BVH_SMALL triangles)
    c.maxChunks = total / CRT_BVH_CHUNK + c.maxBig + 1;        // sum of ceil(n / CRT_BVH_CHUNK) over them
    size_t off = 0;
    auto bump = [&off](size_t bytes) { off = (off + 255) & ~(size_t)255; const size_t at = off; off += bytes; return at; };
    const size_t offNodes = bump(c.maxNodes * sizeof(CrtBuildNode));
    const size_t offRank = bump(3 * total * sizeof(uint32_t));
    const size_t offLists = bump(6 * listCap * sizeof(uint32_t));
    const size_t offBig = bump(2 * c.maxBig * sizeof(CrtBigScratch));
    const size_t offChunks = bump(5 * c.maxChunks * sizeof(uint32_t));
    const size_t offSmall = bump((2 * nm + 8) * sizeof(uint32_t) + kBuildCtlLevels * sizeof(CrtBuildCtl) + 16);
    RCCHK(g.buildBuf.grow(off, g.stream));                     // (the stream is idle: crt1_build_bvh has just waited for it in sync_all)
    char* base = g.buildBuf;
    c.bn = reinterpret_cast<CrtBuildNode*>(base + offNodes);
    c.rank = reinterpret_cast<uint32_t*>(base + offRank); c.holes = c.rank + total; c.backL = c.holes + total;
    uint32_t* listMem = reinterpret_cast<uint32_t*>(base + offLists);
    for (int p = 0; p < 2; ++p) for (int k = 0; k < 3; ++k) c.lists[p].list[k] = listMem + ((size_t)p * 3 + (size_t)k) * listCap;
    c.bigs[0] = reinterpret_cast<CrtBigScratch*>(base + offBig); c.bigs[1] = c.bigs[0] + c.maxBig;
    uint32_t* chunkMem = reinterpret_cast<uint32_t*>(base + offChunks);
    c.chunkNode[0] = chunkMem; c.chunkNode[1] = chunkMem + c.maxChunks;
    c.chunkL = chunkMem + 2 * c.maxChunks; c.chunkFR = c.chunkL + c.maxChunks; c.chunkBL = c.chunkFR + c.maxChunks;
    c.dCounts = reinterpret_cast<uint32_t*>(base + offSmall); c.dRoots = c.dCounts + nm; c.dScal = c.dRoots + nm;
    c.dCtls = reinterpret_cast<CrtBuildCtl*>((reinterpret_cast<uintptr_t>(c.dScal + 2) + 15) & ~(uintptr_t)15);
    c.st = g.stream; c.src = g.rawTris; c.dst = g.buildTris;
    return CRT_OK;
}

// level 0 = the roots, classified here; their centroids, records and (BIG ones) chunks on the device
static int seed_roots(BuildCtx& c)
{
    HIPCHK(hipMemsetAsync(c.dCtls, 0, kBuildCtlLevels * sizeof(CrtBuildCtl), c.st));
    HIPCHK(hipMemcpyAsync(c.dCounts, c.meshTriCounts, (size_t)c.numMeshes * sizeof(uint32_t), hipMemcpyHostToDevice, c.st));
    std::vector<uint32_t> ids[3];
    for (int m = 0; m < c.numMeshes; ++m) {
        const int cls = bvh_class(c.meshTriCounts[m]);
        ids[cls].push_back((uint32_t)m);
        if (cls == CRT_BVH_CLASS_BIG) c.chunks += bvh_chunks(c.meshTriCounts[m]);
    }
    for (int k = 0; k < 3; ++k) {
        c.cnt[k] = (uint32_t)ids[k].size();
        if (c.cnt[k]) HIPCHK(hipMemcpyAsync(c.lists[0].list[k], ids[k].data(), c.cnt[k] * sizeof(uint32_t), hipMemcpyHostToDevice, c.st));
    }
    HIPCHK(hipStreamSynchronize(c.st));                        // ids[] go out of scope
    c.end = (uint32_t)c.numMeshes;
    BVH_LAUNCH(crt_bvh_centroids, (unsigned)((c.total + 255) / 256), 256, c.src, c.firstTri, c.total);
    BVH_LAUNCH(crt_bvh_init_roots, 1, 1, c.bn, c.dCounts, c.numMeshes, (uint32_t)c.firstTri, c.bigs[0], c.chunkNode[0]);
    HIPCHK(hipGetLastError());
    return CRT_OK;
}

// FNV-1a over what determines the level structure besides the triangles themselves
static unsigned long long replay_key(const BuildCtx& c)
{
    unsigned long long key = 1469598103934665603ull;
    auto mix = [&](unsigned long long v) { for (int b = 0; b < 8; ++b) { key ^= (v >> (8 * b)) & 0xFFu; key *= 1099511628211ull; } };
    mix(c.firstTri); mix(c.total); mix((unsigned long long)c.numMeshes);
    for (int m = 0; m < c.numMeshes; ++m) mix(c.meshTriCounts[m]);
    return key;
}
// Measurement hook (CRT_DEBUG_HOOKS=1 + CRT_DEBUG_BVH_REPLAY=1): the builder is deterministic, so a build of the SAME input can
// take every level's list sizes from a recording of the previous one and enqueue all its launches back to back -- exact grids, no publish
// kernel, no host round trip per level. That is the floor of ANY one-submission scheme (a HIP graph re-launched with device-read grid sizes,
// a persistent kernel with a device-side level counter): what `crt_build_bvh` would take if the level hand-shake cost nothing.
// (The caller must rebuild the SAME triangles -- tools/bvh_build_time.py does; the key covers only the mesh sizes. A mismatch ends in
// CRT_E_OUT_OF_RANGE at the final node-count check.)
static void arm_replay(BuildCtx& c)
{
    const char* h = getenv("CRT_DEBUG_HOOKS"); const char* r = getenv("CRT_DEBUG_BVH_REPLAY");
    if (!(h && atoi(h) != 0 && r && atoi(r) != 0)) { g.buildReplay.clear(); return; }
    const unsigned long long key = replay_key(c);
    c.replaying = !g.buildReplay.empty() && g.buildReplayKey == key;
    if (!c.replaying) { g.buildReplay.clear(); g.buildReplayKey = key; c.recording = true; }
}

// one level: every node of lists[cur] is decided, and the triangles of those that split move from src to dst
static int launch_level(BuildCtx& c)
{
    const unsigned W = CRT_BVH_WAVES, T = CRT_BVH_BIG_THREADS;
    const CrtBuildLists& L = c.lists[c.cur]; const CrtBuildLists& N = c.lists[c.cur ^ 1];
    const uint32_t first = (uint32_t)c.firstTri;
    c.dCtl = c.dCtls + (c.level < kBuildCtlLevels ? c.level : kBuildCtlLevels - 1);
    if (c.level >= kBuildCtlLevels - 1) HIPCHK(hipMemsetAsync(c.dCtl, 0, sizeof(CrtBuildCtl), c.st));   // the shared last record (zero already on its first use: harmless)
    ++c.level; ++g.buildLevels;
    if (c.cnt[0]) {
        CrtBigScratch* big = c.bigs[c.cur]; const uint32_t* cn = c.chunkNode[c.cur];
        // (bounds of MID and TINY nodes: at the top of crt_bvh_mid / crt_bvh_tiny, 26 launches fewer per 1 M-triangle build)
        BVH_LAUNCH(crt_bvh_big_reset, (c.cnt[0] + 255) / 256, 256, big, c.cnt[0]);
        BVH_LAUNCH(crt_bvh_big_bounds, c.chunks, T, c.bn, L.list[0], big, cn, c.src);
        BVH_LAUNCH(crt_bvh_big_bins, c.chunks, T, c.bn, L.list[0], big, cn, c.src);
        BVH_LAUNCH(crt_bvh_big_sweep, c.chunks, T, c.bn, L.list[0], big, cn, c.src, c.dst, c.chunkL);
        BVH_LAUNCH(crt_bvh_big_count, c.chunks, T, c.bn, L.list[0], big, cn, c.src, c.chunkL, c.chunkFR, c.chunkBL);
        BVH_LAUNCH(crt_bvh_big_tables, c.chunks, T, c.bn, L.list[0], big, cn, c.src, first, c.chunkFR, c.chunkBL, c.rank, c.holes, c.backL);
        BVH_LAUNCH(crt_bvh_big_scatter, c.chunks, T, c.bn, L.list[0], big, cn, c.src, c.dst, first, c.rank, c.holes, c.backL, c.end, c.dCtl, N, c.bigs[c.cur ^ 1], c.chunkNode[c.cur ^ 1]);
    }
    if (c.cnt[1]) BVH_LAUNCH(crt_bvh_mid, (c.cnt[1] + W - 1) / W, 64 * W, c.bn, L.list[1], c.cnt[1], c.src, c.dst, first, c.rank, c.holes, c.backL, c.end, &c.dCtl->packed, N);
    if (c.cnt[2]) BVH_LAUNCH(crt_bvh_tiny, (c.cnt[2] + 63) / 64, 64, c.bn, L.list[2], c.cnt[2], c.src, c.dst, c.end, &c.dCtl->packed, N);
    HIPCHK(hipGetLastError());
    return CRT_OK;
}

// The level's list sizes into c.ctl: published into pinned memory behind the level's kernels; spin on the sequence number (a copy + stream
// synchronisation per level cost ~40 us x 23 levels of a 1 M-triangle build), fall back to the stream if it does not arrive
static int read_level_sizes(BuildCtx& c)
{
    if (c.replaying && (size_t)(c.level - 1) < g.buildReplay.size()) {
        // measurement hook (arm_replay): the level's list sizes are known from the recorded build of the same input -- no publish, no wait
        c.ctl = g.buildReplay[(size_t)(c.level - 1)];
        return CRT_OK;
    }
    const uint32_t seq = ++g.buildSeq;
    BVH_LAUNCH(crt_bvh_publish, 1, 1, c.dCtl, g.buildCtlHost, seq);
    HIPCHK(hipGetLastError());
    bool arrived = false;
    for (unsigned spin = 0; spin < (1u << 22) && !g.buildNoSpin; ++spin) {
        if (g.buildCtlHost->seq == seq) { arrived = true; break; }
        if ((spin & 0x3FFu) == 0x3FFu && hipStreamQuery(c.st) != hipErrorNotReady) {
            // finished (or failed) between two looks at the flag: the record may have landed in that window -- look once more
            // before blaming coherence; a failed stream is sorted out by the synchronisation below
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            arrived = g.buildCtlHost->seq == seq;
            break;
        }
        crt_cpu_relax();
    }
    if (!arrived) {
        HIPCHK(hipStreamSynchronize(c.st)); if (g.buildCtlHost->seq != seq) return CRT_E_UNSUPPORTED;
        // Latched only when the record really was invisible while the level ran: the spin budget ran out with the stream still busy, or
        // the stream had drained and the record was STILL stale at the re-read above (host memory not coherent with running kernels).
        // From then on wait for the stream at once instead of burning the spin budget on every level.
        if (!g.buildNoSpin) { g.buildNoSpin = true; fprintf(stderr, "[crt] crt_build_bvh: the pinned control record is not visible before the stream drains; using stream synchronisation per level\n"); }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    c.ctl = g.buildCtlHost->ctl;
    if (c.recording) g.buildReplay.push_back(c.ctl);
    return CRT_OK;
}

// what c.ctl says: a degenerate BIG partition to finish; then the children become the current level, dst becomes src
static int next_level(BuildCtx& c)
{
    if (c.ctl.degenerate) {                                    // BVH.cpp:194 hit a BIG node: its permuted triangles go to both buffers
        BVH_LAUNCH(crt_bvh_big_degenerate, c.chunks, CRT_BVH_BIG_THREADS, c.bn, c.lists[c.cur].list[0], c.bigs[c.cur], c.chunkNode[c.cur], c.src, c.dst);
        BVH_LAUNCH(crt_bvh_big_degenerate_mark, (c.cnt[0] + 255) / 256, 256, c.bn, c.lists[c.cur].list[0], c.bigs[c.cur], c.cnt[0]);
    }
    for (int k = 0; k < 3; ++k) c.cnt[k] = bvh_unpack(c.ctl.packed, k);
    c.chunks = c.ctl.nextChunks;
    const uint32_t newEnd = c.end + c.cnt[0] + c.cnt[1] + c.cnt[2];
    if (newEnd > (uint32_t)c.maxNodes || c.cnt[0] > c.maxBig || c.chunks > c.maxChunks) return refuse(c);
    c.end = newEnd;
    std::swap(c.src, c.dst);
    c.cur ^= 1;
    return CRT_OK;
}

// numbering in closed form (crt_bvh_build.h): leaf starts -> exclusive prefix counts S (flags in `rank`, S in `holes`..: total + 1 words) -> one pass
static int number_and_emit(BuildCtx& c)
{
    const uint32_t numBuilt = c.end, total = (uint32_t)c.total, first = (uint32_t)c.firstTri;
    if (c.firstNode + numBuilt > g.nodeCap) return refuse(c);
    uint32_t* flags = c.rank; uint32_t* S = c.holes; uint32_t* sums = c.chunkL;
    const uint32_t nb = (uint32_t)(c.total / CRT_BVH_SCAN_ITEMS) + 1;
    if (nb > c.maxChunks) return refuse(c);
    HIPCHK(hipMemsetAsync(flags, 0, c.total * sizeof(uint32_t), c.st));
    HIPCHK(hipMemsetAsync(c.dScal, 0, 2 * sizeof(uint32_t), c.st));
    BVH_LAUNCH(crt_bvh_leaf_flags, (numBuilt + 255) / 256, 256, c.bn, numBuilt, first, flags);
    BVH_LAUNCH(crt_bvh_scan_sums, nb, CRT_BVH_SCAN_THREADS, flags, total, sums);
    BVH_LAUNCH(crt_bvh_scan_blocks, 1, CRT_BVH_SCAN_THREADS, sums, nb);
    BVH_LAUNCH(crt_bvh_scan_apply, nb, CRT_BVH_SCAN_THREADS, flags, total, sums, S);
    BVH_LAUNCH(crt_bvh_emit, (numBuilt + 255) / 256, 256, c.bn, numBuilt, c.numMeshes, S, first, total, (uint32_t)c.firstNode, g.rawNodes, c.dRoots, c.dScal, c.dScal + 1);
    HIPCHK(hipGetLastError());
    return CRT_OK;
}

// read-backs, the triangles' render layout, the final consistency check, the nodes' render layout
static int finish(BuildCtx& c, uint32_t* nodesUsedOut)
{
    const size_t rootBytes = (size_t)c.numMeshes * sizeof(uint32_t);
    uint32_t scal[2] = { 0, 0 };
    HIPCHK(hipMemcpyAsync(scal, c.dScal, sizeof scal, hipMemcpyDeviceToHost, c.st));
    HIPCHK(hipMemcpyAsync(g.roots + c.firstMesh, c.dRoots, rootBytes, hipMemcpyDeviceToDevice, c.st));
    HIPCHK(hipMemcpyAsync(g.hRoots + c.firstMesh, c.dRoots, rootBytes, hipMemcpyDeviceToHost, c.st));
    BVH_LAUNCH(crt_relayout_tris, (unsigned)((c.total + 255) / 256), 256, g.rawTris, c.firstTri, c.total, g.triHot, g.triCold);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c.st));
    const uint32_t used = scal[0];
    if (scal[1] != 0 || used != c.end) return CRT_E_OUT_OF_RANGE;   // the closed form and the level loop disagree: never seen, would mean a damaged tree
    if (c.firstNode + used > g.nodeCount) g.nodeCount = (uint32_t)(c.firstNode + used);
    if (c.firstMesh + (size_t)c.numMeshes > g.numRoots) g.numRoots = (uint32_t)(c.firstMesh + (size_t)c.numMeshes);
    if (nodesUsedOut) *nodesUsedOut = used;
    return rebuild_bvh_layout();
}

// BuildBVH on the device (crt_bvh_build.h): same triangle order, node numbering and bounds as the host builder.
int crt1_build_bvh(size_t firstTri, const uint32_t* meshTriCounts, int numMeshes, size_t firstNode, size_t firstMesh, uint32_t* nodesUsedOut)
{
    BuildCtx c;
    c.firstTri = firstTri; c.meshTriCounts = meshTriCounts; c.numMeshes = numMeshes; c.firstNode = firstNode; c.firstMesh = firstMesh;
    RCCHK(validate(c));
    RCCHK(sync_all());
    g.buildLaunches = 0; g.buildLevels = 0;
    RCCHK(carve_scratch(c));
    RCCHK(seed_roots(c));
    arm_replay(c);
    while (c.cnt[0] + c.cnt[1] + c.cnt[2] > 0) {
        RCCHK(launch_level(c));
        RCCHK(read_level_sizes(c));
        RCCHK(next_level(c));
    }
    RCCHK(number_and_emit(c));
    return finish(c, nodesUsedOut);
}

#undef BVH_LAUNCH

} // namespace
