// crt_query_host.h -- the queries on device buffers, host half: the context (State::rayQuery), the one launch sequence and the one statistics
// reader of every family, and crt_trace_rays. crt_trace_ao / crt_frame_ao: crt_ao_host.h; crt_shade_rays: crt_shade_host.h. The kernels' half: crt_query.h.
// Part of the one translation unit crt_shim.hip (included there behind crt_frame.h and in front of crt_ao_host.h); everything here has
// internal linkage.
#pragma once
namespace {

#define CRT_RAYS_MAX ((uint64_t)1 << 30)

// first query of the session: the context's stream, tables, control words and event (the one allocation a query may wait for, besides a
// growing overflow area)
static int ensure_ray_query_context()
{
    QueryContext& q = g.rayQuery;
    if (q.ready) return CRT_OK;
    if (!q.tables.stream) RCCHK(q.tables.stream.create(hipStreamNonBlocking));
    if (!q.tables.instBlock) RCCHK(create_slot_tables(q.tables));
    if (!q.ctl) RCCHK(q.ctl.alloc(6));
    if (!q.raysDone) RCCHK(q.raysDone.create(hipEventDisableTiming));
    q.ready = true;
    return CRT_OK;
}

// The three steps of launch_query that deal with the context; all of the caller's checks come first.
// 1. The scene as the query sees it: the context exists, its instance tables are current -- an instance upload since the last query is
//    refreshed on the context's own stream behind the query that may still read the old tables.
static int query_scene(uint32_t numInstances, CrtDevScene& S)
{
    RCCHK(ensure_ray_query_context());
    QueryContext& q = g.rayQuery;
    SlotTables& fs = q.tables;
    if (fs.instVersion != g.instVersion) {
        if (q.inFlight) HIPCHK(hipStreamWaitEvent(fs.stream, q.raysDone, 0));
        q.refreshPending = true;               // until a raysDone lies behind it: a step that fails below must not leave it unseen by quiesce()
        RCCHK(ensure_slot_instances(fs));
    }
    fill_scene(S, numInstances, fs);
    return CRT_OK;
}
// 2. The persistent grid -- min(chunks, CUs x resident workgroups, CRT_RAYS_GRID) -- with an overflow block per workgroup (the host waits
//    only when the area has to grow), and the caller's stream ordered, on the device, behind the query before and the table refresh.
static int query_grid(uint64_t chunks, int perCU, hipStream_t stream, CrtDevScene& S, uint64_t& grid)
{
    QueryContext& q = g.rayQuery;
    SlotTables& fs = q.tables;
    grid = (uint64_t)g.numCUs * (uint64_t)perCU;
    if (g.raysGridCap > 0 && grid > (uint64_t)g.raysGridCap) grid = (uint64_t)g.raysGridCap;
    if (grid > chunks) grid = chunks;
    if (grid * CRT_OVF_WORDS_PER_BLOCK > fs.ovf.capacity()) {
        if (q.inFlight) { HIPCHK(hipEventSynchronize(q.raysDone)); q.inFlight = false; }      // the query before still owns the old area (grow() frees it)
        RCCHK(ensure_overflow(fs, (size_t)grid));
    }
    S.stackOverflow = fs.ovf;
    if (q.inFlight) HIPCHK(hipStreamWaitEvent(stream, q.raysDone, 0));
    HIPCHK(hipStreamWaitEvent(stream, fs.staged, 0));
    return CRT_OK;
}
// 3. Behind the query's last launch: the event the next query, and whatever edits shared device state (quiesce), waits for.
static int end_query(hipStream_t stream)
{
    QueryContext& q = g.rayQuery;
    HIPCHK(hipEventRecord(q.raysDone, stream));
    q.inFlight = true; q.refreshPending = false;      // (raysDone lies behind `staged`: the stream waited for it)
    return CRT_OK;
}

// A query of family `fam`, enqueue-and-return: the host waits only for the context's first allocation and for a growing overflow area.
// Ordering: the caller's stream waits (hipStreamWaitEvent) for the query before -- queries share the context -- and for the context's
// instance tables, which are refreshed on the context's own stream behind that same query (it may still read the old tables). Frames
// in flight are neither waited for nor touched.
// kernels: the family's instantiations under the box rule asked for (inclusive: those of crt_inclusive.hip), [2 * x + TLAS] -- four, x a
// bool; the shaded queries have six, x = 0 .. 2, and no inclusive form (QueryFamily::residentPerCU holds either) --, launched as
// kernel(S, A, extra...); A: the form's own arguments, its `q` and
// `chunks` are filled here; before(stream) queues what the kernel must wait for, after(stream) what belongs to the query behind it.
template <class Kernel, size_t N, class Args, class Before, class After, class... Extra>
static int launch_query(QueryFamily& fam, Kernel* const (&kernels)[N], bool inclusive, int x, uint32_t numInstances, uint64_t chunks, hipStream_t stream,
                        Before&& before, After&& after, Args A, const Extra&... extra)
{
    CrtDevScene S;
    RCCHK(query_scene(numInstances, S));
    static_assert(N == 4 || N == 6, "a family's instantiations");
    const int which = 2 * x + (int)use_tlas(S);
    if (which < 0 || which >= (int)N || 4 * (int)inclusive + which >= 8) return CRT_E_BAD_ARGUMENT;
    int& resident = fam.residentPerCU[4 * (int)inclusive + which];
    if (resident == 0) {         // as the runtime computes it for this device, asked once per instantiation
        int n = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernels[which], CRT_BLOCK, 0));
        resident = n > 0 ? n : 1;
    }
    uint64_t grid = 0;
    RCCHK(query_grid(chunks, resident, stream, S, grid));
    RCCHK(before(stream));
    uint32_t* ctl = g.rayQuery.ctl + fam.ctl0;
    HIPCHK(hipMemsetAsync(ctl, 0, 2 * sizeof(uint32_t), stream));
    A.q.ctl = ctl; A.q.cullOriginLimit = (double)g.cullOriginLimit; A.q.noCullBounds = g.noCullBounds; A.chunks = (uint32_t)chunks;
    kernels[which]<<<(unsigned)grid, CRT_BLOCK, 0, stream>>>(S, A, extra...);
    HIPCHK(hipGetLastError());
    RCCHK(after(stream));
    RCCHK(end_query(stream));
    fam.chunks = chunks; fam.grid = grid;
    return CRT_OK;
}
static int no_query_step(hipStream_t) { return CRT_OK; }

// {chunks, chunks traced without the cull, workgroups launched} of the family's last query, after waiting for it
static int query_stats(QueryFamily QueryContext::* family, uint64_t out[3])
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!out) return CRT_E_BAD_ARGUMENT;
    QueryContext& q = g.rayQuery;
    const QueryFamily& fam = q.*family;
    out[0] = fam.chunks; out[1] = 0; out[2] = fam.grid;
    if (!q.ready || fam.chunks == 0) return CRT_OK;
    HIPCHK(hipEventSynchronize(q.raysDone));
    q.inFlight = false;
    uint32_t ctl[2] = { 0, 0 };
    HIPCHK(hipMemcpy(ctl, q.ctl + fam.ctl0, sizeof ctl, hipMemcpyDeviceToHost));
    out[1] = ctl[1];
    return CRT_OK;
}

// ---- crt_trace_rays ----
typedef void CrtRaysKernel(CrtDevScene, CrtRaysArgs);
static CrtRaysKernel* const kRaysKernels[4] = { crt_rays_kernel<false, false>, crt_rays_kernel<false, true>, crt_rays_kernel<true, false>, crt_rays_kernel<true, true> };
static CrtRaysKernel* const kRaysInclusiveKernels[4] = { crt_rays_inclusive_kernel<false, false>, crt_rays_inclusive_kernel<false, true>,
                                                         crt_rays_inclusive_kernel<true, false>, crt_rays_inclusive_kernel<true, true> };

// every check comes before the first thing that is queued (launch_query)
int crt1_trace_rays(const CrtRayBatch* rays, uint32_t numInstances, int mode, void* out, hipStream_t stream)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!rays) return CRT_E_BAD_ARGUMENT;
    if (rays->n == 0) return CRT_OK;
    if (!rays->origins || !rays->dirs || !out) return CRT_E_BAD_ARGUMENT;
    if (rays->originStride == 1 || rays->originStride == 2 || rays->dirStride == 1 || rays->dirStride == 2) return CRT_E_BAD_ARGUMENT;
    const bool inclusive = (mode & CRT_RAYS_INCLUSIVE) != 0;
    const int what = mode & ~CRT_RAYS_INCLUSIVE;
    if (what != CRT_RAYS_CLOSEST && what != CRT_RAYS_OCCLUDED) return CRT_E_BAD_ARGUMENT;
    if (numInstances > CRT_MAX_INSTANCES || !g.sceneValid) return CRT_E_BAD_ARGUMENT;
    if (rays->n > CRT_RAYS_MAX) return CRT_E_OUT_OF_RANGE;
    CrtRaysArgs A;
    A.origins = rays->origins; A.dirs = rays->dirs; A.tmax = rays->tmax; A.out = out;
    A.originStride = rays->originStride; A.dirStride = rays->dirStride; A.n = (uint32_t)rays->n;
    return launch_query(g.rayQuery.rays, inclusive ? kRaysInclusiveKernels : kRaysKernels, inclusive, what == CRT_RAYS_OCCLUDED, numInstances, (rays->n + CRT_BLOCK - 1) / CRT_BLOCK, stream,
                        no_query_step, no_query_step, A);
}

int crt1_debug_rays_stats(uint64_t out[3]) { return query_stats(&QueryContext::rays, out); }

} // namespace
