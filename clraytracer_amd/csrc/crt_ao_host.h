// crt_ao_host.h -- ambient occlusion on device points and on G-buffer frames: crt_trace_ao, crt_frame_ao, the AO plane's reads, statistics
// Part of the one translation unit crt_shim.hip (included there behind crt_query_host.h, whose launch_query and query_stats it uses);
// everything here has internal linkage. The kernels: crt_ao.h (declared), crt_ao.hip (compiled); under CRT_AO_INCLUSIVE crt_inclusive.h, crt_inclusive.hip.
#pragma once
namespace {

// the direction table on the host (crt_ao_directions): the same generated rows the kernels' unit compiles into device memory
struct CrtAoDirHost { float x, y, z, w; };
#define CRT_AO_TABLE_DECL static const CrtAoDirHost kAoTable[CRT_AO_TABLE_SIZE]
#include "crt_ao_table.h"
#undef CRT_AO_TABLE_DECL

// CRT_E_BAD_ARGUMENT rules of CrtAoParams; `allowed`: the flags the form accepts
static int check_ao_params(const CrtAoParams* p, uint32_t allowed)
{
    if (!p) return CRT_E_BAD_ARGUMENT;
    const uint32_t n = p->samples;
    if (n == 0 || n > 64 || (n & (n - 1)) != 0) return CRT_E_BAD_ARGUMENT;      // 1, 2, 4, ..., 64
    if (!(p->radius > 0.0f) || !std::isfinite(p->bias)) return CRT_E_BAD_ARGUMENT;   // (a NaN radius fails the comparison)
    if (p->flags & ~allowed) return CRT_E_BAD_ARGUMENT;
    return CRT_OK;
}

// The launch both forms share, a query of the AO family (launch_query): `A` holds the form's own arguments, the parameters are filled here
typedef void CrtAoKernel(CrtDevScene, CrtAoArgs, CrtFrame);
static CrtAoKernel* const kAoKernels[4] = { crt_ao_kernel<CRT_AO_POINTS, false>, crt_ao_kernel<CRT_AO_POINTS, true>, crt_ao_kernel<CRT_AO_FRAME, false>, crt_ao_kernel<CRT_AO_FRAME, true> };
static CrtAoKernel* const kAoInclusiveKernels[4] = { crt_ao_inclusive_kernel<CRT_AO_POINTS, false>, crt_ao_inclusive_kernel<CRT_AO_POINTS, true>,
                                                     crt_ao_inclusive_kernel<CRT_AO_FRAME, false>, crt_ao_inclusive_kernel<CRT_AO_FRAME, true> };
template <class Before, class After>
static int launch_ao(bool frame, CrtAoArgs A, const CrtFrame& F, const CrtAoParams& p, uint32_t numInstances, uint64_t chunks, hipStream_t stream, Before&& before, After&& after)
{
    A.samples = p.samples; A.step = CRT_AO_TABLE_SIZE / p.samples; A.seedMul = p.seed * 0x9E3779B9u; A.radius = p.radius; A.bias = p.bias;
    const bool inclusive = (p.flags & CRT_AO_INCLUSIVE) != 0;
    return launch_query(g.rayQuery.ao, inclusive ? kAoInclusiveKernels : kAoKernels, inclusive, frame, numInstances, chunks, stream, before, after, A, F);
}

// Enqueue-and-return like crt1_trace_rays: every check comes before the first thing that is queued.
int crt1_trace_ao(const CrtAoPoints* pts, const CrtAoParams* params, uint32_t numInstances, float* out, hipStream_t stream)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    if (!pts || !params) return CRT_E_BAD_ARGUMENT;
    if (pts->n == 0) return CRT_OK;
    RCCHK(check_ao_params(params, (uint32_t)CRT_AO_INCLUSIVE));      // (the filter needs a frame's neighbours)
    if (!pts->positions || !pts->normals || !out) return CRT_E_BAD_ARGUMENT;
    if (pts->positionStride == 1 || pts->positionStride == 2 || pts->normalStride == 1 || pts->normalStride == 2) return CRT_E_BAD_ARGUMENT;
    if (numInstances > CRT_MAX_INSTANCES || !g.sceneValid) return CRT_E_BAD_ARGUMENT;
    if (pts->n > CRT_RAYS_MAX) return CRT_E_OUT_OF_RANGE;
    CrtAoArgs A; memset(&A, 0, sizeof A);
    A.positions = pts->positions; A.normals = pts->normals; A.positionStride = pts->positionStride; A.normalStride = pts->normalStride;
    A.out = out; A.n = (uint32_t)pts->n;
    CrtFrame F; memset(&F, 0, sizeof F);
    return launch_ao(false, A, F, *params, numInstances, (pts->n + CRT_BLOCK - 1) / CRT_BLOCK, stream, no_query_step, no_query_step);
}

// The slot of the most recently submitted G-buffer frame, if its planes exist (what crt_read_gbuffer asks too)
static FrameSlot* gbuffer_slot() { return (g.gbufSlot >= 0 && g.slot[g.gbufSlot].gbuf) ? &g.slot[g.gbufSlot] : nullptr; }

// AO of the pixels of the most recently submitted CRT_RENDER_GBUFFER frame into its slot's AO plane. The same query context and ordering
// as crt1_trace_ao; in addition the caller's stream waits, on the device, for that frame (FrameSlot::gbufDone), and the slot's next
// G-buffer frame waits, on the device, for this query (FrameSlot::aoPending, launch_passes). No host wait beyond a first allocation.
int crt1_frame_ao(const CrtAoParams* params, hipStream_t stream)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    RCCHK(check_ao_params(params, (uint32_t)(CRT_AO_FILTER | CRT_AO_INCLUSIVE)));
    FrameSlot* fsp = gbuffer_slot();
    if (!fsp || !g.sceneValid) return CRT_E_BAD_ARGUMENT;
    FrameSlot& fs = *fsp;
    const bool filter = (params->flags & CRT_AO_FILTER) != 0;
    if (filter && g.nRanks > 1) return CRT_E_UNSUPPORTED;      // the filter reads across band edges (as FXAA)
    const size_t pixels = (size_t)g.width * (size_t)g.height;
    // (first use of the slot's planes: nothing queued reads them yet; later calls find them large enough)
    RCCHK(fs.ao.grow(pixels, fs.stream));
    if (filter) RCCHK(fs.aoRaw.grow(pixels, fs.stream));
    CrtFrame F;
    fill_frame(F, &fs.gbufArgs, fs.gbufInvView, fs.gbufInvProj);      // this rank's tile rows, plain order
    const uint64_t chunks = (uint64_t)F.ownedTileRows * (uint64_t)F.tilesX;
    if (chunks == 0) { g.aoSlot = g.gbufSlot; return CRT_OK; }      // this rank owns no row of the frame
    CrtAoArgs A; memset(&A, 0, sizeof A);
    A.geometry = reinterpret_cast<const float4*>(slot_gbuffer(fs).geometry());
    A.out = filter ? fs.aoRaw : fs.ao;
    const hipEvent_t frameDone = fs.gbufDone;
    float* raw = fs.aoRaw; float* plane = fs.ao; const float4* geometry = A.geometry;
    const int w = g.width, h = g.height;
    const float depthTol = params->filterDepthTol, normalCos = params->filterNormalCos;
    fs.aoPending = true;
    const int rc = launch_ao(true, A, F, *params, fs.gbufArgs.numMeshes, chunks, stream,
        [=](hipStream_t s) { HIPCHK(hipStreamWaitEvent(s, frameDone, 0)); return (int)CRT_OK; },
        [=](hipStream_t s) {
            if (!filter) return (int)CRT_OK;
            const unsigned tiles = (unsigned)(((w + CRT_TILE - 1) / CRT_TILE) * ((h + CRT_TILE - 1) / CRT_TILE));
            crt_ao_filter_kernel<<<tiles, CRT_BLOCK, 0, s>>>(raw, geometry, plane, w, h, depthTol, normalCos);
            HIPCHK(hipGetLastError());
            return (int)CRT_OK;
        });
    if (rc == CRT_OK) g.aoSlot = g.gbufSlot;
    return rc;
}

// The AO plane of the most recent crt_frame_ao (its slot keeps it until a resize or the shutdown)
static float* ao_plane() { return (g.aoSlot >= 0 && g.slot[g.aoSlot].ao) ? (float*)g.slot[g.aoSlot].ao : nullptr; }

int crt1_read_ao(float* dst, size_t floats)
{
    if (!g.initialized) return CRT_E_NOT_INITIALIZED;
    const float* src = ao_plane();
    if (!dst || !src || floats != (size_t)g.width * (size_t)g.height) return CRT_E_BAD_ARGUMENT;
    RCCHK(sync_all());                           // (waits for the query in flight)
    HIPCHK(hipMemcpy(dst, src, floats * sizeof(float), hipMemcpyDeviceToHost));
    return CRT_OK;
}

void* crt1_ao_device_ptr(void) { return g.initialized ? (void*)ao_plane() : nullptr; }

int crt1_debug_ao_stats(uint64_t out[3]) { return query_stats(&QueryContext::ao, out); }

} // namespace
