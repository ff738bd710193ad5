/* crt_api.h -- C-ABI of the MI355X ray-trace path (libcrt_hip.so).
 *
 * This is the drop-in boundary: every entry point replaces one group of OpenCL call sites of the
 * reference's Renderer.cpp / ResourceManager.cpp (cited per function, paths relative to the
 * upstream tree CLRayTracer/...). Plain pointers and sizes only; buffers are passed in the
 * reference's own struct layouts (crt_types.h) and re-laid-out for CDNA4 on the device.
 *
 * Conventions
 *   - every function returns 0 on success, a positive hipError_t on a HIP failure, or a negative
 *     CRT_E_* code for argument/state errors; crt_error_string() explains either.
 *   - state is process-global and NOT thread-safe, like the reference's file-static state
 *     (Renderer.cpp:23-39, ResourceManager.cpp:49-90). One process drives one GPU.
 *   - host pointers only need to stay valid for the duration of the call (uploads are
 *     synchronous; the reference's CL_FALSE writes required the arenas to outlive the queue).
 *   - there is no CPU fallback: without a usable GPU crt_init fails and everything else returns
 *     CRT_E_NOT_INITIALIZED.
 */
#ifndef CRT_API_H
#define CRT_API_H

#include <stddef.h>
#include <stdint.h>
#include "crt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    CRT_OK = 0,
    CRT_E_NOT_INITIALIZED = -1,
    CRT_E_BAD_ARGUMENT    = -2,
    CRT_E_OUT_OF_RANGE    = -3,   /* upload beyond a fixed-size device pool; crt_pick_pixel outside the frame */
    CRT_E_NO_DEVICE       = -4,
    CRT_E_UNSUPPORTED     = -5
};

/* crt_render flags */
enum {
    CRT_RENDER_POSTPROCESS = 1,   /* also run PostProcess (kernel_main.cl:342-359) on the output */
    CRT_RENDER_WRITE_RAYS  = 2,   /* materialise the RayGen buffer (kernel_main.cl:277-287) in HBM */
    CRT_RENDER_ASYNC       = 4,   /* do not wait for completion (the reference always clFinish()es); see crt_render */
    CRT_RENDER_COUNTERS    = 8,   /* instrumented launch that fills the work counters (slower) */
    CRT_RENDER_STAMPS      = 16,  /* diagnostic launch: per-wave start/end clock stamps (crt_debug_read_stamps) */
    CRT_RENDER_SHADOWS     = 32,  /* extension (kernel_main.cl:256-258 is a TODO upstream): one any-hit shadow ray from the first
                                     hit towards the sun sets the `shadow` factor of kernel_main.cl:264; see DESIGN.md */
    CRT_RENDER_UNORM8      = 64,  /* hazard H8: upstream renders into an RGBA8-UNORM texture (Renderer.cpp:63,192): quantise the
                                     Trace result like write_imagef/read_imagef before PostProcess and the final frame after it */
    CRT_RENDER_READBACK    = 128, /* also copy the finished frame to pinned host memory behind its kernels (float4, or RGBA8 bytes
                                     with CRT_RENDER_UNORM8); fetch it with crt_map_host_frame. Overlaps with the other frames in flight */
    CRT_RENDER_REFRACTION  = 256, /* extension (upstream README TODO "refraction / transculency", no upstream code): at the first hit
                                     of a material whose MTL `d` (opacity, Material::roughness) is below 1 the bounce ray is the
                                     refracted ray (index 1.5) with (1 - opacity) of the energy; defined by the oracle, see DESIGN.md */
    CRT_RENDER_DIAG_MIX3   = 1024, /* diagnostic (profiling aid): ONE Trace dispatch that traces the frame three times, tile lists
                                     interleaved a third of the frame apart -- the wave mix of three frames in flight in a dispatch a
                                     PMC pass can see (rocprofv3 serialises dispatches, so real frames in flight cannot be profiled).
                                     Same pixels (every copy stores the same value). One device, synchronous, default kernel only */
    CRT_RENDER_FXAA        = 512  /* extension: upstream's FXAA function (kernel_main.cl:289-340) is dead code -- its call is commented out
                                     (kernel_main.cl:349), it returns nothing and would read pixels PostProcess is rewriting. Run it
                                     as the first PostProcess stage (or alone, without CRT_RENDER_POSTPROCESS), reading the unmodified
                                     Trace result; semantics defined by the oracle (orc_fxaa). Whole frames only: refused while
                                     crt_set_row_bands leaves this device a share of the rows (an in-process multi-GPU session
                                     gathers first and filters on its first device) */,
    CRT_RENDER_SSAA2       = 2048, /* extension: 2x2 ordered-grid supersampling. The frame is traced as the VIRTUAL frame 2W x 2H (its
                                     rays exactly those of a plain 2W x 2H frame with the same invView / invProj: subsample (sx, sy) of
                                     pixel (x, y) is virtual pixel (2x + sx, 2y + sy), so samples sit at x + s/2 like upstream's
                                     corner-sampled pixel and the image is shifted by 1/4 px against the 1-spp frame) and resolved in
                                     the Trace kernel: sums of horizontal then vertical pairs, times 1/4. The stages behind Trace
                                     (UNORM8, PostProcess, FXAA, read-back) see the resolved W x H frame. Counters count every subsample
                                     ray. With CRT_RENDER_SSAA4: CRT_E_BAD_ARGUMENT. Refused (CRT_E_UNSUPPORTED): with STAMPS, WRITE_RAYS
                                     or DIAG_MIX3, under a CRT_KERNEL form other than the default, above 7680 x 4320 virtual pixels */
    CRT_RENDER_SSAA4       = 4096, /* extension: the same with 4x4 subsamples (virtual frame 4W x 4H, shift 3/8 px; the pair sums are
                                     repeated: sx bit 0, sy bit 0, sx bit 1, sy bit 1, then times 1/16) */
    CRT_RENDER_GBUFFER     = 8192  /* extension: the Trace launch also writes the three first-hit planes below (CRT_GBUFFER_*), what the
                                     pixel's PRIMARY ray hit, for picking, denoisers and ID views: crt_read_gbuffer, crt_pick_pixel,
                                     crt_gbuffer_device_ptr. The colour frame is the same bits as without the flag; the planes do not
                                     depend on the other flags (with REFRACTION: the first hit, whichever ray continues). The planes
                                     belong to the frame slot (frames in flight keep their own; 36 B per pixel, allocated on the slot's
                                     first such frame); under crt_set_row_bands only this rank's rows are written. Refused
                                     (CRT_E_UNSUPPORTED): with SSAA2 / SSAA4, STAMPS, DIAG_MIX3 or COUNTERS, under a CRT_KERNEL form other
                                     than the default, in a session of several devices */
};

/* The planes of a CRT_RENDER_GBUFFER frame: W x H elements each, row-major like the frame. The world-space hit point is
 * cameraPos + t * rayDir (t is the same parameter in instance space and in world space).
 *   GEOMETRY  float[4]: record.normal of kernel_main.cl:236 (x, y, z), then t.                 Miss: 0, 0, 0, 99999.0f
 *   IDS       { int32 instance; uint32 triIndex; float u; float v; }: what crt_query_hits
 *             returns for the pixel's ray.                                                     Miss: -1, 0, 0.0f, 0.0f
 *   ALBEDO    uint32: 0xFF000000 | b << 16 | g << 8 | r, the bytes of MultiplyColorU32(pixel,
 *             material.color) (kernel_main.cl:245) before the / 255.                           Miss: 0
 * A hit beyond upstream's InfMinusOne (t > 99998, shaded as sky, kernel_main.cl:219) keeps its ids and t but has the normal and
 * albedo of a miss. */
enum { CRT_GBUFFER_GEOMETRY = 0, CRT_GBUFFER_IDS = 1, CRT_GBUFFER_ALBEDO = 2 };

/* Device work counters of the last CRT_RENDER_COUNTERS / crt_query_hits launch. Same meaning as
 * the oracle's OrcStats so tests can require exact equality. */
typedef struct CrtCounters {
    uint64_t rays, primary, secondary, hits, misses;
    uint64_t traversals, pops, innerVisits, triTests, capHits, stackOverflows, maxStack;
    uint64_t shadowRays, shadowHits;   /* CRT_RENDER_SHADOWS: shadow rays traced (also in `rays`) / found occluded */
} CrtCounters;

/* Renderer.cpp:122-193 (InitializeOpenCL + buffer creation) and ResourceManager.cpp:145-178
 * (device pools, default white/black texels). `device` is the HIP ordinal this process owns.
 * Allocates every pool at its reference capacity once; nothing is resized later except by
 * crt_resize. */
int crt_init(int device, int width, int height);
/* Several GPUs of one node behind the same entry points (no reference counterpart: Renderer.cpp:134 asks
 * clGetDeviceIDs for ONE device). The scene is replicated by every upload; the frame is cut into 16-row
 * bands dealt round-robin to the devices; every device traces its bands on its own streams and copies them into the first
 * device's frame (peer copies over xGMI, no collective, no host staging). crt_render keeps its meaning -- without
 * CRT_RENDER_ASYNC it returns when the WHOLE frame is complete -- and crt_read_output / crt_map_host_frame /
 * crt_output_device_ptr deliver the whole frame from the first device. Counters are summed over the devices.
 * Not available in such a session: crt_set_row_bands (the bands are the library's), CRT_RENDER_WRITE_RAYS, CRT_RENDER_STAMPS.
 * `devices` may name the same GPU more than once (functional rehearsal of the multi-device path on a one-GPU box). */
int crt_init_devices(const int* devices, int numDevices, int width, int height);
int crt_init_gpus(int numGpus, int width, int height);        /* devices 0 .. numGpus-1 */
int crt_num_devices(void);                                    /* 0 = no session */
/* How device `device` of the session (0 = the primary) delivers its bands into the primary's frame: 2 = it is the same
 * physical GPU as the primary (a rehearsal session), 1 = peer mapping enabled (hipDeviceEnablePeerAccess: xGMI), 0 = no peer
 * access -- the HIP runtime stages every gather copy through host memory (correct, slow; crt_init_devices says so once on
 * stderr). crt_gather_path() names the slowest path any device of the session uses: "xgmi-peer", "host-staged", ... */
int crt_peer_access(int device);
const char* crt_gather_path(void);
/* Renderer.cpp:377-394, ResourceManager.cpp:303-319 */
int crt_shutdown(void);
/* Renderer.cpp:198-211: ignores sizes below 16 like the reference (returns CRT_OK, no change). */
int crt_resize(int width, int height);
/* Multi-GPU image tiling (no reference counterpart: upstream is single-device). The frame is cut
 * into horizontal bands of `bandRows` rows (a multiple of 8, the tile height); this process renders bands
 * rank, rank+nRanks, ... RayGen and Vignette still use full-frame coordinates. Default (16,0,1). */
int crt_set_row_bands(int bandRows, int rank, int nRanks);
/* Which rank renders frame row `row` under that tiling (pure function, needs no device). */
int crt_row_owner(int row, int bandRows, int nRanks);
/* The rows a rank owns as the block list its gather / read-back copies use (pure function): out = { firstRow, fullBands,
 * tailRow, tailRows }: `fullBands` bands of bandRows rows from firstRow, every bandRows * nRanks rows, then tailRows rows
 * of a last partial band at tailRow. */
int crt_band_plan(int height, int bandRows, int rank, int nRanks, int out[4]);

/* ResourceManager.cpp:286 -- triangles in the 80-byte reference layout, offsets in bytes. */
int crt_upload_triangles(const void* tris, size_t byteOffset, size_t bytes);
/* ResourceManager.cpp:293 -- BVH nodes (32 B each), offsets in bytes, indices as built on the host.
 * Trees from BuildBVH / crt_build_bvh bound their triangles; uploaded nodes need not (leaf triangles are tested without a box test,
 * kernel_main.cl:135-140). The instance cull stays exact either way: the range of bounce-ray origins it is proven for is taken from the
 * uploaded triangles' extents as well as from the root boxes (crt_get_cull_range: bounceReach). */
int crt_upload_bvh_nodes(const void* nodes, size_t byteOffset, size_t bytes);
/* ResourceManager.cpp:291 -- per-mesh root node indices (uint32). */
int crt_upload_bvh_roots(const uint32_t* roots, size_t firstMesh, size_t count);
/* ResourceManager.cpp:142,295 */
int crt_upload_materials(const void* materials, size_t first, size_t count);
/* ResourceManager.cpp:236 */
int crt_upload_texture_table(const void* textures, size_t count);
/* ResourceManager.cpp:177,203 -- packed RGB8 bytes at a byte offset into the texel pool. Any offset and length: the span need not begin or
 * end on a texel; every texel it touches whose three bytes have been uploaded (now or earlier) shows its new bytes in the next frame. */
int crt_upload_texels(const void* rgb8, size_t byteOffset, size_t bytes);
/* Renderer.cpp:245,314. Host-side only: the instance table is versioned, frames already submitted keep the version they were
 * submitted with and every later frame refreshes its slot's device copy on its own stream -- no waiting for frames in flight. */
int crt_upload_instances(const void* instances, size_t first, size_t count);

/* BuildBVH (BVH.cpp:218-255; called from ResourceManager.cpp:282) on the device, for triangles already uploaded with
 * crt_upload_triangles: `numMeshes` meshes of meshTriCounts[m] triangles each, stored back to back from triangle
 * `firstTri`. Writes the triangle centroids, reorders the triangles, writes the nodes from node index `firstNode` and
 * the roots of meshes firstMesh.. -- byte for byte what the host BuildBVH produces for the same input (triangle
 * order, node numbering by the recursion's allocation order, bounds) -- and re-lays everything out for rendering.
 * *nodesUsedOut = number of nodes written. The crt_download_* calls read the reference-layout pools back. */
int crt_build_bvh(size_t firstTri, const uint32_t* meshTriCounts, int numMeshes, size_t firstNode, size_t firstMesh, uint32_t* nodesUsedOut);
int crt_download_triangles(void* dst, size_t byteOffset, size_t bytes);
int crt_download_bvh_nodes(void* dst, size_t byteOffset, size_t bytes);
int crt_download_bvh_roots(uint32_t* dst, size_t firstMesh, size_t count);

/* Renderer.cpp:337-367: RayGen + Trace (+ PostProcess) for one frame, then (unless ASYNC) wait.
 * invView / invProj are the camera's inverse matrices, row-major (hazard H10: taken as inputs).
 * Frames in flight (no reference counterpart): consecutive CRT_RENDER_ASYNC frames rotate over three frame
 * slots (CRT_FRAMES_IN_FLIGHT=1..8 in the environment, default 3; every slot's stream wants a hardware queue of its own, so
 * crt_init / crt_init_devices / crt_init_gpus set GPU_MAX_HW_QUEUES=8 before their first HIP call unless it is set -- effective only if
 * nothing in the process has started the HIP runtime before; otherwise export it yourself), each with its own HIP stream, output buffer and
 * launch lists, so frames run concurrently and the long-ray tail of one is hidden behind the others; the call
 * blocks only to keep at most two frames queued per slot. Mesh / texture / material uploads, resize, queries and reads
 * wait for every frame in flight first; instance uploads do not need to (see crt_upload_instances). Either way scene
 * edits between frames stay ordered. crt_read_output* and crt_output_device_ptr refer
 * to the most recently submitted frame. */
int crt_render(const CrtTraceArgs* args, const float invView[16], const float invProj[16], int flags);
int crt_sync(void);                                           /* wait for every frame in flight */

/* Closest-hit query for arbitrary world-space rays (host pointers, n rays) against the first
 * `numInstances` instances: the instance loop + IntersectBVH of kernel_main.cl:198-217 exposed for
 * hit-record parity tests. Also fills the work counters. (The counted route over host memory; rays on the device: crt_trace_rays.) */
int crt_query_hits(const float* origins, const float* dirs, int n, uint32_t numInstances, CrtRayHit* out);

/* Ray queries on device buffers (no reference counterpart: upstream's only rays are the camera's): closest hit or occlusion for a
 * batch of world-space rays that is already on the device, answered on the device -- visibility between points, light-map and
 * ambient-occlusion baking, range sensors, collision probes. The instance loop + IntersectBVH of kernel_main.cl:124-160, 189-217 with
 * its own kernel (CRT_KERNEL forms do not apply, as for crt_query_hits), against the first `numInstances` instances.
 *   rays    CrtRayBatch (crt_types.h): origins / dirs / tmax are device-accessible; strides in floats, 0 = one value for every ray,
 *           otherwise >= 3. Directions are not normalised: t and tmax are in units of the given direction's length (hazard H6).
 *   out     device-accessible: CrtRayHit[n] (20 B each) for CRT_RAYS_CLOSEST, uint8_t[n] (0 or 1) for CRT_RAYS_OCCLUDED.
 *   stream  a hipStream_t; NULL = HIP's null stream (what torch.cuda.current_stream().cuda_stream is for torch's default stream).
 * Semantics, one definition for both modes: upstream's loop started with a smaller "closest so far". The bound is
 * B = !(tmax >= 99999.0f) ? tmax : 99999.0f (no tmax array: 99999.0f); besthit.distance starts at B instead of 99999, nothing else
 * changes. A NaN tmax stays NaN and makes the ray a miss through the loop's own comparisons (t < out.t, tnear < minSoFar).
 *   CRT_RAYS_CLOSEST   a hit record is exactly crt_query_hits' CrtRayHit {t, u, v, triIndex, instance}; a miss is always
 *                      {99999.0f, 0, 0, 0, -1}, whatever B was.
 *   CRT_RAYS_OCCLUDED  1 where the bounded closest-hit query of the same ray reports a hit, else 0 -- exactly, not approximately: the
 *                      any-hit traversal (as shadow rays use it) and the bounded closest-hit traversal are in identical states until
 *                      the first triangle passes, and the any-hit traversal stops there.
 * What is promised: equality with that bounded loop, always; and equality with "the unbounded record (crt_query_hits) if its
 * t < tmax, else the miss record" whenever the unbounded record's u and v are finite. (The bound may prune a subtree whose degenerate
 * triangle would have left a NaN u / v in the unbounded loop's arithmetic blend, kernel_main.cl:101-104.)
 * The call ENQUEUES AND RETURNS: no ray is read on the host, results are valid once `stream` reaches this point. The host waits only
 * for the first query's allocations and for an overflow area that has to grow. Queries have a context of their own (instance tables,
 * overflow area): they neither wait for the frames in flight nor delay them; one query runs at a time -- a query's stream waits, on
 * the device, for the query before it. Whatever waits for the frames in flight also waits, on the host, for the query in flight -- and
 * so for everything the caller queued ahead of it on `stream`: scene edits (mesh / node / root / material / texture uploads,
 * crt_build_bvh, crt_resize, crt_set_row_bands, crt_shutdown, crt_sync), the reads (crt_read_output*, crt_read_rays, crt_read_gbuffer,
 * crt_pick_pixel, crt_download_*), crt_query_hits, and every frame that is not pipelined (a crt_render without CRT_RENDER_ASYNC, or
 * with a diagnostic flag). Pipelined frames do not wait. crt_upload_instances waits for nothing, and a query submitted after it sees
 * the new table. A ray origin beyond the cull's proven range (crt_get_cull_range) costs only its own 64-ray chunk the instance cull.
 * Work counters, crt_get_counters and noCullFrames are not touched. n == 0: CRT_OK, no pointer is looked at. Errors, all before
 * anything is enqueued: CRT_E_NOT_INITIALIZED; CRT_E_BAD_ARGUMENT (rays, origins, dirs or out NULL; a stride of 1 or 2; an unknown
 * mode; numInstances > 401; an invalid scene); CRT_E_OUT_OF_RANGE (n > 2^30); CRT_E_UNSUPPORTED (a session of several devices: the
 * pointers belong to one GPU). CRT_RAYS_GRID=n in the environment (read by crt_init) caps the launch at n workgroups.
 *
 * CRT_RAYS_INCLUSIVE (OR-ed into `mode`; the valid modes are 0, 1, 0x100, 0x101) -- the inclusive box test, for rays that start ON a
 * surface: shadow and visibility rays, ambient-occlusion samples, bounce rays. Upstream's IntersectAABB never enters a box the ray starts
 * in (tnear > 0, hazard H1) nor one of zero thickness (tnear < tfar), so such a ray sees a fraction of the scene, the mesh it starts on
 * least of all. With the flag the box test, in float32 without contraction, is: tnear and tfar as upstream computes them;
 * entry = fmaxf(tnear, 0.0f); the box passes iff tnear <= tfar && tfar >= 0.0f && entry < minSoFar; the function returns entry on a
 * pass and 1e30f otherwise. Nothing else changes: near child first by the returned distance (swap iff dist1 > dist2, so two boxes that
 * both hold the origin keep left-first order), the 32-slot stack with its modulo wrap, the 250-pop cap per instance (kept: it bounds every
 * traversal, so no input can make a kernel run on), IntersectTriangle with its arithmetic blend, the instance loop in ascending order,
 * the bound B (a NaN bound included), the miss record, and CRT_RAYS_OCCLUDED = the anyHit of the bounded closest-hit query under the
 * same rule, exactly. The instance cull stays on (it is proven for this rule too). Without the flag every call is what it was; frames,
 * crt_query_hits and the counters never use the rule. crt_debug_rays_stats counts inclusive launches as any other. */
enum { CRT_RAYS_CLOSEST = 0, CRT_RAYS_OCCLUDED = 1, CRT_RAYS_INCLUSIVE = 0x100 };
int crt_trace_rays(const CrtRayBatch* rays, uint32_t numInstances, int mode, void* out, void* stream);

/* Ambient occlusion (no reference counterpart: upstream's ambient term is the flat max(-ndl, 0.1) * atmosphere of kernel_main.cl:262), for
 * points on the device (crt_trace_ao) and for the pixels of the most recently submitted CRT_RENDER_GBUFFER frame (crt_frame_ao). One fused
 * kernel generates the sample rays in registers, traces them with the any-hit traversal of crt_trace_rays(CRT_RAYS_OCCLUDED) and reduces per
 * item: no ray is materialised. Every value is defined in float32 arithmetic without contraction; dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *
 * Direction table  T[256], unit vectors, spherical Fibonacci in index order: in double precision z_i = 1 - (2i + 1) / 256,
 *   phi_i = i * pi * (3 - sqrt 5), T_i = (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z), rounded to float32 once by tools/make_ao_table.py
 *   (committed as literals: csrc/crt_ao_table.h). crt_ao_directions copies the 256 xyz triples out: a pure function, needs no device.
 * Per item k (the point's index; y * W + x for a pixel) with position P, normal n and CrtAoParams {samples = N, radius = R, bias, seed}:
 *   1. h = lowbias32(k ^ (seed * 0x9E3779B9u)); lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (uint32).
 *   2. o = P + n * bias (a multiply, then an add, per component): the origin of every sample ray.
 *   3. for s = 0 .. N-1: j = (h + s * (256 / N)) & 255; d = T[j] with x, y, z negated where bits 8, 9, 10 of h are set, then all of d negated
 *      if dot3(d, n) < 0; w = dot3(d, n) of the final d; occ = exactly what crt_trace_rays(CRT_RAYS_OCCLUDED) answers for the ray
 *      (o, d, tmax = R) -- the same bound rule B, the same any-hit form -- as 1.0f or 0.0f; num += w * occ; den += w, in this order.
 *   4. ao = den > 0 ? 1 - num / den : 1.            1 = open, 0 = every weighted sample occluded.
 *   5. an item whose normal is exactly (0, 0, 0) traces nothing and gets 1.0f. NaNs get what these expressions give.
 * Frame form: dir = the pixel's RayGen direction (kernel_main.cl:277-287) from the matrices of that G-buffer frame, t and the normal from its
 *   GEOMETRY plane: P = cameraPos + dir * t, n = the plane's normal turned towards the viewer (dot3(n, dir) > 0 ? -n : n). A miss pixel
 *   (t > 99998: a miss carries t = 99999 and a zero normal) gets 1.0f.
 * CRT_AO_FILTER (frame form only): a second small kernel writes the AO plane from the raw one -- for a hit centre pixel c the 5 x 5 window
 *   clipped to the frame, dy = -2..2 outside, dx = -2..2 inside: m = 1 for the centre; m = 1 for a hit neighbour with
 *   fabsf(t_n - t_c) <= filterDepthTol * t_c and dot3(n_n, n_c) >= filterNormalCos (the plane's normals as stored); else m = 0;
 *   sum += ao * m; cnt += m; the result is sum / cnt. Miss pixels stay 1.0f. Refused (CRT_E_UNSUPPORTED) while crt_set_row_bands leaves this
 *   rank a share of the rows: the window crosses band edges.
 *
 * crt_trace_ao follows crt_trace_rays in every respect: it ENQUEUES AND RETURNS on the caller's stream, in the ray queries' context -- one
 * query at a time (the stream waits, on the device, for the query before, of either kind), instance tables refreshed behind the query
 * before, an overflow area owned per workgroup, CRT_RAYS_GRID caps the persistent grid; whatever waits for the ray query in flight also waits
 * for an AO query. positions / normals / out (n floats) are device-accessible; strides in floats, 0 = one value for every point. A ray origin
 * beyond the cull's proven range costs only its 64-point chunk (8 x 8 tile) the instance cull. The colour frame, the G-buffer planes, the work
 * counters and noCullFrames are not touched. n == 0: CRT_OK, no pointer is looked at. Errors, all before anything is enqueued:
 * CRT_E_NOT_INITIALIZED; CRT_E_BAD_ARGUMENT (points or params NULL; samples not one of 1, 2, 4, 8, 16, 32, 64; !(radius > 0), so a NaN too;
 * a bias that is not finite; an unknown flag, CRT_AO_FILTER on the points form; positions, normals or out NULL; a stride of 1 or 2;
 * numInstances > 401; an invalid scene); CRT_E_OUT_OF_RANGE (n > 2^30); CRT_E_UNSUPPORTED (a session of several devices).
 * crt_frame_ao: the same context and ordering, against the instances that frame was rendered with (as last uploaded). In addition the caller's
 * stream waits, on the device, for the G-buffer frame it reads, and a later G-buffer frame into the same frame slot waits, on the device, for
 * the AO query: pipelined frames get no host wait. The AO plane -- float, W x H, row-major -- belongs to the frame slot and is allocated by the
 * slot's first crt_frame_ao (the one host wait); under crt_set_row_bands only this rank's rows are written. CRT_E_BAD_ARGUMENT when no
 * G-buffer frame has been submitted since crt_init or the last crt_resize that changed the frame (when crt_read_gbuffer refuses).
 * crt_read_ao (floats = width * height, after waiting for the frames and the query in flight) and crt_ao_device_ptr refer to the most recent
 * crt_frame_ao and refuse (CRT_E_BAD_ARGUMENT / NULL) when there is none since crt_init or such a crt_resize.
 * CRT_AO_INCLUSIVE (both forms; combines with CRT_AO_FILTER on the frame form): occ = what crt_trace_rays(CRT_RAYS_OCCLUDED |
 * CRT_RAYS_INCLUSIVE) answers for the sample ray -- the inclusive box test defined there, under which a point sees the mesh it lies on.
 * Everything else in the definition above is unchanged. */
enum { CRT_AO_FILTER = 1, CRT_AO_INCLUSIVE = 4 };
int crt_ao_directions(float out[768]);
int crt_trace_ao(const CrtAoPoints* points, const CrtAoParams* params, uint32_t numInstances, float* out, void* stream);
int crt_frame_ao(const CrtAoParams* params, void* stream);
int crt_read_ao(float* dst, size_t floats);                   /* width*height */
void* crt_ao_device_ptr(void);

/* Shaded ray queries on device buffers (no reference counterpart: upstream shades the camera's rays only): what a frame computes for a
 * pixel, for any ray that is already on the device -- a fisheye or panoramic camera, a cube-map probe, a stereo pair, a range sensor that
 * wants intensity, a light-map texel, the next bounce of a path tracer written by the caller. Against the first `numInstances` instances.
 *   rays      CrtRayBatch as crt_trace_rays takes it. Ray k is (o, d) of the batch; d is not normalised (hazard H6).
 *   params    CrtShadeParams {sunAngle, flags = 0}: lightDir = (0, (float)sin((double)sunAngle), (float)cos((double)sunAngle)), computed
 *             on the host as a frame's is from CrtTraceArgs::sunAngle.
 *   radiance  device-accessible float4[n], or NULL: radiance[k] = (result, 1.0f).
 *   surface   device-accessible CrtSurfaceHit[n] (48 B each, crt_types.h), or NULL. Not both NULL; with radiance == NULL only the first
 *             traversal runs.
 * Definition, one for every ray, float32 without contraction: kernel_main.cl:187-272 exactly as a frame without flags runs it for a pixel
 * whose ray is (o, d) -- energy (1, 1, 1), atmosphericLight (0.255, 0.25, 0.27), two bounces: the instance loop + IntersectBVH
 * (kernel_main.cl:189-217), the sky for a ray that found nothing or something beyond InfMinusOne (kernel_main.cl:219-223), else the
 * material (kernel_main.cl:229), the interpolated normal and uv (kernel_main.cl:232-240), the albedo texel times the material's colour
 * (kernel_main.cl:242-245), the reflected ray 0.01 off the surface (kernel_main.cl:252-254), ambient, diffuse and specular terms
 * (kernel_main.cl:260-268) and, after the first bounce, lightDir = the bounce ray's direction and atmosphericLight * 0.4
 * (kernel_main.cl:269-271). None of the extensions (shadow rays, refraction, supersampling) and none of the stages behind Trace (the RGBA8
 * target, PostProcess, FXAA): they belong to pixels.
 * The bound: B = the bound of crt_trace_rays, !(tmax[k] >= 99999.0f) ? tmax[k] : 99999.0f (no tmax array: 99999.0f), for the given ray
 * only -- besthit.distance starts at B; the bounce ray is unbounded. A ray without a hit inside the bound (a NaN bound: every ray) is a
 * miss: it ends in the sky as kernel_main.cl:219-223 does and gets the miss record.
 * The surface record describes what the given ray found. Its first 36 bytes are CrtGBufferPixel -- exactly the three G-buffer planes'
 * values for a pixel with that ray: hit: record.normal, t, instance, triIndex, u, v, albedo = 0xFF000000 | b << 16 | g << 8 | r of
 * record.color. material = min(materialStart + triangle.materialIndex, 255), the index the material was read at; texU, texV = the
 * interpolated uv before SampleTexture's fract. A miss: normal 0, t = 99999, instance -1, everything else 0. A hit beyond InfMinusOne
 * (t > 99998, shaded as sky) keeps instance, triIndex, u, v and t and has the normal, albedo, material and uv of a miss.
 * What is promised: for the rays of a frame -- origins = cameraPos with stride 0, dirs = what crt_read_rays returns for that frame --
 * radiance is, bit for bit, crt_read_output of the frame rendered with flags = 0 and surface the three planes of crt_read_gbuffer of the
 * CRT_RENDER_GBUFFER frame; for any rays, the CPU oracle's trace of them.
 * Everything else is crt_trace_rays, word for word: the call ENQUEUES AND RETURNS on the caller's stream, in the ray queries' context --
 * one query at a time, of any kind; instance tables refreshed behind the query before; a persistent grid (CRT_RAYS_GRID) with an
 * overflow area per workgroup; the cull decided per 64-ray chunk on the given origins (a chunk without it keeps its scene for its bounce
 * rays); frames in flight neither waited for nor delayed; whatever waits for a ray query waits for this one; work counters,
 * crt_get_counters and noCullFrames untouched; n == 0: CRT_OK. While a query runs, radiance[k] also holds ray k's unfinished path.
 * Errors, all before anything is enqueued: CRT_E_NOT_INITIALIZED; CRT_E_BAD_ARGUMENT (rays, params, origins or dirs NULL; both outputs
 * NULL; a stride of 1 or 2; a sunAngle that is not finite; flags other than 0; numInstances > 401; an invalid scene); CRT_E_OUT_OF_RANGE
 * (n > 2^30); CRT_E_UNSUPPORTED (a session of several devices). */
int crt_shade_rays(const CrtRayBatch* rays, const CrtShadeParams* params, uint32_t numInstances, float* radiance, CrtSurfaceHit* surface, void* stream);

/* Output: the HDR float4 frame (the reference writes a CL-GL RGBA8 texture, Renderer.cpp:63,192). */
int crt_read_output(float* dstRGBA, size_t floats);           /* full frame, width*height*4 floats */
int crt_read_output_rows(float* dstRGBA, int row0, int rows); /* rows [row0,row0+rows) */
int crt_read_output_rgba8(uint8_t* dstRGBA, size_t bytes);    /* the frame as RGBA8 (convert_uchar_sat_rte(x*255)), width*height*4 bytes */
/* Host copy of the most recent CRT_RENDER_READBACK frame: waits for that copy only; the pointer (pinned memory owned by
 * the library) stays valid until as many further READBACK frames as there are frame slots have been submitted. */
int crt_map_host_frame(const void** ptr, size_t* bytes);
/* The same for the READBACK frame submitted `framesBack` READBACK frames earlier (0 = the latest), while its slot has not
 * been reused: lets a consumer work on frame k-1 while frame k renders. */
int crt_map_host_frame_back(int framesBack, const void** ptr, size_t* bytes);
int crt_read_rays(float* dst, size_t floats);                 /* width*height*3, after WRITE_RAYS */
/* The frame on the device. The library orders nothing against work of the caller's that reads this buffer or a crt_gbuffer_device_ptr
 * plane on a stream of the caller's (crtd_denoise, crtt_accumulate, crtv_filter, a kernel of its own): order that stream -- wait for it,
 * or for an event recorded behind the reader -- before the next crt_render that reuses the frame slot (a synchronous frame always reuses
 * slot 0), and before crt_resize and crt_shutdown, which free it. */
void* crt_output_device_ptr(void);
/* The first-hit planes of the most recently submitted CRT_RENDER_GBUFFER frame (later frames without the flag leave them alone).
 * crt_read_gbuffer copies a whole plane (bytes = width * height * 16, or * 4 for CRT_GBUFFER_ALBEDO) after waiting for the frames in
 * flight; CRT_E_BAD_ARGUMENT for an unknown plane, a wrong size, or when no such frame has been submitted since crt_init or the last
 * crt_resize that changed the frame. crt_gbuffer_device_ptr: the plane on the device, NULL under the same conditions;
 * a caller that reads it on a stream of its own orders that stream before the next crt_render that reuses the slot (crt_output_device_ptr).
 * crt_pick_pixel: one pixel of all three planes (36 bytes travel, not a frame) -- the GPU's answer to upstream's mouse pick
 * CPU_RayCast(camera.ScreenPointToRaySSE(mouse)) (Engine.cpp:112-126); CRT_E_OUT_OF_RANGE outside the frame. */
int crt_read_gbuffer(int plane, void* dst, size_t bytes);
void* crt_gbuffer_device_ptr(int plane);
int crt_pick_pixel(int x, int y, CrtGBufferPixel* out);
int crt_owned_rows(void);                                     /* rows this rank renders per frame */

/* Timing of the last crt_render measured with HIP events on the launch stream.
 * which: 0 = whole frame, 1 = RayGen (only with WRITE_RAYS), 2 = Trace, 3 = PostProcess (and the RGBA8 stores, FXAA) --
 * close to zero for the default kernel, which applies PostProcess and the RGBA8 target to the pixel in its registers
 * before storing it; the stages run as launches of their own behind FXAA and the opt-in kernel variants. */
float crt_last_kernel_ms(int which);
/* Event timing accumulated over every frame since the last reset. Read back lazily per frame slot, so this does
 * not serialise ASYNC frames the way asking crt_last_kernel_ms after each frame would. With frames in flight the
 * per-frame durations overlap: sumMs[2] / frames is the mean duration of one Trace launch (what a kernel trace
 * shows), extentMs / frames the device time the frames took per frame. */
typedef struct CrtFrameStats {
    uint64_t frames;
    double sumMs[4];      /* same four intervals as crt_last_kernel_ms */
    double extentMs;      /* start of the first frame -> end of the last one to finish */
    double firstFrameMs;  /* start -> end of the first frame since the reset: the pipeline's fill time. (extentMs - firstFrameMs) /
                             (frames - 1) is the steady-state device time per frame, independent of how many frames were timed */
} CrtFrameStats;
int crt_frame_time_stats(CrtFrameStats* out, int reset);
int crt_get_counters(CrtCounters* out);
/* Of the last counted launch's `traversals` (= pops = root visits, one per ray and instance as upstream spends them,
 * kernel_main.cl:198-217), how many the conservative instance cull answered without fetching anything: the device's
 * real child-pair fetches are innerVisits - this. (Measurement aid for bench.py's gather-rate figure.) */
int crt_get_culled_visits(uint64_t* out);
/* The range of ray origins for which the instance cull is provably exact (derivation: csrc/crt_device.h above sphere_culls):
 * limits[i] (i < n <= 401) = the largest |origin| instance i may be culled for, 0 = never culled; *sceneLimit = the smallest over
 * the cullable instances -- a crt_render whose camera, or a crt_query_hits whose farthest origin, lies beyond it runs without the
 * cull (same results, every instance entered as upstream does, kernel_main.cl:198); *bounceReach = how far out bounce-ray origins
 * can lie (object-space hit points, hazard H6); *noCullFrames = launches that ran without the cull so far. Any pointer may be NULL. */
int crt_get_cull_range(float* limits, int n, float* sceneLimit, float* bounceReach, uint64_t* noCullFrames);
const char* crt_error_string(int code);
const char* crt_device_name(void);

#ifdef __cplusplus
}
#endif
#endif
