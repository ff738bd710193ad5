// crt_present.hip -- libcrt_present.so: crtp_present and crtp_view of include/crt_present.h (definition there), their kernels and the C ABI over
// them. The only translation unit of the library, written over the shared steps of the image libraries (../image/crt_image_device.h and
// crt_image_host.h: vector loads, the 32 x 8 tile and its halo, the two guide layouts, the hit predicate, the rules of the argument check) and
// over ../csrc/crt_post.h, the per-pixel stages of the frame -- post_pixel, quantize3, pack_rgba8, fxaa_pixel -- which libcrt_hip.so compiles
// from the same text: nothing of them is restated here. It shares no state; its one environment switch chooses where the FXAA form's taps come
// from (CRTP_TAPS=l1|lds). No kernel uses an atomic or reads what its own launch writes.
// Build: the Makefile's $(PRESENT_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include "../../include/crt_present.h"
#include "../image/crt_image_host.h"
#include "../image/crt_image_env.h"
#include "../csrc/crt_post.h"

#define CRTP_FLAGS_ALL (CRTP_UNORM8 | CRTP_POST | CRTP_FXAA | CRTP_HEAL)
// where the FXAA form's taps come from unless CRTP_TAPS says otherwise: 1 = the staged tile in LDS, 0 = color and ao again through L1
// (profiles/present_rate.txt: lds is 1.0-2.15 x faster than l1 over the FXAA forms, never slower)
#define CRTP_STAGED_DEFAULT 1
// the ABI of crt_present.h (clraytracer_amd/_lib.py mirrors it)
static_assert(sizeof(CrtpPresent) == 40 && offsetof(CrtpPresent, height) == 4 && offsetof(CrtpPresent, color) == 8 && offsetof(CrtpPresent, ao) == 16
              && offsetof(CrtpPresent, aoStrength) == 24 && offsetof(CrtpPresent, exposure) == 28 && offsetof(CrtpPresent, flags) == 32, "CrtpPresent");
static_assert(sizeof(CrtpView) == 64 && offsetof(CrtpView, height) == 4 && offsetof(CrtpView, guides) == 8 && offsetof(CrtpView, mode) == 12
              && offsetof(CrtpView, geometry) == 16 && offsetof(CrtpView, ids) == 24 && offsetof(CrtpView, albedo) == 32 && offsetof(CrtpView, plane) == 40
              && offsetof(CrtpView, scale) == 48 && offsetof(CrtpView, lo) == 52 && offsetof(CrtpView, hi) == 56 && sizeof(float4) == 16, "CrtpView");
static_assert(CRTP_OK == CRTI_OK && CRTP_E_BAD_ARGUMENT == CRTI_E_BAD_ARGUMENT && CRTP_E_OUT_OF_RANGE == CRTI_E_OUT_OF_RANGE && CRTP_GUIDES_PLANES == CRTI_GUIDES_PLANES
              && CRTP_GUIDES_SURFACE == CRTI_GUIDES_SURFACE, "the codes and layouts of crt_image_host.h");
static_assert(CRTI_BLOCK == 256 && CRTP_FLAGS_ALL == 15, "256-lane workgroups; four flags");

// ---- crtp_present ------------------------------------------------------------------------------------------------------------------------------
struct CrtpPresentLaunch {
    const float4* color;
    const float* ao;                // NULL: step 2 does not exist
    float4* outColor;               // may be NULL
    uint32_t* outBytes;             // may be NULL
    int width, height;
    float aoStrength, exposure;
    bool expose;                    // exposure != 1.0f: step 3 exists
};

// steps 1-4 at pixel k: the value the filter, PostProcess or the store sees. ao and expose are kernel-uniform
template <uint32_t FLAGS> __device__ __forceinline__ v3 crtp_source(const CrtpPresentLaunch& P, size_t k)
{
    const float4 p = crti_load4(P.color + k);
    v3 c = mk3(p.x, p.y, p.z);
    if (FLAGS & CRTP_HEAL) c = mk3(crti_finite(c.x) ? c.x : 0.0f, crti_finite(c.y) ? c.y : 0.0f, crti_finite(c.z) ? c.z : 0.0f);
    if (P.ao) {
        float f = (1.0f - P.aoStrength) + P.aoStrength * P.ao[k];
        if (FLAGS & CRTP_HEAL) f = crti_finite(f) ? f : 1.0f;
        c = scale3(c, f);
    }
    if (P.expose) c = scale3(c, P.exposure);
    if (FLAGS & CRTP_UNORM8) c = quantize3(c);
    return c;
}

// the image S of step 5 as fxaa_pixel takes it (csrc/crt_post.h: an overload of fxaa_fetch per image type; texel (i, j) lies in the frame) -- made
// again at every tap ...
template <uint32_t FLAGS> struct CrtpSourceTexels { const CrtpPresentLaunch& P; };
template <uint32_t FLAGS> __device__ __forceinline__ v3 fxaa_fetch(CrtpSourceTexels<FLAGS> src, int width, int i, int j)
{
    return crtp_source<FLAGS>(src.P, (size_t)(uint32_t)(j * width + i));
}
// ... or read from the workgroup's tile and halo in LDS, {S, 0} per texel. A tap lies in the halo (crt_present.h); whatever did not would
// read the tile's edge, never outside it
typedef CrtiTile<CRTP_FXAA_HALO> CrtpTile;
struct CrtpTileTexels {
    const crti_f4* tile;
    int x0, y0;                     // the frame position of the tile's texel (0, 0)
};
__device__ __forceinline__ v3 fxaa_fetch(CrtpTileTexels src, int width, int i, int j)
{
    const int tx = min(max(i - src.x0, 0), CrtpTile::TW - 1), ty = min(max(j - src.y0, 0), CrtpTile::TH - 1);
    const crti_f4 t = src.tile[ty * CrtpTile::TW + tx];
    return mk3(t.x, t.y, t.z);
}

// One lane per pixel of a 32 x 8 tile. STAGED (FXAA forms only): S over the tile and its halo goes through LDS once per workgroup
template <uint32_t FLAGS, bool STAGED>
__global__ __launch_bounds__(CRTI_BLOCK) void crtp_present_kernel(CrtpPresentLaunch P)
{
    const CrtiLane L;
    const int W = P.width, H = P.height;
    v3 c;
    if ((FLAGS & CRTP_FXAA) && STAGED) {
        __shared__ crti_f4 s_tile[CrtpTile::N];
#pragma unroll
        for (int j = 0; j < CrtpTile::ROUNDS; ++j) {
            const CrtpTile T(j, L.x0, L.y0);
            if (T.i < CrtpTile::N) {
                const v3 s = crtp_source<FLAGS>(P, T.clamped(W, H));
                crti_f4 r; r.x = s.x; r.y = s.y; r.z = s.z; r.w = 0.0f;
                s_tile[T.i] = r;
            }
        }
        __syncthreads();
        if (L.x >= W || L.y >= H) return;
        const CrtpTileTexels texels = { s_tile, L.x0 - CRTP_FXAA_HALO, L.y0 - CRTP_FXAA_HALO };
        c = fxaa_pixel(texels, W, H, L.x, L.y);
    } else {
        if (L.x >= W || L.y >= H) return;
        if (FLAGS & CRTP_FXAA) {
            const CrtpSourceTexels<FLAGS> texels = { P };
            c = fxaa_pixel(texels, W, H, L.x, L.y);
        } else
            c = crtp_source<FLAGS>(P, (size_t)(uint32_t)(L.y * W + L.x));
    }
    if (FLAGS & CRTP_POST) c = post_pixel(c, L.x, L.y, W, H);
    if ((FLAGS & CRTP_UNORM8) && (FLAGS & (CRTP_POST | CRTP_FXAA))) c = quantize3(c);
    const size_t k = (size_t)(uint32_t)(L.y * W + L.x);
    if (P.outColor) crti_store4(P.outColor + k, make_float4(c.x, c.y, c.z, 1.0f));
    if (P.outBytes) P.outBytes[k] = pack_rgba8(c);
}

// ---- crtp_view ---------------------------------------------------------------------------------------------------------------------------------
struct CrtpViewLaunch {
    const char* geometry;           // {n.x, n.y, n.z, t} at geometry + k * stride
    const char* instance;           // {int32 instance, uint32 triIndex} at instance + k * stride
    const char* albedo;             // uint32 at albedo + k * stride
    const void* plane;              // float[W*H] (SCALAR) or uint32[W*H] (STATE)
    float4* outColor;
    uint32_t* outBytes;
    int width, height;
    float scale, lo, hi;
};

__device__ __forceinline__ uint32_t crtp_hash(uint32_t h)
{
    h *= 0x9E3779B1u; h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ uint32_t crtp_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }
#define CRTP_MAGENTA crtp_rgb(255u, 0u, 255u)

// One lane per pixel: the mode's three bytes, then both outputs from them
template <int MODE, bool SURFACE>
__global__ __launch_bounds__(CRTI_BLOCK) void crtp_view_kernel(CrtpViewLaunch P)
{
    const CrtiLane L;
    if (L.x >= P.width || L.y >= P.height) return;
    const size_t k = (size_t)(uint32_t)(L.y * P.width + L.x);
    uint32_t w = 0u;
    if (MODE == CRTP_VIEW_NORMAL) {
        const float4 g = crti_geometry<SURFACE>(P, k);
        if (crti_hit(g.w)) w = crtp_rgb(unorm8(g.x * 0.5f + 0.5f), unorm8(g.y * 0.5f + 0.5f), unorm8(g.z * 0.5f + 0.5f));
    } else if (MODE == CRTP_VIEW_DEPTH) {
        const float t = crti_distance<SURFACE>(P, k);
        if (crti_hit(t)) { const uint32_t v = unorm8(P.scale / (t + P.scale)); w = crtp_rgb(v, v, v); }
    } else if (MODE == CRTP_VIEW_INSTANCE) {
        const int inst = crti_instance<SURFACE>(P, k);
        if (inst >= 0) w = crtp_hash((uint32_t)inst) & 0xFFFFFFu;
    } else if (MODE == CRTP_VIEW_TRIANGLE) {
        const int inst = crti_instance<SURFACE>(P, k);
        const uint32_t tri = *(const uint32_t*)(P.instance + k * (SURFACE ? 48 : 16) + 4);
        if (inst >= 0) w = crtp_hash((uint32_t)inst * 0x9E3779B1u + tri) & 0xFFFFFFu;
    } else if (MODE == CRTP_VIEW_ALBEDO) {
        w = crti_albedo<SURFACE>(P, k) & 0xFFFFFFu;
    } else if (MODE == CRTP_VIEW_SCALAR) {
        const float v = ((const float*)P.plane)[k];
        if (v != v) w = CRTP_MAGENTA;
        else { const uint32_t b = unorm8((v - P.lo) / (P.hi - P.lo)); w = crtp_rgb(b, b, b); }
    } else {
        const uint32_t s = ((const uint32_t*)P.plane)[k];
        w = s == 0u ? crtp_rgb(32u, 32u, 32u) : s == 1u ? crtp_rgb(255u, 160u, 0u) : s == 2u ? crtp_rgb(255u, 0u, 0u) : s == 3u ? crtp_rgb(0u, 200u, 80u) : CRTP_MAGENTA;
    }
    if (P.outColor) crti_store4(P.outColor + k, make_float4((float)(w & 255u) / 255.0f, (float)((w >> 8) & 255u) / 255.0f, (float)((w >> 16) & 255u) / 255.0f, 1.0f));
    if (P.outBytes) P.outBytes[k] = w | 0xFF000000u;
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------------------
static int crtp_check_size(int32_t width, int32_t height)
{
    if (width < 1 || height < 1) return CRTP_E_BAD_ARGUMENT;
    if (width > CRTI_MAX_DIM || height > CRTI_MAX_DIM) return CRTP_E_OUT_OF_RANGE;
    return CRTP_OK;
}

static int crtp_check_present(const CrtpPresent* p, const void* outColor, const void* outBytes)
{
    if (!p || !p->color || (!outColor && !outBytes)) return CRTP_E_BAD_ARGUMENT;
    if (p->flags & ~(uint32_t)CRTP_FLAGS_ALL) return CRTP_E_BAD_ARGUMENT;
    if (!isfinite(p->aoStrength) || !isfinite(p->exposure)) return CRTP_E_BAD_ARGUMENT;
    if (p->aoStrength < 0.0f || p->aoStrength > 1.0f || !(p->exposure > 0.0f)) return CRTP_E_BAD_ARGUMENT;
    const void* const ins[2] = {p->color, p->ao};
    const void* const outs[2] = {outColor, outBytes};
    if (crti_aliased(ins, outs)) return CRTP_E_BAD_ARGUMENT;
    return crtp_check_size(p->width, p->height);       // (no form needs scratch: crtp_scratch_bytes is 0 and scratch is not looked at)
}

static int crtp_check_view(const CrtpView* v, const void* outColor, const void* outBytes)
{
    if (!v || (!outColor && !outBytes)) return CRTP_E_BAD_ARGUMENT;
    if (v->mode < CRTP_VIEW_NORMAL || v->mode > CRTP_VIEW_STATE) return CRTP_E_BAD_ARGUMENT;
    const bool ids = v->mode == CRTP_VIEW_INSTANCE || v->mode == CRTP_VIEW_TRIANGLE, albedo = v->mode == CRTP_VIEW_ALBEDO;
    const bool plane = v->mode == CRTP_VIEW_SCALAR || v->mode == CRTP_VIEW_STATE;
    if (!crti_guides_ok(v->guides, ids, v->ids, albedo, v->albedo)) return CRTP_E_BAD_ARGUMENT;
    if (!plane && !v->geometry && (v->guides == CRTP_GUIDES_SURFACE || !(ids || albedo))) return CRTP_E_BAD_ARGUMENT;
    if (plane && !v->plane) return CRTP_E_BAD_ARGUMENT;
    if (v->mode == CRTP_VIEW_DEPTH && (!isfinite(v->scale) || !(v->scale > 0.0f))) return CRTP_E_BAD_ARGUMENT;
    if (v->mode == CRTP_VIEW_SCALAR && (!isfinite(v->lo) || !isfinite(v->hi) || !(v->lo < v->hi))) return CRTP_E_BAD_ARGUMENT;
    const void* const ins[4] = {v->geometry, v->ids, v->albedo, v->plane};
    const void* const outs[2] = {outColor, outBytes};
    if (crti_aliased(ins, outs)) return CRTP_E_BAD_ARGUMENT;
    return crtp_check_size(v->width, v->height);
}

static inline int crtp_launched()
{
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : CRTP_OK;
}

// where the FXAA form's taps come from: CRTP_TAPS=l1|lds in the environment (crt_image_env.h), else the built-in choice
static bool crtp_taps_lds() { return crti_env_choice("CRTP_TAPS", "l1", "lds", CRTP_STAGED_DEFAULT != 0); }

template <uint32_t FLAGS> static void crtp_launch_present(const CrtpPresentLaunch& P, bool staged, dim3 grid, hipStream_t s)
{
    if (staged) crtp_present_kernel<FLAGS, (FLAGS & CRTP_FXAA) != 0><<<grid, CRTI_BLOCK, 0, s>>>(P);      // (staged only under CRTP_FXAA)
    else crtp_present_kernel<FLAGS, false><<<grid, CRTI_BLOCK, 0, s>>>(P);
}

template <int MODE> static void crtp_launch_view(const CrtpViewLaunch& P, bool surface, dim3 grid, hipStream_t s)
{
    if (surface && MODE < CRTP_VIEW_SCALAR) crtp_view_kernel<MODE, (MODE < CRTP_VIEW_SCALAR)><<<grid, CRTI_BLOCK, 0, s>>>(P);
    else crtp_view_kernel<MODE, false><<<grid, CRTI_BLOCK, 0, s>>>(P);
}

extern "C" {

size_t crtp_scratch_bytes(int32_t width, int32_t height, uint32_t flags)
{
    (void)width; (void)height; (void)flags;
    return 0;       // every form is one launch that keeps what it stages in LDS
}

int crtp_present(const CrtpPresent* p, void* outColor, void* outBytes, void* scratch, void* stream)
{
    (void)scratch;
    const int rc = crtp_check_present(p, outColor, outBytes);
    if (rc != CRTP_OK) return rc;
    CrtpPresentLaunch P;
    P.color = (const float4*)p->color; P.ao = (const float*)p->ao; P.outColor = (float4*)outColor; P.outBytes = (uint32_t*)outBytes;
    P.width = p->width; P.height = p->height; P.aoStrength = p->aoStrength; P.exposure = p->exposure; P.expose = p->exposure != 1.0f;
    const dim3 grid = crti_grid(p->width, p->height);
    const hipStream_t s = (hipStream_t)stream;
    const bool staged = (p->flags & CRTP_FXAA) && crtp_taps_lds();
    switch (p->flags) {
#define CRTP_CASE(F) case F: crtp_launch_present<F>(P, staged, grid, s); break;
    CRTP_CASE(0) CRTP_CASE(1) CRTP_CASE(2) CRTP_CASE(3) CRTP_CASE(4) CRTP_CASE(5) CRTP_CASE(6) CRTP_CASE(7)
    CRTP_CASE(8) CRTP_CASE(9) CRTP_CASE(10) CRTP_CASE(11) CRTP_CASE(12) CRTP_CASE(13) CRTP_CASE(14) CRTP_CASE(15)
#undef CRTP_CASE
    }
    return crtp_launched();
}

int crtp_view(const CrtpView* v, void* outColor, void* outBytes, void* stream)
{
    const int rc = crtp_check_view(v, outColor, outBytes);
    if (rc != CRTP_OK) return rc;
    const bool surface = v->guides == CRTP_GUIDES_SURFACE;
    const char* g = (const char*)v->geometry;
    CrtpViewLaunch P;
    P.geometry = g; P.instance = surface ? g + 16 : (const char*)v->ids; P.albedo = surface ? g + 32 : (const char*)v->albedo;
    P.plane = v->plane; P.outColor = (float4*)outColor; P.outBytes = (uint32_t*)outBytes;
    P.width = v->width; P.height = v->height; P.scale = v->scale; P.lo = v->lo; P.hi = v->hi;
    const dim3 grid = crti_grid(v->width, v->height);
    const hipStream_t s = (hipStream_t)stream;
    switch (v->mode) {
    case CRTP_VIEW_NORMAL: crtp_launch_view<CRTP_VIEW_NORMAL>(P, surface, grid, s); break;
    case CRTP_VIEW_DEPTH: crtp_launch_view<CRTP_VIEW_DEPTH>(P, surface, grid, s); break;
    case CRTP_VIEW_INSTANCE: crtp_launch_view<CRTP_VIEW_INSTANCE>(P, surface, grid, s); break;
    case CRTP_VIEW_TRIANGLE: crtp_launch_view<CRTP_VIEW_TRIANGLE>(P, surface, grid, s); break;
    case CRTP_VIEW_ALBEDO: crtp_launch_view<CRTP_VIEW_ALBEDO>(P, surface, grid, s); break;
    case CRTP_VIEW_SCALAR: crtp_launch_view<CRTP_VIEW_SCALAR>(P, surface, grid, s); break;
    default: crtp_launch_view<CRTP_VIEW_STATE>(P, surface, grid, s); break;
    }
    return crtp_launched();
}

const char* crtp_error_string(int rc) { return CRTI_ERROR_STRING("crtp", rc); }

}
