// crt_upsample.hip -- libcrt_upsample.so: the guided upsample of include/crt_upsample.h (definition there), its kernel and the C ABI over it. The
// only translation unit of the library, and the first written over the shared steps of the image libraries instead of beside them: vector loads,
// guide layouts, predicates, a lane's place in the 32 x 8 tile; the grid, the rules of the argument check, the error strings; the two-word switch's
// parser -- all from ../image/crt_image_device.h, crt_image_host.h and crt_image_env.h. It shares no state.
// Build: the Makefile's $(UPSAMPLE_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include "../../include/crt_upsample.h"
#include "../image/crt_image_host.h"
#include "../image/crt_image_env.h"

// DESIGN.md 4q, what was measured at both factors and under both guide layouts: with CRTU_MATCH_INSTANCE (a second gathered word per tap) the taps
// from LDS are faster, without it the taps through L1 are (or tie)
#define CRTU_STAGED_DEFAULT(match) ((match) ? 1 : 0)
// the ABI of crt_upsample.h (clraytracer_amd/_lib.py mirrors it)
static_assert(sizeof(CrtuFrame) == 40 && offsetof(CrtuFrame, height) == 4 && offsetof(CrtuFrame, guides) == 8 && offsetof(CrtuFrame, geometry) == 16
              && offsetof(CrtuFrame, ids) == 24 && offsetof(CrtuFrame, albedo) == 32, "CrtuFrame");
static_assert(sizeof(CrtuLow) == 24 && offsetof(CrtuLow, channels) == 8 && offsetof(CrtuLow, factor) == 12 && offsetof(CrtuLow, offsetX) == 16
              && offsetof(CrtuLow, offsetY) == 20, "CrtuLow");
static_assert(sizeof(CrtuParams) == 12 && offsetof(CrtuParams, depthTol) == 4 && offsetof(CrtuParams, normalCos) == 8 && sizeof(float4) == 16, "CrtuParams");
static_assert(CRTU_OK == CRTI_OK && CRTU_E_BAD_ARGUMENT == CRTI_E_BAD_ARGUMENT && CRTU_E_OUT_OF_RANGE == CRTI_E_OUT_OF_RANGE && CRTU_GUIDES_PLANES == CRTI_GUIDES_PLANES
              && CRTU_GUIDES_SURFACE == CRTI_GUIDES_SURFACE, "the codes and layouts of crt_image_host.h");

struct CrtuLaunch {
    const char* low;                // float (channels 1) or float4 (channels 4) at low + i * 4 * channels
    char* out;                      // likewise
    uint32_t* state;                // may be NULL
    const char* geometry;           // {n.x, n.y, n.z, t} at geometry + i * stride
    const char* instance;           // int32 at instance + i * stride, NULL without CRTU_MATCH_INSTANCE
    const char* albedo;             // uint32 at albedo + i * stride, NULL without CRTU_MODULATE
    int width, height, lowWidth, lowHeight, offsetX, offsetY;
    uint32_t flags;
    float depthTol, normalCos;
};

// a low sample's value; one channel rides in .x beside three zeros that nothing reads
__device__ __forceinline__ crti_f4 crtu_vec(float4 v) { crti_f4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; return r; }
template <int CHANNELS> __device__ __forceinline__ crti_f4 crtu_value(const char* low, size_t i)
{
    if (CHANNELS == 4) return crtu_vec(crti_load4(low + i * 16));
    crti_f4 r = {*(const float*)(low + i * 4), 0.0f, 0.0f, 0.0f};
    return r;
}
template <int CHANNELS> __device__ __forceinline__ bool crtu_finite(crti_f4 v)
{
    if (CHANNELS == 4) return ((int)crti_finite(v.x) & (int)crti_finite(v.y) & (int)crti_finite(v.z) & (int)crti_finite(v.w)) != 0;
    return crti_finite(v.x);
}
__device__ __forceinline__ float crtu_den_of(uint32_t a, int ch)
{
    const uint32_t b = (a >> (8 * ch)) & 255u;
    return b == 0u ? 1.0f : (float)b / 255.0f;
}

// One lane per full pixel. Its four taps are the low samples (X0 + 0|1, Y0 + 0|1) around it; a tile of 32 x 8 pixels touches sample columns
// floor((x0 - offsetX) / F) .. that + 32/F + 1 and as many rows as 8/F + 2. STAGED: the workgroup's first TW x TH lanes stage those samples -- the
// guide of the pixel each sits on, its instance and its value -- in LDS, and every lane takes its taps from there. Else each lane gathers its
// four taps' guides and values through L1. Either way the address of a sample that does not exist is clamped to one that does (LW, LH >= 1, and
// F * (LW - 1) + offsetX <= W - 1 by crtu_low_size), whether a tap exists is decided from its coordinates, and what must not count is chosen away
// afterwards: the four taps are straight-line code.
template <bool SURFACE, int CHANNELS, int FACTOR, bool STAGED>
__global__ __launch_bounds__(CRTI_BLOCK) void crtu_upsample_kernel(CrtuLaunch P)
{
    constexpr int SHIFT = FACTOR == 2 ? 1 : 2;
    constexpr int TW = CRTI_TILE_W / FACTOR + 2, TH = CRTI_TILE_H / FACTOR + 2, N = TW * TH;
    static_assert((FACTOR == 2 || FACTOR == 4) && (CHANNELS == 1 || CHANNELS == 4) && N <= CRTI_BLOCK, "one staging round");
    __shared__ float4 s_g[STAGED ? N : 1];
    __shared__ int s_i[STAGED ? N : 1];
    __shared__ float4 s_v4[STAGED && CHANNELS == 4 ? N : 1];
    __shared__ float s_v1[STAGED && CHANNELS == 1 ? N : 1];
    const int W = P.width, H = P.height, LW = P.lowWidth, LH = P.lowHeight, ox = P.offsetX, oy = P.offsetY;
    const CrtiLane lane;
    const int x0 = lane.x0, y0 = lane.y0, x = lane.x, y = lane.y;
    const bool match = (P.flags & CRTU_MATCH_INSTANCE) != 0, modulate = (P.flags & CRTU_MODULATE) != 0;
    const bool mine = x < W && y < H;                 // a lane without a pixel stages its sample and stores nothing
    if (!STAGED && !mine) return;
    const size_t ci = crti_clamped_own(x, y, W, H);
    const float4 gc = crti_geometry<SURFACE>(P, ci);
    const int ic = match ? crti_instance<SURFACE>(P, ci) : 0;
    const uint32_t ac = modulate ? crti_albedo<SURFACE>(P, ci) : 0u;
    // the tile's first sample column and row: a floor (an arithmetic shift), -1 for the first tile under an offset
    const int sx0 = (x0 - ox) >> SHIFT, sy0 = (y0 - oy) >> SHIFT;
    if (STAGED) {
        const int i = (int)threadIdx.x;
        if (i < N) {
            const int ty = i / TW, tx = i - ty * TW;
            const int X = min(max(sx0 + tx, 0), LW - 1), Y = min(max(sy0 + ty, 0), LH - 1);
            const size_t li = (size_t)(uint32_t)(Y * LW + X), gi = (size_t)(uint32_t)((Y * FACTOR + oy) * W + (X * FACTOR + ox));
            const float4 g = crti_geometry<SURFACE>(P, gi);
            const crti_f4 v = crtu_value<CHANNELS>(P.low, li);
            const int inst = match ? crti_instance<SURFACE>(P, gi) : 0;
            crti_store4(s_g + i, g); s_i[i] = inst;
            if (CHANNELS == 4) *(crti_f4*)(s_v4 + i) = v;
            else s_v1[i] = v.x;
        }
        __syncthreads();
        if (!mine) return;
    }
    // ---- the four taps
    const int rx = x - ox, ry = y - oy;
    const int X0 = rx >> SHIFT, Y0 = ry >> SHIFT;
    const float fx = (float)(rx - X0 * FACTOR) / (float)FACTOR, fy = (float)(ry - Y0 * FACTOR) / (float)FACTOR;
    const float ex = 1.0f - fx, ey = 1.0f - fy;
    const float b[4] = {ex * ey, fx * ey, ex * fy, fx * fy};
    crti_f4 gq[4], vq[4]; int iq[4], eq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int X = X0 + (k & 1), Y = Y0 + (k >> 1);
        eq[k] = CRTI_INSIDE(X, Y, LW, LH) ? 1 : 0;
        if (STAGED) {
            const int q = (Y - sy0) * TW + (X - sx0);
            gq[k] = crtu_vec(crti_load4(s_g + q)); iq[k] = match ? s_i[q] : 0;
            if (CHANNELS == 4) vq[k] = crtu_vec(crti_load4(s_v4 + q));
            else { const crti_f4 r = {s_v1[q], 0.0f, 0.0f, 0.0f}; vq[k] = r; }
        } else {
            const int Xc = min(max(X, 0), LW - 1), Yc = min(max(Y, 0), LH - 1);
            const size_t li = (size_t)(uint32_t)(Yc * LW + Xc), gi = (size_t)(uint32_t)((Yc * FACTOR + oy) * W + (Xc * FACTOR + ox));
            gq[k] = crtu_vec(crti_geometry<SURFACE>(P, gi)); iq[k] = match ? crti_instance<SURFACE>(P, gi) : 0;
            vq[k] = crtu_value<CHANNELS>(P.low, li);
        }
    }
    const bool hc = crti_hit(gc.w);
    const float dtol = P.depthTol * gc.w;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f, ws = 0.0f, bd = 0.0f;
    crti_f4 nv = {0.0f, 0.0f, 0.0f, 0.0f}, fv = nv;             // the nearest candidate's value, the first candidate's
    int counted = 0, anyNear = 0, anyFirst = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const crti_f4 g = gq[k], v = vq[k];
        const int hg = (int)crti_hit(g.w);
        const float d = fabsf(g.w - gc.w);
        // & and | on ints, not && and ||: straight-line code, as the siblings' taps
        const int cand = eq[k] & (int)crtu_finite<CHANNELS>(v);
        const int geo = hg & (int)(d <= dtol) & (int)(crti_dot3(g.x, g.y, g.z, gc.x, gc.y, gc.z) >= P.normalCos) & (int)(iq[k] == ic);
        const int ok = cand & (int)(b[k] > 0.0f) & (hc ? geo : (hg ^ 1));
        // a tap that does not count is selected away, never multiplied by zero
        sx = ok ? sx + v.x * b[k] : sx; ws = ok ? ws + b[k] : ws;
        if (CHANNELS == 4) { sy = ok ? sy + v.y * b[k] : sy; sz = ok ? sz + v.z * b[k] : sz; sw = ok ? sw + v.w * b[k] : sw; }
        counted |= ok;
        // the fall-back's two choices, kept as values: no tap is indexed afterwards
        const int near = cand & (int)hc & hg & (int)!__builtin_isnan(d);
        const int take = near & ((anyNear ^ 1) | (int)(d < bd));
        nv = take ? v : nv; bd = take ? d : bd; anyNear |= near;
        const int first = cand & (anyFirst ^ 1);
        fv = first ? v : fv; anyFirst |= cand;
    }
    crti_f4 o = {sx / ws, 0.0f, 0.0f, 0.0f};
    if (CHANNELS == 4) { o.y = sy / ws; o.z = sz / ws; o.w = sw / ws; }
    uint32_t st = CRTU_STATE_INTERPOLATED;
    if (!counted) {
        o = anyNear ? nv : fv;                        // fv is zero while there is no candidate
        st = anyFirst ? CRTU_STATE_NEAREST : CRTU_STATE_EMPTY;
    }
    if (CHANNELS == 4) {
        if (modulate && hc) { o.x = o.x * crtu_den_of(ac, 0); o.y = o.y * crtu_den_of(ac, 1); o.z = o.z * crtu_den_of(ac, 2); }
        *(crti_f4*)(P.out + ci * 16) = o;
    } else {
        *(float*)(P.out + ci * 4) = o.x;
    }
    if (P.state) P.state[ci] = st;
}

template <bool SURFACE, int CHANNELS, int FACTOR>
static void crtu_launch_taps(const CrtuLaunch& P, bool staged, hipStream_t stream)
{
    const dim3 grid = crti_grid(P.width, P.height);
    if (staged) crtu_upsample_kernel<SURFACE, CHANNELS, FACTOR, true><<<grid, CRTI_BLOCK, 0, stream>>>(P);
    else crtu_upsample_kernel<SURFACE, CHANNELS, FACTOR, false><<<grid, CRTI_BLOCK, 0, stream>>>(P);
}

template <bool SURFACE>
static void crtu_launch(const CrtuLaunch& P, int channels, int factor, bool staged, hipStream_t stream)
{
    if (channels == 4 && factor == 2) crtu_launch_taps<SURFACE, 4, 2>(P, staged, stream);
    else if (channels == 4) crtu_launch_taps<SURFACE, 4, 4>(P, staged, stream);
    else if (factor == 2) crtu_launch_taps<SURFACE, 1, 2>(P, staged, stream);
    else crtu_launch_taps<SURFACE, 1, 4>(P, staged, stream);
}

// where the four taps come from: CRTU_TAPS=l1|lds in the environment (crt_image_env.h), else the built-in choice
static bool crtu_taps_lds(bool match) { return crti_env_choice("CRTU_TAPS", "l1", "lds", CRTU_STAGED_DEFAULT(match) != 0); }

// what both entry points refuse of the frame's size and the low image's place in it
static int crtu_check_size(int32_t width, int32_t height, int32_t factor, int32_t offsetX, int32_t offsetY)
{
    if (width < 1 || height < 1) return CRTU_E_BAD_ARGUMENT;
    if (factor != 2 && factor != 4) return CRTU_E_BAD_ARGUMENT;
    if (offsetX < 0 || offsetX >= factor || offsetY < 0 || offsetY >= factor) return CRTU_E_BAD_ARGUMENT;
    if (offsetX >= width || offsetY >= height) return CRTU_E_BAD_ARGUMENT;      // no sample would lie in the frame
    if (width > CRTI_MAX_DIM || height > CRTI_MAX_DIM) return CRTU_E_OUT_OF_RANGE;
    return CRTU_OK;
}

static int crtu_check(const CrtuFrame* f, const CrtuLow* l, const CrtuParams* p, const void* out, const void* outState)
{
    if (!f || !l || !p || !out || !l->low || !f->geometry) return CRTU_E_BAD_ARGUMENT;
    if (l->channels != 1 && l->channels != 4) return CRTU_E_BAD_ARGUMENT;
    if (p->flags & ~(uint32_t)(CRTU_MATCH_INSTANCE | CRTU_MODULATE)) return CRTU_E_BAD_ARGUMENT;
    if ((p->flags & CRTU_MODULATE) && l->channels != 4) return CRTU_E_BAD_ARGUMENT;
    if (!crti_guides_ok(f->guides, (p->flags & CRTU_MATCH_INSTANCE) != 0, f->ids, (p->flags & CRTU_MODULATE) != 0, f->albedo)) return CRTU_E_BAD_ARGUMENT;
    if (!(p->depthTol >= 0.0f) || isnan(p->normalCos)) return CRTU_E_BAD_ARGUMENT;
    const void* const outs[2] = {out, outState};
    const void* const ins[4] = {l->low, f->geometry, f->ids, f->albedo};
    if (crti_aliased(ins, outs)) return CRTU_E_BAD_ARGUMENT;
    return crtu_check_size(f->width, f->height, l->factor, l->offsetX, l->offsetY);
}

extern "C" {

int crtu_low_size(int32_t width, int32_t height, int32_t factor, int32_t offsetX, int32_t offsetY, int32_t* lowWidth, int32_t* lowHeight)
{
    if (!lowWidth || !lowHeight) return CRTU_E_BAD_ARGUMENT;
    const int rc = crtu_check_size(width, height, factor, offsetX, offsetY);
    if (rc != CRTU_OK) return rc;
    *lowWidth = (width - offsetX + factor - 1) / factor;
    *lowHeight = (height - offsetY + factor - 1) / factor;
    return CRTU_OK;
}

int crtu_upsample(const CrtuFrame* f, const CrtuLow* l, const CrtuParams* p, void* out, void* outState, void* stream)
{
    const int rc = crtu_check(f, l, p, out, outState);
    if (rc != CRTU_OK) return rc;
    const bool surface = f->guides == CRTU_GUIDES_SURFACE;
    const bool match = (p->flags & CRTU_MATCH_INSTANCE) != 0, modulate = (p->flags & CRTU_MODULATE) != 0;
    const char* g = (const char*)f->geometry;
    CrtuLaunch P;
    P.low = (const char*)l->low; P.out = (char*)out; P.state = (uint32_t*)outState;
    P.geometry = g;
    P.instance = !match ? nullptr : surface ? g + 16 : (const char*)f->ids;
    P.albedo = !modulate ? nullptr : surface ? g + 32 : (const char*)f->albedo;
    P.width = f->width; P.height = f->height;
    P.lowWidth = (f->width - l->offsetX + l->factor - 1) / l->factor; P.lowHeight = (f->height - l->offsetY + l->factor - 1) / l->factor;
    P.offsetX = l->offsetX; P.offsetY = l->offsetY;
    P.flags = p->flags; P.depthTol = p->depthTol; P.normalCos = p->normalCos;
    if (surface) crtu_launch<true>(P, l->channels, l->factor, crtu_taps_lds(match), (hipStream_t)stream);
    else crtu_launch<false>(P, l->channels, l->factor, crtu_taps_lds(match), (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : CRTU_OK;
}

const char* crtu_error_string(int rc)
{
    return CRTI_ERROR_STRING("crtu", rc);
}

}
