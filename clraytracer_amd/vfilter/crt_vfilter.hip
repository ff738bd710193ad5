// crt_vfilter.hip -- libcrt_vfilter.so: the variance-guided a-trous filter of include/crt_vfilter.h (definition there), its two kernels and the
// C ABI over them. The only translation unit of the library. The steps it has in common with the other image libraries -- vector loads, guide
// layouts, predicates, weights, the tile and its staging arithmetic; the grid, the rules of the argument check, the ping-pong, the error strings;
// the two switches' parsers -- come from ../image/crt_image_device.h, crt_image_host.h and crt_image_env.h. It shares no state.
// Build: the Makefile's $(VFILTER_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include "../../include/crt_vfilter.h"
#include "../image/crt_image_host.h"
#include "../image/crt_image_env.h"

#define CRTV_MAX_ITERATIONS 5
#define CRTV_STAGE_MAX_STEP_DEFAULT 4   // what was measured for each step
#define CRTV_ESTIMATE_LDS_DEFAULT 1
// the ABI of crt_vfilter.h (clraytracer_amd/_lib.py mirrors it)
static_assert(sizeof(CrtvFrame) == 56 && offsetof(CrtvFrame, color) == 8 && offsetof(CrtvFrame, moments) == 16 && offsetof(CrtvFrame, guides) == 24
              && offsetof(CrtvFrame, geometry) == 32 && offsetof(CrtvFrame, ids) == 40 && offsetof(CrtvFrame, albedo) == 48, "CrtvFrame");
static_assert(sizeof(CrtvParams) == 28 && offsetof(CrtvParams, flags) == 4 && offsetof(CrtvParams, depthTol) == 8 && offsetof(CrtvParams, normalCos) == 12
              && offsetof(CrtvParams, lumaSigma) == 16 && offsetof(CrtvParams, lumaFloor) == 20 && offsetof(CrtvParams, minHistory) == 24
              && sizeof(float4) == 16, "CrtvParams");
static_assert(CRTV_OK == CRTI_OK && CRTV_E_BAD_ARGUMENT == CRTI_E_BAD_ARGUMENT && CRTV_E_OUT_OF_RANGE == CRTI_E_OUT_OF_RANGE && CRTV_GUIDES_PLANES == CRTI_GUIDES_PLANES
              && CRTV_GUIDES_SURFACE == CRTI_GUIDES_SURFACE, "the codes and layouts of crt_image_host.h");
// a bit of CrtvLaunch::flags beside CRTV_DEMODULATE and CRTV_MATCH_INSTANCE
#define CRTV_PASS_LAST 0x100u       // the last pass: store {rgb * den, color.a} and the variance plane

struct CrtvLaunch {
    const float4 *color, *moments;  // the caller's inputs
    const float4* in;               // I, a pass's input image {rgb, var}
    float4* out;                    // the estimate's or the pass's output
    float* outVariance;             // the last pass only; may be NULL
    const char* geometry;           // {n.x, n.y, n.z, t} at geometry + i * stride
    const char* instance;           // int32 at instance + i * stride, NULL without CRTV_MATCH_INSTANCE
    const char* albedo;             // uint32 at albedo + i * stride, NULL without CRTV_DEMODULATE
    int width, height, step;
    uint32_t flags;
    float depthTol, normalCos, lumaSigma, lumaFloor, minHistory;
};

// den of channel ch (0 = r, 1 = g, 2 = b) of an albedo word; `on`: CRTV_DEMODULATE
__device__ __forceinline__ float crtv_den_of(uint32_t a, int ch, bool on)
{
    const uint32_t b = (a >> (8 * ch)) & 255u;
    return (!on || b == 0u) ? 1.0f : (float)b / 255.0f;
}
__device__ __forceinline__ float crtv_g(int d) { return d == 0 ? 0.25f : 0.125f; }   // G[0], G[1]: the prefilter reaches no further

// The estimate: I0 = {rgb, var}, demodulated. STAGE: a workgroup with a pixel in need of the spatial estimate stages geometry, {m1, m2} and the
// instance id over its tile and a halo of 3 in LDS (28 B per pixel) and takes the 49 taps from there; else they are row reads through L1 / L2, a
// row of seven at a time. Either way the pixel's own loads are one round, the taps a second one that most workgroups of a long history skip.
// Addresses are clamped into the frame; a pixel outside it is taken as no hit, and what must not count is chosen away afterwards.
template <bool SURFACE, bool STAGE>
__global__ __launch_bounds__(CRTI_BLOCK) void crtv_estimate_kernel(CrtvLaunch P)
{
    constexpr int HALO = 3;
    using Tile = CrtiTile<HALO>;
    constexpr int TW = Tile::TW, N = Tile::N, ROUNDS = Tile::ROUNDS;
    __shared__ float4 s_g[STAGE ? N : 1];
    __shared__ float2 s_m[STAGE ? N : 1];
    __shared__ int s_i[STAGE ? N : 1];
    const int W = P.width, H = P.height;
    const CrtiLane lane;
    const int lx = lane.lx, ly = lane.ly, x0 = lane.x0, y0 = lane.y0, x = lane.x, y = lane.y;
    const bool match = (P.flags & CRTV_MATCH_INSTANCE) != 0, demod = (P.flags & CRTV_DEMODULATE) != 0;
    const bool mine = x < W && y < H;                 // a lane without a pixel reads the clamped one and stores nothing
    if (!STAGE && !mine) return;
    const size_t ci = crti_clamped(x, y, W, H);
    const float4 c = crti_load4(P.color + ci), m = crti_load4(P.moments + ci), g = crti_geometry<SURFACE>(P, ci);
    const int ic = match ? crti_instance<SURFACE>(P, ci) : 0;
    const uint32_t ac = demod ? crti_albedo<SURFACE>(P, ci) : 0u;
    const bool hit = crti_hit(g.w);
    const bool spatial = mine && hit && !(m.z >= P.minHistory);
    float var = m.w >= 0.0f ? m.w : 0.0f;
    if (STAGE) {
        // does any pixel of the workgroup need the taps? Asked through the tile's first word, before anything is staged there
        if (threadIdx.x == 0) s_i[0] = 0;
        __syncthreads();
        if (spatial) s_i[0] = 1;
        __syncthreads();
        const bool any = s_i[0] != 0;
        __syncthreads();
        if (any) {
            float4 sg[ROUNDS]; float2 sm[ROUNDS]; int si[ROUNDS];
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) {
                const size_t q = Tile(j, x0, y0).clamped(W, H);
                sg[j] = crti_geometry<SURFACE>(P, q);
                sm[j] = crti_load2(P.moments + q);
                si[j] = match ? crti_instance<SURFACE>(P, q) : 0;
            }
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) {
                const Tile t(j, x0, y0);
                const int i = t.i;
                if (!CRTI_INSIDE(t.px, t.py, W, H)) sg[j].w = CRTI_MISS;
                if (i < N) { crti_store4(s_g + i, sg[j]); crti_store2(s_m + i, sm[j]); s_i[i] = si[j]; }
            }
            __syncthreads();
        }
    }
    if (spatial) {
        const float dtol = (P.depthTol * g.w) * 1.0f;
        float S1 = 0.0f, S2 = 0.0f, n = 0.0f;
#pragma unroll 1
        for (int dy = -3; dy <= 3; ++dy) {
            float4 gq[7]; float2 mq[7]; int iq[7];
#pragma unroll
            for (int dx = -3; dx <= 3; ++dx) {
                const int k = dx + 3;
                if (STAGE) {
                    const int q = (ly + HALO + dy) * TW + lx + HALO + dx;
                    gq[k] = crti_load4(s_g + q); mq[k] = crti_load2(s_m + q); iq[k] = match ? s_i[q] : 0;
                } else {
                    const int qx = x + dx, qy = y + dy;
                    const size_t q = crti_clamped(qx, qy, W, H);
                    gq[k] = crti_geometry<SURFACE>(P, q); mq[k] = crti_load2(P.moments + q); iq[k] = match ? crti_instance<SURFACE>(P, q) : 0;
                    if (!CRTI_INSIDE(qx, qy, W, H)) gq[k].w = CRTI_MISS;
                }
            }
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                // & and | on ints, not && and ||: straight-line code, as CrtdSum::tap
                const int ok = ((int)crti_hit(gq[k].w) & (int)(fabsf(gq[k].w - g.w) <= dtol) & (int)(crti_dot3(gq[k], g) >= P.normalCos) & (int)(iq[k] == ic)
                                & (int)crti_finite(mq[k].x) & (int)crti_finite(mq[k].y)) | (int)(dy == 0 && k == 3);
                S1 = ok ? S1 + mq[k].x : S1; S2 = ok ? S2 + mq[k].y : S2; n = ok ? n + 1.0f : n;
            }
        }
        const float a = S1 / n, v = S2 / n - a * a;
        var = v > 0.0f ? v : 0.0f;
        var = var * (4.0f / fmaxf(m.z, 1.0f));
    }
    if (!mine) return;
    float4 o = make_float4(c.x, c.y, c.z, 0.0f);
    if (hit) {
        const float dx_ = crtv_den_of(ac, 0, demod), dy_ = crtv_den_of(ac, 1, demod), dz_ = crtv_den_of(ac, 2, demod);
        o.w = var;
        if (demod) {
            const float ld = crti_luma(dx_, dy_, dz_);
            o.x = c.x / dx_; o.y = c.y / dy_; o.z = c.z / dz_; o.w = var / (ld * ld);
        }
    }
    crti_store4(P.out + ci, o);
}

// One pass. STAGE = 1, 2 or 4: the pass of that step with its taps from LDS -- the workgroup stages its tile and a halo of 2 * STAGE pixels as three
// planes: geometry and {I.rgb, var} as float4 (a 16-B stride per lane keeps ds_read_b128 conflict-free) and the instance id. STAGE = 0: any step
// (P.step), the taps are row reads through L1 / L2. The staging loads, the nine of the prefilter and the five taps of a row are each issued before
// the first of them is waited for: the loads are unconditional (a pixel outside the frame reads the clamped pixel) and what must not count is
// chosen away afterwards; a pixel outside the frame is taken as no hit. The loop over the five rows stays rolled: unrolled, the scheduler hoists
// all 25 taps' loads over the divisions and needs 250 VGPRs (two waves per SIMD) where this form needs 72-79. The 3 x 3 prefilter
// lies inside any staged halo (2 * STAGE >= 2).
template <bool SURFACE, int STAGE>
__global__ __launch_bounds__(CRTI_BLOCK) void crtv_pass_kernel(CrtvLaunch P)
{
    constexpr int HALO = 2 * STAGE;
    using Tile = CrtiTile<HALO>;
    constexpr int TW = Tile::TW, N = Tile::N, ROUNDS = Tile::ROUNDS;
    __shared__ float4 s_g[STAGE ? N : 1];
    __shared__ float4 s_c[STAGE ? N : 1];
    __shared__ int s_i[STAGE ? N : 1];
    const int W = P.width, H = P.height, s = STAGE ? STAGE : P.step;
    const CrtiLane lane;
    const int lx = lane.lx, ly = lane.ly, x0 = lane.x0, y0 = lane.y0, x = lane.x, y = lane.y;
    const bool match = (P.flags & CRTV_MATCH_INSTANCE) != 0, demod = (P.flags & CRTV_DEMODULATE) != 0, last = (P.flags & CRTV_PASS_LAST) != 0;
    const bool mine = x < W && y < H;                 // a lane without a pixel reads the clamped one and stores nothing
    if (!STAGE && !mine) return;
    const size_t ci = crti_clamped(x, y, W, H);
    const float4 cc = crti_load4(P.in + ci);          // a pixel that is no hit copies I
    const uint32_t ac = (last && demod) ? crti_albedo<SURFACE>(P, ci) : 0u;
    const float alpha = last ? ((const float*)(P.color + ci))[3] : 0.0f;
    float4 gc; int ic;
    if (STAGE) {
        float4 sg[ROUNDS], sc[ROUNDS]; int si[ROUNDS];
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const size_t q = Tile(j, x0, y0).clamped(W, H);
            sg[j] = crti_geometry<SURFACE>(P, q);
            sc[j] = crti_load4(P.in + q);
            si[j] = match ? crti_instance<SURFACE>(P, q) : 0;
        }
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const Tile t(j, x0, y0);
            const int i = t.i;
            if (!CRTI_INSIDE(t.px, t.py, W, H)) sg[j].w = CRTI_MISS;
            if (i < N) { crti_store4(s_g + i, sg[j]); crti_store4(s_c + i, sc[j]); s_i[i] = si[j]; }
        }
        __syncthreads();
        if (!mine) return;
        gc = crti_load4(s_g + (ly + HALO) * TW + lx + HALO);
        ic = match ? s_i[(ly + HALO) * TW + lx + HALO] : 0;
    } else {
        gc = crti_geometry<SURFACE>(P, ci);
        ic = match ? crti_instance<SURFACE>(P, ci) : 0;
    }
    if (!crti_hit(gc.w)) {
        crti_store4(P.out + ci, make_float4(cc.x, cc.y, cc.z, last ? alpha : cc.w));
        if (last && P.outVariance) P.outVariance[ci] = 0.0f;
        return;
    }
    // ---- the prefiltered variance and the luminance stop
    float tq[9], vq[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int dx = k % 3 - 1, dy = k / 3 - 1;
        if (STAGE) {
            const int q = (ly + HALO + dy) * TW + lx + HALO + dx;
            tq[k] = s_g[q].w; vq[k] = s_c[q].w;
        } else {
            const int qx = x + dx, qy = y + dy;
            const size_t q = crti_clamped(qx, qy, W, H);
            tq[k] = crti_distance<SURFACE>(P, q); vq[k] = ((const float*)(P.in + q))[3];
            if (!CRTI_INSIDE(qx, qy, W, H)) tq[k] = CRTI_MISS;
        }
    }
    float gsum = 0.0f, gw = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int ok = (int)crti_hit(tq[k]) & (int)(vq[k] >= 0.0f);
        const float gg = crtv_g(k / 3 - 1) * crtv_g(k % 3 - 1);
        gsum = ok ? gsum + vq[k] * gg : gsum; gw = ok ? gw + gg : gw;
    }
    const float gv = gw > 0.0f ? gsum / gw : 0.0f;
    const float sd = P.lumaSigma * sqrtf(gv) + P.lumaFloor;
    // ---- the 25 taps
    const float lc = crti_luma(cc.x, cc.y, cc.z), dtol = (P.depthTol * gc.w) * (float)s;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, vs = 0.0f, ws = 0.0f;
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float k = crti_k(dy) * crti_k(dx);
            float4 g, c; int inst;
            if (STAGE) {
                const int q = (ly + HALO + dy * STAGE) * TW + lx + HALO + dx * STAGE;
                g = crti_load4(s_g + q); c = crti_load4(s_c + q); inst = match ? s_i[q] : 0;
            } else {
                const int qx = x + dx * s, qy = y + dy * s;
                const size_t q = crti_clamped(qx, qy, W, H);
                g = crti_geometry<SURFACE>(P, q); c = crti_load4(P.in + q); inst = match ? crti_instance<SURFACE>(P, q) : 0;
                if (!CRTI_INSIDE(qx, qy, W, H)) g.w = CRTI_MISS;
            }
            const bool centre = (dx | dy) == 0;
            const float xl = fabsf(crti_luma(c.x, c.y, c.z) - lc) / sd, om = 1.0f - xl;
            const float w = centre ? k : k * (om * om);
            // & and | on ints, not && and ||: 25 taps of straight-line code instead of a branch per condition
            const int ok = ((int)crti_hit(g.w) & (int)(fabsf(g.w - gc.w) <= dtol) & (int)(crti_dot3(g, gc) >= P.normalCos) & (int)(inst == ic)
                            & (int)(c.w >= 0.0f) & (int)(xl < 1.0f)) | (int)centre;
            // a tap that does not count is selected away, never multiplied by zero
            sx = ok ? sx + c.x * w : sx; sy = ok ? sy + c.y * w : sy; sz = ok ? sz + c.z * w : sz;
            vs = ok ? vs + c.w * (w * w) : vs; ws = ok ? ws + w : ws;
        }
    }
    float4 o = make_float4(sx / ws, sy / ws, sz / ws, vs / (ws * ws));
    if (last) {
        const float dx_ = crtv_den_of(ac, 0, demod), dy_ = crtv_den_of(ac, 1, demod), dz_ = crtv_den_of(ac, 2, demod);
        const float ld = crti_luma(dx_, dy_, dz_);
        if (P.outVariance) P.outVariance[ci] = o.w * (ld * ld);
        o.x = o.x * dx_; o.y = o.y * dy_; o.z = o.z * dz_; o.w = alpha;
    }
    crti_store4(P.out + ci, o);
}

static dim3 crtv_grid(const CrtvLaunch& P) { return crti_grid(P.width, P.height); }

template <bool SURFACE>
static void crtv_launch_estimate(const CrtvLaunch& P, bool stage, hipStream_t stream)
{
    if (stage) crtv_estimate_kernel<SURFACE, true><<<crtv_grid(P), CRTI_BLOCK, 0, stream>>>(P);
    else crtv_estimate_kernel<SURFACE, false><<<crtv_grid(P), CRTI_BLOCK, 0, stream>>>(P);
}

template <bool SURFACE>
static void crtv_launch_pass(const CrtvLaunch& P, int stageMaxStep, hipStream_t stream)
{
    const int stage = P.step <= stageMaxStep ? P.step : 0;
    if (stage == 1) crtv_pass_kernel<SURFACE, 1><<<crtv_grid(P), CRTI_BLOCK, 0, stream>>>(P);
    else if (stage == 2) crtv_pass_kernel<SURFACE, 2><<<crtv_grid(P), CRTI_BLOCK, 0, stream>>>(P);
    else if (stage == 4) crtv_pass_kernel<SURFACE, 4><<<crtv_grid(P), CRTI_BLOCK, 0, stream>>>(P);
    else crtv_pass_kernel<SURFACE, 0><<<crtv_grid(P), CRTI_BLOCK, 0, stream>>>(P);
}

// CRTV_STAGE_MAX_STEP in the environment (crt_image_env.h), else the measured default: the largest step whose taps come from LDS.
// Step 4 stages (32 + 16) x (8 + 16) x 36 B = 40.5 KiB; step 8 would stage 90 KiB for a 9 KiB tile and is not offered.
static int crtv_stage_max_step() { return crti_env_step("CRTV_STAGE_MAX_STEP", CRTV_STAGE_MAX_STEP_DEFAULT); }

// where the estimate's 49 taps come from: CRTV_ESTIMATE_TAPS=l1|lds in the environment, else the measured default
static bool crtv_estimate_lds() { return crti_env_choice("CRTV_ESTIMATE_TAPS", "l1", "lds", CRTV_ESTIMATE_LDS_DEFAULT != 0); }

static int crtv_check(const CrtvFrame* f, const CrtvParams* p, const void* out, const void* outVariance, const void* scratch)
{
    if (!f || !p || !out || !scratch || !f->color || !f->moments || !f->geometry) return CRTV_E_BAD_ARGUMENT;
    if (f->width < 1 || f->height < 1) return CRTV_E_BAD_ARGUMENT;
    if (p->iterations < 1 || p->iterations > CRTV_MAX_ITERATIONS) return CRTV_E_BAD_ARGUMENT;
    if (p->flags & ~(uint32_t)(CRTV_DEMODULATE | CRTV_MATCH_INSTANCE)) return CRTV_E_BAD_ARGUMENT;
    if (!crti_guides_ok(f->guides, (p->flags & CRTV_MATCH_INSTANCE) != 0, f->ids, (p->flags & CRTV_DEMODULATE) != 0, f->albedo)) return CRTV_E_BAD_ARGUMENT;
    if (!(p->depthTol >= 0.0f) || !isfinite(p->normalCos)) return CRTV_E_BAD_ARGUMENT;
    if (!(p->lumaSigma >= 0.0f) || !(p->lumaFloor >= 0.0f) || !isfinite(p->lumaSigma) || !isfinite(p->lumaFloor)) return CRTV_E_BAD_ARGUMENT;
    if (isnan(p->minHistory)) return CRTV_E_BAD_ARGUMENT;
    const void* const outs[3] = {out, scratch, outVariance};
    const void* const ins[5] = {f->color, f->moments, f->geometry, f->ids, f->albedo};
    if (crti_aliased(ins, outs)) return CRTV_E_BAD_ARGUMENT;
    if (f->width > CRTI_MAX_DIM || f->height > CRTI_MAX_DIM) return CRTV_E_OUT_OF_RANGE;
    return CRTV_OK;
}

extern "C" {

size_t crtv_scratch_bytes(int32_t width, int32_t height, int32_t iterations)
{
    if (width < 1 || height < 1 || iterations < 1 || iterations > CRTV_MAX_ITERATIONS) return 0;
    return (size_t)width * (size_t)height * sizeof(float4);
}

int crtv_filter(const CrtvFrame* f, const CrtvParams* p, void* out, void* outVariance, void* scratch, void* stream)
{
    const int rc = crtv_check(f, p, out, outVariance, scratch);
    if (rc != CRTV_OK) return rc;
    const bool surface = f->guides == CRTV_GUIDES_SURFACE;
    const bool demod = (p->flags & CRTV_DEMODULATE) != 0, match = (p->flags & CRTV_MATCH_INSTANCE) != 0;
    const char* g = (const char*)f->geometry;
    CrtvLaunch P;
    P.color = (const float4*)f->color; P.moments = (const float4*)f->moments;
    P.outVariance = (float*)outVariance;
    P.geometry = g;
    P.instance = !match ? nullptr : surface ? g + 16 : (const char*)f->ids;
    P.albedo = !demod ? nullptr : surface ? g + 32 : (const char*)f->albedo;
    P.width = f->width; P.height = f->height;
    P.depthTol = p->depthTol; P.normalCos = p->normalCos; P.lumaSigma = p->lumaSigma; P.lumaFloor = p->lumaFloor; P.minHistory = p->minHistory;
    const int stageMax = crtv_stage_max_step(), n = p->iterations;
    // launch -1 is the estimate; the last pass lands in `out`, the launch before it in `scratch`, and so on backwards
    for (int pass = -1; pass < n; ++pass) {
        float4* dst = (float4*)crti_pingpong(n, pass, out, scratch);
        P.in = (const float4*)(dst == out ? scratch : out);
        P.out = dst;
        P.step = pass < 0 ? 1 : 1 << pass;
        P.flags = (p->flags & (uint32_t)(CRTV_DEMODULATE | CRTV_MATCH_INSTANCE)) | (pass == n - 1 ? CRTV_PASS_LAST : 0u);
        if (pass < 0) {
            if (surface) crtv_launch_estimate<true>(P, crtv_estimate_lds(), (hipStream_t)stream);
            else crtv_launch_estimate<false>(P, crtv_estimate_lds(), (hipStream_t)stream);
        } else {
            if (surface) crtv_launch_pass<true>(P, stageMax, (hipStream_t)stream);
            else crtv_launch_pass<false>(P, stageMax, (hipStream_t)stream);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return CRTV_OK;
}

const char* crtv_error_string(int rc)
{
    return CRTI_ERROR_STRING("crtv", rc);
}

}
