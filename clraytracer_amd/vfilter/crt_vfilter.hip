// crt_vfilter.hip -- libcrt_vfilter.so: the variance-guided a-trous filter of include/crt_vfilter.h (definition there), its two kernels and the
// C ABI over them. The only translation unit of the library; it shares no state and no source with the others.
// Build: the Makefile's $(VFILTER_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/crt_vfilter.h"

#define CRTV_TILE_W 32              // 256 lanes over a 32 x 8 tile, as crtd_pass_kernel: a wave is two 512-B rows of float4
#define CRTV_TILE_H 8
#define CRTV_BLOCK (CRTV_TILE_W * CRTV_TILE_H)
#define CRTV_MAX_DIM 16384
#define CRTV_MAX_ITERATIONS 5
#define CRTV_STAGE_MAX_STEP_DEFAULT 4   // what was measured for each step
#define CRTV_ESTIMATE_LDS_DEFAULT 1
// the ABI of crt_vfilter.h (clraytracer_amd/_lib.py mirrors it)
static_assert(sizeof(CrtvFrame) == 56 && offsetof(CrtvFrame, color) == 8 && offsetof(CrtvFrame, moments) == 16 && offsetof(CrtvFrame, guides) == 24
              && offsetof(CrtvFrame, geometry) == 32 && offsetof(CrtvFrame, ids) == 40 && offsetof(CrtvFrame, albedo) == 48, "CrtvFrame");
static_assert(sizeof(CrtvParams) == 28 && offsetof(CrtvParams, flags) == 4 && offsetof(CrtvParams, depthTol) == 8 && offsetof(CrtvParams, normalCos) == 12
              && offsetof(CrtvParams, lumaSigma) == 16 && offsetof(CrtvParams, lumaFloor) == 20 && offsetof(CrtvParams, minHistory) == 24
              && sizeof(float4) == 16, "CrtvParams");
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

// 16-B rows as one vector load or store each (a float4 copied as a struct can be split into a 12-B copy through the stack and a float)
typedef float crtv_f4 __attribute__((ext_vector_type(4)));
typedef float crtv_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 crtv_load4(const void* p) { const crtv_f4 v = *(const crtv_f4*)p; return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void crtv_store4(float4* p, float4 v) { crtv_f4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; *(crtv_f4*)p = r; }
__device__ __forceinline__ float2 crtv_load2(const void* p) { const crtv_f2 v = *(const crtv_f2*)p; return make_float2(v.x, v.y); }
__device__ __forceinline__ void crtv_store2(float2* p, float2 v) { crtv_f2 r; r.x = v.x; r.y = v.y; *(crtv_f2*)p = r; }

// the strides of the two guide layouts: three planes (16, 16, 4 B) or CrtSurfaceHit records (48 B; geometry at 0, instance at 16, albedo at 32)
template <bool SURFACE> __device__ __forceinline__ float4 crtv_geometry(const CrtvLaunch& P, size_t i) { return crtv_load4(P.geometry + i * (SURFACE ? 48 : 16)); }
template <bool SURFACE> __device__ __forceinline__ float crtv_distance(const CrtvLaunch& P, size_t i) { return *(const float*)(P.geometry + i * (SURFACE ? 48 : 16) + 12); }
template <bool SURFACE> __device__ __forceinline__ int crtv_instance(const CrtvLaunch& P, size_t i) { return *(const int*)(P.instance + i * (SURFACE ? 48 : 16)); }
template <bool SURFACE> __device__ __forceinline__ uint32_t crtv_albedo(const CrtvLaunch& P, size_t i) { return *(const uint32_t*)(P.albedo + i * (SURFACE ? 48 : 4)); }

__device__ __forceinline__ bool crtv_hit(float t) { return t <= 99998.0f; }
__device__ __forceinline__ float crtv_dot3(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float crtv_luma(float x, float y, float z) { return (0.299f * x + 0.587f * y) + 0.114f * z; }
__device__ __forceinline__ bool crtv_finite(float v) { return __builtin_isfinite(v); }
// den of channel ch (0 = r, 1 = g, 2 = b) of an albedo word; `on`: CRTV_DEMODULATE
__device__ __forceinline__ float crtv_den_of(uint32_t a, int ch, bool on)
{
    const uint32_t b = (a >> (8 * ch)) & 255u;
    return (!on || b == 0u) ? 1.0f : (float)b / 255.0f;
}
__device__ __forceinline__ float crtv_k(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }
__device__ __forceinline__ float crtv_g(int d) { return d == 0 ? 0.25f : 0.125f; }   // G[0], G[1]: the prefilter reaches no further

// (pixel indices fit 32 bits: 16384 x 16384 at most) the pixel (qx, qy) clamped into the frame
__device__ __forceinline__ size_t crtv_clamped(int qx, int qy, int W, int H) { return (size_t)(uint32_t)(min(max(qy, 0), H - 1) * W + min(max(qx, 0), W - 1)); }

// The estimate: I0 = {rgb, var}, demodulated. STAGE: a workgroup with a pixel in need of the spatial estimate stages geometry, {m1, m2} and the
// instance id over its tile and a halo of 3 in LDS (28 B per pixel) and takes the 49 taps from there; else they are row reads through L1 / L2, a
// row of seven at a time. Either way the pixel's own loads are one round, the taps a second one that most workgroups of a long history skip.
// Addresses are clamped into the frame; a pixel outside it is taken as no hit, and what must not count is chosen away afterwards.
template <bool SURFACE, bool STAGE>
__global__ __launch_bounds__(CRTV_BLOCK) void crtv_estimate_kernel(CrtvLaunch P)
{
    constexpr int HALO = 3, TW = CRTV_TILE_W + 2 * HALO, TH = CRTV_TILE_H + 2 * HALO, N = TW * TH, ROUNDS = (N + CRTV_BLOCK - 1) / CRTV_BLOCK;
    __shared__ float4 s_g[STAGE ? N : 1];
    __shared__ float2 s_m[STAGE ? N : 1];
    __shared__ int s_i[STAGE ? N : 1];
    const int W = P.width, H = P.height;
    const int lx = (int)(threadIdx.x & (CRTV_TILE_W - 1)), ly = (int)(threadIdx.x / CRTV_TILE_W);
    const int x0 = (int)blockIdx.x * CRTV_TILE_W, y0 = (int)blockIdx.y * CRTV_TILE_H;
    const int x = x0 + lx, y = y0 + ly;
    const bool match = (P.flags & CRTV_MATCH_INSTANCE) != 0, demod = (P.flags & CRTV_DEMODULATE) != 0;
    const bool mine = x < W && y < H;                 // a lane without a pixel reads the clamped one and stores nothing
    if (!STAGE && !mine) return;
    const size_t ci = crtv_clamped(x, y, W, H);
    const float4 c = crtv_load4(P.color + ci), m = crtv_load4(P.moments + ci), g = crtv_geometry<SURFACE>(P, ci);
    const int ic = match ? crtv_instance<SURFACE>(P, ci) : 0;
    const uint32_t ac = demod ? crtv_albedo<SURFACE>(P, ci) : 0u;
    const bool hit = crtv_hit(g.w);
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
                const int i = (int)threadIdx.x + j * CRTV_BLOCK, ty = i / TW, tx = i - ty * TW;
                const size_t q = crtv_clamped(x0 - HALO + tx, y0 - HALO + ty, W, H);
                sg[j] = crtv_geometry<SURFACE>(P, q);
                sm[j] = crtv_load2(P.moments + q);
                si[j] = match ? crtv_instance<SURFACE>(P, q) : 0;
            }
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) {
                const int i = (int)threadIdx.x + j * CRTV_BLOCK, ty = i / TW, tx = i - ty * TW;
                const int px = x0 - HALO + tx, py = y0 - HALO + ty;
                if (!(px >= 0 && px < W && py >= 0 && py < H)) sg[j].w = 99999.0f;
                if (i < N) { crtv_store4(s_g + i, sg[j]); crtv_store2(s_m + i, sm[j]); s_i[i] = si[j]; }
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
                    gq[k] = crtv_load4(s_g + q); mq[k] = crtv_load2(s_m + q); iq[k] = match ? s_i[q] : 0;
                } else {
                    const int qx = x + dx, qy = y + dy;
                    const size_t q = crtv_clamped(qx, qy, W, H);
                    gq[k] = crtv_geometry<SURFACE>(P, q); mq[k] = crtv_load2(P.moments + q); iq[k] = match ? crtv_instance<SURFACE>(P, q) : 0;
                    if (!(qx >= 0 && qx < W && qy >= 0 && qy < H)) gq[k].w = 99999.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                // & and | on ints, not && and ||: straight-line code, as CrtdSum::tap
                const int ok = ((int)crtv_hit(gq[k].w) & (int)(fabsf(gq[k].w - g.w) <= dtol) & (int)(crtv_dot3(gq[k], g) >= P.normalCos) & (int)(iq[k] == ic)
                                & (int)crtv_finite(mq[k].x) & (int)crtv_finite(mq[k].y)) | (int)(dy == 0 && k == 3);
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
            const float ld = crtv_luma(dx_, dy_, dz_);
            o.x = c.x / dx_; o.y = c.y / dy_; o.z = c.z / dz_; o.w = var / (ld * ld);
        }
    }
    crtv_store4(P.out + ci, o);
}

// One pass. STAGE = 1, 2 or 4: the pass of that step with its taps from LDS -- the workgroup stages its tile and a halo of 2 * STAGE pixels as three
// planes: geometry and {I.rgb, var} as float4 (a 16-B stride per lane keeps ds_read_b128 conflict-free) and the instance id. STAGE = 0: any step
// (P.step), the taps are row reads through L1 / L2. The staging loads, the nine of the prefilter and the five taps of a row are each issued before
// the first of them is waited for: the loads are unconditional (a pixel outside the frame reads the clamped pixel) and what must not count is
// chosen away afterwards; a pixel outside the frame is taken as no hit. The loop over the five rows stays rolled: unrolled, the scheduler hoists
// all 25 taps' loads over the divisions and needs 250 VGPRs (two waves per SIMD) where this form needs 72-79. The 3 x 3 prefilter
// lies inside any staged halo (2 * STAGE >= 2).
template <bool SURFACE, int STAGE>
__global__ __launch_bounds__(CRTV_BLOCK) void crtv_pass_kernel(CrtvLaunch P)
{
    constexpr int HALO = 2 * STAGE, TW = CRTV_TILE_W + 2 * HALO, TH = CRTV_TILE_H + 2 * HALO, N = TW * TH, ROUNDS = (N + CRTV_BLOCK - 1) / CRTV_BLOCK;
    __shared__ float4 s_g[STAGE ? N : 1];
    __shared__ float4 s_c[STAGE ? N : 1];
    __shared__ int s_i[STAGE ? N : 1];
    const int W = P.width, H = P.height, s = STAGE ? STAGE : P.step;
    const int lx = (int)(threadIdx.x & (CRTV_TILE_W - 1)), ly = (int)(threadIdx.x / CRTV_TILE_W);
    const int x0 = (int)blockIdx.x * CRTV_TILE_W, y0 = (int)blockIdx.y * CRTV_TILE_H;
    const int x = x0 + lx, y = y0 + ly;
    const bool match = (P.flags & CRTV_MATCH_INSTANCE) != 0, demod = (P.flags & CRTV_DEMODULATE) != 0, last = (P.flags & CRTV_PASS_LAST) != 0;
    const bool mine = x < W && y < H;                 // a lane without a pixel reads the clamped one and stores nothing
    if (!STAGE && !mine) return;
    const size_t ci = crtv_clamped(x, y, W, H);
    const float4 cc = crtv_load4(P.in + ci);          // a pixel that is no hit copies I
    const uint32_t ac = (last && demod) ? crtv_albedo<SURFACE>(P, ci) : 0u;
    const float alpha = last ? ((const float*)(P.color + ci))[3] : 0.0f;
    float4 gc; int ic;
    if (STAGE) {
        float4 sg[ROUNDS], sc[ROUNDS]; int si[ROUNDS];
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const int i = (int)threadIdx.x + j * CRTV_BLOCK, ty = i / TW, tx = i - ty * TW;
            const size_t q = crtv_clamped(x0 - HALO + tx, y0 - HALO + ty, W, H);
            sg[j] = crtv_geometry<SURFACE>(P, q);
            sc[j] = crtv_load4(P.in + q);
            si[j] = match ? crtv_instance<SURFACE>(P, q) : 0;
        }
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const int i = (int)threadIdx.x + j * CRTV_BLOCK, ty = i / TW, tx = i - ty * TW;
            const int px = x0 - HALO + tx, py = y0 - HALO + ty;
            if (!(px >= 0 && px < W && py >= 0 && py < H)) sg[j].w = 99999.0f;
            if (i < N) { crtv_store4(s_g + i, sg[j]); crtv_store4(s_c + i, sc[j]); s_i[i] = si[j]; }
        }
        __syncthreads();
        if (!mine) return;
        gc = crtv_load4(s_g + (ly + HALO) * TW + lx + HALO);
        ic = match ? s_i[(ly + HALO) * TW + lx + HALO] : 0;
    } else {
        gc = crtv_geometry<SURFACE>(P, ci);
        ic = match ? crtv_instance<SURFACE>(P, ci) : 0;
    }
    if (!crtv_hit(gc.w)) {
        crtv_store4(P.out + ci, make_float4(cc.x, cc.y, cc.z, last ? alpha : cc.w));
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
            const size_t q = crtv_clamped(qx, qy, W, H);
            tq[k] = crtv_distance<SURFACE>(P, q); vq[k] = ((const float*)(P.in + q))[3];
            if (!(qx >= 0 && qx < W && qy >= 0 && qy < H)) tq[k] = 99999.0f;
        }
    }
    float gsum = 0.0f, gw = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int ok = (int)crtv_hit(tq[k]) & (int)(vq[k] >= 0.0f);
        const float gg = crtv_g(k / 3 - 1) * crtv_g(k % 3 - 1);
        gsum = ok ? gsum + vq[k] * gg : gsum; gw = ok ? gw + gg : gw;
    }
    const float gv = gw > 0.0f ? gsum / gw : 0.0f;
    const float sd = P.lumaSigma * sqrtf(gv) + P.lumaFloor;
    // ---- the 25 taps
    const float lc = crtv_luma(cc.x, cc.y, cc.z), dtol = (P.depthTol * gc.w) * (float)s;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, vs = 0.0f, ws = 0.0f;
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float k = crtv_k(dy) * crtv_k(dx);
            float4 g, c; int inst;
            if (STAGE) {
                const int q = (ly + HALO + dy * STAGE) * TW + lx + HALO + dx * STAGE;
                g = crtv_load4(s_g + q); c = crtv_load4(s_c + q); inst = match ? s_i[q] : 0;
            } else {
                const int qx = x + dx * s, qy = y + dy * s;
                const size_t q = crtv_clamped(qx, qy, W, H);
                g = crtv_geometry<SURFACE>(P, q); c = crtv_load4(P.in + q); inst = match ? crtv_instance<SURFACE>(P, q) : 0;
                if (!(qx >= 0 && qx < W && qy >= 0 && qy < H)) g.w = 99999.0f;
            }
            const bool centre = (dx | dy) == 0;
            const float xl = fabsf(crtv_luma(c.x, c.y, c.z) - lc) / sd, om = 1.0f - xl;
            const float w = centre ? k : k * (om * om);
            // & and | on ints, not && and ||: 25 taps of straight-line code instead of a branch per condition
            const int ok = ((int)crtv_hit(g.w) & (int)(fabsf(g.w - gc.w) <= dtol) & (int)(crtv_dot3(g, gc) >= P.normalCos) & (int)(inst == ic)
                            & (int)(c.w >= 0.0f) & (int)(xl < 1.0f)) | (int)centre;
            // a tap that does not count is selected away, never multiplied by zero
            sx = ok ? sx + c.x * w : sx; sy = ok ? sy + c.y * w : sy; sz = ok ? sz + c.z * w : sz;
            vs = ok ? vs + c.w * (w * w) : vs; ws = ok ? ws + w : ws;
        }
    }
    float4 o = make_float4(sx / ws, sy / ws, sz / ws, vs / (ws * ws));
    if (last) {
        const float dx_ = crtv_den_of(ac, 0, demod), dy_ = crtv_den_of(ac, 1, demod), dz_ = crtv_den_of(ac, 2, demod);
        const float ld = crtv_luma(dx_, dy_, dz_);
        if (P.outVariance) P.outVariance[ci] = o.w * (ld * ld);
        o.x = o.x * dx_; o.y = o.y * dy_; o.z = o.z * dz_; o.w = alpha;
    }
    crtv_store4(P.out + ci, o);
}

static dim3 crtv_grid(const CrtvLaunch& P)
{
    return dim3((unsigned)((P.width + CRTV_TILE_W - 1) / CRTV_TILE_W), (unsigned)((P.height + CRTV_TILE_H - 1) / CRTV_TILE_H));
}

template <bool SURFACE>
static void crtv_launch_estimate(const CrtvLaunch& P, bool stage, hipStream_t stream)
{
    if (stage) crtv_estimate_kernel<SURFACE, true><<<crtv_grid(P), CRTV_BLOCK, 0, stream>>>(P);
    else crtv_estimate_kernel<SURFACE, false><<<crtv_grid(P), CRTV_BLOCK, 0, stream>>>(P);
}

template <bool SURFACE>
static void crtv_launch_pass(const CrtvLaunch& P, int stageMaxStep, hipStream_t stream)
{
    const int stage = P.step <= stageMaxStep ? P.step : 0;
    if (stage == 1) crtv_pass_kernel<SURFACE, 1><<<crtv_grid(P), CRTV_BLOCK, 0, stream>>>(P);
    else if (stage == 2) crtv_pass_kernel<SURFACE, 2><<<crtv_grid(P), CRTV_BLOCK, 0, stream>>>(P);
    else if (stage == 4) crtv_pass_kernel<SURFACE, 4><<<crtv_grid(P), CRTV_BLOCK, 0, stream>>>(P);
    else crtv_pass_kernel<SURFACE, 0><<<crtv_grid(P), CRTV_BLOCK, 0, stream>>>(P);
}

// the largest step whose taps come from LDS: CRTV_STAGE_MAX_STEP in the environment (0, 1, 2 or 4), else the measured default.
// Step 4 stages (32 + 16) x (8 + 16) x 36 B = 40.5 KiB; step 8 would stage 90 KiB for a 9 KiB tile and is not offered.
static int crtv_stage_max_step()
{
    const char* e = getenv("CRTV_STAGE_MAX_STEP");
    if (e && e[0] && !e[1] && (e[0] == '0' || e[0] == '1' || e[0] == '2' || e[0] == '4')) return e[0] - '0';
    return CRTV_STAGE_MAX_STEP_DEFAULT;
}

// where the estimate's 49 taps come from: CRTV_ESTIMATE_TAPS=l1|lds in the environment, else the measured default
static bool crtv_estimate_lds()
{
    const char* e = getenv("CRTV_ESTIMATE_TAPS");
    if (e && !strcmp(e, "lds")) return true;
    if (e && !strcmp(e, "l1")) return false;
    return CRTV_ESTIMATE_LDS_DEFAULT != 0;
}

static int crtv_check(const CrtvFrame* f, const CrtvParams* p, const void* out, const void* outVariance, const void* scratch)
{
    if (!f || !p || !out || !scratch || !f->color || !f->moments || !f->geometry) return CRTV_E_BAD_ARGUMENT;
    if (f->width < 1 || f->height < 1) return CRTV_E_BAD_ARGUMENT;
    if (p->iterations < 1 || p->iterations > CRTV_MAX_ITERATIONS) return CRTV_E_BAD_ARGUMENT;
    if (p->flags & ~(uint32_t)(CRTV_DEMODULATE | CRTV_MATCH_INSTANCE)) return CRTV_E_BAD_ARGUMENT;
    if (f->guides == CRTV_GUIDES_PLANES) {
        if (((p->flags & CRTV_MATCH_INSTANCE) && !f->ids) || ((p->flags & CRTV_DEMODULATE) && !f->albedo)) return CRTV_E_BAD_ARGUMENT;
    } else if (f->guides == CRTV_GUIDES_SURFACE) {
        if (f->ids || f->albedo) return CRTV_E_BAD_ARGUMENT;
    } else {
        return CRTV_E_BAD_ARGUMENT;
    }
    if (!(p->depthTol >= 0.0f) || !isfinite(p->normalCos)) return CRTV_E_BAD_ARGUMENT;
    if (!(p->lumaSigma >= 0.0f) || !(p->lumaFloor >= 0.0f) || !isfinite(p->lumaSigma) || !isfinite(p->lumaFloor)) return CRTV_E_BAD_ARGUMENT;
    if (isnan(p->minHistory)) return CRTV_E_BAD_ARGUMENT;
    const void* outs[3] = {out, scratch, outVariance};
    const void* inputs[5] = {f->color, f->moments, f->geometry, f->ids, f->albedo};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        for (const void* in : inputs)
            if (in == outs[i]) return CRTV_E_BAD_ARGUMENT;
        for (int j = 0; j < i; ++j)
            if (outs[j] == outs[i]) return CRTV_E_BAD_ARGUMENT;
    }
    if (f->width > CRTV_MAX_DIM || f->height > CRTV_MAX_DIM) return CRTV_E_OUT_OF_RANGE;
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
        float4* dst = (float4*)(((n - 1 - pass) & 1) ? scratch : out);
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
    switch (rc) {
    case CRTV_OK: return "ok";
    case CRTV_E_BAD_ARGUMENT: return "crtv: bad argument";
    case CRTV_E_OUT_OF_RANGE: return "crtv: out of range (a frame wider or taller than 16384)";
    default: return rc > 0 ? hipGetErrorString((hipError_t)rc) : "crtv: unknown error";
    }
}

}
