// crt_temporal.hip -- libcrt_temporal.so: temporal reprojection and accumulation of include/crt_temporal.h (definition there), its kernel, the
// host-only camera maps and the C ABI over them. The only translation unit of the library; it shares no state and no source with the others.
// Build: the Makefile's $(TEMPORAL_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/crt_temporal.h"

#define CRTT_TILE_W 32              // 256 lanes over a 32 x 8 tile, as crtd_pass_kernel: a wave is two 512-B rows of float4
#define CRTT_TILE_H 8
#define CRTT_BLOCK (CRTT_TILE_W * CRTT_TILE_H)
#define CRTT_MAX_DIM 16384
#define CRTT_TAPS_GATED_DEFAULT 1   // what was measured
#define CRTT_CLAMP_LDS_DEFAULT 1
// the ABI of crt_temporal.h (clraytracer_amd/_lib.py mirrors it)
static_assert(sizeof(CrttCamera) == 84 && offsetof(CrttCamera, toRay) == 12 && offsetof(CrttCamera, toScreen) == 48, "CrttCamera");
static_assert(sizeof(CrttFrame) == 128 && offsetof(CrttFrame, color) == 8 && offsetof(CrttFrame, guides) == 16 && offsetof(CrttFrame, geometry) == 24
              && offsetof(CrttFrame, ids) == 32 && offsetof(CrttFrame, camera) == 40, "CrttFrame");
static_assert(sizeof(CrttHistory) == 120 && offsetof(CrttHistory, moments) == 8 && offsetof(CrttHistory, geometry) == 16
              && offsetof(CrttHistory, instance) == 24 && offsetof(CrttHistory, camera) == 32, "CrttHistory");
static_assert(sizeof(CrttParams) == 24 && offsetof(CrttParams, normalCos) == 20 && sizeof(float4) == 16, "CrttParams");

struct CrttPass {
    const float4* color;            // cur
    const char* geometry;           // {n.x, n.y, n.z, t} at geometry + i * stride
    const char* instance;           // int32 at instance + i * stride; NULL when nobody asks for it
    const float4 *pColor, *pMoments, *pGeometry;   // prev; pColor == NULL: reset
    const int* pInstance;
    float4 *nColor, *nMoments, *nGeometry;         // next
    int* nInstance;
    int width, height;
    uint32_t flags;
    float alpha, momentsAlpha, maxHistory, depthTol, normalCos;
    float toRay[9], dpos[3], toScreen[9];          // cur's toRay, pos_cur - pos_prev, prev's toScreen
};

// 16-B rows as one vector load or store each (a float4 copied as a struct can be split into a 12-B copy through the stack and a float)
typedef float crtt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 crtt_load4(const void* p) { const crtt_f4 v = *(const crtt_f4*)p; return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void crtt_store4(float4* p, float4 v) { crtt_f4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; *(crtt_f4*)p = r; }

// the strides of the two guide layouts of cur: planes (16, 16 B) or CrtSurfaceHit records (48 B; geometry at 0, instance at 16)
template <bool SURFACE> __device__ __forceinline__ float4 crtt_geometry(const CrttPass& P, size_t i) { return crtt_load4(P.geometry + i * (SURFACE ? 48 : 16)); }
template <bool SURFACE> __device__ __forceinline__ int crtt_instance(const CrttPass& P, size_t i) { return *(const int*)(P.instance + i * (SURFACE ? 48 : 16)); }

__device__ __forceinline__ bool crtt_hit(float t) { return t <= 99998.0f; }
__device__ __forceinline__ float crtt_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
__device__ __forceinline__ float crtt_luma(float4 c) { return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z; }
__device__ __forceinline__ float crtt_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float crtt_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ bool crtt_finite(float v) { return __builtin_isfinite(v); }

// One frame. GATED: the taps' colour and moments are loaded only behind the geometry test (else with the geometry, unconditionally). STAGE: the
// workgroup stages cur's colour over its tile and a halo of 1 in LDS and CRTT_CLAMP takes its 3 x 3 pixels from there (else they are row reads
// through L1; launched only under CRTT_CLAMP). Every global load of a lane's round is issued before the first is waited for: round one is the
// pixel itself (and its neighbourhood), round two the four taps, whose addresses need round one's distance. Addresses are clamped into the
// frame; what must not count is chosen away afterwards.
template <bool SURFACE, bool GATED, bool STAGE>
__global__ __launch_bounds__(CRTT_BLOCK) void crtt_accumulate_kernel(CrttPass P)
{
    constexpr int TW = CRTT_TILE_W + 2, TH = CRTT_TILE_H + 2, N = TW * TH, ROUNDS = (N + CRTT_BLOCK - 1) / CRTT_BLOCK;
    __shared__ float4 s_tile[STAGE ? N : 1];
    const int W = P.width, H = P.height;
    const int lx = (int)(threadIdx.x & (CRTT_TILE_W - 1)), ly = (int)(threadIdx.x / CRTT_TILE_W);
    const int bx = (int)blockIdx.x * CRTT_TILE_W, by = (int)blockIdx.y * CRTT_TILE_H;
    const int x = bx + lx, y = by + ly;
    const bool mine = x < W && y < H;                 // a lane without a pixel reads the clamped one and stores nothing
    const bool match = (P.flags & CRTT_MATCH_INSTANCE) != 0, clampOn = (P.flags & CRTT_CLAMP) != 0;
    if (!STAGE && !mine) return;
    // (pixel indices fit 32 bits: 16384 x 16384 at most)
    const size_t ci = (size_t)(uint32_t)(min(y, H - 1) * W + min(x, W - 1));

    // ---- round one: the pixel, and the 3 x 3 pixels around it
    const float4 c = crtt_load4(P.color + ci);
    const float4 g = crtt_geometry<SURFACE>(P, ci);
    const int inst = P.instance ? crtt_instance<SURFACE>(P, ci) : 0;
    float4 nb[9];
    if (STAGE) {
        float4 st[ROUNDS];
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const int i = (int)threadIdx.x + j * CRTT_BLOCK, ty = i / TW, tx = i - ty * TW;
            st[j] = crtt_load4(P.color + (size_t)(uint32_t)(min(max(by - 1 + ty, 0), H - 1) * W + min(max(bx - 1 + tx, 0), W - 1)));
        }
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const int i = (int)threadIdx.x + j * CRTT_BLOCK;
            if (i < N) crtt_store4(s_tile + i, st[j]);
        }
        __syncthreads();
        if (!mine) return;
#pragma unroll
        for (int k = 0; k < 9; ++k) nb[k] = crtt_load4(s_tile + (ly + k / 3) * TW + lx + k % 3);
    } else if (clampOn) {
#pragma unroll
        for (int k = 0; k < 9; ++k)
            nb[k] = crtt_load4(P.color + (size_t)(uint32_t)(min(max(y - 1 + k / 3, 0), H - 1) * W + min(max(x - 1 + k % 3, 0), W - 1)));
    }

    const bool hit = crtt_hit(g.w);
    const float L = crtt_luma(c);
    crtt_store4(P.nGeometry + ci, g);
    if (P.nInstance) P.nInstance[ci] = inst;

    // ---- reprojection
    const float fxp = (float)x, fyp = (float)y;
    float dx_ = crtt_dot3(P.toRay[0], P.toRay[1], P.toRay[2], fxp, fyp, 1.0f);
    float dy_ = crtt_dot3(P.toRay[3], P.toRay[4], P.toRay[5], fxp, fyp, 1.0f);
    float dz_ = crtt_dot3(P.toRay[6], P.toRay[7], P.toRay[8], fxp, fyp, 1.0f);
    const float dl = sqrtf(crtt_dot3(dx_, dy_, dz_, dx_, dy_, dz_));
    dx_ = dx_ / dl; dy_ = dy_ / dl; dz_ = dz_ / dl;
    const float vx = P.dpos[0] + dx_ * g.w, vy = P.dpos[1] + dy_ * g.w, vz = P.dpos[2] + dz_ * g.w;
    const float dist = sqrtf(crtt_dot3(vx, vy, vz, vx, vy, vz));
    const float ux = crtt_dot3(P.toScreen[0], P.toScreen[1], P.toScreen[2], vx, vy, vz);
    const float uy = crtt_dot3(P.toScreen[3], P.toScreen[4], P.toScreen[5], vx, vy, vz);
    const float uz = crtt_dot3(P.toScreen[6], P.toScreen[7], P.toScreen[8], vx, vy, vz);
    const float fx = ux / uz, fy = uy / uz;
    const bool onScreen = uz > 0.0f && fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H;
    bool have = false;
    float hx = 0.0f, hy = 0.0f, hz = 0.0f, m1h = 0.0f, m2h = 0.0f, Nh = 0.0f;
    if (P.pColor && hit && onScreen) {
        // ---- round two: the four taps
        const float flx = floorf(fx), fly = floorf(fy), ax = fx - flx, ay = fy - fly;
        const int x0 = (int)flx, y0 = (int)fly;                                 // -1 .. W - 1, -1 .. H - 1
        const float dtol = P.depthTol * dist;
        size_t q[4]; int geo[4];                                // & on ints, not && on bools: straight-line code, as CrtdSum::tap
        float4 gq[4], cq[4], mq[4]; int iq[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
            geo[k] = (int)(qx >= 0 && qx < W && qy >= 0 && qy < H);
            q[k] = (size_t)(uint32_t)(min(max(qy, 0), H - 1) * W + min(max(qx, 0), W - 1));
            gq[k] = crtt_load4(P.pGeometry + q[k]);
            iq[k] = match ? P.pInstance[q[k]] : 0;
            if (!GATED) { cq[k] = crtt_load4(P.pColor + q[k]); mq[k] = crtt_load4(P.pMoments + q[k]); }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            geo[k] &= (int)crtt_hit(gq[k].w) & (int)(fabsf(gq[k].w - dist) <= dtol) & (int)(crtt_dot3(gq[k].x, gq[k].y, gq[k].z, g.x, g.y, g.z) >= P.normalCos)
                    & (int)(!match || iq[k] == inst);
        if (GATED) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                cq[k] = mq[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (geo[k]) { cq[k] = crtt_load4(P.pColor + q[k]); mq[k] = crtt_load4(P.pMoments + q[k]); }
            }
        }
        float sx = 0.0f, sy = 0.0f, sz = 0.0f, s1 = 0.0f, s2 = 0.0f, sN = 0.0f, ws = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ok = geo[k] & (int)(mq[k].z >= 1.0f) & (int)crtt_finite(cq[k].x) & (int)crtt_finite(cq[k].y) & (int)crtt_finite(cq[k].z)
                         & (int)crtt_finite(mq[k].x) & (int)crtt_finite(mq[k].y);
            const float b = ((k & 1) ? ax : 1.0f - ax) * ((k >> 1) ? ay : 1.0f - ay);
            // a tap that does not count is selected away, never multiplied by zero
            sx = ok ? sx + cq[k].x * b : sx; sy = ok ? sy + cq[k].y * b : sy; sz = ok ? sz + cq[k].z * b : sz;
            s1 = ok ? s1 + mq[k].x * b : s1; s2 = ok ? s2 + mq[k].y * b : s2; sN = ok ? sN + mq[k].z * b : sN;
            ws = ok ? ws + b : ws;
        }
        have = ws > 0.01f;
        hx = sx / ws; hy = sy / ws; hz = sz / ws; m1h = s1 / ws; m2h = s2 / ws; Nh = sN / ws;
    }
    float4 o = make_float4(c.x, c.y, c.z, c.w), m = make_float4(L, L * L, hit ? 1.0f : 0.0f, 0.0f);
    if (have) {
        if (clampOn) {
            const float inf = __builtin_inff();
            float mnx = inf, mny = inf, mnz = inf, mxx = -inf, mxy = -inf, mxz = -inf;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int qx = x - 1 + k % 3, qy = y - 1 + k / 3;
                if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
                    mnx = crtt_min(mnx, nb[k].x); mny = crtt_min(mny, nb[k].y); mnz = crtt_min(mnz, nb[k].z);
                    mxx = crtt_max(mxx, nb[k].x); mxy = crtt_max(mxy, nb[k].y); mxz = crtt_max(mxz, nb[k].z);
                }
            }
            hx = crtt_min(crtt_max(hx, mnx), mxx); hy = crtt_min(crtt_max(hy, mny), mxy); hz = crtt_min(crtt_max(hz, mnz), mxz);
        }
        const float Nn = fminf(Nh + 1.0f, P.maxHistory);
        const float a = fmaxf(P.alpha, 1.0f / Nn), am = fmaxf(P.momentsAlpha, 1.0f / Nn);
        o.x = hx * (1.0f - a) + c.x * a; o.y = hy * (1.0f - a) + c.y * a; o.z = hz * (1.0f - a) + c.z * a;
        m.x = m1h * (1.0f - am) + L * am;
        m.y = m2h * (1.0f - am) + (L * L) * am;
        m.z = Nn;
        const float var = m.y - m.x * m.x;
        m.w = var > 0.0f ? var : 0.0f;
    }
    crtt_store4(P.nColor + ci, o);
    crtt_store4(P.nMoments + ci, m);
}

template <bool SURFACE>
static void crtt_launch(const CrttPass& P, bool gated, bool stage, hipStream_t stream)
{
    const dim3 grid((unsigned)((P.width + CRTT_TILE_W - 1) / CRTT_TILE_W), (unsigned)((P.height + CRTT_TILE_H - 1) / CRTT_TILE_H));
    if (gated && stage) crtt_accumulate_kernel<SURFACE, true, true><<<grid, CRTT_BLOCK, 0, stream>>>(P);
    else if (gated) crtt_accumulate_kernel<SURFACE, true, false><<<grid, CRTT_BLOCK, 0, stream>>>(P);
    else if (stage) crtt_accumulate_kernel<SURFACE, false, true><<<grid, CRTT_BLOCK, 0, stream>>>(P);
    else crtt_accumulate_kernel<SURFACE, false, false><<<grid, CRTT_BLOCK, 0, stream>>>(P);
}

// the two measured choices: NAME=a|b in the environment (read by every call), else the measured default
static bool crtt_choice(const char* name, const char* off, const char* on, bool deflt)
{
    const char* e = getenv(name);
    if (e && !strcmp(e, on)) return true;
    if (e && !strcmp(e, off)) return false;
    return deflt;
}

static int crtt_check(const CrttFrame* cur, const CrttHistory* prev, const CrttHistory* next, const CrttParams* p)
{
    if (!cur || !next || !p || !cur->color || !cur->geometry) return CRTT_E_BAD_ARGUMENT;
    if (!next->color || !next->moments || !next->geometry) return CRTT_E_BAD_ARGUMENT;
    if (prev && (!prev->color || !prev->moments || !prev->geometry)) return CRTT_E_BAD_ARGUMENT;
    if (cur->width < 1 || cur->height < 1) return CRTT_E_BAD_ARGUMENT;
    if (p->flags & ~(uint32_t)(CRTT_MATCH_INSTANCE | CRTT_CLAMP)) return CRTT_E_BAD_ARGUMENT;
    const bool match = (p->flags & CRTT_MATCH_INSTANCE) != 0;
    if (cur->guides == CRTT_GUIDES_PLANES) {
        if ((match || next->instance) && !cur->ids) return CRTT_E_BAD_ARGUMENT;
    } else if (cur->guides == CRTT_GUIDES_SURFACE) {
        if (cur->ids) return CRTT_E_BAD_ARGUMENT;
    } else {
        return CRTT_E_BAD_ARGUMENT;
    }
    if (match && (!next->instance || (prev && !prev->instance))) return CRTT_E_BAD_ARGUMENT;
    if (!(p->alpha > 0.0f && p->alpha <= 1.0f) || !(p->momentsAlpha > 0.0f && p->momentsAlpha <= 1.0f)) return CRTT_E_BAD_ARGUMENT;
    if (!(p->maxHistory >= 1.0f) || !isfinite(p->maxHistory)) return CRTT_E_BAD_ARGUMENT;
    if (!(p->depthTol >= 0.0f) || !isfinite(p->normalCos)) return CRTT_E_BAD_ARGUMENT;
    const void* outs[4] = {next->color, next->moments, next->geometry, next->instance};
    const void* ins[7] = {cur->color, cur->geometry, cur->ids, prev ? prev->color : nullptr, prev ? prev->moments : nullptr,
                          prev ? prev->geometry : nullptr, prev ? prev->instance : nullptr};
    for (int i = 0; i < 4; ++i) {
        if (!outs[i]) continue;
        for (const void* in : ins)
            if (in == outs[i]) return CRTT_E_BAD_ARGUMENT;
        for (int j = 0; j < i; ++j)
            if (outs[j] == outs[i]) return CRTT_E_BAD_ARGUMENT;
    }
    if (cur->width > CRTT_MAX_DIM || cur->height > CRTT_MAX_DIM) return CRTT_E_OUT_OF_RANGE;
    return CRTT_OK;
}

extern "C" {

int crtt_camera(const float invView[16], const float invProj[16], const float pos[3], int32_t width, int32_t height, CrttCamera* out)
{
    if (!invView || !invProj || !pos || !out || width < 1 || height < 1) return CRTT_E_BAD_ARGUMENT;
    for (int i = 0; i < 16; ++i)
        if (!isfinite(invView[i]) || !isfinite(invProj[i])) return CRTT_E_BAD_ARGUMENT;
    for (int i = 0; i < 3; ++i)
        if (!isfinite(pos[i])) return CRTT_E_BAD_ARGUMENT;
    // the matrices are stored as RayGen reads them: element (row r, column c) at [4c + r]
    auto w_at = [&](double cx, double cy) { return ((double)invProj[3] * cx + (double)invProj[7] * cy) + ((double)invProj[11] + (double)invProj[15]); };
    const double wc = w_at(0.0, 0.0);
    if (wc == 0.0) return CRTT_E_BAD_ARGUMENT;
    for (int k = 0; k < 4; ++k) {
        const double w = w_at((k & 1) ? 1.0 : -1.0, (k >> 1) ? 1.0 : -1.0);
        if (!((w > 0.0) == (wc > 0.0)) || w == 0.0) return CRTT_E_BAD_ARGUMENT;
    }
    const double sign = wc > 0.0 ? 1.0 : -1.0;
    double M[3][3], R[3][3], I[3][3];
    for (int r = 0; r < 3; ++r) {
        double A[4];
        for (int c = 0; c < 4; ++c) {
            A[c] = 0.0;
            for (int k = 0; k < 4; ++k) A[c] += (double)invView[4 * k + r] * (double)invProj[4 * c + k];
        }
        M[r][0] = A[0]; M[r][1] = A[1]; M[r][2] = A[2] + A[3];
        R[r][0] = sign * (M[r][0] * (2.0 / (double)width));
        R[r][1] = sign * (M[r][1] * (2.0 / (double)height));
        R[r][2] = sign * (M[r][2] - M[r][0] - M[r][1]);
    }
    const double c00 = R[1][1] * R[2][2] - R[1][2] * R[2][1], c01 = R[1][2] * R[2][0] - R[1][0] * R[2][2], c02 = R[1][0] * R[2][1] - R[1][1] * R[2][0];
    const double det = R[0][0] * c00 + R[0][1] * c01 + R[0][2] * c02;
    double scale = 1.0;
    for (int r = 0; r < 3; ++r) scale *= sqrt(R[r][0] * R[r][0] + R[r][1] * R[r][1] + R[r][2] * R[r][2]);
    if (!isfinite(det) || !isfinite(scale) || !(fabs(det) > 1e-12 * scale)) return CRTT_E_BAD_ARGUMENT;     // singular: the rows span no volume
    I[0][0] = c00 / det; I[1][0] = c01 / det; I[2][0] = c02 / det;
    I[0][1] = (R[0][2] * R[2][1] - R[0][1] * R[2][2]) / det; I[1][1] = (R[0][0] * R[2][2] - R[0][2] * R[2][0]) / det; I[2][1] = (R[0][1] * R[2][0] - R[0][0] * R[2][1]) / det;
    I[0][2] = (R[0][1] * R[1][2] - R[0][2] * R[1][1]) / det; I[1][2] = (R[0][2] * R[1][0] - R[0][0] * R[1][2]) / det; I[2][2] = (R[0][0] * R[1][1] - R[0][1] * R[1][0]) / det;
    CrttCamera cam;
    for (int r = 0; r < 3; ++r) {
        cam.pos[r] = pos[r];
        for (int c = 0; c < 3; ++c) {
            cam.toRay[3 * r + c] = (float)R[r][c];
            cam.toScreen[3 * r + c] = (float)I[r][c];
            if (!isfinite(cam.toRay[3 * r + c]) || !isfinite(cam.toScreen[3 * r + c])) return CRTT_E_BAD_ARGUMENT;
        }
    }
    *out = cam;
    return CRTT_OK;
}

size_t crtt_history_bytes(int32_t width, int32_t height, int plane)
{
    if (width < 1 || height < 1 || plane < CRTT_PLANE_COLOR || plane > CRTT_PLANE_INSTANCE) return 0;
    return (size_t)width * (size_t)height * (plane == CRTT_PLANE_INSTANCE ? sizeof(int32_t) : sizeof(float4));
}

int crtt_accumulate(const CrttFrame* cur, const CrttHistory* prev, const CrttHistory* next, const CrttParams* p, void* stream)
{
    const int rc = crtt_check(cur, prev, next, p);
    if (rc != CRTT_OK) return rc;
    const bool surface = cur->guides == CRTT_GUIDES_SURFACE, match = (p->flags & CRTT_MATCH_INSTANCE) != 0;
    const char* g = (const char*)cur->geometry;
    CrttPass P;
    P.color = (const float4*)cur->color;
    P.geometry = g;
    P.instance = !(match || next->instance) ? nullptr : surface ? g + 16 : (const char*)cur->ids;
    P.pColor = prev ? (const float4*)prev->color : nullptr;
    P.pMoments = prev ? (const float4*)prev->moments : nullptr;
    P.pGeometry = prev ? (const float4*)prev->geometry : nullptr;
    P.pInstance = prev && match ? (const int*)prev->instance : nullptr;
    P.nColor = (float4*)next->color; P.nMoments = (float4*)next->moments; P.nGeometry = (float4*)next->geometry; P.nInstance = (int*)next->instance;
    P.width = cur->width; P.height = cur->height;
    P.flags = p->flags;
    P.alpha = p->alpha; P.momentsAlpha = p->momentsAlpha; P.maxHistory = p->maxHistory; P.depthTol = p->depthTol; P.normalCos = p->normalCos;
    for (int i = 0; i < 9; ++i) { P.toRay[i] = cur->camera.toRay[i]; P.toScreen[i] = prev ? prev->camera.toScreen[i] : 0.0f; }
    for (int i = 0; i < 3; ++i) P.dpos[i] = prev ? cur->camera.pos[i] - prev->camera.pos[i] : 0.0f;
    const bool gated = crtt_choice("CRTT_TAPS", "all", "gated", CRTT_TAPS_GATED_DEFAULT != 0);
    const bool stage = (p->flags & CRTT_CLAMP) && crtt_choice("CRTT_CLAMP_TAPS", "l1", "lds", CRTT_CLAMP_LDS_DEFAULT != 0);
    if (surface) crtt_launch<true>(P, gated, stage, (hipStream_t)stream);
    else crtt_launch<false>(P, gated, stage, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : CRTT_OK;
}

const char* crtt_error_string(int rc)
{
    switch (rc) {
    case CRTT_OK: return "ok";
    case CRTT_E_BAD_ARGUMENT: return "crtt: bad argument";
    case CRTT_E_OUT_OF_RANGE: return "crtt: out of range (a frame wider or taller than 16384)";
    default: return rc > 0 ? hipGetErrorString((hipError_t)rc) : "crtt: unknown error";
    }
}

}
