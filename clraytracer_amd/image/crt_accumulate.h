// crt_accumulate.h -- the accumulate kernel of libcrt_temporal.so and libcrt_motion.so (definitions: include/crt_temporal.h, include/crt_motion.h),
// its two pass structs, the argument check both C ABIs open with and the fill of the fields both passes have. The kernel is a template over the
// pass type, so each library instantiates kernels of its own from one body (DESIGN.md 4p says why it is no inlined function). Headers only.
#pragma once
#include "../../include/crt_motion.h"      // (includes crt_temporal.h)
#include "crt_image_host.h"

#define CRT_ACCUMULATE_HALO 1       // the staged tile of CRTT_CLAMP: (CRTI_TILE_W + 2) x (CRTI_TILE_H + 2) float4 in LDS, the clamp's 3 x 3 pixels

// The kernel arguments; their field order is the kernels' argument layout.
struct CrttPass {
    static constexpr bool motion = false;
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

struct CrtmPass {
    static constexpr bool motion = true;
    const float4* color;            // cur
    const char* geometry;           // {n.x, n.y, n.z, t} at geometry + i * stride
    const char* instance;           // int32 at instance + i * stride; NULL when nobody asks for it (then there is no table either)
    const float4 *pColor, *pMoments, *pGeometry;   // prev; pColor == NULL: reset
    const int* pInstance;
    float4 *nColor, *nMoments, *nGeometry;         // next
    int* nInstance;
    const CrtmMotion* table;        // NULL: every pixel is CRTM_STATIC
    float4* vectors;                // NULL: not asked for
    int width, height;
    uint32_t flags, count;
    float alpha, momentsAlpha, maxHistory, depthTol, normalCos;
    float toRay[9], dpos[3], pos[3], ppos[3], toScreen[9];   // cur's toRay, pos_cur - pos_prev, pos_cur, pos_prev, prev's toScreen
};

__device__ __forceinline__ float crti_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float crti_max(float a, float b) { return a > b ? a : b; }

// A moving lane's reprojection (crt_motion.h): v and the normal its taps are tested against, through the record at r
__device__ __forceinline__ void crtm_through(const CrtmMotion* r, const CrtmPass& P, float Px, float Py, float Pz, const float4& g,
                                             float& vx, float& vy, float& vz, float& nx, float& ny, float& nz)
{
    float pt[12], nr[9];
#pragma unroll
    for (int k = 0; k < 12; ++k) pt[k] = r->point[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) nr[k] = r->normal[k];
    vx = (crti_dot3(pt[0], pt[1], pt[2], Px, Py, Pz) + pt[3]) - P.ppos[0];
    vy = (crti_dot3(pt[4], pt[5], pt[6], Px, Py, Pz) + pt[7]) - P.ppos[1];
    vz = (crti_dot3(pt[8], pt[9], pt[10], Px, Py, Pz) + pt[11]) - P.ppos[2];
    const float mx = crti_dot3(nr[0], nr[1], nr[2], g.x, g.y, g.z), my = crti_dot3(nr[3], nr[4], nr[5], g.x, g.y, g.z),
                mz = crti_dot3(nr[6], nr[7], nr[8], g.x, g.y, g.z);
    const float ml = sqrtf(crti_dot3(mx, my, mz, mx, my, mz));
    nx = mx / ml; ny = my / ml; nz = mz / ml;
}

// One frame. GATED: the taps' colour and moments are loaded only behind the geometry test (else with the geometry, unconditionally). STAGE: the
// workgroup stages cur's colour over its tile and a halo of 1 in LDS and CRTT_CLAMP takes its 3 x 3 pixels from there (else they are row reads
// through L1). Under a CrttPass the clamp is the runtime flag; a CrtmPass is launched with STAGE exactly under CRTT_CLAMP, and always GATED.
// Every global load of a lane's round is issued before the first is waited for: round one is the pixel itself, its neighbourhood and -- under a
// CrtmPass, behind the instance id -- the `kind` of its motion record, whose matrices are loaded, and their arithmetic done, only in a wave that
// has a moving lane; round two is the four taps, whose addresses need round one's distance. Addresses are clamped into the frame and the record
// index is used only when it lies below `count`; what must not count is chosen away afterwards.
template <class PASS, bool SURFACE, bool GATED, bool STAGE>
__global__ __launch_bounds__(CRTI_BLOCK) void crt_accumulate_kernel(PASS P)
{
    using Tile = CrtiTile<CRT_ACCUMULATE_HALO, true>;
    constexpr int TW = Tile::TW, N = Tile::N, ROUNDS = Tile::ROUNDS;
    __shared__ float4 s_tile[STAGE ? N : 1];
    const int W = P.width, H = P.height;
    const CrtiLane lane;
    const int lx = lane.lx, ly = lane.ly, bx = lane.x0, by = lane.y0, x = lane.x, y = lane.y;
    const bool mine = x < W && y < H;                 // a lane without a pixel reads the clamped one and stores nothing
    const bool match = (P.flags & CRTT_MATCH_INSTANCE) != 0, clampOn = PASS::motion ? STAGE : (P.flags & CRTT_CLAMP) != 0;
    if (!STAGE && !mine) return;
    const size_t ci = crti_clamped_own(x, y, W, H);

    // ---- round one: the pixel, the 3 x 3 pixels around it, and what its instance's record says
    const float4 c = crti_load4(P.color + ci);
    const float4 g = crti_geometry<SURFACE>(P, ci);
    const int inst = P.instance ? crti_instance<SURFACE>(P, ci) : 0;
    [[maybe_unused]] const CrtmMotion* rec = nullptr;
    [[maybe_unused]] uint32_t kind = (uint32_t)CRTM_STATIC;
    if constexpr (PASS::motion) {
        const bool listed = P.table && (uint32_t)inst < P.count;  // an id < 0 or >= count: CRTM_STATIC
        rec = P.table + (listed ? inst : 0);
        kind = listed ? rec->kind : (uint32_t)CRTM_STATIC;
    }
    float4 nb[9];
    if (STAGE) {
        float4 st[ROUNDS];
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) st[j] = crti_load4(P.color + Tile(j, bx, by).clamped(W, H));
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const int i = Tile(j, bx, by).i;
            if (i < N) crti_store4(s_tile + i, st[j]);
        }
        __syncthreads();
        if (!mine) return;
#pragma unroll
        for (int k = 0; k < 9; ++k) nb[k] = crti_load4(s_tile + (ly + k / 3) * TW + lx + k % 3);
    } else if (clampOn) {
#pragma unroll
        for (int k = 0; k < 9; ++k) nb[k] = crti_load4(P.color + crti_clamped(x - 1 + k % 3, y - 1 + k / 3, W, H));
    }

    const bool hit = crti_hit(g.w);
    const float L = crti_luma(c);
    crti_store4(P.nGeometry + ci, g);
    if (P.nInstance) P.nInstance[ci] = inst;

    // ---- reprojection
    const float fxp = (float)x, fyp = (float)y;
    float dx_ = crti_dot3(P.toRay[0], P.toRay[1], P.toRay[2], fxp, fyp, 1.0f);
    float dy_ = crti_dot3(P.toRay[3], P.toRay[4], P.toRay[5], fxp, fyp, 1.0f);
    float dz_ = crti_dot3(P.toRay[6], P.toRay[7], P.toRay[8], fxp, fyp, 1.0f);
    const float dl = sqrtf(crti_dot3(dx_, dy_, dz_, dx_, dy_, dz_));
    dx_ = dx_ / dl; dy_ = dy_ / dl; dz_ = dz_ / dl;
    float vx = P.dpos[0] + dx_ * g.w, vy = P.dpos[1] + dy_ * g.w, vz = P.dpos[2] + dz_ * g.w;
    float nx = g.x, ny = g.y, nz = g.z;               // the normal the taps' normals are tested against
    bool wanted = P.pColor && hit;
    if constexpr (PASS::motion) {
        wanted = wanted && kind != (uint32_t)CRTM_NEW;
        const bool moving = wanted && kind == (uint32_t)CRTM_MOVING;
        const float Px = P.pos[0] + dx_ * g.w, Py = P.pos[1] + dy_ * g.w, Pz = P.pos[2] + dz_ * g.w;
        if (__ballot(moving) != 0) {                  // a wave without a moving lane neither loads a matrix nor multiplies by one
            if (moving) crtm_through(rec, P, Px, Py, Pz, g, vx, vy, vz, nx, ny, nz);
        }
    }
    const float dist = sqrtf(crti_dot3(vx, vy, vz, vx, vy, vz));
    const float ux = crti_dot3(P.toScreen[0], P.toScreen[1], P.toScreen[2], vx, vy, vz);
    const float uy = crti_dot3(P.toScreen[3], P.toScreen[4], P.toScreen[5], vx, vy, vz);
    const float uz = crti_dot3(P.toScreen[6], P.toScreen[7], P.toScreen[8], vx, vy, vz);
    const float fx = ux / uz, fy = uy / uz;
    const bool onScreen = uz > 0.0f && fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H;
    bool have = false;
    float hx = 0.0f, hy = 0.0f, hz = 0.0f, m1h = 0.0f, m2h = 0.0f, Nh = 0.0f;
    if (wanted && onScreen) {
        // ---- round two: the four taps
        const float flx = floorf(fx), fly = floorf(fy), ax = fx - flx, ay = fy - fly;
        const int x0 = (int)flx, y0 = (int)fly;                                 // -1 .. W - 1, -1 .. H - 1
        const float dtol = P.depthTol * dist;
        size_t q[4]; int geo[4];                                // & on ints, not && on bools: straight-line code, as CrtdSum::tap
        float4 gq[4], cq[4], mq[4]; int iq[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
            geo[k] = (int)CRTI_INSIDE(qx, qy, W, H);
            q[k] = crti_clamped(qx, qy, W, H);
            gq[k] = crti_load4(P.pGeometry + q[k]);
            iq[k] = match ? P.pInstance[q[k]] : 0;
            if (!GATED) { cq[k] = crti_load4(P.pColor + q[k]); mq[k] = crti_load4(P.pMoments + q[k]); }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            geo[k] &= (int)crti_hit(gq[k].w) & (int)(fabsf(gq[k].w - dist) <= dtol) & (int)(crti_dot3(gq[k].x, gq[k].y, gq[k].z, nx, ny, nz) >= P.normalCos)
                    & (int)(!match || iq[k] == inst);
        if (GATED) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                cq[k] = mq[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (geo[k]) { cq[k] = crti_load4(P.pColor + q[k]); mq[k] = crti_load4(P.pMoments + q[k]); }
            }
        }
        float sx = 0.0f, sy = 0.0f, sz = 0.0f, s1 = 0.0f, s2 = 0.0f, sN = 0.0f, ws = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ok = geo[k] & (int)(mq[k].z >= 1.0f) & (int)crti_finite(cq[k].x) & (int)crti_finite(cq[k].y) & (int)crti_finite(cq[k].z)
                         & (int)crti_finite(mq[k].x) & (int)crti_finite(mq[k].y);
            const float b = ((k & 1) ? ax : 1.0f - ax) * ((k >> 1) ? ay : 1.0f - ay);
            // a tap that does not count is selected away, never multiplied by zero
            sx = ok ? sx + cq[k].x * b : sx; sy = ok ? sy + cq[k].y * b : sy; sz = ok ? sz + cq[k].z * b : sz;
            s1 = ok ? s1 + mq[k].x * b : s1; s2 = ok ? s2 + mq[k].y * b : s2; sN = ok ? sN + mq[k].z * b : sN;
            ws = ok ? ws + b : ws;
        }
        have = ws > 0.01f;
        hx = sx / ws; hy = sy / ws; hz = sz / ws; m1h = s1 / ws; m2h = s2 / ws; Nh = sN / ws;
    }
    if constexpr (PASS::motion) {
        if (P.vectors) {
            float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (wanted && onScreen) mv = make_float4(fx - fxp, fy - fyp, dist, have ? 2.0f : 1.0f);
            crti_store4(P.vectors + ci, mv);
        }
    }
    float4 o = make_float4(c.x, c.y, c.z, c.w), m = make_float4(L, L * L, hit ? 1.0f : 0.0f, 0.0f);
    if (have) {
        if (clampOn) {
            const float inf = __builtin_inff();
            float mnx = inf, mny = inf, mnz = inf, mxx = -inf, mxy = -inf, mxz = -inf;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int qx = x - 1 + k % 3, qy = y - 1 + k / 3;
                if (CRTI_INSIDE(qx, qy, W, H)) {
                    mnx = crti_min(mnx, nb[k].x); mny = crti_min(mny, nb[k].y); mnz = crti_min(mnz, nb[k].z);
                    mxx = crti_max(mxx, nb[k].x); mxy = crti_max(mxy, nb[k].y); mxz = crti_max(mxz, nb[k].z);
                }
            }
            hx = crti_min(crti_max(hx, mnx), mxx); hy = crti_min(crti_max(hy, mny), mxy); hz = crti_min(crti_max(hz, mnz), mxz);
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
    crti_store4(P.nColor + ci, o);
    crti_store4(P.nMoments + ci, m);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
// the planes a call reads and the planes it writes, for the alias rule
struct CrtAccumulatePlanes { const void *ins[7], *outs[4]; };
static inline CrtAccumulatePlanes crt_accumulate_planes(const CrttFrame* cur, const CrttHistory* prev, const CrttHistory* next)
{
    return {{cur->color, cur->geometry, cur->ids, prev ? prev->color : nullptr, prev ? prev->moments : nullptr, prev ? prev->geometry : nullptr,
             prev ? prev->instance : nullptr}, {next->color, next->moments, next->geometry, next->instance}};
}

// The refusals of crtt_accumulate, which are crtm_accumulate's first: every CRTT_E_BAD_ARGUMENT in the header's order, then CRTT_E_OUT_OF_RANGE.
// (A caller with refusals of its own returns a CRTT_E_BAD_ARGUMENT at once and any other answer after them.)
static inline int crt_accumulate_check(const CrttFrame* cur, const CrttHistory* prev, const CrttHistory* next, const CrttParams* p)
{
    if (!cur || !next || !p || !cur->color || !cur->geometry) return CRTT_E_BAD_ARGUMENT;
    if (!next->color || !next->moments || !next->geometry) return CRTT_E_BAD_ARGUMENT;
    if (prev && (!prev->color || !prev->moments || !prev->geometry)) return CRTT_E_BAD_ARGUMENT;
    if (cur->width < 1 || cur->height < 1) return CRTT_E_BAD_ARGUMENT;
    if (p->flags & ~(uint32_t)(CRTT_MATCH_INSTANCE | CRTT_CLAMP)) return CRTT_E_BAD_ARGUMENT;
    const bool match = (p->flags & CRTT_MATCH_INSTANCE) != 0;
    if (!crti_guides_ok(cur->guides, match || next->instance, cur->ids, false, nullptr)) return CRTT_E_BAD_ARGUMENT;
    if (match && (!next->instance || (prev && !prev->instance))) return CRTT_E_BAD_ARGUMENT;
    if (!(p->alpha > 0.0f && p->alpha <= 1.0f) || !(p->momentsAlpha > 0.0f && p->momentsAlpha <= 1.0f)) return CRTT_E_BAD_ARGUMENT;
    if (!(p->maxHistory >= 1.0f) || !isfinite(p->maxHistory)) return CRTT_E_BAD_ARGUMENT;
    if (!(p->depthTol >= 0.0f) || !isfinite(p->normalCos)) return CRTT_E_BAD_ARGUMENT;
    const CrtAccumulatePlanes planes = crt_accumulate_planes(cur, prev, next);
    if (crti_aliased(planes.ins, planes.outs)) return CRTT_E_BAD_ARGUMENT;
    if (cur->width > CRTI_MAX_DIM || cur->height > CRTI_MAX_DIM) return CRTT_E_OUT_OF_RANGE;
    return CRTT_OK;
}

// the fields both passes have; wantIds: does anybody ask for cur's instance ids?
template <class PASS>
static inline void crt_accumulate_fill(PASS& P, const CrttFrame* cur, const CrttHistory* prev, const CrttHistory* next, const CrttParams* p, bool wantIds)
{
    const bool surface = cur->guides == CRTT_GUIDES_SURFACE, match = (p->flags & CRTT_MATCH_INSTANCE) != 0;
    const char* g = (const char*)cur->geometry;
    P.color = (const float4*)cur->color;
    P.geometry = g;
    P.instance = !wantIds ? nullptr : surface ? g + 16 : (const char*)cur->ids;
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
}
