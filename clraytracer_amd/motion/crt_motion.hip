// crt_motion.hip -- libcrt_motion.so: temporal accumulation that reprojects through each instance's own motion (include/crt_motion.h, definition
// there), its kernel, the host-only motion records and the C ABI over them. The only translation unit of the library; it shares no state and no
// source with the others: the blend of crt_temporal.h is restated here, and tests/test_gpu_motion.py ties the two libraries bit for bit.
// Build: the Makefile's $(MOTION_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <string.h>
#include "../../include/crt_motion.h"

#define CRTM_TILE_W 32              // 256 lanes over a 32 x 8 tile, as crtt_accumulate_kernel
#define CRTM_TILE_H 8
#define CRTM_HALO 1                 // the staged tile of CRTT_CLAMP: (CRTM_TILE_W + 2 * CRTM_HALO) x (CRTM_TILE_H + 2 * CRTM_HALO) float4 in LDS
#define CRTM_TABLE_LDS 0            // bytes of the motion table staged in LDS: none, the records come through L1
#define CRTM_BLOCK (CRTM_TILE_W * CRTM_TILE_H)
// Dynamic LDS the unstaged kernels are launched with and never touch: at 54-56 VGPRs they would run 8 waves per SIMD, where the taps' gathers
// of a dense frame take 7 % longer than at 5; 28 KiB per workgroup holds a CU's 160 KiB to 5 workgroups of 4 waves, the staged
// kernels' occupancy and crtt_accumulate_kernel's
#define CRTM_UNSTAGED_PAD 28672
#define CRTM_MAX_DIM 16384
#define CRTM_INSTANCE_STRIDE 80     // sizeof(CrtMeshInstance) (crt_types.h), the matrix first
// the ABI of crt_motion.h (clraytracer_amd/_lib.py mirrors it), and what it takes from crt_temporal.h
static_assert(sizeof(CrtmMotion) == 88 && alignof(CrtmMotion) == 4 && offsetof(CrtmMotion, point) == 4 && offsetof(CrtmMotion, normal) == 52, "CrtmMotion");
static_assert(sizeof(CrtmMotionArgs) == 24 && offsetof(CrtmMotionArgs, count) == 8 && offsetof(CrtmMotionArgs, vectors) == 16, "CrtmMotionArgs");
static_assert(sizeof(CrttCamera) == 84 && sizeof(CrttFrame) == 128 && sizeof(CrttHistory) == 120 && sizeof(CrttParams) == 24 && sizeof(float4) == 16, "crt_temporal.h");

struct CrtmPass {
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

// 16-B rows as one vector load or store each
typedef float crtm_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 crtm_load4(const void* p) { const crtm_f4 v = *(const crtm_f4*)p; return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void crtm_store4(float4* p, float4 v) { crtm_f4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; *(crtm_f4*)p = r; }

// the strides of the two guide layouts of cur: planes (16, 16 B) or CrtSurfaceHit records (48 B; geometry at 0, instance at 16)
template <bool SURFACE> __device__ __forceinline__ float4 crtm_geometry(const CrtmPass& P, size_t i) { return crtm_load4(P.geometry + i * (SURFACE ? 48 : 16)); }
template <bool SURFACE> __device__ __forceinline__ int crtm_instance(const CrtmPass& P, size_t i) { return *(const int*)(P.instance + i * (SURFACE ? 48 : 16)); }

__device__ __forceinline__ bool crtm_hit(float t) { return t <= 99998.0f; }
__device__ __forceinline__ float crtm_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
__device__ __forceinline__ float crtm_luma(float4 c) { return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z; }
__device__ __forceinline__ float crtm_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float crtm_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ bool crtm_finite(float v) { return __builtin_isfinite(v); }

// A moving lane's reprojection (crt_motion.h): v and the normal its taps are tested against, through the record at r
__device__ __forceinline__ void crtm_through(const CrtmMotion* r, const CrtmPass& P, float Px, float Py, float Pz, const float4& g,
                                             float& vx, float& vy, float& vz, float& nx, float& ny, float& nz)
{
    float pt[12], nr[9];
#pragma unroll
    for (int k = 0; k < 12; ++k) pt[k] = r->point[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) nr[k] = r->normal[k];
    vx = (crtm_dot3(pt[0], pt[1], pt[2], Px, Py, Pz) + pt[3]) - P.ppos[0];
    vy = (crtm_dot3(pt[4], pt[5], pt[6], Px, Py, Pz) + pt[7]) - P.ppos[1];
    vz = (crtm_dot3(pt[8], pt[9], pt[10], Px, Py, Pz) + pt[11]) - P.ppos[2];
    const float mx = crtm_dot3(nr[0], nr[1], nr[2], g.x, g.y, g.z), my = crtm_dot3(nr[3], nr[4], nr[5], g.x, g.y, g.z),
                mz = crtm_dot3(nr[6], nr[7], nr[8], g.x, g.y, g.z);
    const float ml = sqrtf(crtm_dot3(mx, my, mz, mx, my, mz));
    nx = mx / ml; ny = my / ml; nz = mz / ml;
}

// One frame. The taps' colour and moments are loaded only behind the geometry test. STAGE (launched exactly under CRTT_CLAMP): the workgroup stages
// cur's colour over its tile and a halo of 1 in LDS and the clamp takes its 3 x 3 pixels from there. Round one is the pixel itself, its
// neighbourhood and -- behind the instance id -- the `kind` of its motion record; the record's matrices are loaded, and their arithmetic done,
// only in a wave that has a moving lane. Round two is the four taps, whose addresses need round one's distance. Addresses are clamped into the
// frame and the record index is used only when it lies below `count`; what must not count is chosen away afterwards.
template <bool SURFACE, bool STAGE>
__global__ __launch_bounds__(CRTM_BLOCK) void crtm_accumulate_kernel(CrtmPass P)
{
    constexpr int TW = CRTM_TILE_W + 2 * CRTM_HALO, TH = CRTM_TILE_H + 2 * CRTM_HALO, N = TW * TH, ROUNDS = (N + CRTM_BLOCK - 1) / CRTM_BLOCK;
    __shared__ float4 s_tile[STAGE ? N : 1];
    const int W = P.width, H = P.height;
    const int lx = (int)(threadIdx.x & (CRTM_TILE_W - 1)), ly = (int)(threadIdx.x / CRTM_TILE_W);
    const int bx = (int)blockIdx.x * CRTM_TILE_W, by = (int)blockIdx.y * CRTM_TILE_H;
    const int x = bx + lx, y = by + ly;
    const bool mine = x < W && y < H;                 // a lane without a pixel reads the clamped one and stores nothing
    const bool match = (P.flags & CRTT_MATCH_INSTANCE) != 0;
    if (!STAGE && !mine) return;
    // (pixel indices fit 32 bits: 16384 x 16384 at most)
    const size_t ci = (size_t)(uint32_t)(min(y, H - 1) * W + min(x, W - 1));

    // ---- round one: the pixel, the 3 x 3 pixels around it, and what its instance's record says
    const float4 c = crtm_load4(P.color + ci);
    const float4 g = crtm_geometry<SURFACE>(P, ci);
    const int inst = P.instance ? crtm_instance<SURFACE>(P, ci) : 0;
    const bool listed = P.table && (uint32_t)inst < P.count;      // an id < 0 or >= count: CRTM_STATIC
    const CrtmMotion* rec = P.table + (listed ? inst : 0);
    const uint32_t kind = listed ? rec->kind : (uint32_t)CRTM_STATIC;
    float4 nb[9];
    if (STAGE) {
        float4 st[ROUNDS];
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const int i = (int)threadIdx.x + j * CRTM_BLOCK, ty = i / TW, tx = i - ty * TW;
            st[j] = crtm_load4(P.color + (size_t)(uint32_t)(min(max(by - CRTM_HALO + ty, 0), H - 1) * W + min(max(bx - CRTM_HALO + tx, 0), W - 1)));
        }
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const int i = (int)threadIdx.x + j * CRTM_BLOCK;
            if (i < N) crtm_store4(s_tile + i, st[j]);
        }
        __syncthreads();
        if (!mine) return;
#pragma unroll
        for (int k = 0; k < 9; ++k) nb[k] = crtm_load4(s_tile + (ly + k / 3) * TW + lx + k % 3);
    }

    const bool hit = crtm_hit(g.w);
    const float L = crtm_luma(c);
    crtm_store4(P.nGeometry + ci, g);
    if (P.nInstance) P.nInstance[ci] = inst;

    // ---- reprojection
    const float fxp = (float)x, fyp = (float)y;
    float dx_ = crtm_dot3(P.toRay[0], P.toRay[1], P.toRay[2], fxp, fyp, 1.0f);
    float dy_ = crtm_dot3(P.toRay[3], P.toRay[4], P.toRay[5], fxp, fyp, 1.0f);
    float dz_ = crtm_dot3(P.toRay[6], P.toRay[7], P.toRay[8], fxp, fyp, 1.0f);
    const float dl = sqrtf(crtm_dot3(dx_, dy_, dz_, dx_, dy_, dz_));
    dx_ = dx_ / dl; dy_ = dy_ / dl; dz_ = dz_ / dl;
    float vx = P.dpos[0] + dx_ * g.w, vy = P.dpos[1] + dy_ * g.w, vz = P.dpos[2] + dz_ * g.w;
    float nx = g.x, ny = g.y, nz = g.z;               // the normal the taps' normals are tested against
    const bool wanted = P.pColor && hit && kind != (uint32_t)CRTM_NEW;
    const bool moving = wanted && kind == (uint32_t)CRTM_MOVING;
    const float Px = P.pos[0] + dx_ * g.w, Py = P.pos[1] + dy_ * g.w, Pz = P.pos[2] + dz_ * g.w;
    if (__ballot(moving) != 0) {                      // a wave without a moving lane neither loads a matrix nor multiplies by one
        if (moving) crtm_through(rec, P, Px, Py, Pz, g, vx, vy, vz, nx, ny, nz);
    }
    const float dist = sqrtf(crtm_dot3(vx, vy, vz, vx, vy, vz));
    const float ux = crtm_dot3(P.toScreen[0], P.toScreen[1], P.toScreen[2], vx, vy, vz);
    const float uy = crtm_dot3(P.toScreen[3], P.toScreen[4], P.toScreen[5], vx, vy, vz);
    const float uz = crtm_dot3(P.toScreen[6], P.toScreen[7], P.toScreen[8], vx, vy, vz);
    const float fx = ux / uz, fy = uy / uz;
    const bool onScreen = uz > 0.0f && fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H;
    bool have = false;
    float hx = 0.0f, hy = 0.0f, hz = 0.0f, m1h = 0.0f, m2h = 0.0f, Nh = 0.0f;
    if (wanted && onScreen) {
        // ---- round two: the four taps
        const float flx = floorf(fx), fly = floorf(fy), ax = fx - flx, ay = fy - fly;
        const int x0 = (int)flx, y0 = (int)fly;                                 // -1 .. W - 1, -1 .. H - 1
        const float dtol = P.depthTol * dist;
        size_t q[4]; int geo[4];                                // & on ints, not && on bools: straight-line code
        float4 gq[4], cq[4], mq[4]; int iq[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
            geo[k] = (int)(qx >= 0 && qx < W && qy >= 0 && qy < H);
            q[k] = (size_t)(uint32_t)(min(max(qy, 0), H - 1) * W + min(max(qx, 0), W - 1));
            gq[k] = crtm_load4(P.pGeometry + q[k]);
            iq[k] = match ? P.pInstance[q[k]] : 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            geo[k] &= (int)crtm_hit(gq[k].w) & (int)(fabsf(gq[k].w - dist) <= dtol) & (int)(crtm_dot3(gq[k].x, gq[k].y, gq[k].z, nx, ny, nz) >= P.normalCos)
                    & (int)(!match || iq[k] == inst);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            cq[k] = mq[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (geo[k]) { cq[k] = crtm_load4(P.pColor + q[k]); mq[k] = crtm_load4(P.pMoments + q[k]); }
        }
        float sx = 0.0f, sy = 0.0f, sz = 0.0f, s1 = 0.0f, s2 = 0.0f, sN = 0.0f, ws = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ok = geo[k] & (int)(mq[k].z >= 1.0f) & (int)crtm_finite(cq[k].x) & (int)crtm_finite(cq[k].y) & (int)crtm_finite(cq[k].z)
                         & (int)crtm_finite(mq[k].x) & (int)crtm_finite(mq[k].y);
            const float b = ((k & 1) ? ax : 1.0f - ax) * ((k >> 1) ? ay : 1.0f - ay);
            // a tap that does not count is selected away, never multiplied by zero
            sx = ok ? sx + cq[k].x * b : sx; sy = ok ? sy + cq[k].y * b : sy; sz = ok ? sz + cq[k].z * b : sz;
            s1 = ok ? s1 + mq[k].x * b : s1; s2 = ok ? s2 + mq[k].y * b : s2; sN = ok ? sN + mq[k].z * b : sN;
            ws = ok ? ws + b : ws;
        }
        have = ws > 0.01f;
        hx = sx / ws; hy = sy / ws; hz = sz / ws; m1h = s1 / ws; m2h = s2 / ws; Nh = sN / ws;
    }
    if (P.vectors) {
        float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (wanted && onScreen) mv = make_float4(fx - fxp, fy - fyp, dist, have ? 2.0f : 1.0f);
        crtm_store4(P.vectors + ci, mv);
    }
    float4 o = make_float4(c.x, c.y, c.z, c.w), m = make_float4(L, L * L, hit ? 1.0f : 0.0f, 0.0f);
    if (have) {
        if (STAGE) {
            const float inf = __builtin_inff();
            float mnx = inf, mny = inf, mnz = inf, mxx = -inf, mxy = -inf, mxz = -inf;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int qx = x - 1 + k % 3, qy = y - 1 + k / 3;
                if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
                    mnx = crtm_min(mnx, nb[k].x); mny = crtm_min(mny, nb[k].y); mnz = crtm_min(mnz, nb[k].z);
                    mxx = crtm_max(mxx, nb[k].x); mxy = crtm_max(mxy, nb[k].y); mxz = crtm_max(mxz, nb[k].z);
                }
            }
            hx = crtm_min(crtm_max(hx, mnx), mxx); hy = crtm_min(crtm_max(hy, mny), mxy); hz = crtm_min(crtm_max(hz, mnz), mxz);
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
    crtm_store4(P.nColor + ci, o);
    crtm_store4(P.nMoments + ci, m);
}

template <bool SURFACE>
static void crtm_launch(const CrtmPass& P, bool stage, hipStream_t stream)
{
    const dim3 grid((unsigned)((P.width + CRTM_TILE_W - 1) / CRTM_TILE_W), (unsigned)((P.height + CRTM_TILE_H - 1) / CRTM_TILE_H));
    if (stage) crtm_accumulate_kernel<SURFACE, true><<<grid, CRTM_BLOCK, 0, stream>>>(P);
    else crtm_accumulate_kernel<SURFACE, false><<<grid, CRTM_BLOCK, CRTM_UNSTAGED_PAD, stream>>>(P);
}

// crtt_check of crt_temporal.hip restated (the same refusals with the same codes in the same order), then what the motion arguments add
static int crtm_check(const CrttFrame* cur, const CrttHistory* prev, const CrttHistory* next, const CrttParams* p, const CrtmMotionArgs* m)
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
    if (!m) return CRTT_E_BAD_ARGUMENT;
    if ((m->table == nullptr) != (m->count == 0) || m->count > (uint32_t)CRTM_MAX_COUNT) return CRTT_E_BAD_ARGUMENT;
    if (m->table && cur->guides == CRTT_GUIDES_PLANES && !cur->ids) return CRTT_E_BAD_ARGUMENT;
    if (m->vectors) {
        for (const void* in : ins)
            if (in == m->vectors) return CRTT_E_BAD_ARGUMENT;
        for (const void* out : outs)
            if (out == m->vectors) return CRTT_E_BAD_ARGUMENT;
    }
    if (cur->width > CRTM_MAX_DIM || cur->height > CRTM_MAX_DIM) return CRTT_E_OUT_OF_RANGE;
    return CRTT_OK;
}

// a 3 x 3 inverse in double by cofactors; false when the rows span no volume (the test of crtt_camera)
static bool crtm_inverse3(const double R[3][3], double I[3][3])
{
    const double c00 = R[1][1] * R[2][2] - R[1][2] * R[2][1], c01 = R[1][2] * R[2][0] - R[1][0] * R[2][2], c02 = R[1][0] * R[2][1] - R[1][1] * R[2][0];
    const double det = R[0][0] * c00 + R[0][1] * c01 + R[0][2] * c02;
    double scale = 1.0;
    for (int r = 0; r < 3; ++r) scale *= sqrt(R[r][0] * R[r][0] + R[r][1] * R[r][1] + R[r][2] * R[r][2]);
    if (!isfinite(det) || !isfinite(scale) || !(fabs(det) > 1e-12 * scale)) return false;
    I[0][0] = c00 / det; I[1][0] = c01 / det; I[2][0] = c02 / det;
    I[0][1] = (R[0][2] * R[2][1] - R[0][1] * R[2][2]) / det; I[1][1] = (R[0][0] * R[2][2] - R[0][2] * R[2][0]) / det; I[2][1] = (R[0][1] * R[2][0] - R[0][0] * R[2][1]) / det;
    I[0][2] = (R[0][1] * R[1][2] - R[0][2] * R[1][1]) / det; I[1][2] = (R[0][2] * R[1][0] - R[0][0] * R[1][2]) / det; I[2][2] = (R[0][0] * R[1][1] - R[0][1] * R[1][0]) / det;
    return true;
}

static void crtm_mul3(const double A[3][3], const double B[3][3], double C[3][3])
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[r][c] = (A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c];
}

extern "C" {

int crtm_motion(const float prevInverse[16], const float curInverse[16], CrtmMotion* out)
{
    if (!curInverse || !out) return CRTT_E_BAD_ARGUMENT;
    for (int i = 0; i < 16; ++i)
        if (!isfinite(curInverse[i]) || (prevInverse && !isfinite(prevInverse[i]))) return CRTT_E_BAD_ARGUMENT;
    CrtmMotion r;
    r.kind = !prevInverse ? CRTM_NEW : !memcmp(prevInverse, curInverse, 16 * sizeof(float)) ? CRTM_STATIC : CRTM_MOVING;
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 4; ++j) r.point[4 * k + j] = j == k ? 1.0f : 0.0f;
        for (int j = 0; j < 3; ++j) r.normal[3 * k + j] = j == k ? 1.0f : 0.0f;
    }
    if (r.kind == CRTM_MOVING) {
        // element (row j, column k) of a CrtMatrix4 at [4j + k]; column 3 is never read (crt_motion.h)
        double Ac[3][3], Ap[3][3], Api[3][3], Aci[3][3], L[3][3], Li[3][3], db[3], t[3];
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) { Ac[j][k] = (double)curInverse[4 * j + k]; Ap[j][k] = (double)prevInverse[4 * j + k]; }
        for (int k = 0; k < 3; ++k) db[k] = (double)curInverse[12 + k] - (double)prevInverse[12 + k];
        if (!crtm_inverse3(Ap, Api)) return CRTT_E_BAD_ARGUMENT;
        crtm_mul3(Ac, Api, L);
        if (!crtm_inverse3(L, Li) || !crtm_inverse3(Ac, Aci)) return CRTT_E_BAD_ARGUMENT;      // (the first: is L singular?)
        crtm_mul3(Ap, Aci, Li);                       // L^-1 = A_prev * A_cur^-1, from the inputs' own factors, not from the product L
        for (int k = 0; k < 3; ++k) t[k] = (db[0] * Api[0][k] + db[1] * Api[1][k]) + db[2] * Api[2][k];
        for (int k = 0; k < 3; ++k) {
            for (int j = 0; j < 3; ++j) { r.point[4 * k + j] = (float)L[j][k]; r.normal[3 * k + j] = (float)Li[k][j]; }
            r.point[4 * k + 3] = (float)t[k];
        }
        for (int i = 0; i < 12; ++i)
            if (!isfinite(r.point[i])) return CRTT_E_BAD_ARGUMENT;
        for (int i = 0; i < 9; ++i)
            if (!isfinite(r.normal[i])) return CRTT_E_BAD_ARGUMENT;
    }
    *out = r;
    return CRTT_OK;
}

int crtm_motions(const void* prevInstances, uint32_t prevCount, const void* curInstances, uint32_t curCount, CrtmMotion* out)
{
    if ((!prevInstances && prevCount) || (!curInstances && curCount) || (!out && curCount)) return CRTT_E_BAD_ARGUMENT;
    for (uint32_t i = 0; i < curCount; ++i) {
        const float* cur = (const float*)((const char*)curInstances + (size_t)i * CRTM_INSTANCE_STRIDE);
        const float* prev = i < prevCount ? (const float*)((const char*)prevInstances + (size_t)i * CRTM_INSTANCE_STRIDE) : nullptr;
        const int rc = crtm_motion(prev, cur, out + i);
        if (rc != CRTT_OK) return rc;
    }
    return CRTT_OK;
}

int crtm_accumulate(const CrttFrame* cur, const CrttHistory* prev, const CrttHistory* next, const CrttParams* p, const CrtmMotionArgs* m, void* stream)
{
    const int rc = crtm_check(cur, prev, next, p, m);
    if (rc != CRTT_OK) return rc;
    const bool surface = cur->guides == CRTT_GUIDES_SURFACE, match = (p->flags & CRTT_MATCH_INSTANCE) != 0;
    const char* g = (const char*)cur->geometry;
    CrtmPass P;
    P.color = (const float4*)cur->color;
    P.geometry = g;
    P.instance = !(match || next->instance || m->table) ? nullptr : surface ? g + 16 : (const char*)cur->ids;
    P.pColor = prev ? (const float4*)prev->color : nullptr;
    P.pMoments = prev ? (const float4*)prev->moments : nullptr;
    P.pGeometry = prev ? (const float4*)prev->geometry : nullptr;
    P.pInstance = prev && match ? (const int*)prev->instance : nullptr;
    P.nColor = (float4*)next->color; P.nMoments = (float4*)next->moments; P.nGeometry = (float4*)next->geometry; P.nInstance = (int*)next->instance;
    P.table = (const CrtmMotion*)m->table; P.count = m->count; P.vectors = (float4*)m->vectors;
    P.width = cur->width; P.height = cur->height;
    P.flags = p->flags;
    P.alpha = p->alpha; P.momentsAlpha = p->momentsAlpha; P.maxHistory = p->maxHistory; P.depthTol = p->depthTol; P.normalCos = p->normalCos;
    for (int i = 0; i < 9; ++i) { P.toRay[i] = cur->camera.toRay[i]; P.toScreen[i] = prev ? prev->camera.toScreen[i] : 0.0f; }
    for (int i = 0; i < 3; ++i) {
        P.pos[i] = cur->camera.pos[i]; P.ppos[i] = prev ? prev->camera.pos[i] : 0.0f;
        P.dpos[i] = prev ? cur->camera.pos[i] - prev->camera.pos[i] : 0.0f;
    }
    const bool stage = (p->flags & CRTT_CLAMP) != 0;
    if (surface) crtm_launch<true>(P, stage, (hipStream_t)stream);
    else crtm_launch<false>(P, stage, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : CRTT_OK;
}

const char* crtm_error_string(int rc)
{
    switch (rc) {
    case CRTT_OK: return "ok";
    case CRTT_E_BAD_ARGUMENT: return "crtm: bad argument";
    case CRTT_E_OUT_OF_RANGE: return "crtm: out of range (a frame wider or taller than 16384)";
    default: return rc > 0 ? hipGetErrorString((hipError_t)rc) : "crtm: unknown error";
    }
}

}
