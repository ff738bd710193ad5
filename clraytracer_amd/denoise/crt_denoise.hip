// crt_denoise.hip -- libcrt_denoise.so: the edge-avoiding a-trous filter of include/crt_denoise.h (definition there), its pass kernel and the
// C ABI over it. The only translation unit of the library; it shares no state and no source with libcrt_hip.so.
// Build: the Makefile's $(DENOISE_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include "../../include/crt_denoise.h"

#define CRTD_TILE_W 32              // 256 lanes over a 32 x 8 tile: a wave is two 512-B rows of float4
#define CRTD_TILE_H 8
#define CRTD_BLOCK (CRTD_TILE_W * CRTD_TILE_H)
#define CRTD_MAX_DIM 16384
#define CRTD_MAX_ITERATIONS 6
#define CRTD_STAGE_MAX_STEP_DEFAULT 4   // what was measured for each step
static_assert(sizeof(CrtdFrame) == 48 && sizeof(CrtdParams) == 20 && sizeof(float4) == 16, "the ABI of crt_denoise.h (clraytracer_amd/_lib.py mirrors it)");
// bits of CrtdPass::flags beside CRTD_MATCH_INSTANCE and CRTD_LUMA_STOP: what CRTD_DEMODULATE means for this pass
#define CRTD_PASS_DEMOD_IN 0x100u   // pass 0: the input is color.rgb / den for hit pixels
#define CRTD_PASS_DEMOD_OUT 0x200u  // the last pass: store result.rgb * den for hit pixels

struct CrtdPass {
    const float4* in;               // I, the pass's input image
    float4* out;
    const char* geometry;           // {n.x, n.y, n.z, t} at geometry + i * stride
    const char* instance;           // int32 at instance + i * stride, NULL without CRTD_MATCH_INSTANCE
    const char* albedo;             // uint32 at albedo + i * stride, NULL without CRTD_DEMODULATE
    int width, height, step;
    uint32_t flags;
    float depthTol, normalCos, lumaTol;
};

// 16-B rows as one vector load or store each (a float4 copied as a struct can be split into a 12-B copy through the stack and a float)
typedef float crtd_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 crtd_load4(const void* p) { const crtd_f4 v = *(const crtd_f4*)p; return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void crtd_store4(float4* p, float4 v) { crtd_f4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; *(crtd_f4*)p = r; }

// the strides of the two guide layouts: three planes (16, 16, 4 B) or CrtSurfaceHit records (48 B; geometry at 0, instance at 16, albedo at 32)
template <bool SURFACE> __device__ __forceinline__ float4 crtd_geometry(const CrtdPass& P, size_t i) { return crtd_load4(P.geometry + i * (SURFACE ? 48 : 16)); }
template <bool SURFACE> __device__ __forceinline__ int crtd_instance(const CrtdPass& P, size_t i) { return *(const int*)(P.instance + i * (SURFACE ? 48 : 16)); }
template <bool SURFACE> __device__ __forceinline__ uint32_t crtd_albedo(const CrtdPass& P, size_t i) { return *(const uint32_t*)(P.albedo + i * (SURFACE ? 48 : 4)); }

__device__ __forceinline__ float crtd_den(uint32_t b) { return b == 0u ? 1.0f : (float)b / 255.0f; }
__device__ __forceinline__ bool crtd_hit(float t) { return t <= 99998.0f; }
__device__ __forceinline__ float crtd_dot3(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float crtd_luma(float4 c) { return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z; }

// den of channel ch (0 = r, 1 = g, 2 = b) of an albedo word
__device__ __forceinline__ float crtd_den_of(uint32_t a, int ch) { return crtd_den((a >> (8 * ch)) & 255u); }
// I of a pixel from its colour c: demodulated where the pixel is a hit (branch-free: the quotient is computed and then chosen or not)
__device__ __forceinline__ float4 crtd_demodulated(float4 c, uint32_t a, bool hit)
{
    const float qx = c.x / crtd_den_of(a, 0), qy = c.y / crtd_den_of(a, 1), qz = c.z / crtd_den_of(a, 2);
    return make_float4(hit ? qx : c.x, hit ? qy : c.y, hit ? qz : c.z, c.w);
}

// The running sums of one hit centre. tap(): one tap in the definition's order; a tap that contributes nothing must have w = 0 AND a colour of 0.
struct CrtdSum {
    float4 gc; float lc, dtol; int ic;
    float x, y, z, w;
    __device__ __forceinline__ void tap(const CrtdPass& P, float k, bool centre, float4 g, float4 c, int inst)
    {
        // & and | on ints, not && and ||: 25 taps of straight-line code instead of a branch per condition
        int m = (int)crtd_hit(g.w) & (int)(fabsf(g.w - gc.w) <= dtol) & (int)(crtd_dot3(g, gc) >= P.normalCos) & (int)(inst == ic);
        if (P.flags & CRTD_LUMA_STOP) m &= (int)(fabsf(crtd_luma(c) - lc) <= P.lumaTol);
        m |= (int)centre;
        const float wt = m ? k : 0.0f;
        x += c.x * wt; y += c.y * wt; z += c.z * wt; w += wt;
    }
};

__device__ __forceinline__ float crtd_k(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// One pass. STAGE = 1, 2 or 4: the pass of that step with its taps from LDS -- the workgroup stages its tile and a halo of 2 * STAGE pixels as two
// planes of float4 (a 16-B stride per lane keeps ds_read_b128 conflict-free): geometry, then {I.rgb, instance}. STAGE = 0: any step (P.step), the
// taps are row reads through L1 / L2. Either way every global load of a lane is issued before the first is waited for: the loads are unconditional
// (a pixel outside the frame reads the clamped pixel) and what must not count is chosen away afterwards. A pixel outside the frame is taken as
// {no hit, colour 0}: its tap adds +0 to sums that start at +0 and so can never be -0 -- the same bits as skipping it (the centre is always inside).
template <bool SURFACE, int STAGE>
__global__ __launch_bounds__(CRTD_BLOCK) void crtd_pass_kernel(CrtdPass P)
{
    constexpr int HALO = 2 * STAGE, TW = CRTD_TILE_W + 2 * HALO, TH = CRTD_TILE_H + 2 * HALO, N = TW * TH, ROUNDS = (N + CRTD_BLOCK - 1) / CRTD_BLOCK;
    __shared__ float4 s_tile[STAGE ? 2 * N : 1];
    const int W = P.width, H = P.height, s = STAGE ? STAGE : P.step;
    const int lx = (int)(threadIdx.x & (CRTD_TILE_W - 1)), ly = (int)(threadIdx.x / CRTD_TILE_W);
    const int x0 = (int)blockIdx.x * CRTD_TILE_W, y0 = (int)blockIdx.y * CRTD_TILE_H;
    const int x = x0 + lx, y = y0 + ly;
    const bool match = (P.flags & CRTD_MATCH_INSTANCE) != 0, demodIn = (P.flags & CRTD_PASS_DEMOD_IN) != 0, demodOut = (P.flags & CRTD_PASS_DEMOD_OUT) != 0;
    const bool mine = x < W && y < H;                 // a lane without a pixel reads the clamped one and stores nothing
    const size_t ci = (size_t)min(y, H - 1) * (size_t)W + (size_t)min(x, W - 1);
    const float4 raw = crtd_load4(P.in + ci);                     // a pixel that is no hit copies I; alpha is the centre's throughout
    const uint32_t ac = (demodIn || demodOut) ? crtd_albedo<SURFACE>(P, ci) : 0u;
    CrtdSum S;
    float4 cc;
    if (STAGE) {
        // round j stages element i = lane + 256 j of the tile + halo, row-major; where(j, q) says whether it lies inside the frame and where it (clamped) is
        auto where = [&](int j, size_t& q) {
            const int i = (int)threadIdx.x + j * CRTD_BLOCK, ty = i / TW, tx = i - ty * TW;
            const int px = x0 - HALO + tx, py = y0 - HALO + ty;
            q = (size_t)min(max(py, 0), H - 1) * (size_t)W + (size_t)min(max(px, 0), W - 1);
            return px >= 0 && px < W && py >= 0 && py < H;
        };
        float4 g[ROUNDS], c[ROUNDS]; int inst[ROUNDS]; uint32_t a[ROUNDS];
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            size_t q; where(j, q);
            g[j] = crtd_geometry<SURFACE>(P, q);
            c[j] = crtd_load4(P.in + q);
            inst[j] = match ? crtd_instance<SURFACE>(P, q) : 0;
            a[j] = demodIn ? crtd_albedo<SURFACE>(P, q) : 0u;
        }
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            size_t q;
            const bool inside = where(j, q);
            const int i = (int)threadIdx.x + j * CRTD_BLOCK;
            if (demodIn) c[j] = crtd_demodulated(c[j], a[j], crtd_hit(g[j].w));
            c[j].w = __int_as_float(inst[j]);
            if (!inside) { g[j] = make_float4(0.0f, 0.0f, 0.0f, 99999.0f); c[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
            if (i < N) { crtd_store4(s_tile + i, g[j]); crtd_store4(s_tile + N + i, c[j]); }
        }
        __syncthreads();
        if (!mine) return;
        S.gc = crtd_load4(s_tile + (ly + HALO) * TW + lx + HALO);
        cc = crtd_load4(s_tile + N + (ly + HALO) * TW + lx + HALO);
        S.ic = __float_as_int(cc.w);
    } else {
        if (!mine) return;
        S.gc = crtd_geometry<SURFACE>(P, ci);
        S.ic = match ? crtd_instance<SURFACE>(P, ci) : 0;
        cc = demodIn ? crtd_demodulated(raw, ac, true) : raw;
    }
    if (!crtd_hit(S.gc.w)) { crtd_store4(P.out + ci, raw); return; }
    S.lc = crtd_luma(cc);
    S.dtol = (P.depthTol * S.gc.w) * (float)s;
    S.x = S.y = S.z = S.w = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float k = crtd_k(dy) * crtd_k(dx);
            if (STAGE) {
                const int q = (ly + HALO + dy * STAGE) * TW + lx + HALO + dx * STAGE;
                const float4 c = crtd_load4(s_tile + N + q);             // (one ds_read_b128 each: as a struct the row is read as 12 + 4 bytes)
                S.tap(P, k, (dx | dy) == 0, crtd_load4(s_tile + q), c, __float_as_int(c.w));
            } else {
                // (pixel indices fit 32 bits: 16384 x 16384 at most; five row and five column terms serve the 25 taps)
                const int qx = x + dx * s, qy = y + dy * s;
                const bool inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
                const size_t q = (size_t)(uint32_t)(min(max(qy, 0), H - 1) * W + min(max(qx, 0), W - 1));
                float4 g = crtd_geometry<SURFACE>(P, q);
                float4 c = crtd_load4(P.in + q);
                if (demodIn) c = crtd_demodulated(c, crtd_albedo<SURFACE>(P, q), crtd_hit(g.w));
                if (!inside) { g.w = 99999.0f; c.x = c.y = c.z = 0.0f; }
                S.tap(P, k, (dx | dy) == 0, g, c, match ? crtd_instance<SURFACE>(P, q) : 0);
            }
        }
    }
    float4 o = make_float4(S.x / S.w, S.y / S.w, S.z / S.w, raw.w);
    if (demodOut) {
        o.x = o.x * crtd_den_of(ac, 0); o.y = o.y * crtd_den_of(ac, 1); o.z = o.z * crtd_den_of(ac, 2);
    }
    crtd_store4(P.out + ci, o);
}

template <bool SURFACE>
static void crtd_launch(const CrtdPass& P, int stageMaxStep, hipStream_t stream)
{
    const dim3 grid((unsigned)((P.width + CRTD_TILE_W - 1) / CRTD_TILE_W), (unsigned)((P.height + CRTD_TILE_H - 1) / CRTD_TILE_H));
    const int stage = P.step <= stageMaxStep ? P.step : 0;
    if (stage == 1) crtd_pass_kernel<SURFACE, 1><<<grid, CRTD_BLOCK, 0, stream>>>(P);
    else if (stage == 2) crtd_pass_kernel<SURFACE, 2><<<grid, CRTD_BLOCK, 0, stream>>>(P);
    else if (stage == 4) crtd_pass_kernel<SURFACE, 4><<<grid, CRTD_BLOCK, 0, stream>>>(P);
    else crtd_pass_kernel<SURFACE, 0><<<grid, CRTD_BLOCK, 0, stream>>>(P);
}

// the largest step whose taps come from LDS: CRTD_STAGE_MAX_STEP in the environment (0, 1, 2 or 4), else the measured default.
// Step 4 stages (32 + 16) x (8 + 16) x 32 B = 36 KiB; step 8 would stage 80 KiB for an 8 KiB tile and is not offered.
static int crtd_stage_max_step()
{
    const char* e = getenv("CRTD_STAGE_MAX_STEP");
    if (e && e[0] && !e[1] && (e[0] == '0' || e[0] == '1' || e[0] == '2' || e[0] == '4')) return e[0] - '0';
    return CRTD_STAGE_MAX_STEP_DEFAULT;
}

static int crtd_check(const CrtdFrame* f, const CrtdParams* p, const void* out, const void* scratch)
{
    if (!f || !p || !out || !f->color || !f->geometry) return CRTD_E_BAD_ARGUMENT;
    if (f->width < 1 || f->height < 1) return CRTD_E_BAD_ARGUMENT;
    if (p->iterations < 1 || p->iterations > CRTD_MAX_ITERATIONS) return CRTD_E_BAD_ARGUMENT;
    if (p->flags & ~(uint32_t)(CRTD_DEMODULATE | CRTD_MATCH_INSTANCE | CRTD_LUMA_STOP)) return CRTD_E_BAD_ARGUMENT;
    if (f->guides == CRTD_GUIDES_PLANES) {
        if (((p->flags & CRTD_MATCH_INSTANCE) && !f->ids) || ((p->flags & CRTD_DEMODULATE) && !f->albedo)) return CRTD_E_BAD_ARGUMENT;
    } else if (f->guides == CRTD_GUIDES_SURFACE) {
        if (f->ids || f->albedo) return CRTD_E_BAD_ARGUMENT;
    } else {
        return CRTD_E_BAD_ARGUMENT;
    }
    if (!(p->depthTol >= 0.0f) || !isfinite(p->normalCos)) return CRTD_E_BAD_ARGUMENT;
    if ((p->flags & CRTD_LUMA_STOP) && !(p->lumaTol >= 0.0f)) return CRTD_E_BAD_ARGUMENT;
    if (p->iterations >= 2 && !scratch) return CRTD_E_BAD_ARGUMENT;
    const void* inputs[4] = {f->color, f->geometry, f->ids, f->albedo};
    for (const void* in : inputs)
        if (in && (in == out || in == scratch)) return CRTD_E_BAD_ARGUMENT;
    if (scratch && scratch == out) return CRTD_E_BAD_ARGUMENT;
    if (f->width > CRTD_MAX_DIM || f->height > CRTD_MAX_DIM) return CRTD_E_OUT_OF_RANGE;
    return CRTD_OK;
}

extern "C" {

size_t crtd_scratch_bytes(int32_t width, int32_t height, int32_t iterations)
{
    if (width < 1 || height < 1 || iterations < 2) return 0;
    return (size_t)width * (size_t)height * sizeof(float4);
}

int crtd_denoise(const CrtdFrame* f, const CrtdParams* p, void* out, void* scratch, void* stream)
{
    const int rc = crtd_check(f, p, out, scratch);
    if (rc != CRTD_OK) return rc;
    const bool surface = f->guides == CRTD_GUIDES_SURFACE;
    const bool demod = (p->flags & CRTD_DEMODULATE) != 0, match = (p->flags & CRTD_MATCH_INSTANCE) != 0;
    const char* g = (const char*)f->geometry;
    CrtdPass P;
    P.geometry = g;
    P.instance = !match ? nullptr : surface ? g + 16 : (const char*)f->ids;
    P.albedo = !demod ? nullptr : surface ? g + 32 : (const char*)f->albedo;
    P.width = f->width; P.height = f->height;
    P.depthTol = p->depthTol; P.normalCos = p->normalCos; P.lumaTol = p->lumaTol;
    const int stageMax = crtd_stage_max_step(), n = p->iterations;
    for (int pass = 0; pass < n; ++pass) {
        // the last pass lands in `out`, the one before it in `scratch`, and so on backwards
        float4* dst = (float4*)(((n - 1 - pass) & 1) ? scratch : out);
        P.in = pass == 0 ? (const float4*)f->color : (const float4*)(dst == out ? scratch : out);
        P.out = dst;
        P.step = 1 << pass;
        P.flags = (p->flags & (uint32_t)(CRTD_MATCH_INSTANCE | CRTD_LUMA_STOP)) | (demod && pass == 0 ? CRTD_PASS_DEMOD_IN : 0u)
                | (demod && pass == n - 1 ? CRTD_PASS_DEMOD_OUT : 0u);
        if (surface) crtd_launch<true>(P, stageMax, (hipStream_t)stream);
        else crtd_launch<false>(P, stageMax, (hipStream_t)stream);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return CRTD_OK;
}

const char* crtd_error_string(int rc)
{
    switch (rc) {
    case CRTD_OK: return "ok";
    case CRTD_E_BAD_ARGUMENT: return "crtd: bad argument";
    case CRTD_E_OUT_OF_RANGE: return "crtd: out of range (a frame wider or taller than 16384)";
    default: return rc > 0 ? hipGetErrorString((hipError_t)rc) : "crtd: unknown error";
    }
}

}
