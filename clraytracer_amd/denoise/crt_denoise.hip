// crt_denoise.hip -- libcrt_denoise.so: the edge-avoiding a-trous filter of include/crt_denoise.h (definition there), its pass kernel and the
// C ABI over it. The only translation unit of the library. The steps it has in common with the other image libraries -- vector loads, guide
// layouts, predicates, weights, the tile and its staging arithmetic; the grid, the rules of the argument check, the ping-pong, the error strings;
// the step switch's parser -- come from ../image/crt_image_device.h, crt_image_host.h and crt_image_env.h. It shares no state.
// Build: the Makefile's $(DENOISE_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/crt_denoise.h"
#include "../image/crt_image_host.h"
#include "../image/crt_image_env.h"

#define CRTD_MAX_ITERATIONS 6
#define CRTD_STAGE_MAX_STEP_DEFAULT 4   // what was measured for each step
static_assert(sizeof(CrtdFrame) == 48 && sizeof(CrtdParams) == 20 && sizeof(float4) == 16, "the ABI of crt_denoise.h (clraytracer_amd/_lib.py mirrors it)");
static_assert(CRTD_OK == CRTI_OK && CRTD_E_BAD_ARGUMENT == CRTI_E_BAD_ARGUMENT && CRTD_E_OUT_OF_RANGE == CRTI_E_OUT_OF_RANGE && CRTD_GUIDES_PLANES == CRTI_GUIDES_PLANES
              && CRTD_GUIDES_SURFACE == CRTI_GUIDES_SURFACE, "the codes and layouts of crt_image_host.h");
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

__device__ __forceinline__ float crtd_den(uint32_t b) { return b == 0u ? 1.0f : (float)b / 255.0f; }

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
        int m = (int)crti_hit(g.w) & (int)(fabsf(g.w - gc.w) <= dtol) & (int)(crti_dot3(g, gc) >= P.normalCos) & (int)(inst == ic);
        if (P.flags & CRTD_LUMA_STOP) m &= (int)(fabsf(crti_luma(c) - lc) <= P.lumaTol);
        m |= (int)centre;
        const float wt = m ? k : 0.0f;
        x += c.x * wt; y += c.y * wt; z += c.z * wt; w += wt;
    }
};

// One pass. STAGE = 1, 2 or 4: the pass of that step with its taps from LDS -- the workgroup stages its tile and a halo of 2 * STAGE pixels as two
// planes of float4 (a 16-B stride per lane keeps ds_read_b128 conflict-free): geometry, then {I.rgb, instance}. STAGE = 0: any step (P.step), the
// taps are row reads through L1 / L2. Either way every global load of a lane is issued before the first is waited for: the loads are unconditional
// (a pixel outside the frame reads the clamped pixel) and what must not count is chosen away afterwards. A pixel outside the frame is taken as
// {no hit, colour 0}: its tap adds +0 to sums that start at +0 and so can never be -0 -- the same bits as skipping it (the centre is always inside).
template <bool SURFACE, int STAGE>
__global__ __launch_bounds__(CRTI_BLOCK) void crtd_pass_kernel(CrtdPass P)
{
    constexpr int HALO = 2 * STAGE;
    using Tile = CrtiTile<HALO>;
    constexpr int TW = Tile::TW, N = Tile::N, ROUNDS = Tile::ROUNDS;
    __shared__ float4 s_tile[STAGE ? 2 * N : 1];
    const int W = P.width, H = P.height, s = STAGE ? STAGE : P.step;
    const CrtiLane lane;
    const int lx = lane.lx, ly = lane.ly, x0 = lane.x0, y0 = lane.y0, x = lane.x, y = lane.y;
    const bool match = (P.flags & CRTD_MATCH_INSTANCE) != 0, demodIn = (P.flags & CRTD_PASS_DEMOD_IN) != 0, demodOut = (P.flags & CRTD_PASS_DEMOD_OUT) != 0;
    const bool mine = x < W && y < H;                 // a lane without a pixel reads the clamped one and stores nothing
    const size_t ci = crti_clamped_own<true>(x, y, W, H);      // (this kernel forms its centre and staging indices by 64-bit multiplies)
    const float4 raw = crti_load4(P.in + ci);                     // a pixel that is no hit copies I; alpha is the centre's throughout
    const uint32_t ac = (demodIn || demodOut) ? crti_albedo<SURFACE>(P, ci) : 0u;
    CrtdSum S;
    float4 cc;
    if (STAGE) {
        // where(j, q) says whether round j's element lies inside the frame and where it (clamped) is
        auto where = [&](int j, size_t& q) {
            const Tile t(j, x0, y0);
            const int px = t.px, py = t.py;
            q = crti_clamped<true>(px, py, W, H);
            return CRTI_INSIDE(px, py, W, H);
        };
        float4 g[ROUNDS], c[ROUNDS]; int inst[ROUNDS]; uint32_t a[ROUNDS];
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            size_t q; where(j, q);
            g[j] = crti_geometry<SURFACE>(P, q);
            c[j] = crti_load4(P.in + q);
            inst[j] = match ? crti_instance<SURFACE>(P, q) : 0;
            a[j] = demodIn ? crti_albedo<SURFACE>(P, q) : 0u;
        }
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            size_t q;
            const bool inside = where(j, q);
            const int i = (int)threadIdx.x + j * CRTI_BLOCK;
            if (demodIn) c[j] = crtd_demodulated(c[j], a[j], crti_hit(g[j].w));
            c[j].w = __int_as_float(inst[j]);
            if (!inside) { g[j] = make_float4(0.0f, 0.0f, 0.0f, CRTI_MISS); c[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
            if (i < N) { crti_store4(s_tile + i, g[j]); crti_store4(s_tile + N + i, c[j]); }
        }
        __syncthreads();
        if (!mine) return;
        S.gc = crti_load4(s_tile + (ly + HALO) * TW + lx + HALO);
        cc = crti_load4(s_tile + N + (ly + HALO) * TW + lx + HALO);
        S.ic = __float_as_int(cc.w);
    } else {
        if (!mine) return;
        S.gc = crti_geometry<SURFACE>(P, ci);
        S.ic = match ? crti_instance<SURFACE>(P, ci) : 0;
        cc = demodIn ? crtd_demodulated(raw, ac, true) : raw;
    }
    if (!crti_hit(S.gc.w)) { crti_store4(P.out + ci, raw); return; }
    S.lc = crti_luma(cc);
    S.dtol = (P.depthTol * S.gc.w) * (float)s;
    S.x = S.y = S.z = S.w = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float k = crti_k(dy) * crti_k(dx);
            if (STAGE) {
                const int q = (ly + HALO + dy * STAGE) * TW + lx + HALO + dx * STAGE;
                const float4 c = crti_load4(s_tile + N + q);             // (one ds_read_b128 each: as a struct the row is read as 12 + 4 bytes)
                S.tap(P, k, (dx | dy) == 0, crti_load4(s_tile + q), c, __float_as_int(c.w));
            } else {
                // (five row and five column terms serve the 25 taps)
                const int qx = x + dx * s, qy = y + dy * s;
                const bool inside = CRTI_INSIDE(qx, qy, W, H);
                const size_t q = crti_clamped(qx, qy, W, H);
                float4 g = crti_geometry<SURFACE>(P, q);
                float4 c = crti_load4(P.in + q);
                if (demodIn) c = crtd_demodulated(c, crti_albedo<SURFACE>(P, q), crti_hit(g.w));
                if (!inside) { g.w = CRTI_MISS; c.x = c.y = c.z = 0.0f; }
                S.tap(P, k, (dx | dy) == 0, g, c, match ? crti_instance<SURFACE>(P, q) : 0);
            }
        }
    }
    float4 o = make_float4(S.x / S.w, S.y / S.w, S.z / S.w, raw.w);
    if (demodOut) {
        o.x = o.x * crtd_den_of(ac, 0); o.y = o.y * crtd_den_of(ac, 1); o.z = o.z * crtd_den_of(ac, 2);
    }
    crti_store4(P.out + ci, o);
}

template <bool SURFACE>
static void crtd_launch(const CrtdPass& P, int stageMaxStep, hipStream_t stream)
{
    const dim3 grid = crti_grid(P.width, P.height);
    const int stage = P.step <= stageMaxStep ? P.step : 0;
    if (stage == 1) crtd_pass_kernel<SURFACE, 1><<<grid, CRTI_BLOCK, 0, stream>>>(P);
    else if (stage == 2) crtd_pass_kernel<SURFACE, 2><<<grid, CRTI_BLOCK, 0, stream>>>(P);
    else if (stage == 4) crtd_pass_kernel<SURFACE, 4><<<grid, CRTI_BLOCK, 0, stream>>>(P);
    else crtd_pass_kernel<SURFACE, 0><<<grid, CRTI_BLOCK, 0, stream>>>(P);
}

// CRTD_STAGE_MAX_STEP in the environment (crt_image_env.h), else the measured default: the largest step whose taps come from LDS.
// Step 4 stages (32 + 16) x (8 + 16) x 32 B = 36 KiB; step 8 would stage 80 KiB for an 8 KiB tile and is not offered.
static int crtd_stage_max_step() { return crti_env_step("CRTD_STAGE_MAX_STEP", CRTD_STAGE_MAX_STEP_DEFAULT); }

static int crtd_check(const CrtdFrame* f, const CrtdParams* p, const void* out, const void* scratch)
{
    if (!f || !p || !out || !f->color || !f->geometry) return CRTD_E_BAD_ARGUMENT;
    if (f->width < 1 || f->height < 1) return CRTD_E_BAD_ARGUMENT;
    if (p->iterations < 1 || p->iterations > CRTD_MAX_ITERATIONS) return CRTD_E_BAD_ARGUMENT;
    if (p->flags & ~(uint32_t)(CRTD_DEMODULATE | CRTD_MATCH_INSTANCE | CRTD_LUMA_STOP)) return CRTD_E_BAD_ARGUMENT;
    if (!crti_guides_ok(f->guides, (p->flags & CRTD_MATCH_INSTANCE) != 0, f->ids, (p->flags & CRTD_DEMODULATE) != 0, f->albedo)) return CRTD_E_BAD_ARGUMENT;
    if (!(p->depthTol >= 0.0f) || !isfinite(p->normalCos)) return CRTD_E_BAD_ARGUMENT;
    if ((p->flags & CRTD_LUMA_STOP) && !(p->lumaTol >= 0.0f)) return CRTD_E_BAD_ARGUMENT;
    if (p->iterations >= 2 && !scratch) return CRTD_E_BAD_ARGUMENT;
    const void* const ins[4] = {f->color, f->geometry, f->ids, f->albedo};
    const void* const outs[2] = {out, scratch};
    if (crti_aliased(ins, outs)) return CRTD_E_BAD_ARGUMENT;
    if (f->width > CRTI_MAX_DIM || f->height > CRTI_MAX_DIM) return CRTD_E_OUT_OF_RANGE;
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
        float4* dst = (float4*)crti_pingpong(n, pass, out, scratch);
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
    return CRTI_ERROR_STRING("crtd", rc);
}

}
