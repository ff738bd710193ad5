// crt_motion.hip -- libcrt_motion.so: temporal accumulation that reprojects through each instance's own motion (include/crt_motion.h, definition
// there), the host-only motion records and the C ABI over them. The only translation unit of the library. Its kernels are instantiations, over
// CrtmPass, of the template in ../image/crt_accumulate.h that libcrt_temporal.so instantiates over CrttPass: one blend, one tap test and one
// clamp for both (tests/test_gpu_motion.py still ties the two libraries bit for bit). crtt_accumulate's refusals and the fill of the fields both
// passes have come from there too, the 3 x 3 inverse from ../image/crt_image_host.h. It shares no state, and reads no environment switch.
// Build: the Makefile's $(MOTION_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <string.h>
#include "../../include/crt_motion.h"
#include "../image/crt_accumulate.h"

#define CRTM_TABLE_LDS 0            // bytes of the motion table staged in LDS: none, the records come through L1
// Dynamic LDS the unstaged kernels are launched with and never touch: at 54-56 VGPRs they would run 8 waves per SIMD, where the taps' gathers
// of a dense frame take 7 % longer than at 5; 28 KiB per workgroup holds a CU's 160 KiB to 5 workgroups of 4 waves, the staged
// kernels' occupancy and libcrt_temporal.so's
#define CRTM_UNSTAGED_PAD 28672
#define CRTM_INSTANCE_STRIDE 80     // sizeof(CrtMeshInstance) (crt_types.h), the matrix first
// the ABI of crt_motion.h (clraytracer_amd/_lib.py mirrors it), and what it takes from crt_temporal.h
static_assert(sizeof(CrtmMotion) == 88 && alignof(CrtmMotion) == 4 && offsetof(CrtmMotion, point) == 4 && offsetof(CrtmMotion, normal) == 52, "CrtmMotion");
static_assert(sizeof(CrtmMotionArgs) == 24 && offsetof(CrtmMotionArgs, count) == 8 && offsetof(CrtmMotionArgs, vectors) == 16, "CrtmMotionArgs");
static_assert(sizeof(CrttCamera) == 84 && sizeof(CrttFrame) == 128 && sizeof(CrttHistory) == 120 && sizeof(CrttParams) == 24 && sizeof(float4) == 16, "crt_temporal.h");

// <SURFACE, STAGE>, always gated: STAGE exactly under CRTT_CLAMP
template <bool SURFACE>
static void crtm_launch(const CrtmPass& P, bool stage, hipStream_t stream)
{
    const dim3 grid = crti_grid(P.width, P.height);
    if (stage) crt_accumulate_kernel<CrtmPass, SURFACE, true, true><<<grid, CRTI_BLOCK, 0, stream>>>(P);
    else crt_accumulate_kernel<CrtmPass, SURFACE, true, false><<<grid, CRTI_BLOCK, CRTM_UNSTAGED_PAD, stream>>>(P);
}

// crtt_accumulate's refusals (the same codes in the same order), then what the motion arguments add, then the frame's size
static int crtm_check(const CrttFrame* cur, const CrttHistory* prev, const CrttHistory* next, const CrttParams* p, const CrtmMotionArgs* m)
{
    const int rc = crt_accumulate_check(cur, prev, next, p);
    if (rc == CRTT_E_BAD_ARGUMENT) return rc;
    if (!m) return CRTT_E_BAD_ARGUMENT;
    if ((m->table == nullptr) != (m->count == 0) || m->count > (uint32_t)CRTM_MAX_COUNT) return CRTT_E_BAD_ARGUMENT;
    if (m->table && cur->guides == CRTT_GUIDES_PLANES && !cur->ids) return CRTT_E_BAD_ARGUMENT;
    const CrtAccumulatePlanes planes = crt_accumulate_planes(cur, prev, next);
    const void* const vectors[1] = {m->vectors};
    if (crti_aliased(planes.ins, vectors) || crti_aliased(planes.outs, vectors)) return CRTT_E_BAD_ARGUMENT;
    return rc;
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
        if (!crti_inverse3(Ap, Api)) return CRTT_E_BAD_ARGUMENT;
        crtm_mul3(Ac, Api, L);
        if (!crti_inverse3(L, Li) || !crti_inverse3(Ac, Aci)) return CRTT_E_BAD_ARGUMENT;      // (the first: is L singular?)
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
    CrtmPass P;
    crt_accumulate_fill(P, cur, prev, next, p, (p->flags & CRTT_MATCH_INSTANCE) || next->instance || m->table);
    P.table = (const CrtmMotion*)m->table; P.count = m->count; P.vectors = (float4*)m->vectors;
    for (int i = 0; i < 3; ++i) { P.pos[i] = cur->camera.pos[i]; P.ppos[i] = prev ? prev->camera.pos[i] : 0.0f; }
    const bool stage = (p->flags & CRTT_CLAMP) != 0;
    if (cur->guides == CRTT_GUIDES_SURFACE) crtm_launch<true>(P, stage, (hipStream_t)stream);
    else crtm_launch<false>(P, stage, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : CRTT_OK;
}

const char* crtm_error_string(int rc)
{
    return CRTI_ERROR_STRING("crtm", rc);
}

}
