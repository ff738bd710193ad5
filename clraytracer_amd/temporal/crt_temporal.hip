// crt_temporal.hip -- libcrt_temporal.so: temporal reprojection and accumulation of include/crt_temporal.h (definition there), the host-only
// camera maps and the C ABI over them. The only translation unit of the library. Its kernels are instantiations, over CrttPass, of the template
// in ../image/crt_accumulate.h, which libcrt_motion.so instantiates over its own pass; the argument check and the pass's fill come from there
// too, the 3 x 3 inverse from ../image/crt_image_host.h and the two switches' parser from ../image/crt_image_env.h. It shares no state.
// Build: the Makefile's $(TEMPORAL_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include "../../include/crt_temporal.h"
#include "../image/crt_accumulate.h"
#include "../image/crt_image_env.h"

#define CRTT_TAPS_GATED_DEFAULT 1   // what was measured
#define CRTT_CLAMP_LDS_DEFAULT 1
// the ABI of crt_temporal.h (clraytracer_amd/_lib.py mirrors it)
static_assert(sizeof(CrttCamera) == 84 && offsetof(CrttCamera, toRay) == 12 && offsetof(CrttCamera, toScreen) == 48, "CrttCamera");
static_assert(sizeof(CrttFrame) == 128 && offsetof(CrttFrame, color) == 8 && offsetof(CrttFrame, guides) == 16 && offsetof(CrttFrame, geometry) == 24
              && offsetof(CrttFrame, ids) == 32 && offsetof(CrttFrame, camera) == 40, "CrttFrame");
static_assert(sizeof(CrttHistory) == 120 && offsetof(CrttHistory, moments) == 8 && offsetof(CrttHistory, geometry) == 16
              && offsetof(CrttHistory, instance) == 24 && offsetof(CrttHistory, camera) == 32, "CrttHistory");
static_assert(sizeof(CrttParams) == 24 && offsetof(CrttParams, normalCos) == 20 && sizeof(float4) == 16, "CrttParams");
static_assert(CRTT_OK == CRTI_OK && CRTT_E_BAD_ARGUMENT == CRTI_E_BAD_ARGUMENT && CRTT_E_OUT_OF_RANGE == CRTI_E_OUT_OF_RANGE && CRTT_GUIDES_PLANES == CRTI_GUIDES_PLANES
              && CRTT_GUIDES_SURFACE == CRTI_GUIDES_SURFACE, "the codes and layouts of crt_image_host.h");

// <SURFACE, GATED, STAGE>: per guide layout, the taps' colour behind the geometry test or with it, the clamp's pixels from LDS or through L1
template <bool SURFACE>
static void crtt_launch(const CrttPass& P, bool gated, bool stage, hipStream_t stream)
{
    const dim3 grid = crti_grid(P.width, P.height);
    if (gated && stage) crt_accumulate_kernel<CrttPass, SURFACE, true, true><<<grid, CRTI_BLOCK, 0, stream>>>(P);
    else if (gated) crt_accumulate_kernel<CrttPass, SURFACE, true, false><<<grid, CRTI_BLOCK, 0, stream>>>(P);
    else if (stage) crt_accumulate_kernel<CrttPass, SURFACE, false, true><<<grid, CRTI_BLOCK, 0, stream>>>(P);
    else crt_accumulate_kernel<CrttPass, SURFACE, false, false><<<grid, CRTI_BLOCK, 0, stream>>>(P);
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
    if (!crti_inverse3(R, I)) return CRTT_E_BAD_ARGUMENT;           // singular: the rows span no volume
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
    const int rc = crt_accumulate_check(cur, prev, next, p);
    if (rc != CRTT_OK) return rc;
    CrttPass P;
    crt_accumulate_fill(P, cur, prev, next, p, (p->flags & CRTT_MATCH_INSTANCE) || next->instance);
    const bool gated = crti_env_choice("CRTT_TAPS", "all", "gated", CRTT_TAPS_GATED_DEFAULT != 0);
    const bool stage = (p->flags & CRTT_CLAMP) && crti_env_choice("CRTT_CLAMP_TAPS", "l1", "lds", CRTT_CLAMP_LDS_DEFAULT != 0);
    if (cur->guides == CRTT_GUIDES_SURFACE) crtt_launch<true>(P, gated, stage, (hipStream_t)stream);
    else crtt_launch<false>(P, gated, stage, (hipStream_t)stream);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : CRTT_OK;
}

const char* crtt_error_string(int rc)
{
    return CRTI_ERROR_STRING("crtt", rc);
}

}
