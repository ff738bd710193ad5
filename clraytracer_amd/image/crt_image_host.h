// crt_image_host.h -- the host steps the image libraries share: the launch grid, the rules every argument check applies, the ping-pong of a
// filter's passes, the error strings and the 3 x 3 inverse of the two host-only maps. Headers only (see crt_image_device.h); nothing here
// reads the environment (crt_image_env.h does, and libcrt_motion.so includes this file without it).
#pragma once
#include <math.h>
#include "crt_image_device.h"

#define CRTI_MAX_DIM 16384          // a frame's width and height at most: pixel indices fit 32 bits
// the codes and the guide layouts are the same numbers in every image library's header (each unit asserts its own)
enum { CRTI_OK = 0, CRTI_E_BAD_ARGUMENT = -2, CRTI_E_OUT_OF_RANGE = -3, CRTI_GUIDES_PLANES = 0, CRTI_GUIDES_SURFACE = 1 };

// one workgroup of CRTI_BLOCK lanes per 32 x 8 tile
static inline dim3 crti_grid(int width, int height)
{
    return dim3((unsigned)((width + CRTI_TILE_W - 1) / CRTI_TILE_W), (unsigned)((height + CRTI_TILE_H - 1) / CRTI_TILE_H));
}

// The guide-layout rule: under planes, a plane that is needed must be given; CrtSurfaceHit records carry both and take no plane beside them;
// any other layout is refused.
static inline bool crti_guides_ok(int guides, bool needIds, const void* ids, bool needAlbedo, const void* albedo)
{
    if (guides == CRTI_GUIDES_PLANES) return !((needIds && !ids) || (needAlbedo && !albedo));
    if (guides == CRTI_GUIDES_SURFACE) return !(ids || albedo);
    return false;
}

// does an output alias an input or an earlier output? (an output that is NULL is not asked for; an input that is NULL equals none)
template <int NI, int NO> static inline bool crti_aliased(const void* const (&ins)[NI], const void* const (&outs)[NO])
{
    for (int i = 0; i < NO; ++i) {
        if (!outs[i]) continue;
        for (const void* in : ins)
            if (in == outs[i]) return true;
        for (int j = 0; j < i; ++j)
            if (outs[j] == outs[i]) return true;
    }
    return false;
}

// where launch `pass` of n passes stores: the last lands in `out`, the one before it in `scratch`, and so on backwards
static inline void* crti_pingpong(int n, int pass, void* out, void* scratch) { return ((n - 1 - pass) & 1) ? scratch : out; }

// the strings of <prefix>_error_string: PREFIX is a string literal ("crtd"), rc one of the codes above or a hipError_t
#define CRTI_ERROR_STRING(PREFIX, rc) crti_error_string(rc, PREFIX ": bad argument", PREFIX ": out of range (a frame wider or taller than 16384)", PREFIX ": unknown error")
static inline const char* crti_error_string(int rc, const char* bad, const char* range, const char* unknown)
{
    switch (rc) {
    case CRTI_OK: return "ok";
    case CRTI_E_BAD_ARGUMENT: return bad;
    case CRTI_E_OUT_OF_RANGE: return range;
    default: return rc > 0 ? hipGetErrorString((hipError_t)rc) : unknown;
    }
}

// a 3 x 3 inverse in double by cofactors; false when the rows span no volume
static inline bool crti_inverse3(const double R[3][3], double I[3][3])
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
