// crt_image_device.h -- the device steps the image libraries share (libcrt_denoise.so, libcrt_temporal.so, libcrt_vfilter.so, libcrt_motion.so):
// vector loads and stores, the two guide layouts, the small predicates and weights, and the 32 x 8 tile with its halo. Headers only: each
// library compiles its own copy, there is no state and no exported name here. Every function is __forceinline__, and every arithmetic
// expression stands as the kernels had it: where two kernels formed the same value by different instructions, both shapes are kept.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define CRTI_TILE_W 32              // 256 lanes over a 32 x 8 tile: a wave is two 512-B rows of float4
#define CRTI_TILE_H 8
#define CRTI_BLOCK (CRTI_TILE_W * CRTI_TILE_H)
#define CRTI_MISS 99999.0f          // the distance of a pixel that is no hit, and of one taken as outside the frame

// 16-B and 8-B rows as one vector load or store each (a float4 copied as a struct can be split into a 12-B copy through the stack and a float)
typedef float crti_f4 __attribute__((ext_vector_type(4)));
typedef float crti_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 crti_load4(const void* p) { const crti_f4 v = *(const crti_f4*)p; return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void crti_store4(float4* p, float4 v) { crti_f4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; *(crti_f4*)p = r; }
__device__ __forceinline__ float2 crti_load2(const void* p) { const crti_f2 v = *(const crti_f2*)p; return make_float2(v.x, v.y); }
__device__ __forceinline__ void crti_store2(float2* p, float2 v) { crti_f2 r; r.x = v.x; r.y = v.y; *(crti_f2*)p = r; }

// the strides of the two guide layouts: three planes (16, 16, 4 B) or CrtSurfaceHit records (48 B; geometry at 0, instance at 16, albedo at 32).
// P is a kernel's launch struct: `geometry`, `instance` and `albedo` are its byte pointers, the record's offset already added
template <bool SURFACE, class P_> __device__ __forceinline__ float4 crti_geometry(const P_& P, size_t i) { return crti_load4(P.geometry + i * (SURFACE ? 48 : 16)); }
template <bool SURFACE, class P_> __device__ __forceinline__ float crti_distance(const P_& P, size_t i) { return *(const float*)(P.geometry + i * (SURFACE ? 48 : 16) + 12); }
template <bool SURFACE, class P_> __device__ __forceinline__ int crti_instance(const P_& P, size_t i) { return *(const int*)(P.instance + i * (SURFACE ? 48 : 16)); }
template <bool SURFACE, class P_> __device__ __forceinline__ uint32_t crti_albedo(const P_& P, size_t i) { return *(const uint32_t*)(P.albedo + i * (SURFACE ? 48 : 4)); }

__device__ __forceinline__ bool crti_hit(float t) { return t <= 99998.0f; }
__device__ __forceinline__ float crti_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
__device__ __forceinline__ float crti_dot3(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float crti_luma(float x, float y, float z) { return (0.299f * x + 0.587f * y) + 0.114f * z; }
__device__ __forceinline__ float crti_luma(float4 c) { return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z; }
__device__ __forceinline__ bool crti_finite(float v) { return __builtin_isfinite(v); }
__device__ __forceinline__ float crti_k(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }      // the a-trous weights

// The index of pixel (qx, qy) clamped into the frame. Pixel indices fit 32 bits (16384 x 16384 at most), so the product is a 32-bit one widened
// afterwards; WIDE forms it by 64-bit multiplies, as crtd_pass_kernel does for its centre and its staging.
template <bool WIDE = false> __device__ __forceinline__ size_t crti_clamped(int qx, int qy, int W, int H)
{
    if (WIDE) return (size_t)min(max(qy, 0), H - 1) * (size_t)W + (size_t)min(max(qx, 0), W - 1);
    return (size_t)(uint32_t)(min(max(qy, 0), H - 1) * W + min(max(qx, 0), W - 1));
}
// ... of a lane's own pixel, which lies neither left of nor above the frame
template <bool WIDE = false> __device__ __forceinline__ size_t crti_clamped_own(int x, int y, int W, int H)
{
    if (WIDE) return (size_t)min(y, H - 1) * (size_t)W + (size_t)min(x, W - 1);
    return (size_t)(uint32_t)(min(y, H - 1) * W + min(x, W - 1));
}
// is pixel (qx, qy) inside the frame? A macro: as a function's result the && chain compiles to other branches than it does as a condition
#define CRTI_INSIDE(qx, qy, W, H) ((qx) >= 0 && (qx) < (W) && (qy) >= 0 && (qy) < (H))

// A lane's place in the launch grid of crt_image_host.h: (lx, ly) in its workgroup's tile, whose first pixel is (x0, y0); (x, y) is its own
struct CrtiLane {
    int lx, ly, x0, y0, x, y;
    __device__ __forceinline__ CrtiLane()
    {
        lx = (int)(threadIdx.x & (CRTI_TILE_W - 1)); ly = (int)(threadIdx.x / CRTI_TILE_W);
        x0 = (int)blockIdx.x * CRTI_TILE_W; y0 = (int)blockIdx.y * CRTI_TILE_H;
        x = x0 + lx; y = y0 + ly;
    }
};

// The tile and a halo of HALO pixels, staged row-major in LDS by the workgroup in ROUNDS rounds: round j of a lane is element i = lane + 256 j,
// which is pixel (px, py) and is stored only where i < N. ROWS_FIRST: py is formed before px, as crt_accumulate_kernel has always done (the
// two orders are scheduled differently, and each kernel keeps its own).
template <int HALO, bool ROWS_FIRST = false> struct CrtiTile {
    static constexpr int TW = CRTI_TILE_W + 2 * HALO, TH = CRTI_TILE_H + 2 * HALO, N = TW * TH, ROUNDS = (N + CRTI_BLOCK - 1) / CRTI_BLOCK;
    int i, px, py;
    __device__ __forceinline__ CrtiTile(int j, int x0, int y0)
    {
        i = (int)threadIdx.x + j * CRTI_BLOCK;
        const int ty = i / TW, tx = i - ty * TW;
        if (ROWS_FIRST) { py = y0 - HALO + ty; px = x0 - HALO + tx; }
        else { px = x0 - HALO + tx; py = y0 - HALO + ty; }
    }
    template <bool WIDE = false> __device__ __forceinline__ size_t clamped(int W, int H) const { return crti_clamped<WIDE>(px, py, W, H); }
};
