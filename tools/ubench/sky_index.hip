// The device self-check of the guarded float skybox index (clraytracer_amd/csrc/crt_device.h: sample_skybox_guarded, sky_index_float) against
// the double form (sample_skybox): a stand-alone program over the library's own header, built with the library's flags (Makefile), so that
// its kernels are no rows of the library's kernel-resource ledger. tests/test_gpu_sky_index.py runs it.
//   sky_index dirs <in> <n> <texW> <texH> <out>
//       <in>: n directions, 3 n floats; direction i on thread i, so 64 consecutive directions share a call and its wave-level decision.
//       <out>: n int32 the index the shipped function returns (sky_index<false>: what the uncounted kernels call), n int32 the double form's,
//       n bytes 1 if the float decision alone answered the lane. Indices are not clamped to a pool.
//   sky_index sweep <axis> <first> <count> <xbits> <ybits> <zbits> <texW> <texH>
//       component <axis> (0 x, 1 y, 2 z) of the direction with the given float bit patterns (hex) takes the <count> (<= 2^32) patterns <first>,
//       <first> + 1, ... (mod 2^32); nothing is normalised. Prints: lanes decided in float, lanes left to the double form, lanes whose shipped index
//       differs from the double form's (must be 0), the first such pattern in sweep order (18446744073709551615 if none).
// Exit status 0, 2 for a bad command line, 1 for a HIP error.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/crt_api.h"
#include "../../clraytracer_amd/csrc/crt_device.h"

__global__ __launch_bounds__(256) void sky_index_kernel(const float* __restrict__ dirs, uint32_t n, int texW, int texH, int* __restrict__ shipped,
                                                        int* __restrict__ doubleOnly, unsigned char* __restrict__ decided)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const v3 d = mk3(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]);
    int theta, phi;
    decided[i] = sky_index_float(d, texW, texH, theta, phi) ? 1 : 0;
    shipped[i] = sky_index<false>(d, texW, texH);
    doubleOnly[i] = sample_skybox(d, texW, texH);
}

__global__ __launch_bounds__(256) void sky_sweep_kernel(int axis, uint32_t first, unsigned long long count, float x, float y, float z, int texW, int texH,
                                                        unsigned long long* __restrict__ out)
{
    const unsigned long long threads = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long nDecided = 0, nUndecided = 0, nDiffer = 0, firstBad = ~0ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += threads) {
        const float v = __uint_as_float(first + (uint32_t)i);
        const v3 d = mk3(axis == 0 ? v : x, axis == 1 ? v : y, axis == 2 ? v : z);
        int theta, phi;
        const bool dec = sky_index_float(d, texW, texH, theta, phi);
        const bool differ = sky_index<false>(d, texW, texH) != sample_skybox(d, texW, texH);
        nDecided += dec ? 1u : 0u;
        nUndecided += dec ? 0u : 1u;
        nDiffer += differ ? 1u : 0u;
        if (differ && i < firstBad) firstBad = i;
    }
    if (nDecided) atomicAdd(&out[0], nDecided);
    if (nUndecided) atomicAdd(&out[1], nUndecided);
    if (nDiffer) atomicAdd(&out[2], nDiffer);
    if (firstBad != ~0ull) atomicMin(&out[3], firstBad);
}

#define CHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

static float bits_to_float(const char* s) { const uint32_t u = (uint32_t)strtoul(s, nullptr, 16); float f; memcpy(&f, &u, 4); return f; }

int main(int argc, char** argv)
{
    if (argc == 7 && !strcmp(argv[1], "dirs")) {
        const unsigned long long n = strtoull(argv[3], nullptr, 10);
        const int texW = atoi(argv[4]), texH = atoi(argv[5]);
        if (n == 0 || n > (1ull << 24)) return 2;
        std::vector<float> h(3 * n);
        FILE* f = fopen(argv[2], "rb");
        if (!f || fread(h.data(), sizeof(float), 3 * n, f) != 3 * n) return 2;
        fclose(f);
        float* dd; int* di; unsigned char* dc;
        CHK(hipMalloc(&dd, 3 * n * sizeof(float))); CHK(hipMalloc(&di, 2 * n * sizeof(int))); CHK(hipMalloc(&dc, n));
        CHK(hipMemcpy(dd, h.data(), 3 * n * sizeof(float), hipMemcpyHostToDevice));
        sky_index_kernel<<<(unsigned)((n + 255) / 256), 256>>>(dd, (uint32_t)n, texW, texH, di, di + n, dc);
        CHK(hipGetLastError());
        std::vector<int> hi(2 * n); std::vector<unsigned char> hc(n);
        CHK(hipMemcpy(hi.data(), di, 2 * n * sizeof(int), hipMemcpyDeviceToHost));
        CHK(hipMemcpy(hc.data(), dc, n, hipMemcpyDeviceToHost));
        CHK(hipFree(dd)); CHK(hipFree(di)); CHK(hipFree(dc));
        FILE* o = fopen(argv[6], "wb");
        if (!o || fwrite(hi.data(), sizeof(int), 2 * n, o) != 2 * n || fwrite(hc.data(), 1, n, o) != n) return 2;
        fclose(o);
        return 0;
    }
    if (argc == 10 && !strcmp(argv[1], "sweep")) {
        const int axis = atoi(argv[2]);
        const uint32_t first = (uint32_t)strtoul(argv[3], nullptr, 0);
        const unsigned long long count = strtoull(argv[4], nullptr, 0);
        const float x = bits_to_float(argv[5]), y = bits_to_float(argv[6]), z = bits_to_float(argv[7]);
        const int texW = atoi(argv[8]), texH = atoi(argv[9]);
        if (axis < 0 || axis > 2 || count > (1ull << 32)) return 2;
        unsigned long long h[4] = { 0, 0, 0, ~0ull }, *d;
        CHK(hipMalloc(&d, sizeof h));
        CHK(hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice));
        if (count) {
            const unsigned long long blocks = (count + 255) / 256;
            sky_sweep_kernel<<<(unsigned)(blocks < 4096 ? blocks : 4096), 256>>>(axis, first, count, x, y, z, texW, texH, d);
            CHK(hipGetLastError());
        }
        CHK(hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost));
        CHK(hipFree(d));
        const unsigned long long bad = h[3] == ~0ull ? ~0ull : (unsigned long long)(uint32_t)(first + (uint32_t)h[3]);
        printf("%llu %llu %llu %llu\n", h[0], h[1], h[2], bad);
        return 0;
    }
    fprintf(stderr, "usage: sky_index dirs <in> <n> <texW> <texH> <out> | sky_index sweep <axis> <first> <count> <xbits> <ybits> <zbits> <texW> <texH>\n");
    return 2;
}
