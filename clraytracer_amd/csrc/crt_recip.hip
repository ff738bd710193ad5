// crt_recip.hip -- crt_recip_sweep_kernel, the kernel of crt_debug_recip_sweep (declaration and description: crt_recip.h); fifth translation
// unit of libcrt_hip.so. Build: with the other four units, same flags (Makefile).
#include <hip/hip_runtime.h>
#include "../../include/crt_api.h"
#include "crt_recip.h"

__global__ __launch_bounds__(256) void crt_recip_sweep_kernel(uint32_t first, unsigned long long count, unsigned long long* __restrict__ out)
{
    const unsigned long long threads = (unsigned long long)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long guarded = 0, unguarded = 0, spare = 0, firstBad = ~0ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += threads) {
        const uint32_t bits = first + (uint32_t)i;
        const float x = __uint_as_float(bits);
        const uint32_t want = __float_as_uint(1.0f / x);
        const bool needs = recip_needs_division(x);
        const bool shortRight = __float_as_uint(recip_short(x)) == want;
        // the lane alone: one lane active per turn, so the helper's wave-level decision is this lane's
        uint32_t alone = 0;
        for (uint32_t l = 0; l < 64u; ++l) { if (lane == l) alone = __float_as_uint(recip(x)); }
        // the wave's 64 consecutive patterns under one decision
        const uint32_t together = __float_as_uint(recip(x));
        // three operands under one decision: x beside a scrambled and a complemented pattern
        const v3 d = mk3(x, __uint_as_float(bits * 0x9E3779B1u), __uint_as_float(~bits));
        const v3 r = recip3(d);
        const uint32_t wrong = (uint32_t)(alone != want) + (uint32_t)(together != want) + (uint32_t)(__float_as_uint(r.x) != want)
                             + (uint32_t)(__float_as_uint(r.y) != __float_as_uint(1.0f / d.y)) + (uint32_t)(__float_as_uint(r.z) != __float_as_uint(1.0f / d.z));
        guarded += wrong;
        const bool missed = !shortRight && !needs;
        unguarded += missed ? 1u : 0u;
        spare += (needs && shortRight) ? 1u : 0u;
        if ((wrong != 0 || missed) && i < firstBad) firstBad = i;
    }
    if (guarded) atomicAdd(&out[0], guarded);
    if (unguarded) atomicAdd(&out[1], unguarded);
    if (spare) atomicAdd(&out[2], spare);
    if (firstBad != ~0ull) atomicMin(&out[3], firstBad);
}
