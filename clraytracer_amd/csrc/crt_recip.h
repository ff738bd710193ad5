// crt_recip.h -- crt_debug_recip_sweep's kernel: the traversal's short reciprocal (crt_device.h: recip, recip3, recip_short) against the
// device's own `1.0f / x`, bit pattern by bit pattern. Compiled in a translation unit of its own (crt_recip.hip, the fifth of
// libcrt_hip.so) and launched from crt_shim.hip, as the query kernels are: the kernel lists of the older units stay what they are.
#pragma once
#include "crt_device.h"

// Patterns first, first + 1, ..., first + count - 1 (mod 2^32; count <= 2^32), pattern first + i on thread i mod (threads of the grid) --
// so a wave holds 64 consecutive patterns. out[0..3], added to / lowered with atomics (the caller sets 0, 0, 0, ~0):
//   out[0]  results of the GUARDED helpers that are not the bits of `1.0f / x`: recip() with the lane alone in its wave step (its
//           guard decision is its own), recip() again with the wave's active lanes deciding together, and recip3() on (x, two other
//           patterns derived from x) deciding for the three at once -- each compared component by component
//   out[1]  patterns the unguarded short sequence gets wrong although the guard does NOT send them to the division
//   out[2]  patterns the guard sends to the division although the short sequence is right (how tight the guard is)
//   out[3]  the smallest i with a pattern counted in out[0] or out[1]
__global__ void crt_recip_sweep_kernel(uint32_t first, unsigned long long count, unsigned long long* __restrict__ out);
