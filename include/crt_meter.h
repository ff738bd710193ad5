/* crt_meter.h -- C ABI of libcrt_meter.so: metering and auto-exposure on device buffers. HIP for gfx950.
 *
 * crtp_present's tone mapper looks right for input near one brightness, and its exposure is a host float. crtx_meter measures a float4 image
 * on the device -- a log-luminance histogram and its sums over a rectangle -- and leaves the exposure that brings the image's average to `key`
 * in a 32-byte record in device memory; crtx_expose multiplies an image by the exposure of such a record, which the kernel reads: the host
 * never sees it, and crtp_present is then called with exposure 1. A library of its own beside libcrt_hip.so and the image libraries
 * (crt_denoise.h, crt_temporal.h, crt_vfilter.h, crt_motion.h, crt_upsample.h, crt_select.h, crt_present.h), stateless like them: every buffer
 * is the caller's; the library creates and destroys no HIP object, allocates nothing, copies nothing and never waits on the host.
 *
 * Conventions: every call returns 0, a negative CRTX_E_* code (the values of CrtStatus) or a positive hipError_t when a launch fails;
 * crtx_error_string explains either. The argument checks need no GPU: the library loads and answers them on a machine without one. Each call
 * ENQUEUES its launches on `stream` (a hipStream_t; NULL: HIP's null stream) AND RETURNS: no synchronisation. Errors come before anything is
 * enqueued.
 *
 * Definition. Every float value is float32 arithmetic without contraction (a*b + c is a multiply, then an add); / is correctly rounded;
 * dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; every comparison with a NaN is false. A pixel's index is k = y*W + x. bits(v) is the uint32 word
 * of a float and as_float(w) the float of a word.
 *   composed(k)    steps 1-2 of crtp_present (crt_present.h), word for word: c = color[k].rgb (alpha is ignored). CRTX_HEAL: a component of c
 *                  that is not finite becomes 0.0f. ao != NULL: f = (1.0f - aoStrength) + aoStrength * ao[k]; under CRTX_HEAL a non-finite f
 *                  becomes 1.0f; c = c * f per component. With ao == NULL the step does not exist.
 *   luminance      the tone mapper's own: l = dot3(composed(k), (0.2126f, 0.7152f, 0.0722f))
 *   log code       a pixel is INVALID if l is a NaN, infinite or < 0 (-0.0f is not). Otherwise q = CRTX_QMIN where l < 0x1p-20f; q = CRTX_QMAX - 1
 *                  where l >= 0x1p12f; q = bits(l) >> 7 elsewhere. CRTX_QMIN = 107 << 16, CRTX_QMAX = 139 << 16: q has 16 fraction bits,
 *                  q / 65536 - 127 is the piecewise-linear log2 of l (the exponent, and the mantissa taken as the fraction), and as_float(q << 7)
 *                  inverts it exactly. That log never exceeds log2 l and falls short of it by at most 0.0861 (at mantissa 1 / ln 2), so an average
 *                  formed in q is the geometric mean of the luminances or up to 6.1 % below it, and never above.
 *   bin            (q - CRTX_QMIN) >> 13: CRTX_HIST_BINS = 256 bins, 8 per octave, over 2^-20 .. 2^12
 *
 * 1. crtx_meter. Statistics over the pixels of the half-open rectangle [x0, x1) x [y0, y1), all of them integers, so that they are the same
 *    bits in whatever order they are summed: valid and invalid (uint32 counts), sumQ (uint64, the sum of q over the valid pixels: at most 2^28
 *    pixels times 2^24), minQ and maxQ (of the valid pixels; both 0 where there is none) and hist[256] (uint32, the valid pixels per bin).
 *    Resolve, with N = valid:
 *      lo = floor((double)lowFraction * N), hi = min(N, ceil((double)highFraction * N)) (both products are exact in double);
 *      if hi <= lo: hi = min(lo + 1, N), then lo = hi - 1.
 *      cum_b = the count below bin b; take_b = max(0, min(cum_b + hist_b, hi) - max(cum_b, lo)): the pixels of bin b among those ranked lo .. hi-1
 *      meanQ = sumQ / N (uint64 floor division) when lowFraction == 0 and highFraction == 1: the exact mean;
 *      else meanQ = (sum over b of take_b * (CRTX_QMIN + (b << 13) + 4096)) / (hi - lo), also uint64: the trimmed mean of the bin centres
 *      average = as_float(meanQ << 7)
 *      target = min(max(key / average, minExposure), maxExposure)
 *      exposure = target, except under CRTX_ADAPT with prev != NULL and p = prev->exposure finite and > 0: then
 *      exposure = min(max(p + (target - p) * (target > p ? rateUp : rateDown), minExposure), maxExposure)
 *      N == 0: meanQ = 0, average = 0.0f and exposure = target = p where p qualifies as above (as it is, not clamped), else 1.0f
 *    result receives a CrtxResult; outHist, where given, hist[256]. result may be the buffer prev names: one lane reads it, then writes it.
 *    The kernels, two launches, no global atomic and no workgroup that waits for another:
 *      histogram  `groups` workgroups of 256 lanes walk the 32 x 8 tiles of the frame's grid that meet the rectangle, workgroup g the tiles g,
 *                 g + groups, ...: a lane reads 16 (+ 4) bytes per pixel, keeps the five sums in registers and adds its bin to its wave's own
 *                 histogram in LDS (4 x 256 words, integer LDS adds). At the end the sums are reduced across the wave's lanes, the waves are
 *                 combined through LDS, and the workgroup stores its partial record -- the 256 bins, then valid, invalid, sumQ (low word, high
 *                 word), minQ, maxQ and two zero words: CRTX_RECORD_WORDS = 264 words -- to scratch[g]. 64 lanes adding to one LDS address is
 *                 the bad case (a constant sky, a black frame, a converged wall), so there are two forms: `plain`, every lane adds 1; `leader`,
 *                 the wave first ballots the lanes whose bin is its first valid lane's, that lane adds their number and only the others add
 *                 1 each. CRTX_BINS=plain|leader in the environment (read by every call; anything else means the built-in choice, plain)
 *                 selects the form. Both give the same bits.
 *      resolve    one workgroup of 256 lanes: lane b sums bin b over the partial records (rows of one stride: coalesced), the sums likewise;
 *                 an exclusive scan over the 256 bins in LDS gives cum_b, the trimmed sum is reduced in 64 bits, lane 0 does the double and
 *                 float arithmetic above and stores the record, and the workgroup stores outHist.
 *    groups: the workgroups of the histogram launch, 1 .. CRTX_MAX_GROUPS, or 0: the library's choice, min(CRTX_DEFAULT_GROUPS, the tiles of
 *    the whole frame). A workgroup without a tile stores an empty record.
 *    scratch: crtx_scratch_bytes(width, height, groups) bytes of the caller's, aligned to 4: one partial record per workgroup, every word of
 *    which the first launch writes. 0 for a size or a groups crtx_meter refuses. Calls on one stream may share their scratch.
 *    CRTX_E_BAD_ARGUMENT  a NULL struct, color, result or scratch; result, outHist or scratch equal to color, ao or one another; outHist or
 *                         scratch equal to prev; an unknown flag; a number that is not finite; aoStrength outside 0..1; !(key > 0);
 *                         lowFraction or highFraction outside 0..1 or lowFraction > highFraction; !(0 < minExposure <= maxExposure); rateUp
 *                         or rateDown outside 0..1; a rectangle that is empty (x0 >= x1 or y0 >= y1) or not inside the frame; groups < 0 or
 *                         > CRTX_MAX_GROUPS; width or height < 1
 *    CRTX_E_OUT_OF_RANGE  width or height > 16384
 *
 * 2. crtx_expose. out[k] = {composed(k) * e per component, color[k].w} with e = ((const CrtxResult*)exposure)->exposure, which the kernel
 *    reads from device memory; e is always multiplied, and used as it is: whatever the record holds. One launch, one lane per pixel over 32 x 8
 *    tiles; e is a kernel-uniform load. out == color is legal (the step is pointwise). crtp_present(out, exposure 1.0f) then gives, for inputs
 *    whose products are finite and without CRTP_HEAL, what crtp_present(color, ao, exposure e) gives, float for float and byte for byte.
 *    CRTX_E_BAD_ARGUMENT  a NULL struct, color, exposure or out; out equal to ao or to exposure; an unknown flag (CRTX_HEAL is the only one);
 *                         a non-finite aoStrength or one outside 0..1; width or height < 1
 *    CRTX_E_OUT_OF_RANGE  width or height > 16384
 *
 * 3. crtx_rate(dt, tau), on the host: the share (float)(1.0 - exp(-dt / tau)) of the way to the target that a frame of dt seconds covers when
 *    the adaptation's time constant is tau seconds -- a value for rateUp or rateDown; 1.0f for tau <= 0 (no adaptation). */
#ifndef CRT_METER_H
#define CRT_METER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CRTX_OK = 0, CRTX_E_BAD_ARGUMENT = -2, CRTX_E_OUT_OF_RANGE = -3 };   /* same values as CrtStatus */
enum { CRTX_HEAL = 1, CRTX_ADAPT = 2 };                                     /* CrtxMeter.flags; CrtxExpose.flags takes CRTX_HEAL only */
enum { CRTX_HIST_BINS = 256, CRTX_QMIN = 107 << 16, CRTX_QMAX = 139 << 16 };     /* the log code and its bins */
enum { CRTX_MAX_GROUPS = 2048, CRTX_DEFAULT_GROUPS = 128, CRTX_RECORD_WORDS = 264 };     /* the histogram launch and its partial records */

/* 32 bytes: exposure 0, target 4, average 8, meanQ 12, valid 16, invalid 20, minQ 24, maxQ 28 */
typedef struct {
    float exposure;         /* what crtx_expose multiplies by */
    float target;           /* the exposure without adaptation: key / average, clamped */
    float average;          /* as_float(meanQ << 7): the metered luminance; 0 where no pixel is valid */
    uint32_t meanQ;
    uint32_t valid, invalid;
    uint32_t minQ, maxQ;    /* of the valid pixels; 0 where there is none */
} CrtxResult;

/* 88 bytes (LP64): width 0, height 4, color 8, ao 16, aoStrength 24, flags 28, x0 32, y0 36, x1 40, y1 44, key 48, lowFraction 52, highFraction 56, minExposure 60, maxExposure 64, rateUp 68, rateDown 72, groups 76, prev 80 */
typedef struct {
    int32_t width, height;
    const void* color;      /* float4[W*H]; alpha is ignored; never written */
    const void* ao;         /* float[W*H] or NULL */
    float aoStrength;       /* 0 .. 1 */
    uint32_t flags;         /* CRTX_HEAL | CRTX_ADAPT */
    int32_t x0, y0, x1, y1; /* the metered rectangle [x0, x1) x [y0, y1), inside the frame and not empty */
    float key;              /* the luminance the average is brought to: finite, > 0 (0.18: middle grey) */
    float lowFraction, highFraction;    /* the ranks that count, 0 <= low <= high <= 1; 0 and 1: all, by the exact mean */
    float minExposure, maxExposure;     /* 0 < min <= max, finite */
    float rateUp, rateDown; /* 0 .. 1: the share of the way to a brighter (darker) target under CRTX_ADAPT; see crtx_rate */
    int32_t groups;         /* workgroups of the histogram launch, 1 .. CRTX_MAX_GROUPS; 0: the library's choice */
    const void* prev;       /* CrtxResult of the frame before, or NULL; may be `result` */
} CrtxMeter;

/* 40 bytes (LP64): width 0, height 4, color 8, ao 16, exposure 24, aoStrength 32, flags 36 */
typedef struct {
    int32_t width, height;
    const void* color;      /* float4[W*H]; may be `out` */
    const void* ao;         /* float[W*H] or NULL */
    const void* exposure;   /* CrtxResult in device memory: its first float is the factor */
    float aoStrength;       /* 0 .. 1 */
    uint32_t flags;         /* CRTX_HEAL */
} CrtxExpose;

size_t crtx_scratch_bytes(int32_t width, int32_t height, int32_t groups);
int crtx_meter(const CrtxMeter* m, void* result /* CrtxResult */, void* outHist /* uint32[256] or NULL */, void* scratch, void* stream);
int crtx_expose(const CrtxExpose* e, void* out /* float4[W*H] */, void* stream);
float crtx_rate(double dt, double tau);
const char* crtx_error_string(int rc);

#ifdef __cplusplus
}
#endif

#endif
