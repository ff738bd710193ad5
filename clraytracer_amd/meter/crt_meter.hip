// crt_meter.hip -- libcrt_meter.so: crtx_meter, crtx_expose and crtx_rate of include/crt_meter.h (definition there), their kernels and the C ABI
// over them. The only translation unit of the library, written over the shared steps of the image libraries (../image/crt_image_device.h and
// crt_image_host.h: vector loads, the 32 x 8 tile, the rules of the argument check; crt_image_env.h: the environment switch). It shares no
// state; its one switch chooses how a wave adds its bins (CRTX_BINS=plain|leader). The only atomics are integer adds to LDS;
// no kernel touches global memory with one, and none waits for another workgroup.
// Build: the Makefile's $(METER_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include "../../include/crt_meter.h"
#include "../image/crt_image_host.h"
#include "../image/crt_image_env.h"

#define CRTX_FLAGS_ALL (CRTX_HEAL | CRTX_ADAPT)
// how a wave adds its bins unless CRTX_BINS says otherwise: 0 = plain, 1 = leader (profiles/meter_rate.txt)
#define CRTX_LEADER_DEFAULT 0
#define CRTX_WAVES (CRTI_BLOCK / 64)
// the ABI of crt_meter.h (clraytracer_amd/_lib.py mirrors it)
static_assert(sizeof(CrtxResult) == 32 && offsetof(CrtxResult, target) == 4 && offsetof(CrtxResult, average) == 8 && offsetof(CrtxResult, meanQ) == 12
              && offsetof(CrtxResult, valid) == 16 && offsetof(CrtxResult, invalid) == 20 && offsetof(CrtxResult, minQ) == 24 && offsetof(CrtxResult, maxQ) == 28,
              "CrtxResult");
static_assert(sizeof(CrtxMeter) == 88 && offsetof(CrtxMeter, height) == 4 && offsetof(CrtxMeter, color) == 8 && offsetof(CrtxMeter, ao) == 16
              && offsetof(CrtxMeter, aoStrength) == 24 && offsetof(CrtxMeter, flags) == 28 && offsetof(CrtxMeter, x0) == 32 && offsetof(CrtxMeter, y0) == 36
              && offsetof(CrtxMeter, x1) == 40 && offsetof(CrtxMeter, y1) == 44 && offsetof(CrtxMeter, key) == 48 && offsetof(CrtxMeter, lowFraction) == 52
              && offsetof(CrtxMeter, highFraction) == 56 && offsetof(CrtxMeter, minExposure) == 60 && offsetof(CrtxMeter, maxExposure) == 64
              && offsetof(CrtxMeter, rateUp) == 68 && offsetof(CrtxMeter, rateDown) == 72 && offsetof(CrtxMeter, groups) == 76 && offsetof(CrtxMeter, prev) == 80,
              "CrtxMeter");
static_assert(sizeof(CrtxExpose) == 40 && offsetof(CrtxExpose, height) == 4 && offsetof(CrtxExpose, color) == 8 && offsetof(CrtxExpose, ao) == 16
              && offsetof(CrtxExpose, exposure) == 24 && offsetof(CrtxExpose, aoStrength) == 32 && offsetof(CrtxExpose, flags) == 36 && sizeof(float4) == 16,
              "CrtxExpose");
static_assert(CRTX_OK == CRTI_OK && CRTX_E_BAD_ARGUMENT == CRTI_E_BAD_ARGUMENT && CRTX_E_OUT_OF_RANGE == CRTI_E_OUT_OF_RANGE, "the codes of crt_image_host.h");
static_assert(CRTI_BLOCK == 256 && CRTX_HIST_BINS == CRTI_BLOCK && CRTX_WAVES == 4, "256-lane workgroups: a lane per bin, four waves");
static_assert(((CRTX_QMAX - 1 - CRTX_QMIN) >> 13) == CRTX_HIST_BINS - 1 && CRTX_RECORD_WORDS >= CRTX_HIST_BINS + 6 && CRTX_RECORD_WORDS % 8 == 0, "bins and records");

// the words of a partial record behind its bins
enum { CRTX_W_VALID = CRTX_HIST_BINS, CRTX_W_INVALID, CRTX_W_SUM_LO, CRTX_W_SUM_HI, CRTX_W_MIN, CRTX_W_MAX, CRTX_W_ZERO };

// ---- the steps both calls share ----------------------------------------------------------------------------------------------------------------
// composed(k) of crt_meter.h: steps 1-2 of crtp_present. ao is kernel-uniform; alpha comes back untouched
template <bool HEAL> __device__ __forceinline__ float4 crtx_composed(const float4* color, const float* ao, float aoStrength, size_t k)
{
    float4 c = crti_load4(color + k);
    if (HEAL) { c.x = crti_finite(c.x) ? c.x : 0.0f; c.y = crti_finite(c.y) ? c.y : 0.0f; c.z = crti_finite(c.z) ? c.z : 0.0f; }
    if (ao) {
        float f = (1.0f - aoStrength) + aoStrength * ao[k];
        if (HEAL) f = crti_finite(f) ? f : 1.0f;
        c.x = c.x * f; c.y = c.y * f; c.z = c.z * f;
    }
    return c;
}

// the five sums as a lane, a wave and a workgroup hold them
struct CrtxSums {
    uint32_t valid, invalid, minQ, maxQ;
    unsigned long long sumQ;
    __device__ __forceinline__ void clear() { valid = 0u; invalid = 0u; minQ = 0xFFFFFFFFu; maxQ = 0u; sumQ = 0ull; }
    __device__ __forceinline__ void join(const CrtxSums& o)
    {
        valid += o.valid; invalid += o.invalid; sumQ += o.sumQ; minQ = min(minQ, o.minQ); maxQ = max(maxQ, o.maxQ);
    }
};
__device__ __forceinline__ unsigned long long crtx_sum_across_wave(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// every lane of the wave receives the wave's sums
__device__ __forceinline__ CrtxSums crtx_across_wave(CrtxSums s)
{
    for (int off = 32; off > 0; off >>= 1) {
        CrtxSums o;
        o.valid = __shfl_xor(s.valid, off, 64); o.invalid = __shfl_xor(s.invalid, off, 64); o.minQ = __shfl_xor(s.minQ, off, 64);
        o.maxQ = __shfl_xor(s.maxQ, off, 64); o.sumQ = __shfl_xor(s.sumQ, off, 64);
        s.join(o);
    }
    return s;
}

// ---- crtx_meter: the histogram launch ----------------------------------------------------------------------------------------------------------
struct CrtxHistogramLaunch {
    const float4* color;
    const float* ao;                // NULL: step 2 does not exist
    uint32_t* records;              // gridDim.x partial records of CRTX_RECORD_WORDS words
    int width;
    int x0, y0, x1, y1;             // the rectangle
    int tx0, ty0, tilesX, tiles;    // the tiles of the frame's grid that meet it: tilesX per row from tile (tx0, ty0), `tiles` in all
    float aoStrength;
};

// Workgroup g walks tiles g, g + groups, ...; a lane's pixel counts where it lies in the rectangle. LEADER: see crt_meter.h. The loop and the
// ballots run with all 64 lanes of a wave active (the tile is workgroup-uniform); only the adds are under a lane's own condition
template <bool HEAL, bool LEADER>
__global__ __launch_bounds__(CRTI_BLOCK) void crtx_histogram_kernel(CrtxHistogramLaunch P)
{
    __shared__ uint32_t s_hist[CRTX_WAVES][CRTX_HIST_BINS];
    __shared__ CrtxSums s_sums[CRTX_WAVES];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lx = tid & (CRTI_TILE_W - 1), ly = tid / CRTI_TILE_W;
#pragma unroll
    for (int w = 0; w < CRTX_WAVES; ++w) s_hist[w][tid] = 0u;
    __syncthreads();
    uint32_t* const hist = s_hist[wave];
    CrtxSums mine;
    mine.clear();
    for (int t = (int)blockIdx.x; t < P.tiles; t += (int)gridDim.x) {
        const int ty = t / P.tilesX, tx = t - ty * P.tilesX;
        const int x = (P.tx0 + tx) * CRTI_TILE_W + lx, y = (P.ty0 + ty) * CRTI_TILE_H + ly;
        bool counts = false;
        uint32_t bin = 0u;
        if (x >= P.x0 && x < P.x1 && y >= P.y0 && y < P.y1) {
            const float4 c = crtx_composed<HEAL>(P.color, P.ao, P.aoStrength, (size_t)(uint32_t)(y * P.width + x));
            const float l = crti_dot3(c.x, c.y, c.z, 0.2126f, 0.7152f, 0.0722f);
            if (l >= 0.0f && l < __builtin_inff()) {
                const uint32_t q = l < 0x1p-20f ? (uint32_t)CRTX_QMIN : l >= 0x1p12f ? (uint32_t)CRTX_QMAX - 1u : __float_as_uint(l) >> 7;
                mine.valid += 1u; mine.sumQ += q; mine.minQ = min(mine.minQ, q); mine.maxQ = max(mine.maxQ, q);
                bin = (q - (uint32_t)CRTX_QMIN) >> 13;
                counts = true;
            } else
                mine.invalid += 1u;
        }
        if (LEADER) {
            const unsigned long long any = __ballot(counts);
            if (any != 0ull) {                                                                  // (wave-uniform)
                const int leader = __ffsll((long long)any) - 1;
                const uint32_t its = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
                const unsigned long long same = __ballot(counts && bin == its);
                if (lane == leader) atomicAdd(&hist[its], (uint32_t)__popcll(same));
                else if (counts && bin != its) atomicAdd(&hist[bin], 1u);
            }
        } else if (counts)
            atomicAdd(&hist[bin], 1u);
    }
    const CrtxSums waves = crtx_across_wave(mine);
    if (lane == 0) s_sums[wave] = waves;
    __syncthreads();
    uint32_t* const record = P.records + (size_t)blockIdx.x * CRTX_RECORD_WORDS;
    record[tid] = (s_hist[0][tid] + s_hist[1][tid]) + (s_hist[2][tid] + s_hist[3][tid]);
    if (tid < CRTX_RECORD_WORDS - CRTX_HIST_BINS) {
        CrtxSums all = s_sums[0];
#pragma unroll
        for (int w = 1; w < CRTX_WAVES; ++w) all.join(s_sums[w]);
        const int word = CRTX_HIST_BINS + tid;
        record[word] = word == CRTX_W_VALID ? all.valid : word == CRTX_W_INVALID ? all.invalid : word == CRTX_W_SUM_LO ? (uint32_t)all.sumQ
                     : word == CRTX_W_SUM_HI ? (uint32_t)(all.sumQ >> 32) : word == CRTX_W_MIN ? all.minQ : word == CRTX_W_MAX ? all.maxQ : 0u;
    }
}

// ---- crtx_meter: the resolve launch ------------------------------------------------------------------------------------------------------------
struct CrtxResolveLaunch {
    const uint32_t* records;
    int groups;
    const CrtxResult* prev;         // NULL unless CRTX_ADAPT and a record was given; may be `result`
    CrtxResult* result;
    uint32_t* outHist;              // may be NULL
    float key, lowFraction, highFraction, minExposure, maxExposure, rateUp, rateDown;
};

__device__ __forceinline__ float crtx_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// One workgroup: lane b owns bin b
__global__ __launch_bounds__(CRTI_BLOCK) void crtx_resolve_kernel(CrtxResolveLaunch P)
{
    __shared__ uint32_t s_scan[2][CRTX_HIST_BINS];
    __shared__ CrtxSums s_sums[CRTX_WAVES];
    __shared__ unsigned long long s_trimmed[CRTX_WAVES];
    __shared__ uint32_t s_range[2];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // (one row after the other: the loop runs at a load's latency per record, 0.13 us each -- profiles/meter_rate.txt)
    uint32_t count = 0u;
    for (int g = 0; g < P.groups; ++g) count += P.records[(size_t)g * CRTX_RECORD_WORDS + tid];
    CrtxSums mine;
    mine.clear();
    for (int g = tid; g < P.groups; g += CRTI_BLOCK) {
        const uint32_t* r = P.records + (size_t)g * CRTX_RECORD_WORDS;
        CrtxSums o;
        o.valid = r[CRTX_W_VALID]; o.invalid = r[CRTX_W_INVALID]; o.minQ = r[CRTX_W_MIN]; o.maxQ = r[CRTX_W_MAX];
        o.sumQ = (unsigned long long)r[CRTX_W_SUM_LO] | ((unsigned long long)r[CRTX_W_SUM_HI] << 32);
        mine.join(o);
    }
    const CrtxSums waves = crtx_across_wave(mine);
    if (lane == 0) s_sums[wave] = waves;
    // inclusive scan of the bins, Hillis and Steele's, between two rows of LDS; 8 steps end in row 0
    s_scan[0][tid] = count;
    __syncthreads();
    int row = 0;
#pragma unroll
    for (int off = 1; off < CRTX_HIST_BINS; off <<= 1) {
        s_scan[row ^ 1][tid] = s_scan[row][tid] + (tid >= off ? s_scan[row][tid - off] : 0u);
        row ^= 1;
        __syncthreads();
    }
    const uint32_t below = s_scan[row][tid] - count;                                           // cum_b
    CrtxSums all = s_sums[0];
#pragma unroll
    for (int w = 1; w < CRTX_WAVES; ++w) all.join(s_sums[w]);
    const uint32_t N = all.valid;
    const bool exact = P.lowFraction == 0.0f && P.highFraction == 1.0f;
    if (tid == 0 && N != 0u) {
        uint32_t lo = (uint32_t)floor((double)P.lowFraction * (double)N), hi = min(N, (uint32_t)ceil((double)P.highFraction * (double)N));
        if (hi <= lo) { hi = min(lo + 1u, N); lo = hi - 1u; }
        s_range[0] = lo; s_range[1] = hi;
    }
    __syncthreads();
    unsigned long long trimmed = 0ull;
    if (N != 0u && !exact) {                                                                    // (workgroup-uniform)
        const int lo = (int)s_range[0], hi = (int)s_range[1];
        const int take = max(0, min((int)(below + count), hi) - max((int)below, lo));
        trimmed = crtx_sum_across_wave((unsigned long long)(uint32_t)take * (unsigned long long)((uint32_t)CRTX_QMIN + ((uint32_t)tid << 13) + 4096u));
    }
    if (lane == 0) s_trimmed[wave] = trimmed;
    __syncthreads();
    if (P.outHist) P.outHist[tid] = count;
    if (tid != 0) return;
    float p = 0.0f;
    if (P.prev) p = P.prev->exposure;
    const bool adapt = P.prev && crti_finite(p) && p > 0.0f;
    CrtxResult R;
    R.valid = N; R.invalid = all.invalid;
    if (N == 0u) {
        R.meanQ = 0u; R.average = 0.0f; R.minQ = 0u; R.maxQ = 0u;
        R.exposure = R.target = adapt ? p : 1.0f;
    } else {
        const unsigned long long sum = exact ? all.sumQ : (s_trimmed[0] + s_trimmed[1]) + (s_trimmed[2] + s_trimmed[3]);
        R.meanQ = (uint32_t)(sum / (unsigned long long)(exact ? N : s_range[1] - s_range[0]));
        R.average = __uint_as_float(R.meanQ << 7);
        R.minQ = all.minQ; R.maxQ = all.maxQ;
        R.target = crtx_clamp(P.key / R.average, P.minExposure, P.maxExposure);
        R.exposure = adapt ? crtx_clamp(p + (R.target - p) * (R.target > p ? P.rateUp : P.rateDown), P.minExposure, P.maxExposure) : R.target;
    }
    uint32_t* const out = (uint32_t*)P.result;
    out[0] = __float_as_uint(R.exposure); out[1] = __float_as_uint(R.target); out[2] = __float_as_uint(R.average); out[3] = R.meanQ;
    out[4] = R.valid; out[5] = R.invalid; out[6] = R.minQ; out[7] = R.maxQ;
}

// ---- crtx_expose -------------------------------------------------------------------------------------------------------------------------------
struct CrtxExposeLaunch {
    const float4* color;
    const float* ao;
    const float* exposure;          // the record's first float
    float4* out;                    // may be `color`
    int width, height;
    float aoStrength;
};

// One lane per pixel of a 32 x 8 tile; the factor is one load for the whole launch
template <bool HEAL>
__global__ __launch_bounds__(CRTI_BLOCK) void crtx_expose_kernel(CrtxExposeLaunch P)
{
    const CrtiLane L;
    if (L.x >= P.width || L.y >= P.height) return;
    const float e = *P.exposure;
    const size_t k = (size_t)(uint32_t)(L.y * P.width + L.x);
    const float4 c = crtx_composed<HEAL>(P.color, P.ao, P.aoStrength, k);
    crti_store4(P.out + k, make_float4(c.x * e, c.y * e, c.z * e, c.w));
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------------------
static int crtx_check_size(int32_t width, int32_t height)
{
    if (width < 1 || height < 1) return CRTX_E_BAD_ARGUMENT;
    if (width > CRTI_MAX_DIM || height > CRTI_MAX_DIM) return CRTX_E_OUT_OF_RANGE;
    return CRTX_OK;
}

static inline bool crtx_unit(float v) { return v >= 0.0f && v <= 1.0f; }        // (false for a NaN)

// the workgroups of the histogram launch for a frame and a `groups` that passed the check
static int crtx_groups(int32_t width, int32_t height, int32_t groups)
{
    if (groups != 0) return groups;
    const dim3 grid = crti_grid(width, height);
    const long long tiles = (long long)grid.x * (long long)grid.y;
    return (int)(tiles < CRTX_DEFAULT_GROUPS ? tiles : CRTX_DEFAULT_GROUPS);
}

static int crtx_check_meter(const CrtxMeter* m, const void* result, const void* outHist, const void* scratch)
{
    if (!m || !m->color || !result || !scratch) return CRTX_E_BAD_ARGUMENT;
    if (m->flags & ~(uint32_t)CRTX_FLAGS_ALL) return CRTX_E_BAD_ARGUMENT;
    const float numbers[8] = {m->aoStrength, m->key, m->lowFraction, m->highFraction, m->minExposure, m->maxExposure, m->rateUp, m->rateDown};
    for (float v : numbers)
        if (!isfinite(v)) return CRTX_E_BAD_ARGUMENT;
    if (!crtx_unit(m->aoStrength) || !(m->key > 0.0f)) return CRTX_E_BAD_ARGUMENT;
    if (!crtx_unit(m->lowFraction) || !crtx_unit(m->highFraction) || m->lowFraction > m->highFraction) return CRTX_E_BAD_ARGUMENT;
    if (!(m->minExposure > 0.0f) || !(m->minExposure <= m->maxExposure)) return CRTX_E_BAD_ARGUMENT;
    if (!crtx_unit(m->rateUp) || !crtx_unit(m->rateDown)) return CRTX_E_BAD_ARGUMENT;
    if (m->groups < 0 || m->groups > CRTX_MAX_GROUPS) return CRTX_E_BAD_ARGUMENT;
    const void* const ins[2] = {m->color, m->ao};
    const void* const outs[3] = {result, outHist, scratch};
    if (crti_aliased(ins, outs)) return CRTX_E_BAD_ARGUMENT;
    if (m->prev && (m->prev == outHist || m->prev == scratch)) return CRTX_E_BAD_ARGUMENT;      // (result may be prev)
    const int rc = crtx_check_size(m->width, m->height);
    if (rc != CRTX_OK) return rc;
    if (m->x0 < 0 || m->y0 < 0 || m->x0 >= m->x1 || m->y0 >= m->y1 || m->x1 > m->width || m->y1 > m->height) return CRTX_E_BAD_ARGUMENT;
    return CRTX_OK;
}

static int crtx_check_expose(const CrtxExpose* e, const void* out)
{
    if (!e || !e->color || !e->exposure || !out) return CRTX_E_BAD_ARGUMENT;
    if (e->flags & ~(uint32_t)CRTX_HEAL) return CRTX_E_BAD_ARGUMENT;
    if (!isfinite(e->aoStrength) || !crtx_unit(e->aoStrength)) return CRTX_E_BAD_ARGUMENT;
    if (out == e->ao || out == e->exposure) return CRTX_E_BAD_ARGUMENT;                         // (out may be color)
    return crtx_check_size(e->width, e->height);
}

static inline int crtx_launched()
{
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : CRTX_OK;
}

// how a wave adds its bins: CRTX_BINS=plain|leader in the environment (crt_image_env.h), else the built-in choice
static bool crtx_bins_leader() { return crti_env_choice("CRTX_BINS", "plain", "leader", CRTX_LEADER_DEFAULT != 0); }

template <bool HEAL> static void crtx_launch_histogram(const CrtxHistogramLaunch& P, bool leader, int groups, hipStream_t s)
{
    if (leader) crtx_histogram_kernel<HEAL, true><<<dim3((unsigned)groups), CRTI_BLOCK, 0, s>>>(P);
    else crtx_histogram_kernel<HEAL, false><<<dim3((unsigned)groups), CRTI_BLOCK, 0, s>>>(P);
}

extern "C" {

size_t crtx_scratch_bytes(int32_t width, int32_t height, int32_t groups)
{
    if (crtx_check_size(width, height) != CRTX_OK || groups < 0 || groups > CRTX_MAX_GROUPS) return 0;
    return (size_t)crtx_groups(width, height, groups) * CRTX_RECORD_WORDS * sizeof(uint32_t);
}

int crtx_meter(const CrtxMeter* m, void* result, void* outHist, void* scratch, void* stream)
{
    int rc = crtx_check_meter(m, result, outHist, scratch);
    if (rc != CRTX_OK) return rc;
    const int groups = crtx_groups(m->width, m->height, m->groups);
    const hipStream_t s = (hipStream_t)stream;
    CrtxHistogramLaunch P;
    P.color = (const float4*)m->color; P.ao = (const float*)m->ao; P.records = (uint32_t*)scratch; P.width = m->width;
    P.x0 = m->x0; P.y0 = m->y0; P.x1 = m->x1; P.y1 = m->y1;
    P.tx0 = m->x0 / CRTI_TILE_W; P.ty0 = m->y0 / CRTI_TILE_H;
    P.tilesX = (m->x1 - 1) / CRTI_TILE_W - P.tx0 + 1;
    P.tiles = P.tilesX * ((m->y1 - 1) / CRTI_TILE_H - P.ty0 + 1);          // (at most 512 x 2048)
    P.aoStrength = m->aoStrength;
    if (m->flags & CRTX_HEAL) crtx_launch_histogram<true>(P, crtx_bins_leader(), groups, s);
    else crtx_launch_histogram<false>(P, crtx_bins_leader(), groups, s);
    rc = crtx_launched();
    if (rc != CRTX_OK) return rc;
    CrtxResolveLaunch R;
    R.records = (const uint32_t*)scratch; R.groups = groups; R.prev = (m->flags & CRTX_ADAPT) ? (const CrtxResult*)m->prev : NULL;
    R.result = (CrtxResult*)result; R.outHist = (uint32_t*)outHist;
    R.key = m->key; R.lowFraction = m->lowFraction; R.highFraction = m->highFraction; R.minExposure = m->minExposure; R.maxExposure = m->maxExposure;
    R.rateUp = m->rateUp; R.rateDown = m->rateDown;
    crtx_resolve_kernel<<<dim3(1), CRTI_BLOCK, 0, s>>>(R);
    return crtx_launched();
}

int crtx_expose(const CrtxExpose* e, void* out, void* stream)
{
    const int rc = crtx_check_expose(e, out);
    if (rc != CRTX_OK) return rc;
    CrtxExposeLaunch P;
    P.color = (const float4*)e->color; P.ao = (const float*)e->ao; P.exposure = (const float*)e->exposure; P.out = (float4*)out;
    P.width = e->width; P.height = e->height; P.aoStrength = e->aoStrength;
    const dim3 grid = crti_grid(e->width, e->height);
    if (e->flags & CRTX_HEAL) crtx_expose_kernel<true><<<grid, CRTI_BLOCK, 0, (hipStream_t)stream>>>(P);
    else crtx_expose_kernel<false><<<grid, CRTI_BLOCK, 0, (hipStream_t)stream>>>(P);
    return crtx_launched();
}

float crtx_rate(double dt, double tau)
{
    if (!(tau > 0.0)) return 1.0f;
    return (float)(1.0 - exp(-dt / tau));
}

const char* crtx_error_string(int rc) { return CRTI_ERROR_STRING("crtx", rc); }

}
