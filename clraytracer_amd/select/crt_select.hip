// crt_select.hip -- libcrt_select.so: compact, gather and scatter of include/crt_select.h (definition there), their kernels and the C ABI over
// them. The only translation unit of the library, written over the shared steps of the image libraries (../image/crt_image_device.h and
// crt_image_host.h: vector loads, the two guide layouts, the hit predicate, dot3, the rules of the argument check, the error strings). It shares
// no state and has no environment switch. No kernel here uses an atomic or reads what another workgroup of its own launch writes: the order of
// the list comes from three launches on one stream (count, scan, write), each a plain function of what the one before it stored.
// Build: the Makefile's $(SELECT_SO) rule, with the flags of libcrt_hip.so (-ffp-contract=off is part of the definition).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include "../../include/crt_select.h"
#include "../image/crt_image_host.h"

#define CRTS_WAVES (CRTI_BLOCK / 64)                // the waves of a workgroup
#define CRTS_ROUNDS (CRTS_CHUNK / CRTI_BLOCK)       // a lane's items of a chunk: item r * CRTI_BLOCK + lane, so that a round is one coalesced row
// the ABI of crt_select.h (clraytracer_amd/_lib.py mirrors it)
static_assert(sizeof(CrtsCompact) == 24 && offsetof(CrtsCompact, wordBytes) == 8 && offsetof(CrtsCompact, values) == 12 && offsetof(CrtsCompact, n) == 16
              && offsetof(CrtsCompact, capacity) == 20, "CrtsCompact");
static_assert(sizeof(CrtsFrame) == 112 && offsetof(CrtsFrame, height) == 4 && offsetof(CrtsFrame, guides) == 8 && offsetof(CrtsFrame, geometry) == 16
              && offsetof(CrtsFrame, camera) == 24 && sizeof(CrttCamera) == 84, "CrtsFrame");
static_assert(sizeof(CrtsItems) == 24 && offsetof(CrtsItems, count) == 8 && offsetof(CrtsItems, factor) == 12 && offsetof(CrtsItems, offsetX) == 16
              && offsetof(CrtsItems, offsetY) == 20, "CrtsItems");
static_assert(sizeof(CrtsScatter) == 48 && offsetof(CrtsScatter, values) == 8 && offsetof(CrtsScatter, out) == 16 && offsetof(CrtsScatter, outState) == 24
              && offsetof(CrtsScatter, count) == 32 && offsetof(CrtsScatter, channels) == 36 && offsetof(CrtsScatter, n) == 40
              && offsetof(CrtsScatter, stateWord) == 44 && sizeof(float4) == 16, "CrtsScatter");
static_assert(CRTS_OK == CRTI_OK && CRTS_E_BAD_ARGUMENT == CRTI_E_BAD_ARGUMENT && CRTS_E_OUT_OF_RANGE == CRTI_E_OUT_OF_RANGE && CRTS_GUIDES_PLANES == CRTI_GUIDES_PLANES
              && CRTS_GUIDES_SURFACE == CRTI_GUIDES_SURFACE, "the codes and layouts of crt_image_host.h");
static_assert(CRTI_BLOCK == 256 && CRTS_CHUNK % CRTI_BLOCK == 0 && CRTS_SCAN == CRTI_BLOCK && CRTS_ROUNDS * CRTS_WAVES <= 64,
              "a scan round is one sum per lane, and a chunk's wave sums fit one wave");
static_assert(CRTS_MAX_ITEMS == CRTI_MAX_DIM * CRTI_MAX_DIM && (uint64_t)CRTS_MAX_ITEMS + CRTS_CHUNK < 0x80000000ull, "item indices fit 31 bits with a chunk to spare");

// ---- crts_compact ------------------------------------------------------------------------------------------------------------------------------
struct CrtsCompactLaunch {
    const char* words;
    uint32_t* list;
    uint32_t* counts;
    uint32_t* sums;                 // scratch: chunk sums, then exclusive offsets; the total behind them at sums[chunks]
    uint32_t values, n, capacity, chunks;
};

// is item k selected? An item behind the last is not (and is not loaded)
template <int WORD> __device__ __forceinline__ bool crts_selected(const CrtsCompactLaunch& P, uint32_t k)
{
    if (k >= P.n) return false;
    const uint32_t w = WORD == 4 ? *(const uint32_t*)(P.words + (size_t)k * 4) : (uint32_t)*(const uint8_t*)(P.words + k);
    return w < 32u && ((P.values >> (w & 31u)) & 1u) != 0u;
}
__device__ __forceinline__ uint32_t crts_lane() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint32_t crts_wave() { return threadIdx.x >> 6; }
// the number of lanes below this one whose bit is set
__device__ __forceinline__ uint32_t crts_rank(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
// the inclusive prefix sum of v over the wave's lanes
__device__ __forceinline__ uint32_t crts_wave_scan(uint32_t v)
{
    const uint32_t lane = crts_lane();
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off, 64);
        v = lane >= off ? v + o : v;
    }
    return v;
}

// launch 1: sums[chunk] = the chunk's number of selected items. A wave's count is the popcount of its ballots, the same in every lane
template <int WORD>
__global__ __launch_bounds__(CRTI_BLOCK) void crts_count_kernel(CrtsCompactLaunch P)
{
    __shared__ uint32_t s_wave[CRTS_WAVES];
    const uint32_t base = blockIdx.x * CRTS_CHUNK + threadIdx.x;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < CRTS_ROUNDS; ++r) c += (uint32_t)__popcll(__ballot(crts_selected<WORD>(P, base + r * CRTI_BLOCK)));
    if (crts_lane() == 0) s_wave[crts_wave()] = c;
    __syncthreads();
    if (threadIdx.x == 0) P.sums[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// launch 2, ONE workgroup: sums becomes its exclusive prefix sum, CRTS_SCAN entries per round, what the rounds before held carried in a register
// every lane keeps; sums[chunks] and counts receive the total. It waits for nobody: the launch before it has ended.
__global__ __launch_bounds__(CRTI_BLOCK) void crts_scan_kernel(CrtsCompactLaunch P)
{
    __shared__ uint32_t s_wave[CRTS_WAVES];
    const uint32_t lane = crts_lane(), wave = crts_wave();
    uint32_t carry = 0;
    for (uint32_t first = 0; first < P.chunks; first += CRTS_SCAN) {
        const uint32_t i = first + threadIdx.x;
        const uint32_t v = i < P.chunks ? P.sums[i] : 0u;
        const uint32_t inc = crts_wave_scan(v);
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        const uint32_t w0 = s_wave[0], w1 = s_wave[1], w2 = s_wave[2], w3 = s_wave[3];
        const uint32_t before = wave == 0 ? 0u : wave == 1 ? w0 : wave == 2 ? w0 + w1 : (w0 + w1) + w2;
        if (i < P.chunks) P.sums[i] = carry + before + (inc - v);
        carry += (w0 + w1) + (w2 + w3);
        __syncthreads();            // s_wave is written again in the next round
    }
    if (threadIdx.x == 0) {
        P.sums[P.chunks] = carry;
        P.counts[0] = carry; P.counts[1] = min(carry, P.capacity);
    }
}

// launch 3: workgroup c pads the entries c * CRTS_CHUNK .. + CRTS_CHUNK - 1 of the list that lie behind the total, and, where it has a chunk with
// selected items that still fit, writes them: entry = the chunk's offset + the sums of the (round, wave) pairs before the lane's + the lane's
// rank in its wave's ballot. The 32 pair sums go through LDS once; every wave scans them for itself and reads its eight by lane index.
template <int WORD>
__global__ __launch_bounds__(CRTI_BLOCK) void crts_write_kernel(CrtsCompactLaunch P)
{
    __shared__ uint32_t s_pair[CRTS_ROUNDS * CRTS_WAVES];
    const uint32_t chunk = blockIdx.x, base = chunk * CRTS_CHUNK + threadIdx.x;
    const uint32_t total = P.sums[P.chunks];
#pragma unroll
    for (int r = 0; r < CRTS_ROUNDS; ++r) {
        const uint32_t j = base + r * CRTI_BLOCK;
        if (j >= total && j < P.capacity) P.list[j] = CRTS_NONE;
    }
    if (chunk >= P.chunks) return;                      // a workgroup that only pads (capacity > n)
    const uint32_t offset = P.sums[chunk];
    if (P.sums[chunk + 1] == offset || offset >= P.capacity) return;     // nothing selected here, or nothing of it fits: uniform
    const uint32_t lane = crts_lane(), wave = crts_wave();
    uint32_t rank[CRTS_ROUNDS], mine = 0;
#pragma unroll
    for (int r = 0; r < CRTS_ROUNDS; ++r) {
        const bool s = crts_selected<WORD>(P, base + r * CRTI_BLOCK);
        const unsigned long long m = __ballot(s);
        rank[r] = crts_rank(m);
        mine |= (s ? 1u : 0u) << r;
        if (lane == 0) s_pair[r * CRTS_WAVES + wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    const uint32_t v = lane < CRTS_ROUNDS * CRTS_WAVES ? s_pair[lane] : 0u;
    const uint32_t before = crts_wave_scan(v) - v;      // lane i: the sum of the pairs before pair i
#pragma unroll
    for (int r = 0; r < CRTS_ROUNDS; ++r) {
        const uint32_t dst = offset + __shfl(before, r * CRTS_WAVES + (int)wave, 64) + rank[r];
        if (((mine >> r) & 1u) && dst < P.capacity) P.list[dst] = base + r * CRTI_BLOCK;
    }
}

// ---- crts_points -------------------------------------------------------------------------------------------------------------------------------
struct CrtsPointsLaunch {
    const uint32_t* list;           // NULL in the grid form
    const char* geometry;           // {n.x, n.y, n.z, t} at geometry + k * stride
    float4* positions;
    float4* normals;
    float4* dirs;                   // may be NULL
    uint32_t count, width, pixels, lowWidth, factor, offsetX, offsetY;
    float pos[3], toRay[9];
};

// One lane per item. GRID: the item's pixel follows from its number and lies in the frame (crts_check_grid). Else it is read from the list, and
// an entry that names no pixel loads pixel 0 in its place and stores zeros.
template <bool SURFACE, bool GRID>
__global__ __launch_bounds__(CRTI_BLOCK) void crts_points_kernel(CrtsPointsLaunch P)
{
    const uint32_t j = blockIdx.x * CRTI_BLOCK + threadIdx.x;
    if (j >= P.count) return;
    uint32_t x, y;
    bool valid = true;
    if (GRID) {
        const uint32_t Y = j / P.lowWidth, X = j - Y * P.lowWidth;
        x = X * P.factor + P.offsetX; y = Y * P.factor + P.offsetY;
    } else {
        const uint32_t k = P.list[j];
        valid = k < P.pixels;
        const uint32_t kc = valid ? k : 0u;
        y = kc / P.width; x = kc - y * P.width;
    }
    const float4 g = crti_geometry<SURFACE>(P, (size_t)(y * P.width + x));
    const float fx = (float)x, fy = (float)y;
    float dx = crti_dot3(P.toRay[0], P.toRay[1], P.toRay[2], fx, fy, 1.0f);
    float dy = crti_dot3(P.toRay[3], P.toRay[4], P.toRay[5], fx, fy, 1.0f);
    float dz = crti_dot3(P.toRay[6], P.toRay[7], P.toRay[8], fx, fy, 1.0f);
    const float dl = sqrtf(crti_dot3(dx, dy, dz, dx, dy, dz));
    dx = dx / dl; dy = dy / dl; dz = dz / dl;
    const bool hit = crti_hit(g.w);
    const bool away = crti_dot3(g.x, g.y, g.z, dx, dy, dz) > 0.0f;     // the stored normal looks away from the viewer
    float4 p = make_float4(0.0f, 0.0f, 0.0f, g.w), n = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d = make_float4(dx, dy, dz, 0.0f);
    if (hit) {
        p.x = P.pos[0] + dx * g.w; p.y = P.pos[1] + dy * g.w; p.z = P.pos[2] + dz * g.w;
        n.x = away ? -g.x : g.x; n.y = away ? -g.y : g.y; n.z = away ? -g.z : g.z;
    }
    if (!valid) { p = make_float4(0.0f, 0.0f, 0.0f, 0.0f); n = p; d = p; }
    crti_store4(P.positions + j, p);
    crti_store4(P.normals + j, n);
    if (P.dirs) crti_store4(P.dirs + j, d);
}

// ---- crts_scatter ------------------------------------------------------------------------------------------------------------------------------
struct CrtsScatterLaunch {
    const uint32_t* list;
    const char* values;             // float (channels 1) or float4 (channels 4) at values + j * 4 * channels
    char* out;                      // likewise, at out + k * 4 * channels
    uint32_t* state;                // may be NULL
    uint32_t count, n, stateWord;
};

// One lane per entry; an entry that names no item of out stores nothing
template <int CHANNELS>
__global__ __launch_bounds__(CRTI_BLOCK) void crts_scatter_kernel(CrtsScatterLaunch P)
{
    const uint32_t j = blockIdx.x * CRTI_BLOCK + threadIdx.x;
    if (j >= P.count) return;
    const uint32_t k = P.list[j];
    if (k >= P.n) return;
    if (CHANNELS == 4) *(crti_f4*)(P.out + (size_t)k * 16) = *(const crti_f4*)(P.values + (size_t)j * 16);
    else *(float*)(P.out + (size_t)k * 4) = *(const float*)(P.values + (size_t)j * 4);
    if (P.state) P.state[k] = P.stateWord;
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------------------
static inline uint32_t crts_chunks(uint32_t n) { return (n + (CRTS_CHUNK - 1)) / CRTS_CHUNK; }
static inline unsigned crts_blocks(uint32_t items) { return (unsigned)((items + (CRTI_BLOCK - 1)) / CRTI_BLOCK); }

// what every call refuses of a number of items
static int crts_check_items(int32_t a, int32_t b)
{
    if (a < 1 || b < 1) return CRTS_E_BAD_ARGUMENT;
    if (a > CRTS_MAX_ITEMS || b > CRTS_MAX_ITEMS) return CRTS_E_OUT_OF_RANGE;
    return CRTS_OK;
}

static int crts_check_compact(const CrtsCompact* c, const void* list, const void* counts, const void* scratch)
{
    if (!c || !c->words || !list || !counts || !scratch) return CRTS_E_BAD_ARGUMENT;
    if (c->wordBytes != 1 && c->wordBytes != 4) return CRTS_E_BAD_ARGUMENT;
    const void* const ins[1] = {c->words};
    const void* const outs[3] = {list, counts, scratch};
    if (crti_aliased(ins, outs)) return CRTS_E_BAD_ARGUMENT;
    return crts_check_items(c->n, c->capacity);
}

// the grid form of crts_points: the low image's place in the frame, as crtu_low_size has it, and factor 1 besides; *lowWidth is LW
static int crts_check_grid(const CrtsFrame* f, const CrtsItems* it, int32_t* lowWidth)
{
    const int32_t F = it->factor;
    if (F != 1 && F != 2 && F != 4) return CRTS_E_BAD_ARGUMENT;
    if (it->offsetX < 0 || it->offsetX >= F || it->offsetY < 0 || it->offsetY >= F) return CRTS_E_BAD_ARGUMENT;
    if (it->offsetX >= f->width || it->offsetY >= f->height) return CRTS_E_BAD_ARGUMENT;      // no sample would lie in the frame
    const int32_t lw = (f->width - it->offsetX + F - 1) / F, lh = (f->height - it->offsetY + F - 1) / F;
    if (it->count != lw * lh) return CRTS_E_BAD_ARGUMENT;
    *lowWidth = lw;
    return CRTS_OK;
}

static int crts_check_points(const CrtsFrame* f, const CrtsItems* it, const void* positions, const void* normals, const void* dirs, int32_t* lowWidth)
{
    if (!f || !it || !f->geometry || !positions || !normals) return CRTS_E_BAD_ARGUMENT;
    if (f->guides != CRTS_GUIDES_PLANES && f->guides != CRTS_GUIDES_SURFACE) return CRTS_E_BAD_ARGUMENT;
    const void* const ins[2] = {it->list, f->geometry};
    const void* const outs[3] = {positions, normals, dirs};
    if (crti_aliased(ins, outs)) return CRTS_E_BAD_ARGUMENT;
    if (f->width < 1 || f->height < 1 || it->count < 1) return CRTS_E_BAD_ARGUMENT;
    if (f->width > CRTI_MAX_DIM || f->height > CRTI_MAX_DIM || it->count > CRTS_MAX_ITEMS) return CRTS_E_OUT_OF_RANGE;
    *lowWidth = 1;
    return it->list ? CRTS_OK : crts_check_grid(f, it, lowWidth);
}

static int crts_check_scatter(const CrtsScatter* s)
{
    if (!s || !s->list || !s->values || !s->out) return CRTS_E_BAD_ARGUMENT;
    if (s->channels != 1 && s->channels != 4) return CRTS_E_BAD_ARGUMENT;
    const void* const ins[2] = {s->list, s->values};
    const void* const outs[2] = {s->out, s->outState};
    if (crti_aliased(ins, outs)) return CRTS_E_BAD_ARGUMENT;
    return crts_check_items(s->count, s->n);
}

static inline int crts_launched()
{
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : CRTS_OK;
}

extern "C" {

size_t crts_scratch_bytes(int32_t n)
{
    if (n < 1 || n > CRTS_MAX_ITEMS) return 0;
    return ((size_t)crts_chunks((uint32_t)n) + 1) * sizeof(uint32_t);      // the chunk sums and the total behind them
}

int crts_compact(const CrtsCompact* c, void* list, void* counts, void* scratch, void* stream)
{
    const int rc = crts_check_compact(c, list, counts, scratch);
    if (rc != CRTS_OK) return rc;
    CrtsCompactLaunch P;
    P.words = (const char*)c->words; P.list = (uint32_t*)list; P.counts = (uint32_t*)counts; P.sums = (uint32_t*)scratch;
    P.values = c->values; P.n = (uint32_t)c->n; P.capacity = (uint32_t)c->capacity; P.chunks = crts_chunks(P.n);
    const unsigned writers = P.chunks > crts_chunks(P.capacity) ? P.chunks : crts_chunks(P.capacity);
    const hipStream_t s = (hipStream_t)stream;
    if (c->wordBytes == 4) crts_count_kernel<4><<<P.chunks, CRTI_BLOCK, 0, s>>>(P);
    else crts_count_kernel<1><<<P.chunks, CRTI_BLOCK, 0, s>>>(P);
    crts_scan_kernel<<<1, CRTI_BLOCK, 0, s>>>(P);
    if (c->wordBytes == 4) crts_write_kernel<4><<<writers, CRTI_BLOCK, 0, s>>>(P);
    else crts_write_kernel<1><<<writers, CRTI_BLOCK, 0, s>>>(P);
    return crts_launched();
}

int crts_points(const CrtsFrame* f, const CrtsItems* items, void* positions, void* normals, void* dirs, void* stream)
{
    int32_t lowWidth = 1;
    const int rc = crts_check_points(f, items, positions, normals, dirs, &lowWidth);
    if (rc != CRTS_OK) return rc;
    const bool surface = f->guides == CRTS_GUIDES_SURFACE, grid = items->list == nullptr;
    CrtsPointsLaunch P;
    P.list = (const uint32_t*)items->list; P.geometry = (const char*)f->geometry;
    P.positions = (float4*)positions; P.normals = (float4*)normals; P.dirs = (float4*)dirs;
    P.count = (uint32_t)items->count; P.width = (uint32_t)f->width; P.pixels = (uint32_t)f->width * (uint32_t)f->height;
    P.lowWidth = (uint32_t)lowWidth; P.factor = grid ? (uint32_t)items->factor : 1u;
    P.offsetX = grid ? (uint32_t)items->offsetX : 0u; P.offsetY = grid ? (uint32_t)items->offsetY : 0u;
    for (int i = 0; i < 3; ++i) P.pos[i] = f->camera.pos[i];
    for (int i = 0; i < 9; ++i) P.toRay[i] = f->camera.toRay[i];
    const unsigned blocks = crts_blocks(P.count);
    const hipStream_t s = (hipStream_t)stream;
    if (surface && grid) crts_points_kernel<true, true><<<blocks, CRTI_BLOCK, 0, s>>>(P);
    else if (surface) crts_points_kernel<true, false><<<blocks, CRTI_BLOCK, 0, s>>>(P);
    else if (grid) crts_points_kernel<false, true><<<blocks, CRTI_BLOCK, 0, s>>>(P);
    else crts_points_kernel<false, false><<<blocks, CRTI_BLOCK, 0, s>>>(P);
    return crts_launched();
}

int crts_scatter(const CrtsScatter* sc, void* stream)
{
    const int rc = crts_check_scatter(sc);
    if (rc != CRTS_OK) return rc;
    CrtsScatterLaunch P;
    P.list = (const uint32_t*)sc->list; P.values = (const char*)sc->values; P.out = (char*)sc->out; P.state = (uint32_t*)sc->outState;
    P.count = (uint32_t)sc->count; P.n = (uint32_t)sc->n; P.stateWord = sc->stateWord;
    const unsigned blocks = crts_blocks(P.count);
    if (sc->channels == 4) crts_scatter_kernel<4><<<blocks, CRTI_BLOCK, 0, (hipStream_t)stream>>>(P);
    else crts_scatter_kernel<1><<<blocks, CRTI_BLOCK, 0, (hipStream_t)stream>>>(P);
    return crts_launched();
}

const char* crts_error_string(int rc)
{
    return crti_error_string(rc, "crts: bad argument", "crts: out of range (a frame wider or taller than 16384, or more than 2^28 items)", "crts: unknown error");
}

}
