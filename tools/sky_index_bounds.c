/* The exhaustive maxima behind the guarded float skybox index (clraytracer_amd/csrc/crt_device.h: sky_index_float, derivation above it),
 * and the decided totals that the sweeps of tools/ubench/sky_index must reproduce on the device (tests/test_gpu_sky_index.py).
 *
 *   cc -O2 -ffp-contract=off -pthread -o /tmp/sky_index_bounds tools/sky_index_bounds.c -lm
 *   /tmp/sky_index_bounds [clraytracer_amd/csrc/crt_device.h] > profiles/sky_index_bounds.txt       (a minute or two on 8 cores)
 *
 * The float sequence is restated here in plain C, one IEEE single-precision operation per statement, with the constants READ FROM THE
 * HEADER (#define CRT_SKY_*); the references are glibc's double atan and acos. A tool, not a test. */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static float A[9], C[8], KA, KC, MINC, MAXC, MAXS;
static const double PI = 3.14159265358979323846;

static float macro(const char* text, const char* name)
{
    char key[64];
    snprintf(key, sizeof key, "#define %s ", name);
    const char* p = strstr(text, key);
    if (!p) { fprintf(stderr, "%s is not in the header\n", name); exit(1); }
    return strtof(p + strlen(key), NULL);
}

static float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static float poly_atan(float q)          /* p ~ atan(q) / pi, q in [0, 1] */
{
    const float u = q * q;
    float p = A[8];
    for (int k = 7; k >= 0; --k) { p = p * u; p = p + A[k]; }
    p = p * q;
    return p;
}

static float fast_acos(float y)          /* ac~ ~ acos(y) / pi */
{
    const float ay = fabsf(y);
    const float r = sqrtf(1.0f - ay);
    float c = C[7];
    for (int k = 6; k >= 0; --k) { c = c * ay; c = c + C[k]; }
    c = c * r;
    return y < 0.0f ? 1.0f - c : c;
}

static float fast_atan2(float x, float z, float* mnOut, float* mxOut)
{
    const float ax = fabsf(x), az = fabsf(z);
    const int steep = ax > az;
    const float mn = steep ? az : ax, mx = steep ? ax : az;
    const float q = mn / mx;
    const float p = poly_atan(q);
    float a = steep ? 0.5f - p : p;
    a = z > 0.0f ? 1.0f - a : a;
    a = x < 0.0f ? -a : a;
    *mnOut = mn; *mxOut = mx;
    return a;
}

/* sky_index_float: 1 = decided, theta and phi then are the definition's */
static int sky_float(float x, float y, float z, int texW, int texH, int* theta, int* phi)
{
    const float fW = (float)texW, fH = (float)texH, ay = fabsf(y);
    float mn, mx;
    const float a = fast_atan2(x, z, &mn, &mx), c = fast_acos(y);
    float s = a * 0.5f; s = s * fW;
    const float sv = c * fH;
    const float es = fabsf(s - rintf(s)), ev = fabsf(sv - rintf(sv));
    const float mW = KA * fabsf(0.5f * fW), mH = KC * fabsf(fH);
    const int ok = es > mW && ev > mH && fabsf(s) < MAXS && sv < MAXS && mn >= MINC && mx <= MAXC && ay >= MINC && ay < 1.0f;
    if (ok) { *theta = (int)s; *phi = (int)sv; }
    return ok;
}

static int f2i(float x) { if (!(x == x)) return 0; if (x >= 2147483648.0f) return 2147483647; if (x <= -2147483648.0f) return -2147483647 - 1; return (int)x; }
static void sky_double(float x, float y, float z, int texW, int texH, int* theta, int* phi)
{
    const float at = (float)(atan2((double)x, (double)(-z)) / PI), ac = (float)(acos((double)y) / PI);
    *theta = f2i((at * 0.5f) * (float)texW);
    *phi = f2i(ac * (float)texH);
}

static const int SIZES[3][2] = { { 64, 32 }, { 90, 37 }, { 2048, 1024 } };
static const float SWEEP_X = 0.3f, SWEEP_Z = -0.9f, SWEEP_Y = 0.3f;     /* the fixed components of the sweeps */

#define CHUNK (1ull << 20)      /* a thread takes every `stride`-th chunk of patterns: the slow and the quick ranges are shared out evenly */
typedef struct {
    uint64_t first, count, stride; int pass;
    double maxErr; uint32_t argmax; uint64_t admitted;
    uint64_t decided[3], mismatch[3], decidedY0[3];
} Job;

static void* run(void* arg)
{
    Job* j = (Job*)arg;
    for (uint64_t base = j->first * CHUNK; base < j->count; base += j->stride * CHUNK)
    for (uint64_t i = base; i < base + CHUNK && i < j->count; ++i) {
        const uint32_t bits = (uint32_t)i;
        const float v = u2f(bits);
        if (j->pass == 0) {                 /* every float q in [0, 1]: E_p, and the q sweeps (q, SWEEP_Y | 0, -1) */
            const double want = atan((double)v) / PI;
            const double e = fabs((double)poly_atan(v) - want);
            if (e > j->maxErr) { j->maxErr = e; j->argmax = bits; }
            j->admitted++;
            for (int k = 0; k < 3; ++k) {
                int t, p, td, pd;
                if (sky_float(v, SWEEP_Y, -1.0f, SIZES[k][0], SIZES[k][1], &t, &p)) {
                    j->decided[k]++;
                    sky_double(v, SWEEP_Y, -1.0f, SIZES[k][0], SIZES[k][1], &td, &pd);
                    if (t != td || p != pd) j->mismatch[k]++;
                }
                if (sky_float(v, 0.0f, -1.0f, SIZES[k][0], SIZES[k][1], &t, &p)) j->decidedY0[k]++;
            }
        } else {                            /* all 2^32 patterns of d.y: E_c over the admitted ones, and the y sweeps (SWEEP_X, y, SWEEP_Z) */
            const float ay = fabsf(v);
            double want = 0.0;
            const int admitted = ay >= MINC && ay < 1.0f;
            if (admitted) {
                want = acos((double)v) / PI;
                const double e = fabs((double)fast_acos(v) - want);
                if (e > j->maxErr) { j->maxErr = e; j->argmax = bits; }
                j->admitted++;
            }
            for (int k = 0; k < 3; ++k) {
                int t, p, td;
                if (sky_float(SWEEP_X, v, SWEEP_Z, SIZES[k][0], SIZES[k][1], &t, &p)) {
                    j->decided[k]++;
                    const float ac = (float)want;
                    const float at = (float)(atan2((double)SWEEP_X, (double)(-SWEEP_Z)) / PI);
                    td = f2i((at * 0.5f) * (float)SIZES[k][0]);
                    if (!admitted || t != td || p != f2i(ac * (float)SIZES[k][1])) j->mismatch[k]++;
                }
            }
        }
    }
    return NULL;
}

static void pass(int which, uint64_t total, int threads, Job* sum)
{
    pthread_t* th = calloc(threads, sizeof *th);
    Job* jobs = calloc(threads, sizeof *jobs);
    for (int t = 0; t < threads; ++t) {
        jobs[t].first = (uint64_t)t; jobs[t].count = total; jobs[t].stride = (uint64_t)threads; jobs[t].pass = which;
        pthread_create(&th[t], NULL, run, &jobs[t]);
    }
    memset(sum, 0, sizeof *sum);
    for (int t = 0; t < threads; ++t) {
        pthread_join(th[t], NULL);
        if (jobs[t].maxErr > sum->maxErr) { sum->maxErr = jobs[t].maxErr; sum->argmax = jobs[t].argmax; }
        sum->admitted += jobs[t].admitted;
        for (int k = 0; k < 3; ++k) { sum->decided[k] += jobs[t].decided[k]; sum->mismatch[k] += jobs[t].mismatch[k]; sum->decidedY0[k] += jobs[t].decidedY0[k]; }
    }
    free(th); free(jobs);
}

static double round_up_3(double v) { const double m = pow(10.0, floor(log10(v)) - 2.0); return ceil(v / m) * m; }

int main(int argc, char** argv)
{
    const char* path = argc > 1 ? argv[1] : "clraytracer_amd/csrc/crt_device.h";
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return 1; }
    static char text[1 << 20];
    text[fread(text, 1, sizeof text - 1, f)] = 0;
    fclose(f);
    char name[32];
    for (int k = 0; k < 9; ++k) { snprintf(name, sizeof name, "CRT_SKY_A%d", k); A[k] = macro(text, name); }
    for (int k = 0; k < 8; ++k) { snprintf(name, sizeof name, "CRT_SKY_C%d", k); C[k] = macro(text, name); }
    KA = macro(text, "CRT_SKY_KA"); KC = macro(text, "CRT_SKY_KC");
    MINC = macro(text, "CRT_SKY_MIN_COMPONENT"); MAXC = macro(text, "CRT_SKY_MAX_COMPONENT"); MAXS = macro(text, "CRT_SKY_MAX_SCALED");
    int threads = (int)sysconf(_SC_NPROCESSORS_ONLN);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;

    Job q, y;
    pass(0, 0x3F800000ull + 1ull, threads, &q);
    pass(1, 1ull << 32, threads, &y);

    const double Ep = q.maxErr, Ec = y.maxErr;
    const double Ea = Ep + ldexp(1.0, -24) / PI + 2.0 * ldexp(1.0, -25);
    const double rounding = ldexp(1.0, -25) + ldexp(1.0, -23) + 1e-15;
    const double Ka = Ea + rounding, Kc = Ec + rounding;
    const double SAFETY = 1.25;
    printf("guarded float skybox index: exhaustive maxima (tools/sky_index_bounds.c, constants read from crt_device.h, glibc double references)\n\n");
    printf("E_p  max |p(q) - atan(q)/pi| over every float q in [0, 1] (%llu values)          %.6e   at q bits 0x%08X\n", (unsigned long long)q.admitted, Ep, q.argmax);
    printf("E_c  max |ac~(y) - acos(y)/pi| over every float y, %.8e <= |y| < 1 (%llu of 2^32)  %.6e   at y bits 0x%08X\n", (double)MINC, (unsigned long long)y.admitted, Ec, y.argmax);
    printf("E_a  = E_p + 2^-24/pi + 2 * 2^-25                                                 %.6e\n", Ea);
    printf("rounding terms 2^-25 + 2^-23 + 1e-15                                              %.6e\n", rounding);
    printf("K_a  = E_a + rounding terms                                                       %.6e\n", Ka);
    printf("K_c  = E_c + rounding terms                                                       %.6e\n", Kc);
    printf("safety factor                                                                     %.2f\n", SAFETY);
    printf("derived CRT_SKY_KA = K_a * safety, rounded up to three digits                     %.2e\n", round_up_3(Ka * SAFETY));
    printf("derived CRT_SKY_KC = K_c * safety, rounded up to three digits                     %.2e\n", round_up_3(Kc * SAFETY));
    printf("header  CRT_SKY_KA %.2e  CRT_SKY_KC %.2e   -> %s\n\n", (double)KA, (double)KC,
           ((double)KA >= Ka * SAFETY && (double)KC >= Kc * SAFETY && (double)KA <= 2.0 * Ka && (double)KC <= 2.0 * Kc) ? "hold (>= derived, <= 2 K)" : "DO NOT HOLD");
    printf("recorded E_p %.6e\nrecorded E_c %.6e\nrecorded K_a %.6e\nrecorded K_c %.6e\n\n", Ep, Ec, Ka, Kc);
    printf("sweeps with the header's constants (decided lanes; lanes whose float index differs from the double definition's must be 0)\n");
    for (int k = 0; k < 3; ++k)
        printf("sweep y  all 2^32 patterns of d.y, (d.x, d.z) = (%.9g, %.9g), sky %dx%d: decided %llu differing %llu\n", (double)SWEEP_X, (double)SWEEP_Z,
               SIZES[k][0], SIZES[k][1], (unsigned long long)y.decided[k], (unsigned long long)y.mismatch[k]);
    for (int k = 0; k < 3; ++k)
        printf("sweep q  every float q in [0, 1], d = (q, %.9g, -1), sky %dx%d: decided %llu differing %llu\n", (double)SWEEP_Y,
               SIZES[k][0], SIZES[k][1], (unsigned long long)q.decided[k], (unsigned long long)q.mismatch[k]);
    for (int k = 0; k < 3; ++k)
        printf("sweep q0 every float q in [0, 1], d = (q, 0, -1), sky %dx%d: decided %llu (d.y = 0 is never decided)\n",
               SIZES[k][0], SIZES[k][1], (unsigned long long)q.decidedY0[k]);
    return 0;
}
