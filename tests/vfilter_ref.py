"""A numpy float32 restatement of the definition in include/crt_vfilter.h: vectorised over the pixels, the 49, 9 and 25 taps in the definition's
order, every operation a float32 operation of its own (numpy contracts nothing; no float64 intermediate). What crtv_filter must give, bit for bit.
The hand-made inputs are those of tests/denoise_ref.py (guides(), noisy_color(), surface_records()) and moments_content() here."""
import numpy as np

from denoise_ref import den_of, guides, luma, noisy_color, shifted, surface_records  # noqa: F401 (the inputs are re-exported)

DEMODULATE, MATCH_INSTANCE = 1, 2
K = (np.float32(0.375), np.float32(0.25), np.float32(0.0625))
G = (np.float32(0.25), np.float32(0.125), np.float32(0.0625))
F = np.float32
DEFAULTS = dict(depth_tol=0.05, normal_cos=0.9, luma_sigma=4.0, luma_floor=1e-4, min_history=4.0)


class Stops:
    """the geometry stops of a centre against the pixel (dx, dy) away, at step s: hit, distance, normal and (by flag) instance"""

    def __init__(self, geometry, instance, flags, depth_tol, normal_cos):
        self.n, self.t = geometry[..., :3], geometry[..., 3]
        self.hit = self.t <= F(99998.0)
        self.instance = instance if flags & MATCH_INSTANCE else None
        self.depth_tol, self.normal_cos = F(depth_tol), F(normal_cos)

    def __call__(self, ox, oy, s):
        """(passes, inside): both (H, W) bool; a tap outside the frame passes nothing"""
        n, t = self.n, self.t
        tq, inside = shifted(t, ox, oy, 0)
        nq, _ = shifted(n, ox, oy, 0)
        hq, _ = shifted(self.hit, ox, oy, False)
        ok = inside & hq & (np.abs(tq - t) <= (self.depth_tol * t) * F(s))
        ok &= ((nq[..., 0] * n[..., 0] + nq[..., 1] * n[..., 1]) + nq[..., 2] * n[..., 2]) >= self.normal_cos
        if self.instance is not None:
            iq, _ = shifted(self.instance, ox, oy, 0)
            ok &= iq == self.instance
        return ok, inside


def estimate(color, moments, stops, den, flags, min_history):
    """step 1 of the definition: the working image I0 (H, W, 4) = {rgb, var}"""
    one, zero = F(1.0), F(0.0)
    hit = stops.hit
    m1, m2, N, mv = (moments[..., k] for k in range(4))
    temporal = N >= F(min_history)
    var_t = np.where(mv >= zero, mv, zero)
    S1, S2, n = (np.zeros(hit.shape, np.float32) for _ in range(3))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            if dx == 0 and dy == 0:
                ok = np.ones(hit.shape, bool)
            else:
                ok, _ = stops(dx, dy, 1)
            a, _ = shifted(m1, dx, dy, 0)
            b, _ = shifted(m2, dx, dy, 0)
            if dx or dy:
                ok = ok & np.isfinite(a) & np.isfinite(b)
            S1 = np.where(ok, S1 + a, S1)
            S2 = np.where(ok, S2 + b, S2)
            n = np.where(ok, n + one, n)
    a = S1 / n
    v = S2 / n - a * a
    var_s = np.where(v > zero, v, zero)
    var_s = var_s * (F(4.0) / np.fmax(N, one))
    var = np.where(hit, np.where(temporal, var_t, var_s), zero).astype(np.float32)
    rgb = color[..., :3]
    if flags & DEMODULATE:
        ld = luma(den)
        rgb = np.where(hit[..., None], rgb / den, rgb)
        var = np.where(hit, var / (ld * ld), var)
    return np.concatenate([rgb, var[..., None]], axis=-1).astype(np.float32)


def one_pass(I, stops, s, luma_sigma, luma_floor):
    """one pass of step 2 at step s: (H, W, 4) = {rgb, var} from the same"""
    one, zero = F(1.0), F(0.0)
    hit = stops.hit
    rgb, var = I[..., :3], I[..., 3]
    gsum, gw = np.zeros(hit.shape, np.float32), np.zeros(hit.shape, np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            vq, inside = shifted(var, dx, dy, 0)
            hq, _ = shifted(hit, dx, dy, False)
            ok = inside & hq & (vq >= zero)
            g = G[abs(dy)] * G[abs(dx)]
            gsum = np.where(ok, gsum + vq * g, gsum)
            gw = np.where(ok, gw + g, gw)
    gv = np.where(gw > zero, gsum / gw, zero).astype(np.float32)
    sd = F(luma_sigma) * np.sqrt(gv) + F(luma_floor)
    L = luma(rgb)
    total = np.zeros_like(rgb)
    vsum, wsum = np.zeros(hit.shape, np.float32), np.zeros(hit.shape, np.float32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            k = K[abs(dy)] * K[abs(dx)]
            Iq, _ = shifted(rgb, dx * s, dy * s, 0)
            vq, _ = shifted(var, dx * s, dy * s, 0)
            if dx == 0 and dy == 0:
                ok = np.ones(hit.shape, bool)
                w = np.full(hit.shape, k, np.float32)
            else:
                ok, _ = stops(dx * s, dy * s, s)
                Lq, _ = shifted(L, dx * s, dy * s, 0)
                xl = np.abs(Lq - L) / sd
                ok = ok & (vq >= zero) & (xl < one)
                w = k * ((one - xl) * (one - xl))
            total = np.where(ok[..., None], total + Iq * w[..., None], total)
            vsum = np.where(ok, vsum + vq * (w * w), vsum)
            wsum = np.where(ok, wsum + w, wsum)
    out = np.concatenate([total / wsum[..., None], (vsum / (wsum * wsum))[..., None]], axis=-1).astype(np.float32)
    return np.where(hit[..., None], out, I)


def filter(color, moments, geometry, instance=None, albedo=None, iterations=4, flags=DEMODULATE, depth_tol=0.05, normal_cos=0.9, luma_sigma=4.0,
           luma_floor=1e-4, min_history=4.0, working=False):
    """color, moments, geometry (H, W, 4) float32; instance (H, W) int32; albedo (H, W) uint32. Returns (out (H, W, 4), variance (H, W)), both
    float32; working=True: the list of working images I0, I1, ... instead (demodulated, before step 3)."""
    color = np.ascontiguousarray(color, np.float32)
    moments = np.ascontiguousarray(moments, np.float32)
    geometry = np.ascontiguousarray(geometry, np.float32)
    with np.errstate(all="ignore"):
        stops = Stops(geometry, instance, flags, depth_tol, normal_cos)
        hit = stops.hit
        den = den_of(albedo) if flags & DEMODULATE else np.ones(color.shape[:2] + (3,), np.float32)
        images = [estimate(color, moments, stops, den, flags, min_history)]
        for p in range(iterations):
            images.append(one_pass(images[-1], stops, 1 << p, luma_sigma, luma_floor))
        if working:
            return images
        I = images[-1]
        ld = luma(den)
        rgb = np.where(hit[..., None], I[..., :3] * den, color[..., :3])
        variance = np.where(hit, I[..., 3] * (ld * ld), F(0.0)).astype(np.float32)
    return np.concatenate([rgb.astype(np.float32), color[..., 3:]], axis=-1), variance


def moments_content(color, geometry, seed=0, history=None, edge_cases=True, infinite=False):
    """A moments plane {m1, m2, N, variance} for `color` over `geometry`, as crtt_accumulate would leave it after some frames: m1 near the
    luminance, m2 = m1^2 + a seeded variance, N among 0, 1, 2, 7.25 and 32 (`history`: that N everywhere), 0 on pixels that are no hit. With
    `edge_cases`: some NaN and +inf m1, NaN and -inf m2, NaN N, and NaN, negative and zero variances -- all of which the estimate heals. With
    `infinite`: one +inf variance and one +inf m2 as well; an infinite variance is a variance and spreads as far as the passes reach."""
    rng = np.random.RandomState(4000 + seed)
    H, W = color.shape[:2]
    m = np.zeros((H, W, 4), np.float32)
    with np.errstate(all="ignore"):
        L = luma(color[..., :3])
    m[..., 0] = np.where(np.isfinite(L), L, 0.5) + rng.normal(0, 0.05, (H, W))
    m[..., 3] = rng.uniform(0.0, 0.05, (H, W))
    m[..., 1] = m[..., 0] ** 2 + m[..., 3]
    m[..., 2] = rng.choice(np.array([0.0, 1.0, 1.0, 2.0, 7.25, 32.0, 32.0, 32.0], np.float32), (H, W)) if history is None else history
    m[..., 2][~(geometry[..., 3] <= 99998.0)] = 0.0
    if edge_cases and H * W > 8:
        k = max(1, H * W // 40)
        pick = lambda: (rng.randint(0, H, k), rng.randint(0, W, k))
        m[pick() + (0,)] = np.nan
        m[pick() + (0,)] = np.inf
        m[pick() + (1,)] = -np.inf
        m[pick() + (1,)] = np.nan
        m[pick() + (2,)] = np.nan
        m[pick() + (3,)] = np.nan
        m[pick() + (3,)] = -0.25
        m[pick() + (3,)] = 0.0
    if infinite:
        m[H // 3, W // 2, 3] = np.inf
        m[H // 3, W // 2, 2] = 32.0
        m[2 * H // 3, W // 4, 1] = np.inf
        m[2 * H // 3, W // 4, 2] = 1.0
    return m
