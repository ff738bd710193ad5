"""A numpy float32 restatement of the definition in include/crt_denoise.h: vectorised over the pixels, the 25 taps in the definition's order,
every operation a float32 operation of its own (numpy contracts nothing). What crtd_denoise must give, bit for bit."""
import numpy as np

DEMODULATE, MATCH_INSTANCE, LUMA_STOP = 1, 2, 4
K = (np.float32(0.375), np.float32(0.25), np.float32(0.0625))
F = np.float32


def den_of(albedo):
    """(H, W, 3) float32: per channel b == 0 ? 1.0f : (float)b / 255.0f of the albedo word's bytes r, g, b"""
    b = np.stack([(albedo >> np.uint32(sh)) & np.uint32(255) for sh in (0, 8, 16)], axis=-1).astype(np.float32)
    with np.errstate(all="ignore"):
        return np.where(b == 0, F(1.0), b / F(255.0)).astype(np.float32)


def luma(rgb):
    return (F(0.299) * rgb[..., 0] + F(0.587) * rgb[..., 1]) + F(0.114) * rgb[..., 2]


def shifted(a, ox, oy, fill):
    """(b, inside): b[y, x] = a[y + oy, x + ox] where that lies inside the frame, `fill` elsewhere"""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((H, W), bool)
    ys, yd = (slice(oy, H), slice(0, H - oy)) if oy >= 0 else (slice(0, H + oy), slice(-oy, H))
    xs, xd = (slice(ox, W), slice(0, W - ox)) if ox >= 0 else (slice(0, W + ox), slice(-ox, W))
    if abs(oy) < H and abs(ox) < W:
        b[yd, xd] = a[ys, xs]
        inside[yd, xd] = True
    return b, inside


def denoise(color, geometry, instance=None, albedo=None, iterations=4, flags=DEMODULATE, depth_tol=0.05, normal_cos=0.9, luma_tol=0.0):
    """color (H, W, 4) float32; geometry (H, W, 4) float32 = normal, t; instance (H, W) int32; albedo (H, W) uint32. Returns (H, W, 4) float32."""
    color = np.ascontiguousarray(color, np.float32)
    geometry = np.ascontiguousarray(geometry, np.float32)
    depth_tol, normal_cos, luma_tol = F(depth_tol), F(normal_cos), F(luma_tol)
    with np.errstate(all="ignore"):
        n, t = geometry[..., :3], geometry[..., 3]
        hit = t <= F(99998.0)
        den = den_of(albedo) if flags & DEMODULATE else None
        I = color[..., :3].copy()
        if flags & DEMODULATE:
            I = np.where(hit[..., None], I / den, I)
        for p in range(iterations):
            s = 1 << p
            dtol = (depth_tol * t) * F(s)
            L = luma(I)
            total = np.zeros_like(I)
            wsum = np.zeros(t.shape, np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    k = K[abs(dy)] * K[abs(dx)]
                    Iq, inside = shifted(I, dx * s, dy * s, 0)
                    if dx == 0 and dy == 0:
                        m = np.ones(t.shape, bool)
                    else:
                        tq, _ = shifted(t, dx * s, dy * s, 0)
                        nq, _ = shifted(n, dx * s, dy * s, 0)
                        hq, _ = shifted(hit, dx * s, dy * s, False)
                        m = hq & (np.abs(tq - t) <= dtol) & (((nq[..., 0] * n[..., 0] + nq[..., 1] * n[..., 1]) + nq[..., 2] * n[..., 2]) >= normal_cos)
                        if flags & MATCH_INSTANCE:
                            iq, _ = shifted(instance, dx * s, dy * s, 0)
                            m &= iq == instance
                        if flags & LUMA_STOP:
                            Lq, _ = shifted(L, dx * s, dy * s, 0)
                            m &= np.abs(Lq - L) <= luma_tol
                    w = np.where(m, k, F(0.0)).astype(np.float32)
                    total = np.where(inside[..., None], total + Iq * w[..., None], total)      # a tap outside the frame is skipped
                    wsum = np.where(inside, wsum + w, wsum)
            I = np.where(hit[..., None], total / wsum[..., None], I)                            # a pixel that is no hit copies I
        if flags & DEMODULATE:
            I = np.where(hit[..., None], I * den, I)
    return np.concatenate([I.astype(np.float32), color[..., 3:]], axis=-1)


def guides(H, W, seed=0):
    """Hand-made planes with everything the filter looks at: a depth edge (vertical, at x = W // 2), a normal edge (horizontal, at y = H // 2),
    two instance ids along a diagonal, pixels that are no hit (a miss, t beyond 99998, a NaN t), albedo bytes 0 and 255 among random ones.
    Returns {"geometry" (H, W, 4) float32, "ids" (H, W) GBUFFER_IDS records, "albedo" (H, W) uint32}."""
    rng = np.random.RandomState(1000 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    g = np.zeros((H, W, 4), np.float32)
    g[..., 3] = np.where(xx < W // 2, 10.0, 40.0) + 0.01 * xx + 0.02 * yy + rng.uniform(-0.02, 0.02, (H, W))
    up = np.array([0.0, 1.0, 0.0], np.float32)
    side = np.array([0.6, 0.0, 0.8], np.float32)
    g[..., :3] = np.where((yy < H // 2)[..., None], up, side) + rng.uniform(-0.02, 0.02, (H, W, 3)).astype(np.float32)
    ids = np.zeros((H, W), np.dtype([("instance", "<i4"), ("tri", "<u4"), ("u", "<f4"), ("v", "<f4")]))
    ids["instance"] = np.where(xx + 2 * yy < (W + 2 * H) // 2, 3, 7)
    ids["tri"] = rng.randint(0, 1 << 20, (H, W))
    ids["u"], ids["v"] = rng.uniform(0, 1, (H, W)), rng.uniform(0, 1, (H, W))
    albedo = (rng.randint(1, 256, (H, W, 3)).astype(np.uint32) * np.array([1, 1 << 8, 1 << 16], np.uint32)).sum(axis=-1).astype(np.uint32) | np.uint32(0xFF000000)
    pick = lambda k: (rng.randint(0, H, k), rng.randint(0, W, k))
    albedo[pick(max(1, H * W // 16))] &= np.uint32(0xFFFF00FF)          # a green byte of 0
    albedo[pick(max(1, H * W // 16))] |= np.uint32(0x00FF0000)          # a blue byte of 255
    if H * W > 1:
        miss = pick(max(1, H * W // 12))
        g[miss] = (0.0, 0.0, 0.0, 99999.0); ids["instance"][miss] = -1; albedo[miss] = 0
        far = pick(max(1, H * W // 40))
        g[far] = (0.0, 0.0, 0.0, 99998.5); albedo[far] = 0
        g[pick(max(1, H * W // 40)) + (3,)] = np.nan
    return {"geometry": g, "ids": ids, "albedo": albedo}


def noisy_color(H, W, seed=0, nans=True):
    """(H, W, 4) float32: a smooth signal plus seeded noise, an alpha that differs per pixel and, with `nans`, a few NaN channels"""
    rng = np.random.RandomState(2000 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    c = np.empty((H, W, 4), np.float32)
    for ch in range(3):
        c[..., ch] = 0.5 + 0.3 * np.sin(0.2 * xx + ch) * np.cos(0.15 * yy) + rng.normal(0, 0.2, (H, W))
    c[..., 3] = rng.uniform(0, 1, (H, W))
    if nans and H * W > 8:
        c[rng.randint(0, H, 2), rng.randint(0, W, 2), rng.randint(0, 3, 2)] = np.nan
    return c


def surface_records(planes):
    """The same guides as CrtSurfaceHit records (H * W, 12) int32: the first 36 bytes are the three planes' pixel, field for field"""
    g, ids, albedo = planes["geometry"], planes["ids"], planes["albedo"]
    H, W = albedo.shape
    rec = np.zeros((H * W, 12), np.int32)
    rec[:, 0:4] = g.reshape(-1, 4).view(np.int32)
    rec[:, 4:8] = ids.reshape(-1).view(np.int32).reshape(-1, 4)
    rec[:, 8] = albedo.reshape(-1).view(np.int32)
    rec[:, 9:12] = 0x5A5A5A5A                                           # material, texU, texV: nothing the filter may look at
    return rec
