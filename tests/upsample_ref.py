"""A numpy float32 restatement of the definition in include/crt_upsample.h, written from the header: vectorised over the full-resolution pixels,
the four taps in the definition's order, every operation a float32 operation of its own (numpy contracts nothing; no float64 intermediate). What
crtu_upsample must give, bit for bit. The hand-made guides are those of tests/denoise_ref.py (guides(), surface_records()); low_image() here
makes the low-resolution image."""
import numpy as np

from denoise_ref import den_of, guides, surface_records  # noqa: F401 (the inputs are re-exported)

MATCH_INSTANCE, MODULATE = 1, 2
INTERPOLATED, NEAREST, EMPTY = 0, 1, 2
F = np.float32
DEFAULTS = dict(depth_tol=0.05, normal_cos=0.9)
UNGUIDED = dict(depth_tol=float("inf"), normal_cos=float("-inf"))


def low_size(width, height, factor, offset=(0, 0)):
    """(LW, LH) of the header: every low sample's pixel lies in the frame"""
    return (width - offset[0] + factor - 1) // factor, (height - offset[1] + factor - 1) // factor


def sample_pixels(width, height, factor, offset=(0, 0)):
    """(ys, xs): the full-resolution pixels the low samples sit on, as index arrays for a[np.ix_(ys, xs)]"""
    lw, lh = low_size(width, height, factor, offset)
    return factor * np.arange(lh) + offset[1], factor * np.arange(lw) + offset[0]


def upsample(low, geometry, instance=None, albedo=None, factor=2, offset=(0, 0), flags=0, depth_tol=0.05, normal_cos=0.9):
    """low (LH, LW) or (LH, LW, 4) float32; geometry (H, W, 4) float32 = normal, t; instance (H, W) int32; albedo (H, W) uint32.
    Returns (out (H, W) or (H, W, 4) float32, state (H, W) uint32)."""
    low = np.ascontiguousarray(low, np.float32)
    geometry = np.ascontiguousarray(geometry, np.float32)
    H, W = geometry.shape[:2]
    ox, oy = offset
    LW, LH = low_size(W, H, factor, offset)
    one_channel = low.ndim == 2
    v = low.reshape(LH, LW, -1)
    assert v.shape[2] in (1, 4) and not (flags & MODULATE and one_channel)
    n, t = geometry[..., :3], geometry[..., 3]
    depth_tol, normal_cos = F(depth_tol), F(normal_cos)
    zero, one = F(0.0), F(1.0)
    with np.errstate(all="ignore"):
        hit = t <= F(99998.0)
        yy, xx = np.mgrid[0:H, 0:W]
        X0, Y0 = np.floor_divide(xx - ox, factor), np.floor_divide(yy - oy, factor)
        fx = ((xx - ox) - X0 * factor).astype(np.float32) / F(factor)
        fy = ((yy - oy) - Y0 * factor).astype(np.float32) / F(factor)
        weights = ((one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy)
        dtol = depth_tol * t
        total = np.zeros((H, W, v.shape[2]), np.float32)
        wsum = np.zeros((H, W), np.float32)
        counted = np.zeros((H, W), bool)
        any_near, any_first = np.zeros((H, W), bool), np.zeros((H, W), bool)
        best = np.zeros((H, W), np.float32)
        nearest, first = np.zeros_like(total), np.zeros_like(total)
        for k in range(4):
            X, Y = X0 + (k & 1), Y0 + (k >> 1)
            exists = (X >= 0) & (X < LW) & (Y >= 0) & (Y < LH)
            Xc, Yc = np.clip(X, 0, LW - 1), np.clip(Y, 0, LH - 1)       # where a tap does not exist, any sample: nothing of it is used
            vq = v[Yc, Xc]
            gy, gx = factor * Yc + oy, factor * Xc + ox
            tg, ng = t[gy, gx], n[gy, gx]
            b = weights[k]
            candidate = exists & np.isfinite(vq).all(axis=-1)
            hg = tg <= F(99998.0)
            d = np.abs(tg - t)
            stops = hg & (d <= dtol) & (((ng[..., 0] * n[..., 0] + ng[..., 1] * n[..., 1]) + ng[..., 2] * n[..., 2]) >= normal_cos)
            if flags & MATCH_INSTANCE:
                stops &= instance[gy, gx] == instance
            ok = candidate & (b > zero) & np.where(hit, stops, ~hg)
            total = np.where(ok[..., None], total + vq * b[..., None], total)
            wsum = np.where(ok, wsum + b, wsum)
            counted |= ok
            near = candidate & hit & hg & ~np.isnan(d)
            take = near & (~any_near | (d < best))
            nearest = np.where(take[..., None], vq, nearest)
            best = np.where(take, d, best)
            any_near |= near
            first = np.where((candidate & ~any_first)[..., None], vq, first)
            any_first |= candidate
        out = np.where(counted[..., None], total / wsum[..., None], np.where(any_near[..., None], nearest, first)).astype(np.float32)
        state = np.where(counted, INTERPOLATED, np.where(any_first, NEAREST, EMPTY)).astype(np.uint32)
        if flags & MODULATE:
            out[..., :3] = np.where(hit[..., None], out[..., :3] * den_of(albedo), out[..., :3])
    return (out[..., 0] if one_channel else out), state


def low_image(width, height, factor, offset=(0, 0), channels=4, seed=0, specials=True):
    """The low image of a width x height frame: a smooth signal plus seeded noise per channel and, with `specials` (and more than 8 samples), NaN,
    +inf and -inf samples, one 2 x 2 block of samples all NaN (its inner pixels have no finite tap among the four) and a sample of zero."""
    lw, lh = low_size(width, height, factor, offset)
    rng = np.random.RandomState(6000 + seed + 17 * factor + 3 * offset[0] + 5 * offset[1])
    yy, xx = np.mgrid[0:lh, 0:lw]
    v = np.empty((lh, lw, channels), np.float32)
    for ch in range(channels):
        v[..., ch] = 0.5 + 0.3 * np.sin(0.4 * xx + ch) * np.cos(0.3 * yy) + rng.normal(0, 0.2, (lh, lw))
    if specials and lw * lh > 8:
        k = max(1, lw * lh // 30)
        pick = lambda: (rng.randint(0, lh, k), rng.randint(0, lw, k), rng.randint(0, channels, k))
        v[pick()] = np.nan
        v[pick()] = np.inf
        v[pick()] = -np.inf
        v[pick()] = 0.0
        if lw >= 4 and lh >= 4:
            v[lh // 2:lh // 2 + 2, lw // 2:lw // 2 + 2, 0] = np.nan
    return v[..., 0].copy() if channels == 1 else v
