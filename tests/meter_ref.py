"""Restatement of include/crt_meter.h for the tests: the composed colour and the luminance in numpy float32, one rounding per operation as the
header orders them; the log code, the statistics and the resolve in integers (Python's own, which cannot overflow); float64 for the two
fraction products only, which are exact there; the exposure's arithmetic in float32 again. Nothing here depends on an order of summation."""
import math

import numpy as np

HEAL, ADAPT = 1, 2
BINS, QMIN, QMAX = 256, 107 << 16, 139 << 16
MAX_GROUPS, DEFAULT_GROUPS, RECORD_WORDS = 2048, 128, 264
F = np.float32
LUMA = (F(0.2126), F(0.7152), F(0.0722))


def composed(color, flags=0, ao=None, ao_strength=1.0):
    """steps 1-2 of crtp_present: (H, W, 4) float32, alpha as it came"""
    color = np.ascontiguousarray(color, np.float32)
    c = color[..., :3].copy()
    with np.errstate(all="ignore"):
        if flags & HEAL:
            c[~np.isfinite(c)] = F(0)
        if ao is not None:
            s = F(ao_strength)
            f = (F(1) - s) + s * np.ascontiguousarray(ao, np.float32)
            if flags & HEAL:
                f = np.where(np.isfinite(f), f, F(1)).astype(np.float32)
            c = c * f[..., None]
    return np.concatenate([c.astype(np.float32), color[..., 3:]], axis=-1)


def luminance(c):
    with np.errstate(all="ignore"):
        return ((c[..., 0] * LUMA[0] + c[..., 1] * LUMA[1]) + c[..., 2] * LUMA[2]).astype(np.float32)


def log_code(l):
    """(valid, q): q is meaningful where valid"""
    l = np.ascontiguousarray(l, np.float32)
    with np.errstate(all="ignore"):
        valid = (l >= F(0)) & (l < F(np.inf))
        q = l.view(np.uint32) >> np.uint32(7)
        q = np.where(l < F(2.0 ** -20), np.uint32(QMIN), np.where(l >= F(2.0 ** 12), np.uint32(QMAX - 1), q)).astype(np.uint32)
    return valid, q


def decode(q):
    """as_float(q << 7)"""
    return (np.asarray(q, np.uint32) << np.uint32(7)).view(np.float32)


def statistics(color, rect=None, flags=0, ao=None, ao_strength=1.0):
    """dict(valid, invalid, sumQ, minQ, maxQ, hist) over the rectangle (x0, y0, x1, y1); None: the whole frame"""
    h, w = color.shape[:2]
    x0, y0, x1, y1 = (0, 0, w, h) if rect is None else rect
    c = composed(color, flags, ao, ao_strength)[y0:y1, x0:x1]
    valid, q = log_code(luminance(c))
    q = q[valid].astype(np.int64)
    n = int(valid.sum())
    return dict(valid=n, invalid=int(valid.size) - n, sumQ=int(q.sum()), minQ=int(q.min()) if n else 0, maxQ=int(q.max()) if n else 0,
                hist=np.bincount((q - QMIN) >> 13, minlength=BINS).astype(np.uint32))


def binned_mean(hist, lo, hi):
    """the mean of the bin centres over the pixels ranked lo .. hi-1: what the resolve forms unless the fractions are (0, 1)"""
    total, cum = 0, 0
    for b in range(BINS):
        n = int(hist[b])
        total += max(0, min(cum + n, hi) - max(cum, lo)) * (QMIN + (b << 13) + 4096)
        cum += n
    return total // (hi - lo)


def ranks(n, low, high):
    lo = int(math.floor(float(F(low)) * n))
    hi = min(n, int(math.ceil(float(F(high)) * n)))
    if hi <= lo:
        hi = min(lo + 1, n)
        lo = hi - 1
    return lo, hi


def clamp(v, lo, hi):
    return min(max(F(v), F(lo)), F(hi))


def resolve(st, key=0.18, low=0.0, high=1.0, min_exposure=2.0 ** -8, max_exposure=2.0 ** 8, prev=None, rate_up=1.0, rate_down=1.0):
    """The eight words of CrtxResult as uint32. prev: the exposure of the record before as a float32 (any bits), or None: CRTX_ADAPT is off
    or no record was given."""
    n = st["valid"]
    p = None
    if prev is not None:
        p = F(prev)
        if not (np.isfinite(p) and p > 0):
            p = None
    if n == 0:
        e = F(1) if p is None else p
        words = [e, e, F(0), 0, 0, st["invalid"], 0, 0]
    else:
        if F(low) == 0 and F(high) == 1:
            mean_q = st["sumQ"] // n
        else:
            mean_q = binned_mean(st["hist"], *ranks(n, low, high))
        average = decode(np.uint32(mean_q))
        with np.errstate(all="ignore"):
            target = clamp(F(key) / average, min_exposure, max_exposure)
            exposure = target
            if p is not None:
                exposure = clamp(p + (target - p) * (F(rate_up) if target > p else F(rate_down)), min_exposure, max_exposure)
        words = [exposure, target, average, mean_q, n, st["invalid"], st["minQ"], st["maxQ"]]
    out = np.zeros(8, np.uint32)
    out[:3] = np.array(words[:3], np.float32).view(np.uint32)
    out[3:] = words[3:]
    return out


def meter(color, rect=None, flags=0, ao=None, ao_strength=1.0, prev=None, **params):
    """(record (8,) uint32, hist (256,) uint32) of crtx_meter; prev counts only under ADAPT"""
    st = statistics(color, rect, flags, ao, ao_strength)
    return resolve(st, prev=prev if flags & ADAPT else None, **params), st["hist"]


def expose(color, exposure, flags=0, ao=None, ao_strength=1.0):
    """crtx_expose: (H, W, 4) float32; exposure: the float32 the record holds"""
    c = composed(color, flags, ao, ao_strength)
    with np.errstate(all="ignore"):
        c[..., :3] = c[..., :3] * F(exposure)
    return c


def rate(dt, tau):
    return F(1) if not tau > 0 else F(1.0 - math.exp(-dt / tau))


def scratch_bytes(w, h, groups):
    if w < 1 or h < 1 or w > 16384 or h > 16384 or not 0 <= groups <= MAX_GROUPS:
        return 0
    return (groups or min(DEFAULT_GROUPS, ((w + 31) // 32) * ((h + 7) // 8))) * RECORD_WORDS * 4
