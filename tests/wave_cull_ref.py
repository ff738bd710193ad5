"""The wave test of the staged instance cull (crt_device.h: wave_cone, cone_rejects) restated in float32 numpy, operation by operation and in the
kernel's order, with the lemma it rests on ((6) above staged_candidate_mask's helpers) as float64 and exact-rational checks.

Shapes: T waves of L lanes and K instances. d (T, L, 3) float32 directions, o (T, 3) float32 shared origins, cf (T, K, 3) / w (T, K) the table's
spheres (fl(c), w). `ulp` (-1, 0, +1) moves every v_rsq_f32 / v_sqrt_f32 result by that many float32 steps: the instructions are good to one ulp,
numpy's are correctly rounded, and the margins must hold for whatever the hardware returns in between."""
from fractions import Fraction

import numpy as np

F = np.float32
M0, M1, M2 = F(4e-6), F(8e-6), F(8e-6)         # CRT_CONE_M0, _M1, _M2


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _bump(x, ulp):
    x = np.asarray(x, F)
    if ulp > 0:
        return np.nextafter(x, F(np.inf))
    if ulp < 0:
        return np.nextafter(x, F(-np.inf))
    return x


def rsq(x, ulp=0):
    with np.errstate(all="ignore"):
        return _bump((1.0 / np.sqrt(np.asarray(x, F).astype(np.float64))).astype(F), ulp)


def sqrt(x, ulp=0):
    with np.errstate(all="ignore"):
        return _bump(np.sqrt(np.asarray(x, F)), ulp)


def fmax0(x):
    """fmaxf(0.0f, x): a NaN x gives 0"""
    return np.where(np.isnan(x), F(0), np.maximum(F(0), x)).astype(F)


def staged_terms(o, cf, w):
    """what the staging lane holds: oc (T, K, 3), oc2, r2 (candidate_mask's), cullable"""
    with np.errstate(all="ignore"):
        oc = (np.asarray(cf, F) - np.asarray(o, F)[:, None, :]).astype(F)
        oc2 = dot3(oc[..., 0], oc[..., 1], oc[..., 2], oc[..., 0], oc[..., 1], oc[..., 2])
        w = np.broadcast_to(np.asarray(w, F), oc2.shape)
        r2 = w * w * F(1.0201) + F(4e-6) * oc2
        return oc, oc2, r2, w >= 0


def wave_cone(d, ulp=0):
    """wave_cone of a full wave: axis a = lane 0's direction, ra = rsq(a.a), ct, st, ok -- all (T,) (a: (T, 3))"""
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        dd = dot3(d[..., 0], d[..., 1], d[..., 2], d[..., 0], d[..., 1], d[..., 2])
        a = d[:, 0, :]
        ra = rsq(dd[:, 0], ulp)
        q = dot3(d[..., 0], d[..., 1], d[..., 2], a[:, None, 0], a[:, None, 1], a[:, None, 2])
        admitted = (dd >= F(0.999)) & (dd <= F(1.001)) & (q > 0)
        qn = np.where(admitted, q * rsq(dd, ulp), F(0)).astype(F)
        m = qn.view(np.uint32).min(axis=1).view(F)          # the unsigned minimum of the bit patterns, as the kernel takes it
        ct = m * ra - M0
        ok = ct >= F(0.5)
        st = sqrt(fmax0(F(1) - ct * ct), ulp)
    return dict(a=a, ra=ra, ct=ct, st=st, ok=ok)


def cone_rejects(cone, oc, oc2, r2, cullable, ulp=0):
    """(T, K): the wave test; False wherever the wave's guard failed"""
    a, ra, ct, st = cone["a"][:, None, :], cone["ra"][:, None], cone["ct"][:, None], cone["st"][:, None]
    with np.errstate(all="ignore"):
        R2 = r2 * (F(1) + M1)
        rs = rsq(oc2, ulp)
        cphi = (dot3(oc[..., 0], oc[..., 1], oc[..., 2], a[..., 0], a[..., 1], a[..., 2]) * rs) * ra
        spsi = sqrt(R2, ulp) * rs
        cpsi = sqrt(fmax0(F(1) - spsi * spsi), ulp)
        rhs = (ct * cpsi - st * spsi) - M2
        rej = cullable & (oc2 > R2) & (oc2 > F(1e-30)) & (oc2 < F(1e30)) & (cphi < rhs)
    return rej & cone["ok"][:, None]


def wave_rejects(o, d, cf, w, ulp=0):
    oc, oc2, r2, cullable = staged_terms(o, cf, w)
    return cone_rejects(wave_cone(d, ulp), oc, oc2, r2, cullable, ulp)


def lane_culls(o, d, cf, w):
    """(T, L, K): candidate_mask's per-lane predicate"""
    oc, oc2, r2, cullable = staged_terms(o, cf, w)
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        dd = dot3(d[..., 0], d[..., 1], d[..., 2], d[..., 0], d[..., 1], d[..., 2])[:, :, None]
        b = dot3(oc[:, None, :, 0], oc[:, None, :, 1], oc[:, None, :, 2], d[:, :, None, 0], d[:, :, None, 1], d[:, :, None, 2])
        oc2, r2 = oc2[:, None, :], r2[:, None, :]
        return cullable[:, None, :] & ((oc2 * dd - b * b > r2 * dd) | ((b < 0) & (oc2 > r2)))


def lemma_margin64(o, d, cf, w):
    """(T, L, K) float64: min over t > 0 of |o + t d - fl(c)|^2, minus (1.02 w^2 + 2.8e-6 x^2), relative to the bound. The lemma: > 0."""
    o, d, cf, w = (np.asarray(v, F).astype(np.float64) for v in (o, d, cf, w))
    oc = cf - o[:, None, :]
    x2 = (oc * oc).sum(-1)
    bound = 1.02 * np.broadcast_to(w, x2.shape) ** 2 + 2.8e-6 * x2
    b = np.einsum("tkc,tlc->tlk", oc, d)
    dd = (d * d).sum(-1)[:, :, None]
    dist2 = np.where(b > 0, x2[:, None, :] - b * b / dd, x2[:, None, :])
    return (dist2 - bound[:, None, :]) / bound[:, None, :]


def lemma_holds_exact(o, d, cf, w):
    """one lane, one instance, in rationals (every float is one): the lemma's inequality for all t > 0"""
    o, d, cf = ([Fraction(float(v)) for v in vec] for vec in (o, d, cf))
    w = Fraction(float(w))
    oc = [c - p for c, p in zip(cf, o)]
    x2 = sum(v * v for v in oc)
    bound = Fraction(102, 100) * w * w + Fraction(28, 10 ** 7) * x2
    b = sum(p * q for p, q in zip(oc, d))
    dd = sum(v * v for v in d)
    if b <= 0:
        return x2 > bound
    return x2 * dd - b * b > bound * dd
