"""The root pre-test of the camera bounce (crt_device.h: root_pretest_misses) restated in float32 numpy, one IEEE operation per numpy operation in
the kernel's order (the library is built with -ffp-contract=off): Traversal::enter's transform and reciprocals and the root's two slab tests,
under an arbitrary "closest so far". The pre-test is the same step at the bound 99999.

Shapes: m (4, 4) float32 inverse transform (row vectors, as the arenas hold it), o (3,) the shared origin, d (n, 3) directions,
kids: the two child records of the instance's root (arena `nodes` rows), or None for a root that is a leaf."""
import numpy as np

F = np.float32
BOUND0 = F(99999.0)          # what closest_hit starts with (no_hit): the pre-test's bound
MISS = F(1e30)


def xform(m, vx, vy, vz, vw):
    """xform_xyz: ((m0 vx + m1 vy) + m2 vz) + m3 vw per column"""
    m = np.asarray(m, F)
    return [((m[0, j] * vx + m[1, j] * vy) + m[2, j] * vz) + m[3, j] * vw for j in range(3)]


def enter(m, o, d):
    """Traversal::enter: mo (3 scalars), md and inv (3 arrays of n). 1.0f / x in IEEE single precision, which is what recip3 returns."""
    o = np.asarray(o, F); d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        mo = xform(m, o[0], o[1], o[2], F(1.0))
        md = xform(m, d[:, 0], d[:, 1], d[:, 2], F(0.0))
        inv = [F(1.0) / md[j] for j in range(3)]
    return mo, md, inv


def slab(mo, inv, bmin, bmax, bound):
    """intersect_aabb<false>: tnear where the box is passed, 1e30 otherwise. fminf / fmaxf return the operand that is not a NaN: np.fmin / np.fmax."""
    with np.errstate(all="ignore"):
        tmin = [(F(bmin[k]) - mo[k]) * inv[k] for k in range(3)]
        tmax = [(F(bmax[k]) - mo[k]) * inv[k] for k in range(3)]
        tnear = np.fmax(np.fmax(np.fmin(tmin[0], tmax[0]), np.fmin(tmin[1], tmax[1])), np.fmin(tmin[2], tmax[2]))
        tfar = np.fmin(np.fmin(np.fmax(tmin[0], tmax[0]), np.fmax(tmin[1], tmax[1])), np.fmax(tmin[2], tmax[2]))
        ok = (tnear < tfar) & (tnear > 0) & (tnear < np.asarray(bound, F))
    return np.where(ok, tnear, MISS).astype(F), tnear.astype(F), tfar.astype(F)


def root_step(m, o, d, kids, bound=BOUND0):
    """(dist1, dist2) of the root's inner step with `bound` as the closest so far (a scalar or one per ray)"""
    mo, _, inv = enter(m, o, d)
    return slab(mo, inv, kids[0]["min"], kids[0]["max"], bound)[0], slab(mo, inv, kids[1]["min"], kids[1]["max"], bound)[0]


def pretest_clears(m, o, d, kids):
    """root_pretest_misses: the bit is cleared iff both slab tests return 1e30 at 99999; a root that is a leaf (kids None) clears nothing"""
    if kids is None:
        return np.zeros(len(d), bool)
    d1, d2 = root_step(m, o, d, kids, BOUND0)
    return (d1 == MISS) & (d2 == MISS)


def instance_terms(arenas, i):
    """(m, kids or None) of instance i from a session's arenas"""
    inst = arenas["instances"][i]
    node = arenas["nodes"][int(arenas["roots"][inst["meshIndex"]])]
    m = np.ascontiguousarray(inst["inv"], F)
    if node["triCount"] != 0:
        return m, None
    return m, arenas["nodes"][int(node["leftFirst"]):int(node["leftFirst"]) + 2]


def frame_clears(arenas, o, d):
    """(n rays, n instances) bool: the (ray, instance) pairs the pre-test clears, for rays d (n, 3) from the shared origin o"""
    cols = []
    for i in range(len(arenas["instances"])):
        m, kids = instance_terms(arenas, i)
        cols.append(pretest_clears(m, o, d, kids))
    return np.stack(cols, 1)
