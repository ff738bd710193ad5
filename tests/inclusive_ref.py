"""Reference for the inclusive box test of the device queries (CRT_RAYS_INCLUSIVE / CRT_AO_INCLUSIVE, include/crt_api.h): the bounded loop of
tests/trace_rays_ref.py -- instance loop + intersect_bvh of tests/test_traversal_independent.py, `best` initialised to the bound -- with ONE
function replaced: the box test. intersect_bvh is not copied: it looks its box test up in its module, so the inclusive function is put there
for the duration of a call and the original restored afterwards (inclusive_rule). Also the surface rays the mode exists for.

The rule, float32 without contraction: tnear and tfar as upstream computes them (kernel_main.cl:108-114); entry = fmax(tnear, 0); the box
passes iff tnear <= tfar and tfar >= 0 and entry < minSoFar; the function returns entry on a pass and 1e30 otherwise."""
import contextlib

import numpy as np

import test_traversal_independent as tti
import trace_rays_ref as rr

F = np.float32


def intersect_aabb_inclusive(o, inv, bmin, bmax, min_so_far):
    tmin = (bmin - o) * inv
    tmax = (bmax - o) * inv
    lo, hi = np.fmin(tmin, tmax), np.fmax(tmin, tmax)
    tnear = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
    tfar = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
    entry = np.fmax(tnear, F(0.0))
    ok = (tnear <= tfar) & (tfar >= F(0.0)) & (entry < min_so_far)
    return np.where(ok, entry, F(1e30)).astype(np.float32)


@contextlib.contextmanager
def inclusive_rule(on=True):
    """intersect_bvh of test_traversal_independent under the inclusive box test while the block runs (on=False: upstream's, untouched)"""
    saved = tti.intersect_aabb
    if on:
        tti.intersect_aabb = intersect_aabb_inclusive
    try:
        yield
    finally:
        tti.intersect_aabb = saved


def closest_hits(a, origins, dirs, tmax=None, inclusive=True):
    """trace_rays_ref.bounded_closest_hits under the given rule, and the work it counted: (records as _lib.RAYHIT_DTYPE, a miss always MISS;
    {"pops", "capHits", "stackOverflows", "maxStack", ...} -- the loop's own `stats`, which it hands to every intersect_bvh call)"""
    seen = []

    def counted(*args):
        seen.append(args[-1])
        return tti.intersect_bvh(*args)

    saved = rr.intersect_bvh
    rr.intersect_bvh = counted
    try:
        with inclusive_rule(inclusive):
            out = rr.bounded_closest_hits(a, origins, dirs, tmax)
    finally:
        rr.intersect_bvh = saved
    assert all(st is seen[0] for st in seen)
    return out, seen[0]


def scene_extent(a):
    """the longest edge of the box around every mesh's root box (object space)"""
    return float((a["nodes"]["max"][a["roots"]].max(axis=0) - a["nodes"]["min"][a["roots"]].min(axis=0)).max())


def surface_rays(a, orc, iv, ip, pos, w, h, seed=7):
    """Rays that start on surfaces: the first hits of the w x h camera grid (the oracle's records, finite t), each stepped back along its
    camera ray by 1e-3 x the scene's extent, with a seeded random unit direction. (origins, dirs), float32, contiguous."""
    cam = orc.raygen(w, h, iv, ip).reshape(-1, 3)
    o0 = np.tile(np.asarray(pos, np.float32), (len(cam), 1))
    rec, _ = orc.closest_hits(o0, cam)
    hit = (rec["instance"] >= 0) & np.isfinite(rec["t"])
    P = (o0[hit] + cam[hit] * rec["t"][hit][:, None]).astype(np.float32)
    o = (P - cam[hit] * F(1e-3 * scene_extent(a))).astype(np.float32)
    rng = np.random.RandomState(seed)
    d = rng.randn(len(o), 3).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def query_rays(a, orc, iv, ip, pos, name, n=4099):
    """The n rays of the query tests: surface_rays of the 256 x 144 grid thinned evenly to n - 2100, then the 1500 rays from inside the scene's
    boxes and the 600 axis-parallel rays from grid points of test_traversal_independent.ray_sets (0 * inf in the slab test)."""
    so, sd = surface_rays(a, orc, iv, ip, pos, 256, 144)
    pick = np.linspace(0, len(so) - 1, n - 2100).astype(np.int64)
    sets = tti.ray_sets(a, iv, ip, pos, orc, np.random.RandomState(sum(map(ord, name))))
    o = np.concatenate([so[pick], sets[1][0], sets[2][0]]).astype(np.float32)
    d = np.concatenate([sd[pick], sets[1][1], sets[2][1]]).astype(np.float32)
    assert len(o) == n
    return np.ascontiguousarray(o), np.ascontiguousarray(d)
