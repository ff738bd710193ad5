"""Reference for the bounded ray queries (crt_trace_rays, include/crt_api.h): the instance loop + IntersectBVH of kernel_main.cl:124-160,
189-217 started with a smaller "closest so far" -- a numpy restatement on intersect_bvh / matmul_xyz of tests/test_traversal_independent.py
(which is the unbounded loop and is pinned against the C oracle there), with `best` initialised to the bound instead of 99999. Also the ten
families of bounds the tests use, the filter "the unbounded record if its t < tmax, else the miss record" the API promises equality with when
the unbounded u, v are finite, and the bit-for-bit comparison of records."""
import numpy as np

from clraytracer_amd import _lib
from test_traversal_independent import intersect_bvh, matmul_xyz

F = np.float32
NO_BOUND = F(99999.0)                        # upstream's `Infinite` (kernel_main.cl:189): the unbounded loop's first "closest so far", and the largest bound
MISS = np.array([(99999.0, 0.0, 0.0, 0, -1)], _lib.RAYHIT_DTYPE)[0]


def bound_of(tmax, n):
    """B = !(tmax >= 99999.0f) ? tmax : 99999.0f per ray (a NaN stays NaN); no tmax array: 99999"""
    if tmax is None:
        return np.full(n, NO_BOUND, np.float32)
    tmax = np.ascontiguousarray(tmax, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(~(tmax >= NO_BOUND), tmax, NO_BOUND).astype(np.float32)


def bounded_closest_hits(a, origins, dirs, tmax=None):
    """closest_hits_numpy of test_traversal_independent with besthit.distance = B; records as _lib.RAYHIT_DTYPE, a miss always MISS"""
    n = len(origins)
    nodes, tris = a["nodes"], a["tris"]
    nodes_min, nodes_max = np.ascontiguousarray(nodes["min"], np.float32), np.ascontiguousarray(nodes["max"], np.float32)
    left_first, tri_count = nodes["leftFirst"].astype(np.int64), nodes["triCount"].astype(np.int64)
    tv0, tv1, tv2 = (np.ascontiguousarray(tris[k], np.float32) for k in ("v0", "v1", "v2"))
    best = bound_of(tmax, n)
    out = np.full(n, MISS, _lib.RAYHIT_DTYPE)
    stats = {"traversals": 0, "pops": 0, "innerVisits": 0, "triTests": 0, "capHits": 0, "stackOverflows": 0, "maxStack": 0}
    o, d = np.ascontiguousarray(origins, np.float32).reshape(-1, 3), np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for i, inst in enumerate(a["instances"]):
            m = np.ascontiguousarray(inst["inv"], np.float32)
            mo, md = matmul_xyz(m, o, 1.0), matmul_xyz(m, d, 0.0)
            inter, t, u, v, tri = intersect_bvh(mo, md, nodes_min, nodes_max, left_first, tri_count, tv0, tv1, tv2, int(a["roots"][inst["meshIndex"]]), best, stats)
            got = inter != 0
            out["t"][got], out["u"][got], out["v"][got], out["tri"][got], out["instance"][got] = t[got], u[got], v[got], tri[got], i
            best[got] = t[got]
    return out


def filtered(ref, tmax):
    """the unbounded records `ref` where t < tmax, the miss record elsewhere (a NaN tmax: a miss)"""
    out = ref.copy()
    if tmax is not None:
        with np.errstate(invalid="ignore"):
            out[~((ref["instance"] >= 0) & (ref["t"] < np.asarray(tmax, np.float32)))] = MISS
    return out


def tmax_families(ref):
    """name -> (tmax per ray, whether the reference hits are kept) from the unbounded records; a missing ray's t is 99999"""
    t = ref["t"].astype(np.float32)
    with np.errstate(all="ignore"):
        return {
            "2t": (t * F(2.0), True), "1.001t": (t * F(1.001), True), "nextafter-up": (np.nextafter(t, F(np.inf)), True),
            "t": (t.copy(), False), "nextafter-down": (np.nextafter(t, F(0.0)), False), "0.999t": (t * F(0.999), False), "0.5t": (t * F(0.5), False),
            "zero": (np.zeros_like(t), False), "minus-one": (np.full_like(t, -1.0), False), "nan": (np.full_like(t, np.nan), False),
        }


def same_records(got, want):
    """bit for bit, field by field"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and all(np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                                                          want[k].view(np.uint32) if want[k].dtype == np.float32 else want[k]) for k in ("t", "u", "v", "tri", "instance"))
