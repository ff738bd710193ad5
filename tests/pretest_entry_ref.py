"""The committing form of the camera bounce's root pre-test (crt_device.h: root_pretest_enters, (7g) above root_pretest_misses) restated in float32
numpy beside the two steps it stands for, on the arithmetic of tests/root_pretest_ref.py.

  enter_then_inner   what Traversal::enter followed by the root's Traversal::inner leave in a lane, written as the traversal writes it: the branch
                     on `dist2 != 1e30` that pushes, the branch on `dist1 == 1e30` that pops (the stack is empty: the lane leaves the instance).
  commit             what root_pretest_enters computes and, for the lanes it takes, stores: selects on one compare, `take = first & (n1 != 1e30)`.
  wave_commits       the pre-test's loop over a wave's surviving instances in ascending order: which lane stays inside which instance, and the
                     mask each lane carries into the trip loop.

A lane's state is a dict of arrays over the rays: mo (3 scalars), md, inv (3 arrays), t, u, v, tri, prot, inters, sp, ref, active, slot0 (stack
row 0; -1 where nothing was written), cur. refs = (left, right): the two child refs of the root's pair record, CRT_LEAF_BIT marking a leaf."""
import os
import sys

import numpy as np

import root_pretest_ref as ref
import wave_cull_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from count_box_pretest import table_sphere      # noqa: E402  (fl(c), w) of crt_instances.h, restated

F = np.float32
LEAF_BIT = np.uint32(0x80000000)
FIELDS = ("mo", "md", "inv", "t", "u", "v", "tri", "prot", "inters", "sp", "ref", "active", "slot0", "cur")


def _dists(m, o, d, kids, bound):
    mo, md, inv = ref.enter(m, o, d)
    d1 = ref.slab(mo, inv, kids[0]["min"], kids[0]["max"], bound)[0]
    d2 = ref.slab(mo, inv, kids[1]["min"], kids[1]["max"], bound)[0]
    return mo, md, inv, d1, d2


def enter_then_inner(m, o, d, kids, refs, inst, bound=ref.BOUND0):
    """Traversal::enter(inst, o, d, bound) and then Traversal::inner on the root, lane by lane as the traversal's branches run"""
    mo, md, inv, d1, d2 = _dists(m, o, d, kids, bound)
    n = len(d)
    st = dict(mo=mo, md=md, inv=inv, t=np.full(n, bound, F), u=np.zeros(n, F), v=np.zeros(n, F), tri=np.zeros(n, np.uint32),
              prot=np.ones(n, np.int32), inters=np.zeros(n, np.int32), sp=np.zeros(n, np.int32), ref=np.zeros(n, np.uint32),
              active=np.ones(n, bool), slot0=np.full(n, -1, np.int64), cur=np.full(n, inst, np.uint32))
    for i in range(n):
        dist1, dist2, near, far = d1[i], d2[i], np.uint32(refs[0]), np.uint32(refs[1])
        if dist1 > dist2:
            dist1, dist2, near, far = dist2, dist1, far, near
        if dist2 != ref.MISS:                       # both children hit: push the far one
            st["slot0"][i] = int(far); st["sp"][i] = 1
        if dist1 == ref.MISS:                       # pop_next on an empty stack: nothing kept, the lane is outside again
            st["active"][i] = False
        else:
            st["ref"][i] = near
    return st


def commit(m, o, d, kids, refs, inst, first, bound=ref.BOUND0):
    """root_pretest_enters: (clear, take, state) -- `clear`: the lane's bit goes; `take`: the lane stays inside `inst` with `state`"""
    n = len(d)
    if kids is None:                                # a root that is a leaf: nothing is tested, nothing cleared, nobody stays
        return np.zeros(n, bool), np.zeros(n, bool), None
    mo, md, inv, d1, d2 = _dists(m, o, d, kids, bound)
    miss = (d1 == ref.MISS) & (d2 == ref.MISS)
    sw = d1 > d2
    n1, n2 = np.where(sw, d2, d1), np.where(sw, d1, d2)
    near = np.where(sw, np.uint32(refs[1]), np.uint32(refs[0])).astype(np.uint32)
    far = np.where(sw, np.uint32(refs[0]), np.uint32(refs[1])).astype(np.uint32)
    take = np.asarray(first, bool) & (n1 != ref.MISS)
    push = n2 != ref.MISS
    st = dict(mo=mo, md=md, inv=inv, t=np.full(n, bound, F), u=np.zeros(n, F), v=np.zeros(n, F), tri=np.zeros(n, np.uint32),
              prot=np.ones(n, np.int32), inters=np.zeros(n, np.int32), sp=push.astype(np.int32), ref=near,
              active=np.ones(n, bool), slot0=np.where(push, far.astype(np.int64), -1), cur=np.full(n, inst, np.uint32))
    return miss | take, take, st


def same_state(a, b, rows):
    """field by field, bit for bit, over the lanes `rows`; returns the names that differ"""
    bad = []
    for f in FIELDS:
        xs, ys = (a[f], b[f]) if f in ("mo", "md", "inv") else ([a[f]], [b[f]])
        for x, y in zip(xs, ys):
            x, y = np.broadcast_to(np.asarray(x), (len(a["t"]),))[rows], np.broadcast_to(np.asarray(y), (len(a["t"]),))[rows]
            if x.dtype.kind == "f":
                x, y = x.astype(F).view(np.uint32), y.astype(F).view(np.uint32)
            if not np.array_equal(x, y):
                bad.append(f)
    return bad


def first_of(mask, k):
    """the device's test on a 64-bit mask in two halves: bit k is the lowest one the lane holds"""
    mask = np.asarray(mask, np.uint64)
    lo, hi = (mask & np.uint64(0xFFFFFFFF)).astype(np.uint32), (mask >> np.uint64(32)).astype(np.uint32)
    if k < 32:
        bit = np.uint32(1 << k)
        return (lo & (bit | np.uint32(bit - 1))) == bit
    bit = np.uint32(1 << (k - 32))
    return (lo == 0) & ((hi & (bit | np.uint32(bit - 1))) == bit)


def wave_commits(masks, terms, o, d, touch=None, ordered=True):
    """The pre-test's loops over one wave: masks (n,) uint64 per lane, terms[k] = (m, kids or None, refs) per instance, the shared origin o and the
    lanes' directions d. Instances in ascending order; an instance no lane holds is skipped. Returns (masks after, committed instance or -1 per lane,
    pushed per lane, executed pre-tests). ordered=False: the loop WITHOUT the order condition -- a lane that holds bit k and is inside no instance
    commits whatever lower bits it holds (what the tests show to be wrong, never what the device does)."""
    masks = np.array(masks, np.uint64)
    n = len(masks)
    inside = np.full(n, -1, np.int64)
    pushed = np.zeros(n, bool)
    executed = 0
    for k in (range(len(terms)) if touch is None else touch):
        bit = np.uint64(1) << np.uint64(k)
        if not (masks & bit).any():
            continue
        executed += 1
        m, kids, refs = terms[k]
        first = (first_of(masks, k) if ordered else (masks & bit) != 0) & (inside < 0)
        clear, take, st = commit(m, o, d, kids, refs, k, first)
        masks = np.where(clear, masks & ~bit, masks)
        inside = np.where(take, k, inside)
        if st is not None:
            pushed |= take & (st["sp"] == 1)
    return masks, inside, pushed, executed


def instance_terms(arenas, i):
    """(m, kids or None, refs) of instance i: refs as the device's pair record names the children -- node index, or CRT_LEAF_BIT for a leaf child (which
    leaf it is does not enter the commit)"""
    m, kids = ref.instance_terms(arenas, i)
    if kids is None:
        return m, None, None
    node = arenas["nodes"][int(arenas["roots"][arenas["instances"][i]["meshIndex"]])]
    first = int(node["leftFirst"])
    refs = tuple(np.uint32(first + j) | (LEAF_BIT if kids[j]["triCount"] != 0 else np.uint32(0)) for j in range(2))
    return m, kids, refs


def spheres(arenas):
    """the cull table's (c, w) of every instance with an inner root, from the arenas (float64 centre, float32 radius), in instance order"""
    out = []
    for inst in arenas["instances"]:
        node = arenas["nodes"][int(arenas["roots"][inst["meshIndex"]])]
        assert node["triCount"] == 0
        kids = arenas["nodes"][int(node["leftFirst"]):int(node["leftFirst"]) + 2]
        fwd = np.linalg.inv(np.ascontiguousarray(inst["inv"], F).astype(np.float64))
        lo = np.minimum(kids[0]["min"], kids[1]["min"]).astype(np.float64)
        hi = np.maximum(kids[0]["max"], kids[1]["max"]).astype(np.float64)
        c, _, w = table_sphere(lo, hi, fwd)
        out.append((c, float(w)))
    return out


def lane_masks(arenas, o, d):
    """(n rays,) uint64: the instances candidate_mask keeps for rays d from the shared origin o. A single-leaf instance is kept for every ray (the
    cull table holds it with radius -1: never culled)."""
    n = len(arenas["instances"])
    inner = [k for k in range(n) if ref.instance_terms(arenas, k)[1] is not None]
    sub = dict(arenas); sub["instances"] = arenas["instances"][inner]
    sph = spheres(sub)
    cf, wr = np.array([c for c, _ in sph], np.float64).astype(F)[None], np.array([r for _, r in sph], F)[None]
    kept = np.ones((len(d), n), bool)
    kept[:, inner] = ~wave_cull_ref.lane_culls(np.asarray(o, F)[None], np.asarray(d, F)[None], cf, wr)[0]
    return (kept.astype(np.uint64) << np.arange(n, dtype=np.uint64)).sum(1).astype(np.uint64)
