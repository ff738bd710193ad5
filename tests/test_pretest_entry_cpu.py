"""The committing form of the camera bounce's root pre-test (crt_device.h: root_pretest_enters, (7g)) without a GPU, on the float32 restatement of
tests/pretest_entry_ref.py.

  1. Same state: for every lane the commit takes, the stored fields equal, bit for bit, what Traversal::enter followed by the root's inner step
     leave -- over the random and adversarial rays, instances and boxes of tests/test_root_pretest_cpu.py (zero, denormal, infinite and NaN
     direction components, origins inside and on a face of a box, zero-thickness boxes), with inner and leaf child refs. Both children hit
     (a push), one child hit, the nearer child a leaf and the right child nearer all occur, equal distances (left first) in a case of their own; a lane the commit does not take is one the
     traversal leaves at the root or one that was not `first`.
  2. Order: a lane commits only to the lowest instance its mask holds; a lane holding the bit of a lower single-leaf instance never commits.
  3. Whole frames: a ray that commits to instance k has the same oracle hit record when every instance below k is taken out of the scene, and
     its hit instance is never below k."""
import numpy as np
import pytest

from clraytracer_amd import driver, scenes
import oracle_lib
import pretest_entry_ref as entry
import root_pretest_ref as ref
from test_root_pretest_cpu import _cases, _kids

F = np.float32
INNER_REFS = (np.uint32(10), np.uint32(11))
LEAF_LEFT = (np.uint32(7) | entry.LEAF_BIT | np.uint32(3 << 24), np.uint32(11))
LEAF_BOTH = (np.uint32(7) | entry.LEAF_BIT | np.uint32(3 << 24), np.uint32(40) | entry.LEAF_BIT | np.uint32(1 << 24))


def test_the_committed_state_is_enter_and_the_root_step_field_by_field():
    rng = np.random.RandomState(20267)
    seen = dict(push=0, one=0, leaf_near=0, swapped=0, special=0, not_taken_miss=0)
    for n, (m, o, d, kids) in enumerate(_cases(rng)):
        refs = (INNER_REFS, LEAF_LEFT, LEAF_BOTH)[n % 3]
        want = entry.enter_then_inner(m, o, d, kids, refs, 5)
        first = np.ones(len(d), bool)
        clear, take, got = entry.commit(m, o, d, kids, refs, 5, first)
        # the lanes taken are exactly those the traversal keeps inside the instance after the root step, and every `first` lane loses the bit then
        assert np.array_equal(take, want["active"])
        assert (clear == (take | ref.pretest_clears(m, o, d, kids))).all()
        assert entry.same_state(got, want, take) == [], (n, entry.same_state(got, want, take))
        # a lane that is not `first` stores nothing and clears exactly what root_pretest_misses clears
        clear0, take0, _ = entry.commit(m, o, d, kids, refs, 5, np.zeros(len(d), bool))
        assert not take0.any() and np.array_equal(clear0, ref.pretest_clears(m, o, d, kids))
        d1, d2 = ref.root_step(m, o, d, kids)
        seen["push"] += int((take & (got["sp"] == 1)).sum()); seen["one"] += int((take & (got["sp"] == 0)).sum())
        seen["leaf_near"] += int((take & ((got["ref"] & entry.LEAF_BIT) != 0)).sum())
        seen["swapped"] += int((take & (d1 > d2)).sum())
        seen["special"] += int((~np.isfinite(d).all(1) | (d == 0).any(1)).sum()); seen["not_taken_miss"] += int((~take).sum())
    assert all(v > 0 for v in seen.values()), seen


def test_equal_distances_go_left_first_and_push_the_right_child():
    """two boxes that start at the same face: dist1 == dist2, `dist1 > dist2` is false, the left child is next and the right one is pushed"""
    kids = _kids([0, 0, 0], [1, 1, 1], [0, 0.25, 0.25], [2, 0.75, 0.75])
    o, d = np.array([-3.0, 0.5, 0.5], F), np.array([[1, 0, 0], [1, 0, -0.0]], F)
    d1, d2 = ref.root_step(np.eye(4, dtype=F), o, d, kids)
    assert (d1 == d2).all() and (d1 == F(3.0)).all()
    for refs in (INNER_REFS, LEAF_LEFT):
        clear, take, got = entry.commit(np.eye(4, dtype=F), o, d, kids, refs, 2, np.ones(2, bool))
        want = entry.enter_then_inner(np.eye(4, dtype=F), o, d, kids, refs, 2)
        assert take.all() and clear.all() and (got["ref"] == refs[0]).all() and (got["slot0"] == int(refs[1])).all() and (got["sp"] == 1).all()
        assert entry.same_state(got, want, take) == []


def test_nan_zero_and_infinite_directions_commit_nothing_the_traversal_would_not_hold():
    kids = _kids([0, 0, 0], [1, 1, 1], [2, 0, 0], [3, 1, 1])
    d = np.array([[np.nan, 0, 1], [0, 0, 0], [np.nan, np.nan, np.nan], [np.inf, 0, 0], [0, 0, 1], [-0.0, 0.0, 1]], F)
    o = np.array([0.5, 0.5, -3.0], F)
    clear, take, got = entry.commit(np.eye(4, dtype=F), o, d, kids, INNER_REFS, 0, np.ones(len(d), bool))
    want = entry.enter_then_inner(np.eye(4, dtype=F), o, d, kids, INNER_REFS, 0)
    assert np.array_equal(take, want["active"]) and np.array_equal(take, [False, False, False, False, True, True]) and clear.all()
    assert entry.same_state(got, want, take) == [] and (got["sp"][take] == 0).all() and (got["ref"][take] == INNER_REFS[0]).all()


def test_a_lane_commits_only_to_the_lowest_instance_its_mask_holds():
    """the loop over a wave's survivors: masks in both 32-bit halves; instance 1 and instance 33 are single-leaf roots"""
    eye = np.eye(4, dtype=F)
    hit = _kids([-1, -1, 2], [1, 1, 3], [-1, -1, 5], [1, 1, 6])              # the ray along +z passes both children
    gone = _kids([10, 10, 2], [11, 11, 3], [10, 10, 5], [11, 11, 6])          # ... and neither of these
    terms = [(eye, hit, INNER_REFS)] * 40
    terms[1] = terms[33] = (eye, None, None)
    terms[2] = terms[34] = (eye, gone, INNER_REFS)
    o, d = np.zeros(3, F), np.tile(np.array([0, 0, 1], F), (8, 1))
    bits = lambda *ks: np.uint64(sum(1 << k for k in set(ks)))
    masks = [bits(0, 3), bits(1, 3), bits(2, 3), bits(3), bits(33, 35), bits(34, 35), bits(1, 35), bits()]
    after, inside, pushed, executed = entry.wave_commits(masks, terms, o, d)
    #        lowest inner: in   leaf below  cleared, then 3   alone   leaf below (high half)   cleared, then 35   low leaf, high inner   nothing
    assert inside.tolist() == [0, -1, 3, 3, -1, 35, -1, -1]
    assert after.tolist() == [bits(3), bits(1, 3), bits(), bits(), bits(33, 35), bits(), bits(1, 35), bits()]
    assert pushed.tolist() == [True, False, True, True, False, True, False, False]
    assert executed == 7                                                          # 0, 1, 2, 3, 33, 34, 35: each once per wave
    for k in (0, 5, 31, 32, 40, 63):                                              # the test on the halves is "the lowest set bit is k"
        ms = np.array([bits(k), bits(k, 63), bits(0, k) if k else bits(0), bits(k - 1, k) if k else bits(0), bits(31, 32, k)], np.uint64)
        want = [(int(m) & -int(m)) == (1 << k) for m in ms]
        assert entry.first_of(ms, k).tolist() == want, k


@pytest.mark.parametrize("n,w,h", [(8, 72, 40), (16, 64, 64)])
def test_frames_keep_their_hit_records_without_the_instances_below_the_committed_one(n, w, h, nthreads, tmp_path):
    from test_gpu_camera_cull import _instances, _one_triangle_mesh, _scene
    insts = _instances(n)
    insts[2] = scenes.Instance(2, 0xFFFF, scenes._trs(1.5, (0.2, 1.0, 0.1), 0.8, (1.0, 3.0, 2.0)))        # a single-leaf root at a low index
    sc = _scene(f"pretest-entry-{n}", insts, [_one_triangle_mesh(tmp_path)])
    with driver.Session(w, h, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        iv, ip, pos = s.camera()
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    d = np.asarray(orc.raygen(w, h, iv, ip), F).reshape(-1, 3)
    o = np.asarray(pos, F)
    terms = [entry.instance_terms(a, k) for k in range(n)]
    assert terms[2][1] is None
    masks = entry.lane_masks(a, o, d)                                                                  # the sphere cull's mask per ray
    after, inside, pushed, _ = entry.wave_commits(masks, terms, o, d)
    full = orc.closest_hits(np.tile(o, (len(d), 1)), d)[0]
    hit = full["instance"] >= 0
    took = inside >= 0
    assert took.any() and pushed.any() and (took & ~pushed).any()
    assert not (hit & took & (full["instance"] < inside)).any()
    checked = 0
    for k in range(1, n):
        rays = np.nonzero(inside == k)[0]
        if not len(rays):
            continue
        assert k < 2 or not (masks[rays] & np.uint64(4)).any()                                          # nobody jumps over the single-leaf instance
        b = dict(a); b["instances"] = np.ascontiguousarray(a["instances"][k:])
        got = oracle_lib.Oracle(b, nthreads=nthreads).closest_hits(np.tile(o, (len(rays), 1)), d[rays])[0]
        want = full[rays].copy()
        want["instance"] = np.where(want["instance"] >= 0, want["instance"] - k, want["instance"])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
        checked += len(rays)
    assert checked > 0
