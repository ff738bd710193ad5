"""What tests/test_gpu_query_deep_stack.py and the deep frames of tests/test_gpu_deep_stack.py rely on, asserted without a GPU for every
`levels` they use (tests/deep_stack_ref.py: the scene, the rays, the points): the batches really walk a stack levels - 1 deep in every 64-ray
chunk beside rays that stay shallow, every instance is somebody's closest hit, the references hold no NaN, the slot index wraps from 34
levels on and the 250-pop cap is met at 300 -- and the bounded loop (tests/trace_rays_ref.py, the reference of record for bounded queries)
equals the filter of the oracle's unbounded records, so the GPU file may assert either."""
import numpy as np
import pytest

import ao_ref
import deep_stack_ref as ds
import inclusive_ref as ir
import trace_rays_ref as rr

CONSTANT_BOUND = np.float32(150.0)


@pytest.mark.parametrize("levels", ds.LEVELS)
def test_conditions_of_the_ray_batches(levels, nthreads):
    o, d = ds.rays(levels)
    orc = ds.oracle(levels, nthreads)
    ref, st = orc.closest_hits(o, d)
    n = len(o)
    misses = int((ref["instance"] < 0).sum())
    per_instance = [int((ref["instance"] == k).sum()) for k in range(len(ds.TRANSLATIONS))]
    chunks = ds.chunk_depths(orc, o, d)
    first = ds.ray_depths(ds.oracle(levels, 1), o[:64], d[:64])
    print(f"levels {levels}: {misses} of {n} miss, closest hits per instance {per_instance}, maxStack per chunk {chunks}, "
          f"{int((first <= 4).sum())} shallow rays in chunk 0, stackOverflows {st['stackOverflows']}, capHits {st['capHits']}")
    assert n == ds.N_RAYS == 321 and len(chunks) == 6
    assert 0.25 * n <= misses <= 0.60 * n
    assert min(per_instance) >= 1
    assert chunks == [levels - 1] * 6 and st["maxStack"] == levels - 1
    assert int((first <= 4).sum()) >= 8 and first.max() == levels - 1
    assert not any(np.isnan(ref[k]).any() for k in ("t", "u", "v"))
    assert (st["stackOverflows"] > 0) == (levels >= 34)
    assert (st["capHits"] > 0) == (levels == 300)


@pytest.mark.parametrize("levels", ds.LEVELS)
def test_every_spilled_slot_decides_some_record(levels, nthreads):
    """A ray that hits the last level's triangle has its record before the first pop: whatever the stack returns afterwards cannot change it,
    and only work counters would notice a lost entry. The edge rays walk as deep and then pop down to T_j, which slot j alone holds (T_k is
    pushed at N_k, above k entries): a stack that loses or mixes up slot j gives them another triangle. Every entry from 15 -- the smallest
    number of LDS slots of any instantiation -- up to the top is such a ray's; on the trees deeper than 33 levels, the top 32 entries: the
    slot index wraps, so these rays also need the wrapped slots to hold what was written last."""
    o, d = ds.rays(levels)
    k = np.arange(len(o))
    edge = (k % 8 == 1) | (k % 16 == 6)
    orc = ds.oracle(levels, nthreads)
    ref, _ = orc.closest_hits(o[edge], d[edge])
    assert int(edge.sum()) == 60 and (ref["instance"] >= 0).all()
    assert (ds.ray_depths(ds.oracle(levels, 1), o[edge], d[edge]) == levels - 1).all()
    assert all(edge[c * 64:(c + 1) * 64].sum() >= 10 for c in range(5))                  # in every whole chunk
    slots = set(ref["tri"].tolist())
    wanted = set(range(max(15, levels - 33), levels - 1))                                 # (32 entries below the top the slot index has wrapped)
    assert wanted <= slots, sorted(wanted - slots)


@pytest.mark.parametrize("levels", ds.LEVELS)
def test_bounded_loop_equals_the_filter(levels, nthreads):
    a = ds.scene(levels)
    o, d = ds.rays(levels)
    ref, st = ds.oracle(levels, nthreads).closest_hits(o, d)
    plain = rr.bounded_closest_hits(a, o, d)
    assert rr.same_records(plain, ref)                           # the unbounded loop is the oracle's, wrap and cap included
    hits = ref["instance"] >= 0
    for fam, (tmax, kept) in list(rr.tmax_families(ref).items()) + [("constant", (np.full(len(o), CONSTANT_BOUND), None))]:
        want = rr.filtered(ref, tmax)
        if kept is not None:
            assert np.array_equal(want["instance"] >= 0, hits if kept else np.zeros_like(hits)), fam
        else:
            assert 0 < int((want["instance"] >= 0).sum()) < int(hits.sum()), fam      # the constant cuts some hits and keeps others
        assert rr.same_records(rr.bounded_closest_hits(a, o, d, tmax), want), fam


@pytest.mark.parametrize("levels", ds.LEVELS)
def test_the_inclusive_rule_walks_as_deep_and_matters(levels, nthreads):
    a = ds.scene(levels)
    o, d = ds.rays(levels)
    ref, _ = ds.oracle(levels, nthreads).closest_hits(o, d)
    inc, st = ir.closest_hits(a, o, d)
    assert st["maxStack"] == levels - 1 and (st["stackOverflows"] > 0) == (levels >= 34) and (st["capHits"] > 0) == (levels == 300)
    assert not any(np.isnan(inc[k]).any() for k in ("t", "u", "v"))
    differ = (inc["tri"] != ref["tri"]) | (inc["instance"] != ref["instance"])
    assert differ.sum() >= 8                                     # the rays that start inside the nested boxes


@pytest.mark.parametrize("levels", ds.LEVELS)
def test_conditions_of_the_ao_points(levels, nthreads):
    P, nrm = ds.ao_points(levels)
    orc = ds.oracle(levels, nthreads)
    table = ao_ref.table()
    traces = (nrm != 0).any(axis=1)
    assert len(P) == ds.N_RAYS and 0 < int((~traces).sum()) < len(P) // 4
    for samples in (1, 8):
        par = {"samples": samples, "radius": 1e9, "bias": 1e-3, "seed": 0}
        o, dirs, w = ao_ref.rays(P, nrm, np.arange(len(P), dtype=np.uint32), par, table)
        oo, dd = np.repeat(o, samples, axis=0), dirs.reshape(-1, 3)
        tr = np.repeat(traces, samples)
        rec, st = orc.closest_hits(oo[tr], dd[tr])
        share = float((rec["instance"] >= 0).mean())
        first = ds.chunk_depths(orc, oo[:64 * samples][tr[:64 * samples]], dd[:64 * samples][tr[:64 * samples]], 64 * samples)
        print(f"levels {levels}, {samples} samples: {share:.3f} of the sample rays occluded, maxStack {st['maxStack']}, first chunk {first}")
        assert 0.05 <= share <= 0.60
        assert st["maxStack"] == levels - 1 and first == [levels - 1]
        assert not any(np.isnan(rec[k]).any() for k in ("t", "u", "v"))
        t = rec["t"][rec["instance"] >= 0]
        assert (t < CONSTANT_BOUND).any() and (t > CONSTANT_BOUND).any()      # the finite radius of the GPU tests cuts some and keeps some


@pytest.mark.parametrize("levels", ds.LEVELS)
def test_conditions_of_the_ao_frame(levels, nthreads):
    """the 72 x 40 frame of the four-instance scene from AO_CAMERA: its pixels see the fourth tree, and their sample rays walk the other three"""
    (P, nrm, k), planes = ds.ao_frame_items(levels, 72, 40, nthreads)
    hit = (nrm != 0).any(axis=1)
    assert (planes["ids"]["instance"].reshape(-1)[hit] == 3).all() and 0.25 * len(P) <= int(hit.sum()) < len(P)
    assert not np.isnan(P).any() and not np.isnan(nrm).any() and (nrm[hit, 2] > 0.99).all()
    par = {"samples": 8, "radius": 1e9, "bias": 1e-3, "seed": 0}
    o, dirs, w = ao_ref.rays(P, nrm, k, par, ao_ref.table())
    rec, st = ds.oracle(levels, nthreads, 4).closest_hits(np.repeat(o, 8, axis=0)[np.repeat(hit, 8)], dirs.reshape(-1, 3)[np.repeat(hit, 8)])
    share = float((rec["instance"] >= 0).mean())
    print(f"levels {levels}: {int(hit.sum())} of {len(P)} pixels hit, {share:.3f} of their sample rays occluded, maxStack {st['maxStack']}")
    assert st["maxStack"] == levels - 1 and 0.05 <= share <= 0.60
    assert not any(np.isnan(rec[f]).any() for f in ("t", "u", "v"))
    t = rec["t"][rec["instance"] >= 0]
    assert (t < CONSTANT_BOUND).any() and (t > CONSTANT_BOUND).any()


@pytest.mark.parametrize("levels", ds.LEVELS)
def test_conditions_of_the_edge_frame(levels, nthreads):
    """the 96 x 64 frame of tests/test_gpu_deep_stack.py from EDGE_CAMERA: primary rays as deep as the tree, every instance seen, sky beside
    them, and every spilled entry the first hit of some pixel (as the edge rays of the batches: T_j is what entry j holds)"""
    import oracle_lib
    a = ds.scene(levels)
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    iv, ip, pos = ds.camera_of(96, 64, ds.EDGE_CAMERA)
    d = orc.raygen(96, 64, iv, ip).reshape(-1, 3)
    rec, st = orc.closest_hits(np.tile(pos, (len(d), 1)), d)
    hit = rec["instance"] >= 0
    per_instance = [int((rec["instance"] == k).sum()) for k in range(3)]
    print(f"levels {levels}: {int(hit.sum())} of {len(d)} pixels hit, per instance {per_instance}, maxStack {st['maxStack']}")
    assert st["maxStack"] == levels - 1 and 0.2 * len(d) <= int(hit.sum()) <= 0.6 * len(d)
    assert per_instance[0] >= 100 and sum(n >= 1 for n in per_instance) >= (2 if levels == 300 else 3)      # (300 levels: the first tree hides the one to its right)
    assert not any(np.isnan(rec[f]).any() for f in ("t", "u", "v"))
    wanted, seen = set(range(max(15, levels - 33), levels - 1)), set(rec["tri"][hit].tolist())
    if levels <= 48:
        assert wanted <= seen, sorted(wanted - seen)
    else:
        assert len(wanted & seen) >= 16              # (levels 0.3 apart: closer than the edge moves between two pixel rows, so not every entry has its pixel)


def test_conditions_of_the_large_batch(nthreads):
    """the 64 and the 2560 rays of the overflow-area growth test: one chunk and 40 chunks, each of them 47 deep"""
    orc = ds.oracle(48, nthreads)
    for n in (64, 2560):
        o, d = ds.rays(48, n)
        ref, _ = orc.closest_hits(o, d)
        assert ds.chunk_depths(orc, o, d) == [47] * (n // 64)
        assert 0.25 * n <= int((ref["instance"] < 0).sum()) <= 0.60 * n and not any(np.isnan(ref[k]).any() for k in ("t", "u", "v"))
