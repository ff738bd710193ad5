"""Hazard H2 through every device-buffer query that owns a traversal stack: crt_query_kernel, crt_rays_kernel / crt_rays_inclusive_kernel,
crt_shade_kernel, crt_ao_kernel / crt_ao_inclusive_kernel (points and frame), each with and without the instance tree (CrtStackT<0>: 20 slots
in LDS, CrtStackT<4>: 16, the rest in the query context's overflow area), on the hand-built caterpillar trees of tests/deep_stack_ref.py: 15 to
21 pushes before the first pop (one below, at and above every LDS boundary), around upstream's 32 slots (33, 34, 48 levels) and into the
250-pop cap (300). CRT_RAYS_GRID=3 unless stated: three workgroups walk the six chunks of 321 rays one after the other -- a stale entry of
the chunk before, a wrong overflow block or a parked row overwritten by a push would each give another record. What the batches are
(depth per chunk, shallow rays beside deep ones, shares of misses, no NaN) and that the bounded loop equals the filter of the unbounded
records is asserted without a GPU in tests/test_query_deep_stack_cpu.py. Everything is compared bit for bit; no ray, point or pixel is excluded."""
import ctypes as C
import functools

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import ao_ref
import deep_stack_ref as ds
import inclusive_ref as ir
import oracle_lib
import shade_ref
import trace_rays_ref as rr
from test_query_deep_stack_cpu import CONSTANT_BOUND
from util import bits

pytestmark = pytest.mark.gpu
W, H = 64, 48
LEVELS = ds.LEVELS
SIZES = (1, 63, 64, 65, 321)
GBUFFER, WRITE_RAYS, ASYNC = 8192, 2, 4
BIAS = 1e-3
RADII = (1e5, float(CONSTANT_BOUND))         # >= 99999: the bound is upstream's `Infinite`; 150: cuts some sample rays and keeps others
SUN = scenes.get("tiny").sun_angle


def session(monkeypatch, grid="3", tlas=None, w=W, h=H):
    for k, v in (("CRT_RAYS_GRID", grid), ("CRT_TLAS", tlas)):
        monkeypatch.delenv(k, raising=False)
        if v is not None:
            monkeypatch.setenv(k, v)
    monkeypatch.delenv("CRT_KERNEL", raising=False)
    s = driver.Session(w, h, device=0)
    s.load_scene(scenes.get("tiny"))                             # materials, textures, skybox
    return s


def upload(s, levels, tlas, n_instances=3):
    ni = ds.upload(s, ds.scene(levels, n_instances))
    if tlas == "1":
        assert ds.tlas_nodes(s) > 0                              # the forced instance tree exists (use_tlas, csrc/crt_frame.h)
    return ni


def bounds_of(ref):
    """name -> tmax: trace_rays_ref.tmax_families of the unbounded records and the constant bound"""
    fam = {k: v[0] for k, v in rr.tmax_families(ref).items()}
    fam["constant"] = np.full(len(ref), CONSTANT_BOUND, np.float32)
    return fam


@functools.lru_cache(maxsize=None)
def reference(levels, inclusive=False):
    """(arenas, origins, dirs, unbounded records, the loop's work counters, {bound: (tmax, records of the bounded loop)}): computed once, never
    modified. Upstream's rule: the C oracle's records (and counters); the inclusive rule: tests/inclusive_ref.py. The bounded loop runs once
    over every bound's copy of the rays."""
    a = ds.scene(levels)
    o, d = ds.rays(levels)
    if inclusive:
        ref, st = ir.closest_hits(a, o, d)
    else:
        ref, st = oracle_lib.Oracle(a, nthreads=16).closest_hits(o, d)
    fam = bounds_of(ref)
    tm = np.concatenate(list(fam.values()))
    want, _ = ir.closest_hits(a, np.tile(o, (len(fam), 1)), np.tile(d, (len(fam), 1)), tm, inclusive=inclusive)
    bounded = {}
    for k, name in enumerate(fam):
        w = want[k * len(o):(k + 1) * len(o)].copy()
        w.setflags(write=False); fam[name].setflags(write=False)
        bounded[name] = (fam[name], w)
    ref.setflags(write=False)
    return a, o, d, ref, st, bounded


# ---- crt_query_hits: records and every work counter ----
@pytest.mark.parametrize("tlas", ["0", "1"])
def test_query_hits_and_counters(monkeypatch, tlas):
    refs = {levels: reference(levels) for levels in LEVELS}      # before the session: the host mirror holds one session at a time
    with session(monkeypatch, tlas=tlas) as s:
        for levels in LEVELS:
            a, o, d, ref, st, _ = refs[levels]
            ni = upload(s, levels, tlas)
            got = np.zeros(len(o), _lib.RAYHIT_DTYPE)
            _lib.check(s.hip.crt_query_hits(o.ctypes.data, d.ctypes.data, len(o), ni, got.ctypes.data), "crt_query_hits")
            assert rr.same_records(got, ref), levels
            assert s.counters() == st, levels
            assert st["maxStack"] == levels - 1 and (st["stackOverflows"] > 0) == (levels >= 34) and (st["capHits"] > 0) == (levels == 300)


# ---- crt_trace_rays: closest and occluded, unbounded and bounded, under both box rules ----
@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("tlas", ["0", "1"])
def test_trace_rays(monkeypatch, tlas, inclusive):
    refs = {levels: reference(levels, inclusive) for levels in LEVELS}
    with session(monkeypatch, tlas=tlas) as s:
        for levels in LEVELS:
            a, o, d, ref, _, bounded = refs[levels]
            ni = upload(s, levels, tlas)
            to, td = ds.dev(o), ds.dev(d)
            hits = ref["instance"] >= 0
            got = ds.records(ds.trace_rays(s, ni, to, td, inclusive=inclusive))
            chunks, no_cull, groups = s.rays_stats()
            assert (chunks, groups) == (6, 3) and no_cull == 0, levels      # every origin within the cull's range: the TLAS forms walk their tree
            assert rr.same_records(got, ref), levels
            assert np.array_equal(ds.trace_rays(s, ni, to, td, occluded=True, inclusive=inclusive).cpu().numpy(), hits.astype(np.uint8)), levels
            for name, (tmax, want) in bounded.items():
                tt = ds.dev(tmax)
                assert rr.same_records(ds.records(ds.trace_rays(s, ni, to, td, tt, inclusive=inclusive)), want), (levels, name)
                occ = ds.trace_rays(s, ni, to, td, tt, occluded=True, inclusive=inclusive).cpu().numpy()
                assert np.array_equal(occ, (want["instance"] >= 0).astype(np.uint8)), (levels, name)
                if not inclusive:                                    # tests/test_query_deep_stack_cpu.py: the loop is the filter on these trees
                    assert rr.same_records(want, rr.filtered(ref, tmax)), (levels, name)
            # the sentinel rows behind n stay untouched
            for n in SIZES:
                rec = ds.trace_rays(s, ni, to, td, inclusive=inclusive, n=n, tail=3).cpu().numpy()
                occ = ds.trace_rays(s, ni, to, td, occluded=True, inclusive=inclusive, n=n, tail=3).cpu().numpy()
                assert s.rays_stats() == ((n + 63) // 64, 0, min(3, (n + 63) // 64))
                assert rr.same_records(ds.records(rec, n), ref[:n]), (levels, n)
                assert np.array_equal(occ[:n], hits[:n].astype(np.uint8)), (levels, n)
                assert (rec[n:] == ds.POISON).all() and (occ[n:] == 0xA5).all(), (levels, n)


# ---- crt_shade_rays: the bounce ray's traversal starts on the stack the first one left ----
@functools.lru_cache(maxsize=None)
def shade_reference(levels):
    a, o, d, _, _, _ = reference(levels)
    orc = oracle_lib.Oracle(a, nthreads=16)
    surf, rad = shade_ref.surface(a, orc, o, d), shade_ref.radiance(orc, o, d, SUN)
    surf.setflags(write=False); rad.setflags(write=False)
    return surf, rad


@pytest.mark.parametrize("tlas", ["0", "1"])
def test_shade_rays(monkeypatch, tlas):
    refs = {levels: reference(levels) + shade_reference(levels) for levels in LEVELS}
    with session(monkeypatch, tlas=tlas) as s:
        for levels in LEVELS:
            a, o, d, ref, _, _, want_surf, want_rad = refs[levels]
            assert np.array_equal(want_surf["instance"], ref["instance"])
            ni = upload(s, levels, tlas)
            to, td = ds.dev(o), ds.dev(d)
            for radiance, surface in ((True, True), (True, False), (False, True)):
                rad, surf = ds.shade_rays(s, ni, to, td, SUN, radiance, surface)
                assert s.shade_stats() == (6, 0, 3)
                if radiance:
                    assert np.array_equal(bits(rad), bits(want_rad)), (levels, radiance, surface)
                if surface:
                    assert shade_ref.same_surface(surf, want_surf), (levels, radiance, surface)


# ---- crt_trace_ao: the fused kernel against its composition over the bounded loop's answers and over the session's own ----
@functools.lru_cache(maxsize=None)
def ao_reference(levels, inclusive):
    """{(samples, radius): ao} by ao_ref.compose over the bounded loop's answers (one run of the loop over every combination's sample rays)"""
    a = ds.scene(levels)
    P, nrm = ds.ao_points(levels)
    table = ao_ref.table()
    parts = {}
    for samples in (1, 8):
        o, d, w = ao_ref.rays(P, nrm, np.arange(len(P), dtype=np.uint32), params(samples, 1.0), table)
        for radius in RADII:
            parts[samples, radius] = (np.repeat(o, samples, axis=0), d.reshape(-1, 3), np.full(len(P) * samples, radius, np.float32), w)
    rec, _ = ir.closest_hits(a, np.concatenate([p[0] for p in parts.values()]), np.concatenate([p[1] for p in parts.values()]),
                             np.concatenate([p[2] for p in parts.values()]), inclusive=inclusive)
    out, at = {}, 0
    for key, (oo, _, _, w) in parts.items():
        occ = (rec["instance"][at:at + len(oo)] >= 0).reshape(len(P), key[0])
        at += len(oo)
        out[key] = ao_ref.compose(w, occ)
        out[key].setflags(write=False)
    return out


def params(samples, radius):
    return {"samples": samples, "radius": radius, "bias": BIAS, "seed": 0}


def composed(s, ni, P, nrm, par, table, inclusive, k=None):
    """ao_ref.compose over the session's own occlusion answers (crt_trace_rays) for ao_ref.rays"""
    S = par["samples"]
    o, d, w = ao_ref.rays(P, nrm, np.arange(len(P), dtype=np.uint32) if k is None else k, par, table)
    tmax = np.full(len(P) * S, par["radius"], np.float32)
    occ = ds.trace_rays(s, ni, ds.dev(np.repeat(o, S, axis=0)), ds.dev(d.reshape(-1, 3)), ds.dev(tmax), occluded=True, inclusive=inclusive).cpu().numpy()
    return ao_ref.compose(w, occ.reshape(len(P), S))


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("tlas", ["0", "1"])
def test_trace_ao(monkeypatch, tlas, inclusive):
    table = ao_ref.table()
    refs = {levels: (ao_reference(levels, inclusive), ao_reference(levels, False)) for levels in LEVELS}
    with session(monkeypatch, tlas=tlas) as s:
        for levels in LEVELS:
            P, nrm = ds.ao_points(levels)
            want, plain = refs[levels]
            ni = upload(s, levels, tlas)
            tp, tn = ds.dev(P), ds.dev(nrm)
            for (samples, radius), ao in want.items():
                par = params(samples, radius)
                got = ds.trace_ao(s, ni, tp, tn, par, inclusive)
                assert s.ao_stats() == (6, 0, 3)
                assert np.array_equal(bits(got), bits(ao)), (levels, samples, radius)
                assert np.array_equal(bits(got), bits(composed(s, ni, P, nrm, par, table, inclusive))), (levels, samples, radius)
                assert (got[(nrm == 0).all(axis=1)] == 1.0).all() and (got < 1.0).any()
            if inclusive:
                assert not np.array_equal(bits(want[8, RADII[0]]), bits(plain[8, RADII[0]])), levels      # the rule matters to these points


# ---- crt_frame_ao on a G-buffer frame whose pixels' sample rays walk the trees ----
@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("tlas", ["0", "1"])
def test_frame_ao(monkeypatch, tlas, inclusive):
    w, h = 72, 40
    table = ao_ref.table()
    refs = {levels: ds.ao_frame_items(levels, w, h, 16) for levels in LEVELS}      # the oracle's planes: tests/test_query_deep_stack_cpu.py's conditions hold for them
    rays = oracle_lib.Oracle(ds.scene(16, 4), nthreads=16).raygen(w, h, *ds.camera_of(w, h, ds.AO_CAMERA)[:2])
    with session(monkeypatch, tlas=tlas, w=w, h=h) as s:
        for levels in LEVELS:
            ni = upload(s, levels, tlas, 4)
            args, iv, ip, pos = ds.frame_args(s, ni, SUN, ds.AO_CAMERA)
            assert ds.render(s, args, iv, ip, WRITE_RAYS) == 0          # the frame's own RayGen buffer is the oracle's
            assert np.array_equal(bits(s.read_rays()), bits(rays))
            assert ds.render(s, args, iv, ip, GBUFFER) == 0
            assert s.last_kernel() == f"crt_trace_gbuffer_kernel<0,{tlas},0>"
            planes = s.read_gbuffer_raw()
            (P, nrm, k), want_planes = refs[levels]
            for p in ("geometry", "ids", "albedo"):
                assert np.array_equal(np.ascontiguousarray(planes[p]).view(np.uint32), np.ascontiguousarray(want_planes[p]).view(np.uint32)), (levels, p)
            tp, tn = ds.dev(P), ds.dev(nrm)
            for radius in RADII:
                par = params(8, radius)
                cp = _lib.CrtAoParams(8, radius, BIAS, 0, _lib.CRT_AO_INCLUSIVE if inclusive else 0, 0.0, 0.0)
                _lib.check(s.hip.crt_frame_ao(C.byref(cp), None), "crt_frame_ao")
                got = np.empty((h, w), np.float32)
                _lib.check(s.hip.crt_read_ao(got.ctypes.data, got.size), "crt_read_ao")
                assert s.ao_stats() == (((w + 7) // 8) * ((h + 7) // 8), 0, 3)
                points = ds.trace_ao(s, ni, tp, tn, par, inclusive).reshape(h, w)
                assert np.array_equal(bits(got), bits(points)), (levels, radius)
                assert np.array_equal(bits(got), bits(composed(s, ni, P, nrm, par, table, inclusive, k).reshape(h, w))), (levels, radius)
                miss = planes["geometry"]["t"] > np.float32(99998.0)
                assert 0 < int(miss.sum()) < w * h and (got[miss] == 1.0).all() and (got < 1.0).any()


# ---- the overflow area of the query context grows between two queries in flight ----
@pytest.mark.parametrize("tlas", ["0", "1"])
def test_overflow_area_grows_behind_a_query_in_flight(monkeypatch, tlas):
    levels = 48
    orc = ds.oracle(levels, 16)
    (o1, d1), (o2, d2) = ds.rays(levels, 64), ds.rays(levels, 2560)
    with session(monkeypatch, grid=None, tlas=tlas) as s:
        ni = upload(s, levels, tlas)
        t1, t2 = (ds.dev(o1), ds.dev(d1)), (ds.dev(o2), ds.dev(d2))
        first = ds.trace_rays(s, ni, *t1)                           # one chunk: a grid of one workgroup, an overflow area of one block
        second = ds.trace_rays(s, ni, *t2)                          # 40 chunks, no host synchronisation in between: the area is reallocated
        chunks, no_cull, groups = s.rays_stats()
        assert (chunks, no_cull) == (40, 0) and 1 < groups <= 40    # the grid grew (the first query's is min(chunks, ...) = 1)
        assert rr.same_records(ds.records(first), orc.closest_hits(o1, d1)[0])
        assert rr.same_records(ds.records(second), orc.closest_hits(o2, d2)[0])
        # and back: the small grid in the large area
        assert rr.same_records(ds.records(ds.trace_rays(s, ni, *t1)), orc.closest_hits(o1, d1)[0])
        assert s.rays_stats() == (1, 0, 1)


# ---- a pipelined deep frame and a deep query on a side stream use separate overflow areas ----
@pytest.mark.parametrize("tlas", ["0", "1"])
def test_frame_in_flight_and_query_on_a_side_stream(monkeypatch, tlas, nthreads):
    import torch
    levels, w, h = 48, 320, 184
    a, o, d, ref, _, _ = reference(levels)
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    iv, ip, pos = ds.camera_of(w, h, ds.EDGE_CAMERA)
    want, st = orc.trace(orc.raygen(w, h, iv, ip), pos, SUN)
    assert st["maxStack"] == levels - 1 and st["stackOverflows"] > 0
    with session(monkeypatch, tlas=tlas, w=w, h=h) as s:
        ni = upload(s, levels, tlas)
        args, iv, ip, pos = ds.frame_args(s, ni, SUN, ds.EDGE_CAMERA)
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip((iv, ip, pos), ds.camera_of(w, h, ds.EDGE_CAMERA)))
        to, td = ds.dev(o), ds.dev(d)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        results = []
        for _ in range(3):
            assert ds.render(s, args, iv, ip, ASYNC) == 0            # a frame in flight on its slot's stream and overflow area
            with torch.cuda.stream(side):
                results.append(ds.trace_rays(s, ni, to, td))        # the query context's area, whatever the frames do
        frame = s.read_output()
        torch.cuda.synchronize()
        assert np.array_equal(bits(frame), bits(want))
        for k, out in enumerate(results):
            assert rr.same_records(ds.records(out), ref), k
