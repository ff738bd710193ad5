"""The inclusive box test of the device queries on the GPU (CRT_RAYS_INCLUSIVE / CRT_AO_INCLUSIVE; Session.trace_rays / trace_ao /
ambient_occlusion with inclusive=True): closest-hit records and occlusion bytes against the numpy reference (tests/inclusive_ref.py, pinned
against the all-triangles search in tests/test_inclusive_cpu.py), the AO forms against their own composition over the inclusive occlusion
query. Everything is compared bit for bit; no ray, point or pixel is excluded.
A 64x48 session and CRT_RAYS_GRID=3 unless stated otherwise: three waves walk the 65 chunks of 4099 rays, the 48 tiles of a frame.
Definition: include/crt_api.h (crt_trace_rays, CRT_RAYS_INCLUSIVE)."""
import ctypes as C
import functools

import numpy as np
import pytest

from clraytracer_amd import _lib, scenes
import ao_ref
import inclusive_ref as ir
import oracle_lib
import trace_rays_ref as rr
from test_gpu_ao import BIAS, PATTERN, RADIUS, params
from test_gpu_ao import reference as ao_reference
from test_gpu_trace_rays import _cull_scene, dev, session
from test_inclusive_cpu import load
from util import bits

pytestmark = pytest.mark.gpu
W, H, N = 64, 48, 4099
FAMILIES = ("nextafter-up", "t", "nan")


@functools.lru_cache(maxsize=None)
def reference(name):
    """arenas, the 4099 rays of inclusive_ref.query_rays (surface rays, rays from inside the boxes, axis-parallel rays), their unbounded records
    under the inclusive rule (numpy) and under upstream's (the C oracle): computed once, never modified"""
    a, (iv, ip, pos), _, _, orc = load(name, 16)
    o, d = ir.query_rays(a, orc, iv, ip, pos, name, N)
    ref, st = ir.closest_hits(a, o, d)
    assert st["capHits"] == 0
    plain, _ = orc.closest_hits(o, d)
    for x in (o, d, ref, plain):
        x.setflags(write=False)
    return a, o, d, ref, plain


@functools.lru_cache(maxsize=None)
def bounded_reference(name, family):
    """(tmax, the reference's records under it) for one of trace_rays_ref.tmax_families of the unbounded inclusive records"""
    a, o, d, ref, _ = reference(name)
    tmax, _ = rr.tmax_families(ref)[family]
    want, _ = ir.closest_hits(a, o, d, tmax)
    tmax.setflags(write=False); want.setflags(write=False)
    return tmax, want


@pytest.mark.parametrize("tlas", ["0", "1"])
@pytest.mark.parametrize("name", ["tiny", "cornell-1k"])
def test_closest_and_occluded_equal_the_reference(monkeypatch, name, tlas):
    a, o, d, ref, plain = reference(name)
    hits = ref["instance"] >= 0
    assert hits.sum() > (plain["instance"] >= 0).sum() + N // 10                  # the rule matters to these rays
    with session(monkeypatch, scenes.get(name), tlas=tlas) as s:
        to, td = dev(o), dev(d)
        got = s.trace_rays(to, td, inclusive=True).numpy()
        assert s.rays_stats() == (65, 0, 3)
        assert rr.same_records(got, ref)
        assert np.array_equal(s.trace_rays(to, td, mode="occluded", inclusive=True).cpu().numpy(), hits)
        assert s.rays_stats() == (65, 0, 3)
        for fam in FAMILIES:
            tmax, want = bounded_reference(name, fam)
            tt = dev(tmax)
            assert rr.same_records(s.trace_rays(to, td, tmax=tt, inclusive=True).numpy(), want), fam
            assert np.array_equal(s.trace_rays(to, td, tmax=tt, mode="occluded", inclusive=True).cpu().numpy(), want["instance"] >= 0), fam
        assert np.array_equal(bounded_reference(name, "nextafter-up")[1]["instance"] >= 0, hits)
        assert not (bounded_reference(name, "nan")[1]["instance"] >= 0).any()


def test_batch_shapes(monkeypatch):
    import torch
    a, o, d, ref, _ = reference("tiny")
    with session(monkeypatch, scenes.get("tiny")) as s:
        to, td = dev(o), dev(d)
        stream = torch.cuda.current_stream().cuda_stream
        ni = s.h.crth_num_instances()
        closest, occluded = _lib.CRT_RAYS_CLOSEST | _lib.CRT_RAYS_INCLUSIVE, _lib.CRT_RAYS_OCCLUDED | _lib.CRT_RAYS_INCLUSIVE
        for n in (0, 1, 63, 64, 65):
            batch = _lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 3, 3, n)
            rec = torch.full((n + 3, 5), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
            occ = torch.full((n + 3,), 0xA5, dtype=torch.uint8, device="cuda:0")
            _lib.check(s.hip.crt_trace_rays(C.byref(batch), ni, closest, rec.data_ptr(), stream), "crt_trace_rays")
            _lib.check(s.hip.crt_trace_rays(C.byref(batch), ni, occluded, occ.data_ptr(), stream), "crt_trace_rays")
            rec, occ = rec.cpu().numpy(), occ.cpu().numpy()
            assert rr.same_records(rec[:n].view(_lib.RAYHIT_DTYPE).reshape(-1), ref[:n]), n
            assert (rec[n:] == 0x5A5A5A5A).all() and (occ[n:] == 0xA5).all(), n
            assert np.array_equal(occ[:n], (ref["instance"][:n] >= 0).astype(np.uint8)), n
            if n:
                assert s.rays_stats() == ((n + 63) // 64, 0, min(3, (n + 63) // 64))
        # one origin -- a point on a surface -- for 130 directions: stride 0, origins of shape (3,)
        k = int(np.flatnonzero(ref["instance"] >= 0)[0])
        shared_o = np.ascontiguousarray(o[k])
        want, _ = ir.closest_hits(a, np.tile(shared_o, (130, 1)), d[:130])
        assert 0 < int((want["instance"] >= 0).sum()) < 130
        assert rr.same_records(s.trace_rays(dev(shared_o), td[:130], inclusive=True).numpy(), want)
        assert s.rays_stats() == (3, 0, 3)
        assert np.array_equal(s.trace_rays(dev(shared_o), td[:130], mode="occluded", inclusive=True).cpu().numpy(), want["instance"] >= 0)
        # the xyz of float4 rows
        o4 = torch.full((N, 4), float("nan"), device="cuda:0"); o4[:, :3] = to
        d4 = torch.full((N, 4), float("nan"), device="cuda:0"); d4[:, :3] = td
        assert o4[:, :3].stride() == (4, 1)
        assert rr.same_records(s.trace_rays(o4[:, :3], d4[:, :3], inclusive=True).numpy(), ref)
        assert np.array_equal(s.trace_rays(o4[:, :3], d4[:, :3], mode="occluded", inclusive=True).cpu().numpy(), ref["instance"] >= 0)


@pytest.mark.parametrize("tlas", ["0", "1"])
def test_origins_beyond_the_cull_range_cost_only_their_chunk(monkeypatch, tlas):
    """tests/test_gpu_trace_rays.py's batch of alternating 64-ray blocks inside and beyond the cull's range, with origins INSIDE instance
    spheres and root boxes in blocks of both kinds: the cull stays on for the near chunks (crt_device.h, sphere_culls: "Inclusive pass")"""
    with session(monkeypatch, _cull_scene(), tlas=tlas) as s:
        a = s.arenas()
        limit = C.c_float()
        _lib.check(s.hip.crt_get_cull_range(None, 0, C.byref(limit), None, None), "crt_get_cull_range")
        limit = float(limit.value)
        assert 1.0 < limit < 1e4
        rng = np.random.RandomState(5)
        blocks = 8
        n = 64 * blocks + 1
        unit = rng.normal(size=(n, 3)); unit /= np.linalg.norm(unit, axis=1, keepdims=True)
        far = (np.arange(n) // 64) % 2 == 1
        centres = np.array([np.linalg.inv(i["inv"].astype(np.float64))[3, :3] for i in a["instances"]])
        target = centres[rng.randint(0, len(centres), n)] + rng.normal(size=(n, 3)) * 0.4
        o = unit * np.where(far, 3.0, 0.5)[:, None] * limit
        d = target - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        # origins inside the instances: the 1e-3 one at the world origin (block 0), the 1e3 one far away (block 1), the unit one (block 2)
        inside = np.zeros(n, bool)
        for block, inst, size in ((0, 0, 2e-4), (1, 2, 200.0), (2, 1, 0.2)):
            rows = np.arange(64 * block + 8, 64 * block + 40)
            o[rows] = centres[inst] + rng.uniform(-1, 1, (len(rows), 3)) * size
            d[rows] = unit[rows]
            inside[rows] = True
        o[-1] = np.nan; d[-1] = (0.0, 0.0, -1.0)
        o, d = o.astype(np.float32), d.astype(np.float32)
        beyond = ~(np.sqrt((o.astype(np.float64) ** 2).sum(axis=1)) <= limit)
        expected = len(set(np.flatnonzero(beyond) // 64))
        assert blocks // 2 + 1 <= expected < blocks + 1
        want, st = ir.closest_hits(a, o, d)
        assert st["capHits"] == 0 and want["instance"][-1] == -1
        assert int((want["instance"][inside] >= 0).sum()) > 20 and int((want["instance"][~inside] >= 0).sum()) > 50
        plain = s.trace_rays(dev(o), dev(d)).numpy()
        plain_stats = s.rays_stats()
        assert plain_stats == (blocks + 1, expected, 3)
        got = s.trace_rays(dev(o), dev(d), inclusive=True)
        assert s.rays_stats() == plain_stats
        assert rr.same_records(got.numpy(), want) and not rr.same_records(plain, want)
        assert np.array_equal(s.trace_rays(dev(o), dev(d), mode="occluded", inclusive=True).cpu().numpy(), want["instance"] >= 0)
        assert s.rays_stats() == plain_stats
        frames = C.c_uint64(7)
        _lib.check(s.hip.crt_get_cull_range(None, 0, None, None, C.byref(frames)), "crt_get_cull_range")
        assert frames.value == 0


def test_no_cross_talk_between_the_modes(monkeypatch):
    a, o, d, ref, plain = reference("cornell-1k")
    with session(monkeypatch, scenes.get("cornell-1k")) as s:
        to, td = dev(o), dev(d)
        before = s.trace_rays(to, td).numpy()
        before_occ = s.trace_rays(to, td, mode="occluded").cpu().numpy()
        inclusive = s.trace_rays(to, td, inclusive=True).numpy()
        inclusive_occ = s.trace_rays(to, td, mode="occluded", inclusive=True).cpu().numpy()
        after = s.trace_rays(to, td).numpy()
        after_occ = s.trace_rays(to, td, mode="occluded").cpu().numpy()
    assert rr.same_records(before, plain) and rr.same_records(after, plain)
    assert np.array_equal(before_occ, plain["instance"] >= 0) and np.array_equal(after_occ, before_occ)
    assert rr.same_records(inclusive, ref) and np.array_equal(inclusive_occ, ref["instance"] >= 0)
    differ = np.zeros(N, bool)
    for k in ("t", "u", "v", "tri", "instance"):
        differ |= bits(np.ascontiguousarray(inclusive[k])) != bits(np.ascontiguousarray(plain[k])) if inclusive[k].dtype == np.float32 else inclusive[k] != plain[k]
    assert differ.sum() >= N // 10 and (inclusive_occ != before_occ).sum() >= N // 10


def composed(s, P, n, par, table, k=None, inclusive=True):
    """ao_ref.compose over Session.trace_rays(mode="occluded", inclusive=...) of ao_ref.rays: the definition, with the session's own answers"""
    P, n = np.ascontiguousarray(P, np.float32).reshape(-1, 3), np.ascontiguousarray(n, np.float32).reshape(-1, 3)
    k = np.arange(len(P), dtype=np.uint32) if k is None else k
    S = par["samples"]
    o, d, w = ao_ref.rays(P, n, k, par, table)
    tmax = np.full(len(P) * S, par["radius"], np.float32)
    occ = s.trace_rays(dev(np.repeat(o, S, axis=0)), dev(d.reshape(-1, 3)), tmax=dev(tmax), mode="occluded", inclusive=inclusive).cpu().numpy()
    return ao_ref.compose(w, occ.reshape(len(P), S)), float(occ.mean())


@pytest.mark.parametrize("tlas", ["0", "1"])
@pytest.mark.parametrize("name", ["tiny", "cornell-1k"])
def test_points_form_is_its_composition(monkeypatch, name, tlas):
    a, P, n, t = ao_reference(name)
    par = params(name, 8)
    kw = {"radius": par["radius"], "bias": par["bias"], "seed": par["seed"]}
    with session(monkeypatch, scenes.get(name), tlas=tlas) as s:
        got = s.trace_ao(dev(P), dev(n), 8, inclusive=True, **kw).cpu().numpy()
        assert s.ao_stats() == (65, 0, 3)
        want, share = composed(s, P, n, par, t)
        plain, plain_share = composed(s, P, n, par, t, inclusive=False)
        print(f"{name}: {share:.4f} of the sample rays occluded under the inclusive rule, {plain_share:.4f} under upstream's")
        assert np.array_equal(bits(got), bits(want)) and share > plain_share
        assert np.array_equal(bits(s.trace_ao(dev(P), dev(n), 8, **kw).cpu().numpy()), bits(plain))      # and the plain form is what it was
        assert not np.array_equal(bits(got), bits(plain))
    assert (got >= 0).all() and (got <= 1).all() and (got[(n == 0).all(axis=1)] == 1).all()


@pytest.mark.parametrize("tlas", ["0", "1"])
def test_frame_form_is_its_composition_and_touches_nothing_else(monkeypatch, tlas):
    name = "cornell-1k"
    sc = scenes.get(name)
    par = params(name, 8)
    t = ao_ref.table()
    kw = {"radius": par["radius"], "bias": par["bias"]}
    with session(monkeypatch, sc, tlas=tlas) as s:
        s.render(gbuffer=True)
        colour, planes, counters = s.read_output(), s.read_gbuffer_raw(), s.counters()
        frames = C.c_uint64(7)
        _lib.check(s.hip.crt_get_cull_range(None, 0, None, None, C.byref(frames)), "crt_get_cull_range")
        no_cull_frames = frames.value
        plain = s.ambient_occlusion(8, **kw).copy()
        got = s.ambient_occlusion(8, inclusive=True, **kw).copy()
        assert s.ao_stats() == (48, 0, 3)
        filtered = s.ambient_occlusion(8, inclusive=True, filter=True, depth_tol=0.05, normal_cos=0.9, **kw).copy()
        assert np.array_equal(bits(s.ambient_occlusion(8, **kw)), bits(plain))                          # the plain form before and after
        # the frame, its planes, the counters and noCullFrames are what they were
        after = s.read_gbuffer_raw()
        assert all(np.array_equal(planes[k].view(np.uint8), after[k].view(np.uint8)) for k in planes)
        assert np.array_equal(bits(colour), bits(s.read_output())) and s.counters() == counters
        _lib.check(s.hip.crt_get_cull_range(None, 0, None, None, C.byref(frames)), "crt_get_cull_range")
        assert frames.value == no_cull_frames
        # the composition on the frame's items
        geometry = s.read_gbuffer()["geometry"]
        s.render_raw(flags=2)                                    # CRT_RENDER_WRITE_RAYS: synchronous, leaves the planes alone
        _, _, pos = s.camera()
        P, n, k = ao_ref.frame_items(s.read_gbuffer(), s.read_rays(), pos)
        want, share = composed(s, P, n, par, t, k)
        assert np.array_equal(bits(got), bits(want.reshape(H, W))) and not np.array_equal(bits(got), bits(plain))
        assert np.array_equal(bits(filtered), bits(ao_ref.filter5x5(got, geometry, 0.05, 0.9))) and not np.array_equal(bits(filtered), bits(got))
        miss = geometry["t"] > np.float32(99998.0)
        assert (got[miss] == 1.0).all() and (got < 1).any()


def test_refusals_launch_nothing(monkeypatch):
    import torch
    a, o, d, ref, plain = reference("tiny")
    _, P, nrm, _ = ao_reference("tiny")
    sc = scenes.get("tiny")
    bad = _lib.CRT_E_BAD_ARGUMENT
    with session(monkeypatch, sc) as s:
        to, td, tp, tn = dev(o), dev(d), dev(P), dev(nrm)
        out = torch.full((N, 5), PATTERN, dtype=torch.int32, device="cuda:0")
        ni = s.h.crth_num_instances()
        good = _lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 3, 3, N)
        pts = _lib.CrtAoPoints(tp.data_ptr(), tn.data_ptr(), 3, 3, N)
        rays_before, ao_before = s.rays_stats(), s.ao_stats()
        assert [s.hip.crt_trace_rays(C.byref(good), ni, mode, out.data_ptr(), None) for mode in (7, 0x102, 0x200)] == [bad] * 3
        inc = _lib.CRT_AO_INCLUSIVE
        for flags in (2, 2 | inc, _lib.CRT_AO_FILTER, _lib.CRT_AO_FILTER | inc, 8 | inc):
            cp = _lib.CrtAoParams(8, RADIUS["tiny"], BIAS, 0, flags, 0.05, 0.9)
            assert s.hip.crt_trace_ao(C.byref(pts), C.byref(cp), ni, out.data_ptr(), None) == bad, flags
        s.render(gbuffer=True)
        for flags in (2, 2 | inc, 8 | inc):
            assert s.hip.crt_frame_ao(C.byref(_lib.CrtAoParams(8, RADIUS["tiny"], BIAS, 0, flags, 0.05, 0.9)), None) == bad, flags
        torch.cuda.synchronize()
        assert s.rays_stats() == rays_before == (0, 0, 0) and s.ao_stats() == ao_before == (0, 0, 0) and (out.cpu().numpy() == PATTERN).all()
        # through the host mirror: reported as Renderer::LastError()
        assert s.h.crth_trace_rays(C.byref(good), 0x102, out.data_ptr(), None) == 0 and s.h.crth_last_error() == bad
        s.h.crth_clear_error()
        assert rr.same_records(s.trace_rays(to, td, inclusive=True).numpy(), ref)      # the session is as usable as before
    with session(monkeypatch, sc, devices=[0, 0]) as s:             # the pointers belong to one GPU
        cp = _lib.CrtAoParams(8, 1.0, BIAS, 0, _lib.CRT_AO_INCLUSIVE, 0.0, 0.0)
        ni = s.h.crth_num_instances()
        for mode in (_lib.CRT_RAYS_INCLUSIVE, _lib.CRT_RAYS_INCLUSIVE | _lib.CRT_RAYS_OCCLUDED):
            assert s.hip.crt_trace_rays(C.byref(good), ni, mode, out.data_ptr(), None) == _lib.CRT_E_UNSUPPORTED
        assert s.hip.crt_trace_ao(C.byref(pts), C.byref(cp), ni, out.data_ptr(), None) == _lib.CRT_E_UNSUPPORTED
        assert s.hip.crt_frame_ao(C.byref(cp), None) == _lib.CRT_E_UNSUPPORTED
        with pytest.raises(_lib.CrtError):
            s.trace_rays(to, td, inclusive=True)
        with pytest.raises(_lib.CrtError):
            s.trace_ao(tp, tn, 8, radius=1.0, bias=BIAS, inclusive=True)
        assert s.rays_stats() == (0, 0, 0) and s.ao_stats() == (0, 0, 0) and (out.cpu().numpy() == PATTERN).all()
