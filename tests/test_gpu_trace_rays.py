"""Ray queries on device buffers (crt_trace_rays / Session.trace_rays) on the GPU: closest-hit records and occlusion bytes for rays given as
torch tensors, against the C oracle's closest-hit records (orc.closest_hits), the session's own counted route (crt_query_hits) and the numpy
restatement of the bounded loop (tests/trace_rays_ref.py). Everything is compared bit for bit; no ray is excluded.
A 64x48 session and CRT_RAYS_GRID=3 unless stated otherwise: three waves walk the 65 chunks of 4099 rays.
Reference: kernel_main.cl:124-160, 189-217, started with besthit.distance = the bound (include/crt_api.h, crt_trace_rays)."""
import ctypes as C
import functools

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import oracle_lib
import trace_rays_ref as rr
from util import bits, rmse, seeded_rays

pytestmark = pytest.mark.gpu
W, H, N = 64, 48, 4099


@functools.lru_cache(maxsize=None)
def reference(name):
    """arenas, the N seeded rays and the oracle's unbounded records of scene `name`: computed once (host-only session), never modified"""
    sc = scenes.get(name)
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
    o, d = seeded_rays(a, sc.camera_pos, N, seed=11)
    ref, _ = oracle_lib.Oracle(a, nthreads=16).closest_hits(o, d)
    for x in (o, d, ref):
        x.setflags(write=False)
    return a, o, d, ref


def session(monkeypatch, sc, grid="3", tlas=None, **kw):
    for k, v in (("CRT_RAYS_GRID", grid), ("CRT_TLAS", tlas)):
        monkeypatch.delenv(k, raising=False)
        if v is not None:
            monkeypatch.setenv(k, v)
    monkeypatch.delenv("CRT_KERNEL", raising=False)
    s = driver.Session(W, H, **({"device": 0} if "devices" not in kw else {}), **kw)
    s.load_scene(sc)
    return s


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")          # (a copy: the shared reference arrays are read-only)


@pytest.mark.parametrize("tlas", ["0", "1"])
@pytest.mark.parametrize("name", ["tiny", "cornell-1k"])
def test_closest_unbounded(monkeypatch, name, tlas):
    a, o, d, ref = reference(name)
    with session(monkeypatch, scenes.get(name), tlas=tlas) as s:
        got = s.trace_rays(dev(o), dev(d)).numpy()
        assert s.rays_stats() == (65, 0, 3)
        assert rr.same_records(got, ref)
        assert rr.same_records(got, s.query_hits(o, d))


def test_sizes_and_sentinels(monkeypatch):
    import torch
    a, o, d, ref = reference("tiny")
    with session(monkeypatch, scenes.get("tiny")) as s:
        to, td = dev(o), dev(d)
        full = s.trace_rays(to, td).numpy()
        assert rr.same_records(full, ref)
        occluded = s.trace_rays(to, td, mode="occluded").cpu().numpy()
        stream = torch.cuda.current_stream().cuda_stream
        for n in (0, 1, 63, 64, 65):
            batch = _lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 3, 3, n)
            rec = torch.full((n + 3, 5), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
            occ = torch.full((n + 3,), 0xA5, dtype=torch.uint8, device="cuda:0")
            _lib.check(s.hip.crt_trace_rays(C.byref(batch), s.h.crth_num_instances(), _lib.CRT_RAYS_CLOSEST, rec.data_ptr(), stream), "crt_trace_rays")
            _lib.check(s.hip.crt_trace_rays(C.byref(batch), s.h.crth_num_instances(), _lib.CRT_RAYS_OCCLUDED, occ.data_ptr(), stream), "crt_trace_rays")
            rec, occ = rec.cpu().numpy(), occ.cpu().numpy()
            assert rr.same_records(rec[:n].view(_lib.RAYHIT_DTYPE).reshape(-1), full[:n]), n
            assert (rec[n:] == 0x5A5A5A5A).all() and (occ[n:] == 0xA5).all(), n
            assert np.array_equal(occ[:n], occluded[:n].astype(np.uint8)), n
            if n:
                assert s.rays_stats() == ((n + 63) // 64, 0, min(3, (n + 63) // 64))
        # a batch of one ray through the session method, every array shared
        one = s.trace_rays(dev(o[0]), dev(d[:1])).numpy()
        assert len(one) == 1 and rr.same_records(one, full[:1])


def test_strides(monkeypatch, nthreads):
    import torch
    a, o, d, ref = reference("tiny")
    half = N // 2                                                # util.seeded_rays: the first half starts at the camera
    assert half == 2049 and (o[:half] == o[0]).all()
    with session(monkeypatch, scenes.get("tiny")) as s:
        to, td = dev(o), dev(d)
        packed = s.trace_rays(to, td).numpy()
        packed_occ = s.trace_rays(to, td, mode="occluded").cpu().numpy()
        assert rr.same_records(packed, ref)
        # A: one origin for the 2049 camera rays, origins of shape (3,)
        shared = s.trace_rays(dev(o[0]), td[:half])
        assert s.rays_stats() == (33, 0, 3)
        assert rr.same_records(shared.numpy(), packed[:half])
        assert np.array_equal(s.trace_rays(dev(o[0]), td[:half], mode="occluded").cpu().numpy(), packed_occ[:half])
        # B: the xyz of float4 rows
        o4 = torch.full((N, 4), float("nan"), device="cuda:0"); o4[:, :3] = to
        d4 = torch.full((N, 4), float("nan"), device="cuda:0"); d4[:, :3] = td
        assert o4[:, :3].stride() == (4, 1)
        assert rr.same_records(s.trace_rays(o4[:, :3], d4[:, :3]).numpy(), packed)
        assert np.array_equal(s.trace_rays(o4[:, :3], d4[:, :3], mode="occluded").cpu().numpy(), packed_occ)
        # C: one direction for every ray (sun visibility from many points)
        sun = np.ascontiguousarray(d[3])
        tiled = np.tile(sun, (N, 1))
        want, _ = oracle_lib.Oracle(a, nthreads=nthreads).closest_hits(o, tiled)
        got = s.trace_rays(to, dev(sun)).numpy()
        assert rr.same_records(got, want) and rr.same_records(got, s.trace_rays(to, dev(tiled)).numpy())
        assert 0 < int((want["instance"] >= 0).sum()) < N
        assert np.array_equal(s.trace_rays(to, dev(sun), mode="occluded").cpu().numpy(), want["instance"] >= 0)


@pytest.mark.parametrize("name", ["tiny", "cornell-1k"])
def test_bounded_closest_and_occlusion(monkeypatch, name):
    a, o, d, ref = reference(name)
    hits = ref["instance"] >= 0
    assert int(hits.sum()) >= 3800 and not any(np.isnan(ref[k]).any() for k in ("t", "u", "v"))      # the filter's precondition (include/crt_api.h)
    with session(monkeypatch, scenes.get(name)) as s:
        to, td = dev(o), dev(d)
        assert np.array_equal(s.trace_rays(to, td, mode="occluded").cpu().numpy(), hits)
        assert s.rays_stats() == (65, 0, 3)
        for fam, (tmax, kept) in rr.tmax_families(ref).items():
            want = rr.filtered(ref, tmax)
            assert np.array_equal(want["instance"] >= 0, hits if kept else np.zeros_like(hits)), fam
            assert rr.same_records(rr.bounded_closest_hits(a, o, d, tmax), want), fam
            tt = dev(tmax)
            assert rr.same_records(s.trace_rays(to, td, tmax=tt).numpy(), want), fam
            assert np.array_equal(s.trace_rays(to, td, tmax=tt, mode="occluded").cpu().numpy(), want["instance"] >= 0), fam
        # an infinite bound is no bound
        inf = dev(np.full(N, np.inf, np.float32))
        assert rr.same_records(s.trace_rays(to, td, tmax=inf).numpy(), ref)


def _cull_scene():
    """tiny's meshes at scales 1e-3, 1 and 1e3 (the transforms of "scales-1e-3-to-1e3" in tests/test_gpu_cull_bound.py): the 1e-3 instance may be
    culled for origins up to ~40 units only, which is the scene's limit"""
    m = scenes._trs(1.0, (0.3, 0.5, 1.0), 0.4, (0, 0, 0)).astype(np.float64)
    m[:3, :3] = np.diag([1.0, 30.0, 0.2]) @ m[:3, :3]
    m[3, :3] = (100.0, 0.0, 0.0)
    inst = [scenes.Instance(0, 0xFFFF, scenes._trs(1e-3, (0.2, 1.0, 0.1), 0.7, (0.01, 0.02, -0.03))),
            scenes.Instance(1, 0xFFFF, scenes._trs(1.0, (1.0, 0.3, 0.2), 1.9, (20.0, 5.0, -30.0))),
            scenes.Instance(0, 0xFFFF, scenes._trs(1e3, (0.1, 0.2, 1.0), 2.6, (5e4, 1e4, -8e4))),
            scenes.Instance(1, 0xFFFF, m.astype(np.float32))]
    base = scenes.get("tiny")
    return scenes.Scene("rays-cull", base.dir, base.skybox, base.meshes, inst, (0.0, 2.0, 30.0), (0.0, 0.0, -1.0))


@pytest.mark.parametrize("tlas", ["0", "1"])
def test_origins_beyond_the_cull_range_cost_only_their_chunk(monkeypatch, nthreads, tlas):
    with session(monkeypatch, _cull_scene(), tlas=tlas) as s:
        a = s.arenas()
        limit = C.c_float()
        _lib.check(s.hip.crt_get_cull_range(None, 0, C.byref(limit), None, None), "crt_get_cull_range")
        limit = float(limit.value)
        assert 1.0 < limit < 1e4
        rng = np.random.RandomState(5)
        blocks = 8
        n = 64 * blocks + 1
        # origins on spheres of 0.5 x and 3 x the limit, in alternating 64-ray blocks; directions towards the instances, so that rays hit
        unit = rng.normal(size=(n, 3)); unit /= np.linalg.norm(unit, axis=1, keepdims=True)
        far = (np.arange(n) // 64) % 2 == 1
        centres = np.array([np.linalg.inv(i["inv"].astype(np.float64))[3, :3] for i in a["instances"]])
        target = centres[rng.randint(0, len(centres), n)] + rng.normal(size=(n, 3)) * 0.4
        orc = oracle_lib.Oracle(a, nthreads=nthreads)

        def batch(scale_far, last):
            o = unit * np.where(far, scale_far, 0.5)[:, None] * limit
            o[-1] = last
            d = target - o
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            d[-1] = (0.0, 0.0, -1.0)
            return o.astype(np.float32), d.astype(np.float32)

        o, d = batch(3.0, np.nan)
        want, _ = orc.closest_hits(o, d)
        assert int((want["instance"] >= 0).sum()) > 50 and want["instance"][-1] == -1
        got = s.trace_rays(dev(o), dev(d))
        chunks, no_cull, groups = s.rays_stats()
        assert (chunks, groups) == (blocks + 1, 3) and no_cull == blocks // 2 + 1 and 0 < no_cull < chunks
        assert rr.same_records(got.numpy(), want)
        assert np.array_equal(s.trace_rays(dev(o), dev(d), mode="occluded").cpu().numpy(), want["instance"] >= 0)
        # every origin inside the limit: every chunk keeps the cull
        o, d = batch(0.5, (0.0, 0.0, 0.25 * limit))
        assert np.linalg.norm(o.astype(np.float64), axis=1).max() < limit
        want, _ = orc.closest_hits(o, d)
        got = s.trace_rays(dev(o), dev(d))
        assert s.rays_stats() == (blocks + 1, 0, 3)
        assert rr.same_records(got.numpy(), want)
        # no frame counter moved: the launches without the cull that crt_get_cull_range counts are frames and crt_query_hits
        frames = C.c_uint64(7)
        _lib.check(s.hip.crt_get_cull_range(None, 0, None, None, C.byref(frames)), "crt_get_cull_range")
        assert frames.value == 0


def test_queries_frames_and_instance_uploads_stay_ordered(monkeypatch, nthreads):
    """Queries on two streams, frames in flight and instance uploads in between: every query sees the instance table it was submitted under."""
    import torch
    a0, o, d, ref0 = reference("tiny")
    sc = scenes.get("tiny")
    moves = [np.array([3.0, 1.5, -2.0], np.float32), np.array([-2.5, 0.5, 1.0], np.float32)]
    with session(monkeypatch, sc) as s:
        to, td = dev(o), dev(d)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        results, oracles = [], [oracle_lib.Oracle(s.arenas(), nthreads=nthreads)]
        with torch.cuda.stream(s1):
            results.append(s.trace_rays(to, td))
        for k, (pos, stream) in enumerate(zip(moves, (s2, s1))):
            s.h.crth_set_mesh_position(0, pos.ctypes.data_as(C.POINTER(C.c_float)))
            s.render(pipelined=True)                              # uploads the table, then a frame in flight
            oracles.append(oracle_lib.Oracle(s.arenas(), nthreads=nthreads))
            with torch.cuda.stream(stream):
                results.append(s.trace_rays(to, td))
        torch.cuda.synchronize()
        wants = [orc.closest_hits(o, d)[0] for orc in oracles]
        assert rr.same_records(wants[0], ref0)
        assert not rr.same_records(wants[0], wants[1]) and not rr.same_records(wants[1], wants[2])      # the moves matter to these rays
        for k, (got, want) in enumerate(zip(results, wants)):
            assert rr.same_records(got.numpy(), want), k
        frame = s.output()
    with session(monkeypatch, sc) as s:                           # a fresh session in the same state
        s.h.crth_set_mesh_position(0, moves[-1].ctypes.data_as(C.POINTER(C.c_float)))
        s.render()
        assert np.array_equal(bits(s.output()), bits(frame))


def test_full_grid(monkeypatch, nthreads):
    a, _, _, _ = reference("tiny")
    sc = scenes.get("tiny")
    parts = [seeded_rays(a, sc.camera_pos, 40000, seed=k) for k in range(11, 16)]
    o, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert len(o) == 200000
    want, _ = oracle_lib.Oracle(a, nthreads=nthreads).closest_hits(o, d)
    with session(monkeypatch, sc, grid=None) as s:
        got = s.trace_rays(dev(o), dev(d))
        chunks, no_cull, groups = s.rays_stats()
        assert chunks == 3125 and no_cull == 0 and 3 < groups <= chunks
        assert rr.same_records(got.numpy(), want)
        assert np.array_equal(s.trace_rays(dev(o), dev(d), mode="occluded").cpu().numpy(), want["instance"] >= 0)


def test_refusals_launch_nothing(monkeypatch, nthreads):
    import torch
    a, o, d, ref = reference("tiny")
    sc = scenes.get("tiny")
    with session(monkeypatch, sc) as s:
        to, td = dev(o), dev(d)
        out = torch.full((N, 5), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        ni = s.h.crth_num_instances()

        def call(batch, mode=_lib.CRT_RAYS_CLOSEST, dst=out.data_ptr(), instances=ni):
            return s.hip.crt_trace_rays(C.byref(batch) if batch is not None else None, instances, mode, dst, None)

        good = _lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 3, 3, N)
        assert call(good, mode=7) == _lib.CRT_E_BAD_ARGUMENT
        assert call(_lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 2, 3, N)) == _lib.CRT_E_BAD_ARGUMENT
        assert call(_lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 3, 1, N)) == _lib.CRT_E_BAD_ARGUMENT
        assert call(good, dst=None) == _lib.CRT_E_BAD_ARGUMENT
        assert call(None) == _lib.CRT_E_BAD_ARGUMENT
        assert call(_lib.CrtRayBatch(None, td.data_ptr(), None, 3, 3, N)) == _lib.CRT_E_BAD_ARGUMENT
        assert call(_lib.CrtRayBatch(to.data_ptr(), None, None, 3, 3, N)) == _lib.CRT_E_BAD_ARGUMENT
        assert call(good, instances=402) == _lib.CRT_E_BAD_ARGUMENT
        assert call(_lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 3, 3, (1 << 30) + 1)) == _lib.CRT_E_OUT_OF_RANGE
        assert call(_lib.CrtRayBatch(None, None, None, 1, 1, 0), dst=None) == _lib.CRT_OK           # n == 0: nothing is looked at
        torch.cuda.synchronize()
        assert s.rays_stats() == (0, 0, 0) and (out.cpu().numpy() == 0x5A5A5A5A).all()
        # through the host mirror: reported as Renderer::LastError()
        assert s.h.crth_trace_rays(C.byref(good), 7, out.data_ptr(), None) == 0 and s.h.crth_last_error() == _lib.CRT_E_BAD_ARGUMENT
        s.h.crth_clear_error()
        assert s.h.crth_last_error() == 0
        assert rr.same_records(s.trace_rays(to, td).numpy(), ref)    # the session is as usable as before
    with session(monkeypatch, sc, devices=[0, 0]) as s:             # the pointers belong to one GPU
        assert s.hip.crt_trace_rays(C.byref(good), s.h.crth_num_instances(), _lib.CRT_RAYS_CLOSEST, out.data_ptr(), None) == _lib.CRT_E_UNSUPPORTED
        with pytest.raises(_lib.CrtError):
            s.trace_rays(to, td)
        assert s.rays_stats() == (0, 0, 0) and (out.cpu().numpy() == 0x5A5A5A5A).all()
        s.render()
        iv, ip, pos = s.camera()
        orc = oracle_lib.Oracle(s.arenas(), nthreads=nthreads)
        want, _ = orc.trace(orc.raygen(W, H, iv, ip), pos, sc.sun_angle)
        assert rmse(s.output(), want) < 1e-4
