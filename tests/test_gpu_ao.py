"""Ambient occlusion on the GPU (crt_trace_ao / crt_frame_ao, Session.trace_ao / ambient_occlusion): the fused kernel against its own
composition -- tests/ao_ref.py's sample rays answered by Session.trace_rays(mode="occluded") or by the C oracle's records, reduced in numpy.
Everything is compared bit for bit; no point and no pixel is excluded.
A 64x48 session and CRT_RAYS_GRID=3 unless stated otherwise: three waves walk the 65 chunks of 4099 points, the 48 tiles of a frame.
Definition: include/crt_api.h (crt_trace_ao)."""
import ctypes as C
import functools

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import ao_ref
import gbuffer_ref
import oracle_lib
from test_gpu_trace_rays import _cull_scene
from util import bits, seeded_rays

pytestmark = pytest.mark.gpu
W, H, N = 64, 48, 4099
BIAS = 1e-3
# The radius per scene: by the oracle, between 10 % and 90 % of the sample rays of the 4099 points are occluded (asserted below). Upstream's
# slab test never enters a box the ray starts in (kernel_main.cl:115, tnear > 0), so a ray from a surface mostly finds OTHER meshes and the
# far side of its own: the shares are low and need a radius of the scene's size (measured on the CPU: tiny 0.125 at 16, cornell-1k 0.209 at 4).
RADIUS = {"tiny": 16.0, "cornell-1k": 4.0}
PATTERN = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def reference(name):
    """arenas, the 4099 points (the oracle's hit points of util.seeded_rays; a miss: the camera position with a zero normal), their normals
    (gbuffer_ref.planes_from_records) and the direction table: computed once, never modified"""
    sc = scenes.get(name)
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
    o, d = seeded_rays(a, sc.camera_pos, N, seed=11)
    rec, _ = oracle_lib.Oracle(a, nthreads=16).closest_hits(o, d)
    geometry, _, _ = gbuffer_ref.planes_from_records(a, rec)
    hit = (rec["instance"] >= 0) & ~(rec["t"] > gbuffer_ref.INF_MINUS_ONE)
    P = (o + d * rec["t"][:, None]).astype(np.float32)
    n = np.ascontiguousarray(geometry["normal"], np.float32).copy()
    P[~hit] = np.asarray(sc.camera_pos, np.float32)
    n[~hit] = 0.0
    assert 3800 <= int(hit.sum()) < N and not np.isnan(n).any()
    t = ao_ref.table()
    for x in (P, n, t):
        x.setflags(write=False)
    return a, P, n, t


@functools.lru_cache(maxsize=None)
def oracle_composition(name, samples):
    """(ao, share of occluded sample rays among the points that trace) by ao_ref.compose over the oracle's unbounded records filtered by t < R"""
    a, P, n, t = reference(name)
    o, d, w = ao_ref.rays(P, n, np.arange(N, dtype=np.uint32), params(name, samples), t)
    rec, _ = oracle_lib.Oracle(a, nthreads=16).closest_hits(np.repeat(o, samples, axis=0), d.reshape(-1, 3))
    assert np.isfinite(rec["u"]).all() and np.isfinite(rec["v"]).all()           # the filter's precondition (include/crt_api.h): nothing is excluded
    occ = ((rec["instance"] >= 0) & (rec["t"] < np.float32(RADIUS[name]))).reshape(N, samples)
    traces = (n != 0).any(axis=1)
    ao = ao_ref.compose(w, occ)
    ao.setflags(write=False)
    return ao, float(occ[traces].mean())


def params(name, samples, seed=0):
    return {"samples": samples, "radius": RADIUS[name], "bias": BIAS, "seed": seed}


def session(monkeypatch, sc, grid="3", tlas=None, w=W, h=H, **kw):
    for k, v in (("CRT_RAYS_GRID", grid), ("CRT_TLAS", tlas)):
        monkeypatch.delenv(k, raising=False)
        if v is not None:
            monkeypatch.setenv(k, v)
    monkeypatch.delenv("CRT_KERNEL", raising=False)
    s = driver.Session(w, h, **({"device": 0} if "devices" not in kw else {}), **kw)
    s.load_scene(sc)
    return s


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")          # (a copy: the shared reference arrays are read-only)


def composed(s, P, n, par, table, k=None):
    """ao_ref.compose over Session.trace_rays(mode="occluded") of ao_ref.rays: the definition, with the session's own occlusion answers"""
    P, n = np.ascontiguousarray(P, np.float32).reshape(-1, 3), np.ascontiguousarray(n, np.float32).reshape(-1, 3)
    k = np.arange(len(P), dtype=np.uint32) if k is None else k
    S = par["samples"]
    o, d, w = ao_ref.rays(P, n, k, par, table)
    tmax = np.full(len(P) * S, par["radius"], np.float32)
    occ = s.trace_rays(dev(np.repeat(o, S, axis=0)), dev(d.reshape(-1, 3)), tmax=dev(tmax), mode="occluded").cpu().numpy()
    return ao_ref.compose(w, occ.reshape(len(P), S))


def ao_of(s, P, n, par):
    return s.trace_ao(dev(P), dev(n), par["samples"], radius=par["radius"], bias=par["bias"], seed=par["seed"]).cpu().numpy()


@pytest.mark.parametrize("tlas", ["0", "1"])
@pytest.mark.parametrize("samples", [1, 8, 64])
@pytest.mark.parametrize("name", ["tiny", "cornell-1k"])
def test_points_form_is_its_composition(monkeypatch, name, samples, tlas):
    a, P, n, t = reference(name)
    par = params(name, samples)
    want, share = oracle_composition(name, samples)
    print(f"{name}, N = {samples}: {share:.4f} of the sample rays occluded")
    assert 0.10 <= share <= 0.90
    with session(monkeypatch, scenes.get(name), tlas=tlas) as s:
        got = ao_of(s, P, n, par)
        assert s.ao_stats() == (65, 0, 3)
        assert np.array_equal(bits(got), bits(composed(s, P, n, par, t)))
        assert np.array_equal(bits(got), bits(want))
        assert s.rays_stats()[0] == (N * samples + 63) // 64                     # the ray queries' statistics are their own
        assert s.ao_stats() == (65, 0, 3)
    assert (got >= 0).all() and (got <= 1).all() and (got[(n == 0).all(axis=1)] == 1).all() and (got < 1).any()


def test_sizes_and_sentinels(monkeypatch):
    import torch
    a, P, n, t = reference("tiny")
    par = params("tiny", 8)
    with session(monkeypatch, scenes.get("tiny")) as s:
        tp, tn = dev(P), dev(n)
        full = ao_of(s, P, n, par)
        assert np.array_equal(bits(full), bits(oracle_composition("tiny", 8)[0]))
        stream = torch.cuda.current_stream().cuda_stream
        cp = _lib.CrtAoParams(8, par["radius"], par["bias"], 0, 0, 0.0, 0.0)
        for m in (0, 1, 63, 64, 65):
            out = torch.full((m + 3,), PATTERN, dtype=torch.int32, device="cuda:0")
            pts = _lib.CrtAoPoints(tp.data_ptr(), tn.data_ptr(), 3, 3, m)
            _lib.check(s.hip.crt_trace_ao(C.byref(pts), C.byref(cp), s.h.crth_num_instances(), out.data_ptr(), stream), "crt_trace_ao")
            got = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:m], bits(full[:m])), m
            assert (got[m:] == PATTERN).all(), m
            if m:
                assert s.ao_stats() == ((m + 63) // 64, 0, min(3, (m + 63) // 64))
        # n == 0 looks at no pointer
        assert s.hip.crt_trace_ao(C.byref(_lib.CrtAoPoints(None, None, 1, 1, 0)), C.byref(cp), 1, None, None) == _lib.CRT_OK
        # one point through the session method, both arrays shared
        one = s.trace_ao(dev(P[0]), dev(n[:1]), 8, radius=par["radius"], bias=par["bias"]).cpu().numpy()
        assert one.shape == (1,) and np.array_equal(bits(one), bits(full[:1]))


def test_strides(monkeypatch):
    import torch
    a, P, n, t = reference("tiny")
    par = params("tiny", 8)
    with session(monkeypatch, scenes.get("tiny")) as s:
        tp, tn = dev(P), dev(n)
        packed = ao_of(s, P, n, par)
        # the xyz of float4 rows
        p4 = torch.full((N, 4), float("nan"), device="cuda:0"); p4[:, :3] = tp
        n4 = torch.full((N, 4), float("nan"), device="cuda:0"); n4[:, :3] = tn
        assert p4[:, :3].stride() == (4, 1)
        got = s.trace_ao(p4[:, :3], n4[:, :3], 8, radius=par["radius"], bias=par["bias"]).cpu().numpy()
        assert np.array_equal(bits(got), bits(packed))
        # one normal for every point (stride 0) is the packed call with that normal repeated
        up = np.ascontiguousarray(n[(n != 0).any(axis=1)][0])
        shared = s.trace_ao(tp, dev(up), 8, radius=par["radius"], bias=par["bias"]).cpu().numpy()
        assert s.ao_stats() == (65, 0, 3)
        tiled = ao_of(s, P, np.tile(up, (N, 1)), par)
        assert np.array_equal(bits(shared), bits(tiled)) and not np.array_equal(bits(shared), bits(packed))
        assert np.array_equal(bits(shared), bits(composed(s, P, np.tile(up, (N, 1)), par, t)))


def test_degenerate_inputs_and_refusals(monkeypatch):
    import torch
    a, P, n, t = reference("tiny")
    par = params("tiny", 8)
    sc = scenes.get("tiny")
    with session(monkeypatch, sc) as s:
        # zero normals: exactly 1.0, whatever the position
        m = 130
        got = ao_of(s, P[:m], np.zeros((m, 3), np.float32), par)
        assert np.array_equal(bits(got), bits(np.ones(m, np.float32)))
        # NaN normals, NaN positions, a NaN component of either: the numpy restatement's bits, and nothing faults
        Pn, nn = P[:m].copy(), n[:m].copy()
        nn[0::5] = np.nan; Pn[1::5] = np.nan; nn[2::5, 1] = np.nan; Pn[3::5, 2] = np.nan
        got = ao_of(s, Pn, nn, par)
        torch.cuda.synchronize()
        assert np.array_equal(bits(got), bits(composed(s, Pn, nn, par, t)))
        assert np.array_equal(bits(got[4::5]), bits(ao_of(s, P[:m], n[:m], par)[4::5]))        # the untouched points are not affected
        # argument errors: the code, nothing launched, `out` untouched
        tp, tn = dev(P), dev(n)
        out = torch.full((N,), PATTERN, dtype=torch.int32, device="cuda:0")
        ni = s.h.crth_num_instances()
        before = s.ao_stats()

        def call(samples=8, radius=par["radius"], bias=BIAS, flags=0, pos=tp.data_ptr(), nrm=tn.data_ptr(), sp=3, sn=3, count=N, dst=out.data_ptr(), instances=ni):
            pts = _lib.CrtAoPoints(pos, nrm, sp, sn, count)
            cp = _lib.CrtAoParams(samples, radius, bias, 0, flags, 0.05, 0.9)
            return s.hip.crt_trace_ao(C.byref(pts), C.byref(cp), instances, dst, None)

        bad = _lib.CRT_E_BAD_ARGUMENT
        assert [call(samples=k) for k in (0, 3, 128)] == [bad] * 3
        assert [call(radius=r) for r in (0.0, -1.0, float("nan"))] == [bad] * 3
        assert [call(bias=b) for b in (float("inf"), float("nan"))] == [bad] * 2
        assert call(pos=None) == bad and call(nrm=None) == bad and call(dst=None) == bad
        assert call(sp=1) == bad and call(sn=2) == bad
        assert call(flags=2) == bad and call(flags=_lib.CRT_AO_FILTER) == bad
        assert call(instances=402) == bad
        assert call(count=(1 << 30) + 1) == _lib.CRT_E_OUT_OF_RANGE
        assert s.hip.crt_trace_ao(None, None, ni, out.data_ptr(), None) == bad
        torch.cuda.synchronize()
        assert s.ao_stats() == before and (out.cpu().numpy() == PATTERN).all()
        # through the host mirror: reported as Renderer::LastError()
        pts, cp = _lib.CrtAoPoints(tp.data_ptr(), tn.data_ptr(), 3, 3, N), _lib.CrtAoParams(3, 1.0, BIAS, 0, 0, 0.0, 0.0)
        assert s.h.crth_trace_ao(C.byref(pts), C.byref(cp), out.data_ptr(), None) == 0 and s.h.crth_last_error() == bad
        s.h.crth_clear_error()
        assert call() == _lib.CRT_OK                             # the session is as usable as before
        assert np.array_equal(out.cpu().numpy().view(np.uint32), bits(oracle_composition("tiny", 8)[0]))
    good_pts, good_cp = _lib.CrtAoPoints(tp.data_ptr(), tn.data_ptr(), 3, 3, N), _lib.CrtAoParams(8, 1.0, BIAS, 0, 0, 0.0, 0.0)
    out = torch.full((N,), PATTERN, dtype=torch.int32, device="cuda:0")
    with session(monkeypatch, sc, devices=[0, 0]) as s:             # the pointers belong to one GPU
        assert s.hip.crt_trace_ao(C.byref(good_pts), C.byref(good_cp), s.h.crth_num_instances(), out.data_ptr(), None) == _lib.CRT_E_UNSUPPORTED
        assert s.hip.crt_frame_ao(C.byref(good_cp), None) == _lib.CRT_E_UNSUPPORTED
        with pytest.raises(_lib.CrtError):
            s.trace_ao(tp, tn, 8, radius=1.0, bias=BIAS)
        assert s.ao_stats() == (0, 0, 0) and (out.cpu().numpy() == PATTERN).all()


@pytest.mark.parametrize("tlas", ["0", "1"])
def test_origins_beyond_the_cull_range_cost_only_their_chunk(monkeypatch, tlas):
    with session(monkeypatch, _cull_scene(), tlas=tlas) as s:
        a = s.arenas()
        limit = C.c_float()
        _lib.check(s.hip.crt_get_cull_range(None, 0, C.byref(limit), None, None), "crt_get_cull_range")
        limit = float(limit.value)
        assert 0.1 < limit < 90.0
        rng = np.random.RandomState(5)
        blocks = 8
        m = 64 * blocks + 1
        # alternating 64-point blocks: points 0.003 from the 1e-3 instance at the world origin (inside the limit) and points 3 from the instance
        # at x = 100 (beyond it), each looking at its instance, so that samples hit
        unit = rng.normal(size=(m, 3)); unit[:, 1] *= 0.2; unit /= np.linalg.norm(unit, axis=1, keepdims=True)
        far = (np.arange(m) // 64) % 2 == 1
        centres = np.array([np.linalg.inv(i["inv"].astype(np.float64))[3, :3] for i in a["instances"]])
        assert np.linalg.norm(centres[0]) < 0.05 and 99.0 < np.linalg.norm(centres[3]) < 101.0
        P = np.where(far[:, None], centres[3] + unit * 3.0, centres[0] + unit * 3e-3).astype(np.float32)
        nrm = (-unit).astype(np.float32)
        P[-1] = np.nan                                           # a NaN origin is beyond every range
        nrm[64:70] = 0.0                                         # points that trace nothing do not decide: block 1 still holds 58 far points that do,
        nrm[192:256] = 0.0                                       # block 3 none -- an idle chunk stores its ones and keeps out of the count
        par = {"samples": 8, "radius": 1e9, "bias": 0.0, "seed": 3}
        t = ao_ref.table()
        o, _, _ = ao_ref.rays(P, nrm, np.arange(m, dtype=np.uint32), par, t)
        beyond = ~(np.sqrt((o.astype(np.float64) ** 2).sum(axis=1)) <= limit) & (nrm != 0).any(axis=1)
        expected = len(set(np.flatnonzero(beyond) // 64))
        assert expected == 4                                     # blocks 1, 5, 7 and the NaN point's chunk
        got = ao_of(s, P, nrm, par)
        assert s.ao_stats() == (blocks + 1, expected, 3)
        want = composed(s, P, nrm, par, t)
        assert np.array_equal(bits(got), bits(want))
        assert (want[far] < 1).sum() > 100 and (want[~far] < 1).sum() > 100 and (got[192:256] == 1.0).all()
        # every origin inside the limit: every chunk keeps the cull
        P2 = (centres[0] + unit * 3e-3).astype(np.float32)
        got = ao_of(s, P2, nrm, par)
        assert s.ao_stats() == (blocks + 1, 0, 3)
        assert np.array_equal(bits(got), bits(composed(s, P2, nrm, par, t)))
        frames = C.c_uint64(7)
        _lib.check(s.hip.crt_get_cull_range(None, 0, None, None, C.byref(frames)), "crt_get_cull_range")
        assert frames.value == 0                                 # noCullFrames counts frames and crt_query_hits


def frame_reference(s, par, t):
    """trace_ao on the items of the session's last G-buffer frame; the frame's rays come from a WRITE_RAYS frame with the same camera"""
    planes = s.read_gbuffer()
    s.render_raw(flags=2)                                        # CRT_RENDER_WRITE_RAYS: synchronous, leaves the planes alone
    rays = s.read_rays()
    _, _, pos = s.camera()
    P, n, k = ao_ref.frame_items(planes, rays, pos)
    miss = planes["geometry"]["t"] > np.float32(99998.0)
    return ao_of(s, P, n, par).reshape(s.height, s.width), miss, (P, n)


@pytest.mark.parametrize("name", ["tiny", "cornell-1k"])
def test_frame_form_is_the_points_form_on_the_frames_items(monkeypatch, name):
    sc = scenes.get(name)
    par = params(name, 8)
    t = ao_ref.table()
    kw = {"radius": par["radius"], "bias": par["bias"]}
    with session(monkeypatch, sc) as s:
        s.render(gbuffer=True)
        colour, planes = s.read_output(), s.read_gbuffer_raw()
        got = s.ambient_occlusion(8, **kw)
        assert s.ao_stats() == (48, 0, 3)
        # the frame and its planes are read, not written
        after = s.read_gbuffer_raw()
        assert all(np.array_equal(planes[k].view(np.uint8), after[k].view(np.uint8)) for k in planes)
        assert np.array_equal(bits(colour), bits(s.read_output()))
        want, miss, (P, n) = frame_reference(s, par, t)
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(got), bits(composed(s, P, n, par, t).reshape(H, W)))
        assert (got[miss] == 1.0).all() and (got < 1).any()
        # through the C-ABI: the plane on the device is the plane that is read
        raw = np.empty((H, W), np.float32)
        _lib.check(s.hip.crt_read_ao(raw.ctypes.data, raw.size), "crt_read_ao")
        assert np.array_equal(bits(raw), bits(got)) and s.hip.crt_ao_device_ptr()
        assert s.hip.crt_read_ao(raw.ctypes.data, raw.size - 1) == _lib.CRT_E_BAD_ARGUMENT
        # three pipelined G-buffer frames with different cameras: AO belongs to the last one
        for front in ((0.2, -0.1, -1.0), (-0.3, 0.0, -1.0), (0.1, 0.05, -1.0)):
            s.set_camera(sc.camera_pos, front)
            s.render(gbuffer=True, pipelined=True)
        last = s.ambient_occlusion(8, **kw)
        want, miss, _ = frame_reference(s, par, t)
        assert np.array_equal(bits(last), bits(want)) and not np.array_equal(bits(last), bits(got))
        # an instance upload: the next frame and its AO see the new table
        pos = np.array([0.4, 0.3, -0.2], np.float32)
        s.h.crth_set_mesh_position(0, pos.ctypes.data_as(C.POINTER(C.c_float)))
        s.render(gbuffer=True)
        moved = s.ambient_occlusion(8, **kw)
        want, miss, (P, n) = frame_reference(s, par, t)
        assert np.array_equal(bits(moved), bits(want)) and not np.array_equal(bits(moved), bits(last))
        assert np.array_equal(bits(moved), bits(composed(s, P, n, par, t).reshape(H, W)))


@pytest.mark.parametrize("w,h", [(64, 48), (70, 50)])
def test_filter(monkeypatch, w, h):
    par = params("cornell-1k", 8)
    kw = {"radius": par["radius"], "bias": par["bias"]}
    with session(monkeypatch, scenes.get("cornell-1k"), w=w, h=h) as s:
        s.render(gbuffer=True)
        raw = s.ambient_occlusion(8, **kw)
        assert s.ao_stats() == (((w + 7) // 8) * ((h + 7) // 8), 0, 3)
        geometry = s.read_gbuffer()["geometry"]
        for tol, cos in ((0.05, 0.9), (1e-3, 0.999), (10.0, -1.0)):
            got = s.ambient_occlusion(8, filter=True, depth_tol=tol, normal_cos=cos, **kw)
            want = ao_ref.filter5x5(raw, geometry, tol, cos)
            assert np.array_equal(bits(got), bits(want)), (tol, cos)
            assert not np.array_equal(bits(got), bits(raw))
        assert np.array_equal(bits(s.ambient_occlusion(8, **kw)), bits(raw))                     # and the unfiltered plane again


def test_refusals_without_a_gbuffer_frame(monkeypatch):
    par = params("tiny", 8)
    kw = {"radius": par["radius"], "bias": par["bias"]}
    cp = _lib.CrtAoParams(8, par["radius"], BIAS, 0, 0, 0.0, 0.0)
    buf = np.zeros((H, W), np.float32)
    bad = _lib.CRT_E_BAD_ARGUMENT
    with session(monkeypatch, scenes.get("tiny")) as s:
        def refused():
            return (s.hip.crt_frame_ao(C.byref(cp), None), s.hip.crt_read_ao(buf.ctypes.data, buf.size), s.hip.crt_ao_device_ptr()) == (bad, bad, None)
        assert refused()
        s.render()                                               # a frame without the planes changes nothing
        assert refused()
        with pytest.raises(_lib.CrtError):
            s.ambient_occlusion(8, **kw)
        assert s.h.crth_last_error() == 0
        s.render(gbuffer=True)
        assert s.hip.crt_read_ao(buf.ctypes.data, buf.size) == bad and s.hip.crt_ao_device_ptr() is None      # no crt_frame_ao yet
        assert [s.hip.crt_frame_ao(C.byref(_lib.CrtAoParams(k, 1.0, BIAS, 0, 0, 0.0, 0.0)), None) for k in (0, 3, 128)] == [bad] * 3
        assert s.hip.crt_frame_ao(C.byref(_lib.CrtAoParams(8, 1.0, BIAS, 0, 2, 0.0, 0.0)), None) == bad           # an unknown flag
        assert s.hip.crt_frame_ao(None, None) == bad and s.ao_stats() == (0, 0, 0)
        first = s.ambient_occlusion(8, **kw)
        s.resize(80, 48)                                         # a resize that changes the frame: the planes are gone
        buf = np.zeros((48, 80), np.float32)
        assert refused()
        s.render(gbuffer=True)
        assert s.ambient_occlusion(8, **kw).shape == (48, 80)
        s.resize(W, H)
        buf = np.zeros((H, W), np.float32)
        assert refused()
        s.render(gbuffer=True)
        assert np.array_equal(bits(s.ambient_occlusion(8, **kw)), bits(first))


def test_determinism_and_seeds(monkeypatch):
    par = params("tiny", 8)
    kw = {"radius": par["radius"], "bias": par["bias"]}
    with session(monkeypatch, scenes.get("tiny")) as s:
        s.render(gbuffer=True)
        miss = s.read_gbuffer()["geometry"]["t"] > np.float32(99998.0)
        one, two = s.ambient_occlusion(8, **kw), s.ambient_occlusion(8, **kw)
        other = s.ambient_occlusion(8, seed=7, **kw)
        assert np.array_equal(bits(one), bits(two))
        assert not np.array_equal(bits(one), bits(other))
        assert 0 < int(miss.sum()) < W * H and (one[miss] == 1.0).all() and (other[miss] == 1.0).all()


def test_row_bands_write_only_the_owned_rows(monkeypatch):
    par = params("tiny", 8)
    kw = {"radius": par["radius"], "bias": par["bias"]}
    with session(monkeypatch, scenes.get("tiny")) as s:
        s.render(gbuffer=True)
        full = s.ambient_occlusion(8, **kw)
        pattern = s.ambient_occlusion(8, seed=7, **kw)          # what the slot's AO plane holds when the bands are set: another seed's values
        differs = (bits(full) != bits(pattern)).any(axis=1)
        s.set_row_bands(16, 1, 2)
        s.render(gbuffer=True)                                   # the same camera and slot: this rank's rows of the planes are written again
        got = s.ambient_occlusion(8, **kw)
        assert s.ao_stats() == (2 * 8, 0, 3)
        owned = np.array([s.hip.crt_row_owner(y, 16, 2) == 1 for y in range(H)])
        assert int(owned.sum()) == 16 == s.owned_rows() and differs[owned].any() and differs[~owned].any()
        assert np.array_equal(bits(got[owned]), bits(full[owned])) and np.array_equal(bits(got[~owned]), bits(pattern[~owned]))
        with pytest.raises(_lib.CrtError):                       # the filter's window crosses band edges
            s.ambient_occlusion(8, filter=True, **kw)
        s.set_row_bands(16, 0, 1)
        s.render(gbuffer=True)
        assert np.array_equal(bits(s.ambient_occlusion(8, **kw)), bits(full))
