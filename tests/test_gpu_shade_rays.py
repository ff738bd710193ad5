"""Shaded ray queries on device buffers (crt_shade_rays / Session.shade_rays) on the GPU: radiance and first-hit surface records for rays given
as torch tensors, against the frame the same rays make (crt_read_output of a frame without flags, the three planes of a CRT_RENDER_GBUFFER
frame), the C oracle's Trace of them and the numpy restatement of the surface record (tests/shade_ref.py). Everything is compared bit for
bit; no ray is excluded. CRT_RAYS_GRID=3 unless stated otherwise: three waves walk the chunks.
Reference: kernel_main.cl:187-272 with the ray (o, d) in the camera ray's place (include/crt_api.h, crt_shade_rays)."""
import ctypes as C
import functools

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import oracle_lib
import shade_ref
import trace_rays_ref as rr
from util import bits, seeded_rays

pytestmark = pytest.mark.gpu
FLAG_RAYS = 2                             # CRT_RENDER_WRITE_RAYS
W, H, N = 64, 48, 1027                    # the sessions that render nothing of interest; 1027 rays: 17 chunks, a ragged last one
POISON = 0x5A5A5A5A


def session(monkeypatch, sc, w=W, h=H, grid="3", tlas=None, **kw):
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


def arenas_of(s):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """arenas, N seeded rays of scene `name`, the oracle's unbounded records, surface records and radiance: computed once, never modified"""
    sc = scenes.get(name)
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(sc)
        a = arenas_of(s)
    o, d = seeded_rays(a, sc.camera_pos, N, seed=23)
    orc = oracle_lib.Oracle(a, nthreads=16)
    rec, _ = orc.closest_hits(o, d)
    surf = shade_ref.surface_from_records(a, rec)
    rad = shade_ref.radiance(orc, o, d, sc.sun_angle)
    for x in (o, d, rec, surf, rad):
        x.setflags(write=False)
    return a, o, d, rec, surf, rad


def c_shade(s, batch, params, radiance, surface, instances=None, stream=None):
    return s.hip.crt_shade_rays(C.byref(batch) if batch is not None else None, C.byref(params) if params is not None else None,
                                s.h.crth_num_instances() if instances is None else instances, radiance, surface, stream)


# ---- 1. a frame's rays give the frame ----
@pytest.mark.parametrize("tlas", ["0", "1"])
@pytest.mark.parametrize("name,w,h", [("tiny", 131, 67), ("cornell-1k", 160, 96), ("nanosuit-demo", 160, 90)])
def test_a_frames_rays_give_the_frame(monkeypatch, nthreads, name, w, h, tlas):
    sc = scenes.get(name)
    with session(monkeypatch, sc, w, h, tlas=tlas) as s:
        s.render_raw(FLAG_RAYS)
        rays = s.read_rays()
        s.render_raw(0)
        frame = s.read_output().reshape(-1, 4)
        s.render_raw(_lib.CRT_RENDER_GBUFFER)
        planes = s.read_gbuffer_raw()
        iv, ip, pos = s.camera()
        a = arenas_of(s)
        rad, surf = s.shade_rays(dev(np.asarray(pos, np.float32)), dev(rays.reshape(-1, 3)), radiance=True, surface=True)
        chunks = (w * h + 63) // 64
        assert s.shade_stats() == (chunks, 0, 3)
        rad, surf = rad.cpu().numpy(), surf.numpy()
    hits = int((surf["instance"] >= 0).sum())
    print(f"{name} {w}x{h} tlas={tlas}: {hits} of {w * h} rays hit; radiance words equal {int((bits(rad) == bits(frame)).sum())} of {rad.size}")
    assert 0 < hits < w * h
    assert np.array_equal(bits(rad), bits(frame))
    assert shade_ref.same_surface(surf, shade_ref.surface_of_planes(planes), shade_ref.PIXEL_FIELDS)
    # ... and both are the reference's
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    assert shade_ref.same_surface(surf, shade_ref.surface(a, orc, pos, rays.reshape(-1, 3)))
    assert np.array_equal(bits(rad), bits(shade_ref.radiance(orc, pos, rays.reshape(-1, 3), sc.sun_angle)))


# ---- 2. rays with their own origins ----
def _own_rays():
    """4 origins x 200 directions around cornell-1k's box (x -1..1, y 0..2, z -1..1, open towards +z): the camera, a point beside it, two inside"""
    rng = np.random.RandomState(41)
    origins = np.array([(0.0, 1.0, 3.5), (2.5, 1.5, 3.0), (0.0, 1.0, 0.5), (-0.5, 1.6, -0.3)], np.float64)
    o = np.repeat(origins, 200, axis=0)
    target = rng.uniform((-1.2, -0.2, -1.2), (1.2, 2.2, 1.2), size=(800, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def test_rays_with_their_own_origins(monkeypatch, nthreads):
    import torch
    sc = scenes.get("cornell-1k")
    o, d = _own_rays()
    with session(monkeypatch, sc) as s:
        a = arenas_of(s)
        orc = oracle_lib.Oracle(a, nthreads=nthreads)
        to, td = dev(o), dev(d)
        rad, surf = s.shade_rays(to, td, surface=True)
        assert s.shade_stats() == (13, 0, 3)
        rad, surf = rad.cpu().numpy(), surf.numpy()
        want_surf, want_rad = shade_ref.surface(a, orc, o, d), shade_ref.radiance(orc, o, d, sc.sun_angle)
        hits = surf["instance"] >= 0
        print(f"own origins: hits per origin {[int(hits[k * 200:(k + 1) * 200].sum()) for k in range(4)]}")
        # (an origin inside the mesh's root box sees what upstream's box test lets it see, hazard H1: possibly nothing)
        assert all(0 < int(hits[k * 200:(k + 1) * 200].sum()) for k in (0, 1)) and 0 < int(hits.sum()) < 800
        assert shade_ref.same_surface(surf, want_surf) and np.array_equal(bits(rad), bits(want_rad))
        # the xyz of float4 rows
        o4 = torch.full((800, 4), float("nan"), device="cuda:0"); o4[:, :3] = to
        d4 = torch.full((800, 4), float("nan"), device="cuda:0"); d4[:, :3] = td
        assert o4[:, :3].stride() == (4, 1)
        rad4, surf4 = s.shade_rays(o4[:, :3], d4[:, :3], surface=True)
        assert np.array_equal(bits(rad4.cpu().numpy()), bits(rad)) and shade_ref.same_surface(surf4.numpy(), surf)
        # one origin for 200 rays, origins of shape (3,)
        for k in range(4):
            sel = slice(k * 200, (k + 1) * 200)
            rad0, surf0 = s.shade_rays(dev(o[k * 200]), td[sel], surface=True)
            assert s.shade_stats() == (4, 0, 3)
            assert np.array_equal(bits(rad0.cpu().numpy()), bits(rad[sel])) and shade_ref.same_surface(surf0.numpy(), surf[sel]), k
        # directions that are no unit vectors (hazard H6): the oracle on the scaled rays
        for scale in (0.5, 3.0):
            ds = (d * np.float32(scale)).astype(np.float32)
            rads, surfs = s.shade_rays(to, dev(ds), surface=True)
            assert shade_ref.same_surface(surfs.numpy(), shade_ref.surface(a, orc, o, ds)), scale
            assert np.array_equal(bits(rads.cpu().numpy()), bits(shade_ref.radiance(orc, o, ds, sc.sun_angle))), scale
            assert np.array_equal(surfs.numpy()["instance"], surf["instance"]), scale
        # one block of 64 rays from beyond the cull's proven range between two near blocks
        limit = C.c_float()
        _lib.check(s.hip.crt_get_cull_range(None, 0, C.byref(limit), None, None), "crt_get_cull_range")
        limit = float(limit.value)
        assert 1.0 < limit < 1e30
        far = np.array([0.3, 0.5, 1.0]) / np.linalg.norm([0.3, 0.5, 1.0]) * 3.0 * limit
        of = np.concatenate([np.tile(o[0].astype(np.float64), (64, 1)), np.tile(far, (64, 1)), np.tile(o[400].astype(np.float64), (64, 1))])
        target = np.random.RandomState(43).uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), size=(192, 3))
        df = target - of
        df /= np.linalg.norm(df, axis=1, keepdims=True)
        of, df = of.astype(np.float32), df.astype(np.float32)
        assert np.linalg.norm(of[64:128].astype(np.float64), axis=1).min() > limit
        radf, surff = s.shade_rays(dev(of), dev(df), surface=True)
        chunks, no_cull, groups = s.shade_stats()
        assert (chunks, groups) == (3, 3) and 1 <= no_cull < chunks
        surff = surff.numpy()
        print(f"far block: {int((surff['instance'][64:128] >= 0).sum())} of 64 far rays hit, limit {limit:g}")
        assert shade_ref.same_surface(surff, shade_ref.surface(a, orc, of, df))
        assert np.array_equal(bits(radf.cpu().numpy()), bits(shade_ref.radiance(orc, of, df, sc.sun_angle)))
        # the other families' statistics and the frames' counter did not move
        assert s.rays_stats() == (0, 0, 0) and s.ao_stats() == (0, 0, 0)
        frames = C.c_uint64(7)
        _lib.check(s.hip.crt_get_cull_range(None, 0, None, None, C.byref(frames)), "crt_get_cull_range")
        assert frames.value == 0


# ---- 3. the bound ----
@pytest.mark.parametrize("name", ["tiny", "cornell-1k"])
def test_the_bound(monkeypatch, name):
    import torch
    a, o, d, rec, surf, rad = reference(name)
    sc = scenes.get(name)
    hits = rec["instance"] >= 0
    assert int(hits.sum()) >= 900 and not any(np.isnan(rec[k]).any() for k in ("t", "u", "v"))      # the filter's precondition (include/crt_api.h)
    with session(monkeypatch, sc) as s:
        to, td = dev(o), dev(d)
        got_rad, got_surf = s.shade_rays(to, td, surface=True)
        assert s.shade_stats() == (17, 0, 3)
        assert np.array_equal(bits(got_rad.cpu().numpy()), bits(rad)) and shade_ref.same_surface(got_surf.numpy(), surf)
        # pure sky: the same directions against no instance
        sky = torch.full((N, 4), POISON, dtype=torch.int32, device="cuda:0")
        batch = _lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 3, 3, N)
        par = _lib.CrtShadeParams(float(sc.sun_angle), 0)
        _lib.check(c_shade(s, batch, par, sky.data_ptr(), None, instances=0, stream=torch.cuda.current_stream().cuda_stream), "crt_shade_rays")
        sky = sky.cpu().numpy().view(np.float32)
        assert np.array_equal(bits(sky[~hits]), bits(rad[~hits])) and (sky[:, 3] == 1.0).all()
        for fam, (tmax, kept) in rr.tmax_families(rec).items():
            want_surf = shade_ref.surface_from_records(a, rr.filtered(rec, tmax))
            keep = hits if kept else np.zeros_like(hits)
            assert np.array_equal(want_surf["instance"] >= 0, keep), fam
            want_rad = np.where(keep[:, None], rad, sky)
            r, sf = s.shade_rays(to, td, tmax=dev(tmax), surface=True)
            r, sf = r.cpu().numpy(), sf.numpy()
            assert shade_ref.same_surface(sf, want_surf), fam
            assert shade_ref.same_surface(sf[~keep], np.full(int((~keep).sum()), shade_ref.MISS)), fam
            assert np.array_equal(bits(r), bits(want_rad)), fam
        # an infinite bound is no bound
        r, sf = s.shade_rays(to, td, tmax=dev(np.full(N, np.inf, np.float32)), surface=True)
        assert np.array_equal(bits(r.cpu().numpy()), bits(rad)) and shade_ref.same_surface(sf.numpy(), surf)


# ---- 4. modes and the bounds of the stores ----
def test_modes_and_store_bounds(monkeypatch):
    import torch
    a, o, d, rec, surf, rad = reference("tiny")
    sc = scenes.get("tiny")
    with session(monkeypatch, sc) as s:
        to, td = dev(o), dev(d)
        both_r, both_s = s.shade_rays(to, td, radiance=True, surface=True)
        only_r = s.shade_rays(to, td)
        only_s = s.shade_rays(to, td, radiance=False, surface=True)
        assert isinstance(only_r, torch.Tensor) and only_r.shape == (N, 4) and isinstance(only_s, driver.SurfaceHits) and len(only_s) == N
        assert np.array_equal(bits(both_r.cpu().numpy()), bits(rad)) and np.array_equal(bits(only_r.cpu().numpy()), bits(rad))
        assert shade_ref.same_surface(both_s.numpy(), surf) and shade_ref.same_surface(only_s.numpy(), surf)
        assert np.array_equal(only_s.t.cpu().numpy(), surf["t"]) and np.array_equal(only_s.material.cpu().numpy().view(np.uint32), surf["material"])
        with pytest.raises(ValueError):
            s.shade_rays(to, td, radiance=False, surface=False)
        stream = torch.cuda.current_stream().cuda_stream
        par = _lib.CrtShadeParams(float(sc.sun_angle), 0)
        for n in (1, 63, 64, 65):
            batch = _lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 3, 3, n)
            for want_r, want_s in ((True, False), (False, True), (True, True)):
                r = torch.full((n + 3, 4), POISON, dtype=torch.int32, device="cuda:0")
                sf = torch.full((n + 3, 12), POISON, dtype=torch.int32, device="cuda:0")
                _lib.check(c_shade(s, batch, par, r.data_ptr() if want_r else None, sf.data_ptr() if want_s else None, stream=stream), "crt_shade_rays")
                assert s.shade_stats() == ((n + 63) // 64, 0, min(3, (n + 63) // 64))
                r, sf = r.cpu().numpy(), sf.cpu().numpy()
                assert (r[n if want_r else 0:] == POISON).all() and (sf[n if want_s else 0:] == POISON).all(), (n, want_r, want_s)
                if want_r:
                    assert np.array_equal(r[:n].view(np.uint32), bits(rad[:n])), (n, want_r, want_s)
                if want_s:
                    assert shade_ref.same_surface(np.ascontiguousarray(sf[:n]).view(_lib.SURFACE_HIT_DTYPE).reshape(-1), surf[:n]), (n, want_r, want_s)


# ---- 5. errors and ordering ----
def test_refusals_launch_nothing(monkeypatch):
    import torch
    a, o, d, rec, surf, rad = reference("tiny")
    sc = scenes.get("tiny")
    with session(monkeypatch, sc) as s:
        to, td = dev(o), dev(d)
        r = torch.full((N, 4), POISON, dtype=torch.int32, device="cuda:0")
        sf = torch.full((N, 12), POISON, dtype=torch.int32, device="cuda:0")
        good, par = _lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 3, 3, N), _lib.CrtShadeParams(float(sc.sun_angle), 0)
        bad = _lib.CRT_E_BAD_ARGUMENT
        assert c_shade(s, None, par, r.data_ptr(), sf.data_ptr()) == bad
        assert c_shade(s, good, None, r.data_ptr(), sf.data_ptr()) == bad
        assert c_shade(s, _lib.CrtRayBatch(None, td.data_ptr(), None, 3, 3, N), par, r.data_ptr(), sf.data_ptr()) == bad
        assert c_shade(s, _lib.CrtRayBatch(to.data_ptr(), None, None, 3, 3, N), par, r.data_ptr(), sf.data_ptr()) == bad
        assert c_shade(s, good, par, None, None) == bad
        for so, sd in ((1, 3), (2, 3), (3, 1), (3, 2)):
            assert c_shade(s, _lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, so, sd, N), par, r.data_ptr(), sf.data_ptr()) == bad, (so, sd)
        for angle in (float("nan"), float("inf"), float("-inf")):
            assert c_shade(s, good, _lib.CrtShadeParams(angle, 0), r.data_ptr(), sf.data_ptr()) == bad, angle
        for flags in (1, 0x100, 0x80000000):
            assert c_shade(s, good, _lib.CrtShadeParams(float(sc.sun_angle), flags), r.data_ptr(), sf.data_ptr()) == bad, flags
        assert c_shade(s, good, par, r.data_ptr(), sf.data_ptr(), instances=402) == bad
        assert c_shade(s, _lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 3, 3, (1 << 30) + 1), par, r.data_ptr(), sf.data_ptr()) == _lib.CRT_E_OUT_OF_RANGE
        assert c_shade(s, _lib.CrtRayBatch(None, None, None, 1, 1, 0), par, None, None) == _lib.CRT_OK          # n == 0: no pointer is looked at
        # an invalid scene: a cyclic BVH is rejected at upload (as tests/test_gpu_edges.py does it) and queries are refused until it is fixed
        nodes = s.arenas()["nodes"].copy()
        fixed = nodes.copy()
        inner = np.where(nodes["triCount"] == 0)[0]
        nodes["leftFirst"][inner[3]] = inner[0]                      # child before parent: cycle
        assert s.hip.crt_upload_bvh_nodes(nodes.ctypes.data, 0, nodes.nbytes) == bad
        assert c_shade(s, good, par, r.data_ptr(), sf.data_ptr()) == bad
        assert s.hip.crt_upload_bvh_nodes(fixed.ctypes.data, 0, fixed.nbytes) == _lib.CRT_OK
        torch.cuda.synchronize()
        assert s.shade_stats() == (0, 0, 0) and (r.cpu().numpy() == POISON).all() and (sf.cpu().numpy() == POISON).all()
        # through the host mirror: reported as Renderer::LastError()
        assert s.h.crth_shade_rays(C.byref(good), C.byref(par), None, None, None) == 0 and s.h.crth_last_error() == bad
        s.h.crth_clear_error()
        assert s.h.crth_shade_rays(None, C.byref(par), r.data_ptr(), None, None) == 0 and s.h.crth_last_error() == bad
        s.h.crth_clear_error()
        with pytest.raises(_lib.CrtError):
            s.shade_rays(to, td, sun_angle=float("nan"))
        assert s.h.crth_last_error() == 0 and s.shade_stats() == (0, 0, 0)
        assert np.array_equal(bits(s.shade_rays(to, td).cpu().numpy()), bits(rad))       # the session is as usable as before
    with session(monkeypatch, sc, devices=[0, 0]) as s:              # the pointers belong to one GPU
        assert c_shade(s, good, par, r.data_ptr(), sf.data_ptr()) == _lib.CRT_E_UNSUPPORTED
        with pytest.raises(_lib.CrtError):
            s.shade_rays(to, td)
        assert s.shade_stats() == (0, 0, 0) and (r.cpu().numpy() == POISON).all() and (sf.cpu().numpy() == POISON).all()


def test_queries_frames_and_instance_uploads_stay_ordered(monkeypatch, nthreads):
    """A query between pipelined frames leaves their bits alone, and a query submitted after an instance upload sees the moved instance."""
    import torch
    a0, o, d, rec0, surf0, rad0 = reference("tiny")
    sc = scenes.get("tiny")
    move = np.array([3.0, 1.5, -2.0], np.float32)
    with session(monkeypatch, sc) as s:
        to, td = dev(o), dev(d)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s.render(pipelined=True)
        with torch.cuda.stream(side):
            first = s.shade_rays(to, td, surface=True)
        s.render(pipelined=True)
        frame_before = s.output().copy()
        s.h.crth_set_mesh_position(0, move.ctypes.data_as(C.POINTER(C.c_float)))
        s.render(pipelined=True)                                      # uploads the table, then a frame in flight
        moved = oracle_lib.Oracle(s.arenas(), nthreads=nthreads)
        a1 = arenas_of(s)
        second = s.shade_rays(to, td, surface=True)
        s.render(pipelined=True)
        torch.cuda.synchronize()
        frame_after = s.output().copy()
        assert np.array_equal(bits(first[0].cpu().numpy()), bits(rad0)) and shade_ref.same_surface(first[1].numpy(), surf0)
        want_surf, want_rad = shade_ref.surface(a1, moved, o, d), shade_ref.radiance(moved, o, d, sc.sun_angle)
        assert not shade_ref.same_surface(want_surf, surf0)          # the move matters to these rays
        assert shade_ref.same_surface(second[1].numpy(), want_surf) and np.array_equal(bits(second[0].cpu().numpy()), bits(want_rad))
    with session(monkeypatch, sc) as s:                               # fresh sessions in the same states, no query
        s.render()
        assert np.array_equal(bits(s.output()), bits(frame_before))
        s.h.crth_set_mesh_position(0, move.ctypes.data_as(C.POINTER(C.c_float)))
        s.render()
        assert np.array_equal(bits(s.output()), bits(frame_after))
