"""CRT_RENDER_GBUFFER: the Trace launch (crt_trace_gbuffer_kernel) also writes what each pixel's primary ray hit -- normal and distance,
instance / triangle / barycentrics, albedo -- into three planes of the frame slot. Every plane is compared bit for bit: `ids` and `t`
with closest-hit records (the oracle's, and the session's own crt_query_hits over its own RayGen buffer), normal and albedo with the
numpy restatement of kernel_main.cl:226-245 on those records (tests/gbuffer_ref.py, pinned to the oracle by tests/test_gbuffer_cpu.py).
The colour frame must be the bits of the same frame without the flag."""
import ctypes as C

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import gbuffer_ref
import oracle_lib
from util import bits

pytestmark = pytest.mark.gpu

POST, WRITE_RAYS, ASYNC, COUNT, STAMPS, SHADOWS, UNORM8, READBACK, REFRACT, FXAA, MIX3 = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024
SSAA2, SSAA4, GBUFFER = 2048, 4096, 8192
PLANES = ("geometry", "ids", "albedo")


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_planes_equal(got, want, rows=None, what=""):
    for p in PLANES:
        g, w = (got[p], want[p]) if rows is None else (got[p][rows], want[p][rows])
        assert np.array_equal(words(g), words(w)), (what, p, int((words(g) != words(w)).sum()))


def assert_ids_are_records(planes, rec, what=""):
    """ids and t of the planes == hit records of the same rays (crt_query_hits / orc_closest_hits layout)"""
    ids, t = planes["ids"].reshape(-1), planes["geometry"]["t"].reshape(-1)
    assert np.array_equal(ids["instance"], rec["instance"]) and np.array_equal(ids["tri"], rec["tri"]), what
    for got, f in ((ids["u"], "u"), (ids["v"], "v"), (t, "t")):
        assert np.array_equal(bits(got), bits(rec[f])), (what, f)


def raw_rc(s, flags):
    a, iv, ip = s.trace_args()
    fp = C.POINTER(C.c_float)
    return s.hip.crt_render(C.byref(a), iv.ctypes.data_as(fp), ip.ctypes.data_as(fp), int(flags))


def read_rc(s, plane=0):
    """crt_read_gbuffer's return code for a correctly sized read"""
    size = s.width * s.height * (4 if plane == 2 else 16)
    buf = np.empty(size, np.uint8)
    return s.hip.crt_read_gbuffer(plane, buf.ctypes.data, size)


def own_records(s):
    """crt_query_hits over the session's own RayGen buffer (of the last WRITE_RAYS frame) from the session camera"""
    rays = s.read_rays().reshape(-1, 3)
    pos = s.camera()[2]
    return s.query_hits(np.tile(pos, (len(rays), 1)), rays)


def oracle_reference(s, sc, nthreads):
    """(oracle, reference planes, oracle colour frame) of the session's current view"""
    iv, ip, pos = s.camera()
    a = s.arenas()
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    rays = orc.raygen(s.width, s.height, iv, ip)
    frame, _ = orc.trace(rays, pos, sc.sun_angle)
    return orc, gbuffer_ref.reference_planes(a, orc, rays, pos), frame


@pytest.mark.parametrize("name,w,h", [("tiny", 200, 120), ("tiny", 16, 16), ("cornell-1k", 333, 187), ("sponza-sibenik", 320, 180), ("nanosuit-demo", 256, 144)])
def test_planes_are_exact(name, w, h, nthreads):
    sc = scenes.get(name)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        orc, want, frame = oracle_reference(s, sc, nthreads)
        s.render_raw(0)
        assert s.last_kernel() == "crt_trace_kernel<0,0,0,0,0>"
        plain = s.read_output()
        s.render_raw(GBUFFER)
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,0,0>", s.last_kernel()
        got = s.read_gbuffer_raw()
        for p in PLANES:
            assert got[p].shape == (h, w)
        assert_planes_equal(got, want, what=name)
        colour = s.read_output()
        assert np.array_equal(bits(colour), bits(plain)) and np.array_equal(bits(colour), bits(frame))
        # the session's own hit records for its own RayGen buffer say the same
        s.render_raw(GBUFFER | WRITE_RAYS)
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,0,0>"
        assert_ids_are_records(s.read_gbuffer_raw(), own_records(s), name)
        assert_planes_equal(s.read_gbuffer_raw(), want, what=name + " after the query")
        hits = int((want["ids"]["instance"] >= 0).sum())
        print(f"{name} {w}x{h}: {hits} of {w * h} pixels hit, all three planes exact")
        if (w, h) != (16, 16):
            assert hits >= 2000
        for plane in range(3):
            assert s.hip.crt_gbuffer_device_ptr(plane)
        assert len({s.hip.crt_gbuffer_device_ptr(plane) for plane in range(3)}) == 3


def test_planes_ignore_the_other_flags(nthreads):
    sc = scenes.get("cornell-1k")
    w, h = 333, 187
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        _, want, _ = oracle_reference(s, sc, nthreads)
        for flags, kern in ((SHADOWS, "<1,0,0>"), (REFRACT, "<0,0,1>"), (POST | UNORM8, "<0,0,0>"), (FXAA, "<0,0,0>"), (READBACK, "<0,0,0>"),
                            (SHADOWS | REFRACT | POST, "<1,0,1>")):
            s.render_raw(flags)
            assert s.last_kernel().startswith("crt_trace_kernel<0,0,")
            colour = s.read_output()
            s.render_raw(flags | GBUFFER)
            assert s.last_kernel() == "crt_trace_gbuffer_kernel" + kern, (flags, s.last_kernel())
            assert_planes_equal(s.read_gbuffer_raw(), want, what=flags)
            assert np.array_equal(bits(s.read_output()), bits(colour)), flags
            if flags & READBACK:
                ptr, nbytes = C.c_void_p(), C.c_size_t()
                assert s.hip.crt_map_host_frame(C.byref(ptr), C.byref(nbytes)) == 0
                host = np.frombuffer((C.c_char * nbytes.value).from_address(ptr.value), np.float32).reshape(h, w, 4)
                assert np.array_equal(bits(host), bits(colour))


def test_instance_tree():
    """401 instances (the construction of test_ssaa_with_the_instance_tree): the TLAS instantiation against the session's own records"""
    tiny = scenes.get("tiny")
    w, h = 192, 128
    with driver.Session(w, h, device=0) as s:
        s.load_scene(tiny)
        s.h.crth_begin_instances()
        for i in range(len(tiny.instances), 401):
            m = scenes._trs(0.6 + 0.1 * (i % 5), (0.3, 1.0, 0.2), 0.37 * i, (float((i % 21) - 10) * 6.0, float((i // 21) - 9) * 6.0, -float(i % 7) * 2.0))
            pm, keep = _lib.fptr(m)
            s.h.crth_register_instance(i % 2, 0xFFFF, pm)
        s.h.crth_end_instances()
        s.set_camera((0.0, 0.0, 23.0 * 6.0), scenes._normalize((0.0, 0.0, -1.0)))
        s.render_raw(0)
        assert s.last_kernel() == "crt_trace_kernel<0,0,0,1,0>"
        plain = s.read_output()
        s.render_raw(GBUFFER | WRITE_RAYS)
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,1,0>", s.last_kernel()
        got = s.read_gbuffer_raw()
        assert np.array_equal(bits(s.read_output()), bits(plain))
        rec = own_records(s)
        assert_ids_are_records(got, rec)
        g, i, c = gbuffer_ref.planes_from_records(s.arenas(), rec)
        assert_planes_equal(got, {"geometry": g.reshape(h, w), "ids": i.reshape(h, w), "albedo": c.reshape(h, w)})
        assert len(np.unique(rec["instance"][rec["instance"] >= 0])) >= 100       # the view does see the grid of instances
        s.render_raw(GBUFFER | SHADOWS | REFRACT)                                  # the one instantiation bounded at 7 waves/SIMD
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<1,1,1>"
        assert_planes_equal(s.read_gbuffer_raw(), got)


def test_launch_without_the_cull(nthreads):
    """A camera beyond crt_get_cull_range's sceneLimit: the launch enters every instance (no cull bounds, no instance tree). The matrices
    are explicit (hazard H10): RayGen normalises invView . target WITH invView's translation (kernel_main.cl:284-286), so a session camera
    that far out would look away from the scene; here the ray directions are those of a camera at the origin looking down -z, narrowed
    until the scene fills the frame again, and only cameraPos -- the rays' origin -- is moved out."""
    sc = scenes.get("cornell-1k")
    w, h = 200, 120
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        lim, frames0 = C.c_float(), C.c_uint64()
        _lib.check(s.hip.crt_get_cull_range(None, 0, C.byref(lim), None, C.byref(frames0)), "crt_get_cull_range")
        dist = float(lim.value) * 1.25 + 1.0
        assert dist < 9e4                                     # upstream's rays end at t = 99999: the scene must stay in reach
        a = s.arenas()
        extent = max(float(np.abs(a["tris"][f]).max()) for f in ("v0", "v1", "v2"))
        fwd = [np.linalg.inv(m.astype(np.float64)) for m in a["instances"]["inv"]]
        reach = max(np.linalg.norm(m[:3, :3], 2) * extent * 3 ** 0.5 + np.linalg.norm(m[3, :3]) for m in fwd)
        s.set_camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
        iv, ip, _ = s.camera()
        pos = np.float32([0.0, 1.0, dist])
        ip = ip.copy()
        ip[0:8] *= np.float32(0.7 * reach / dist)              # the x and y rows of invProj: a frame about 1.5 x `reach` wide at the scene
        orc = oracle_lib.Oracle(a, nthreads=nthreads)
        rays = orc.raygen(w, h, iv, ip)
        frame, _ = orc.trace(rays, pos, sc.sun_angle)
        want = gbuffer_ref.reference_planes(a, orc, rays, pos)
        hits = int((want["ids"]["instance"] >= 0).sum())
        print(f"scene limit {lim.value}: camera at {dist}, scene reach {reach:.2f}, {hits} of {w * h} pixels hit")
        assert hits >= 2000
        s.render_raw(GBUFFER, view=(iv, ip, pos))
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,0,0>"
        frames1 = C.c_uint64()
        _lib.check(s.hip.crt_get_cull_range(None, 0, None, None, C.byref(frames1)), "crt_get_cull_range")
        assert frames1.value == frames0.value + 1
        assert_planes_equal(s.read_gbuffer_raw(), want)
        assert np.array_equal(bits(s.read_output()), bits(frame))
        # the same view with the instance tree forced would still run without it: the kernel name says so
        s.render_raw(GBUFFER | SHADOWS, view=(iv, ip, pos))
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<1,0,0>"
        assert_planes_equal(s.read_gbuffer_raw(), want)


def far_view(s, sc, nthreads):
    """A view of the scene `s` holds whose hits straddle upstream's InfMinusOne (99998) and the rays' starting distance (99999): the
    rays of test_launch_without_the_cull, their origin moved out until the MEDIAN hit distance is 99998.5. -> (view, oracle, rays)"""
    a = s.arenas()
    extent = max(float(np.abs(a["tris"][f]).max()) for f in ("v0", "v1", "v2"))
    fwd = [np.linalg.inv(m.astype(np.float64)) for m in a["instances"]["inv"]]
    reach = max(np.linalg.norm(m[:3, :3], 2) * extent * 3 ** 0.5 + np.linalg.norm(m[3, :3]) for m in fwd)
    s.set_camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    iv, ip, _ = s.camera()
    ip = ip.copy()
    ip[0:8] *= np.float32(0.7 * reach / 9e4)
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    rays = orc.raygen(s.width, s.height, iv, ip)
    d = np.ascontiguousarray(rays.reshape(-1, 3), np.float32)
    rec, _ = orc.closest_hits(np.tile(np.float32([0.0, 1.0, 9e4]), (len(d), 1)), d)
    t = rec["t"][rec["instance"] >= 0]
    assert len(t) >= 2000
    pos = np.float32([0.0, 1.0, 9e4 + (99998.5 - float(np.median(t)))])
    return (iv, ip, pos), orc, rays


def test_hits_beyond_inf_minus_one(nthreads):
    """kernel_main.cl:219 shades a hit with t > InfMinusOne (99998) as sky, and a ray starts with distance 99999, so a triangle
    further than that is no hit at all. One view with all three classes of pixel: a shaded hit; a hit in (99998, 99999), which keeps
    the ids and t that crt_query_hits reports and has the normal and albedo of a miss (include/crt_api.h; GBufferSink::miss takes
    `anyHit` from distance < 99999); and a miss."""
    sc = scenes.get("cornell-1k")
    w, h = 200, 120
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        view, orc, rays = far_view(s, sc, nthreads)
        pos = view[2]
        frame, _ = orc.trace(rays, pos, sc.sun_angle)
        want = gbuffer_ref.reference_planes(s.arenas(), orc, rays, pos)
        inst, t = want["ids"]["instance"], want["geometry"]["t"]
        shaded, far, miss = (inst >= 0) & ~(t > gbuffer_ref.INF_MINUS_ONE), (inst >= 0) & (t > gbuffer_ref.INF_MINUS_ONE), inst < 0
        print(f"camera at z = {pos[2]}: {int(shaded.sum())} shaded hits, {int(far.sum())} hits beyond InfMinusOne, {int(miss.sum())} misses")
        assert shaded.sum() >= 100 and far.sum() >= 100 and miss.sum() >= 100
        assert (t[far] < gbuffer_ref.MISS_T).all() and (t[miss] == gbuffer_ref.MISS_T).all()
        assert (want["albedo"][far] == 0).all() and (want["geometry"]["normal"][far] == 0).all()
        s.render_raw(0, view=view)
        plain = s.read_output()
        for flags, kern in ((WRITE_RAYS, "<0,0,0>"), (SHADOWS | REFRACT, "<1,0,1>")):
            s.render_raw(GBUFFER | flags, view=view)
            assert s.last_kernel() == "crt_trace_gbuffer_kernel" + kern, s.last_kernel()
            got = s.read_gbuffer_raw()
            assert_planes_equal(got, want, what=flags)
            if flags == WRITE_RAYS:
                assert np.array_equal(bits(s.read_output()), bits(plain)) and np.array_equal(bits(plain), bits(frame))
                r = s.read_rays().reshape(-1, 3)
                assert_ids_are_records(got, s.query_hits(np.tile(pos, (len(r), 1)), r))
        y, x = [int(v[0]) for v in np.nonzero(far)]
        px = np.zeros(1, _lib.GBUFFER_PIXEL_DTYPE)
        assert s.hip.crt_pick_pixel(x, y, px.ctypes.data) == 0
        assert px["instance"][0] == inst[y, x] >= 0 and px["albedo"][0] == 0 and (px["normal"][0] == 0).all()
        assert bits(px["t"])[0] == bits(t[y, x])[0] and px["tri"][0] == want["ids"]["tri"][y, x]


def test_frames_in_flight_keep_their_planes(monkeypatch, nthreads):
    monkeypatch.setenv("CRT_FRAMES_IN_FLIGHT", "3")
    sc = scenes.get("cornell-1k")
    w, h = 256, 144
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        cams = [(sc.camera_pos, sc.camera_front),
                (tuple(np.asarray(sc.camera_pos, np.float32) + np.float32([0.4, 0.2, -0.3])), scenes._normalize(tuple(np.asarray(sc.camera_front, np.float32) + np.float32([0.15, -0.05, 0.0]))))]
        want, frames = [], []
        for pos, front in cams:
            s.set_camera(pos, front)
            _, p, f = oracle_reference(s, sc, nthreads)
            want.append(p); frames.append(f)
        assert not np.array_equal(words(want[0]["ids"]), words(want[1]["ids"]))
        for n in (7, 3, 6):                                   # the last G-buffer frame lands on slot 0, 1, 2 in turn
            for k in range(n):
                s.set_camera(*cams[k & 1])
                s.render_raw(ASYNC | GBUFFER)
                assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,0,0>"
            last = (n - 1) & 1
            assert_planes_equal(s.read_gbuffer_raw(), want[last], what=n)
            assert np.array_equal(bits(s.read_output()), bits(frames[last])), n
            # a plain frame in flight afterwards (the next slot) leaves the planes of the last G-buffer frame readable
            s.set_camera(*cams[1 - last])
            s.render_raw(ASYNC)
            assert s.last_kernel() == "crt_trace_kernel<0,0,0,0,0>"
            assert_planes_equal(s.read_gbuffer_raw(), want[last], what=(n, "behind a plain frame"))
            assert np.array_equal(bits(s.read_output()), bits(frames[1 - last])), n


def test_row_bands(nthreads):
    sc = scenes.get("cornell-1k")
    w, h = 200, 120                                           # 7.5 bands of 16 rows
    hip = _lib.hip()
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        _, want, _ = oracle_reference(s, sc, nthreads)
        owner = np.array([hip.crt_row_owner(y, 16, 2) for y in range(h)])
        whole = {p: np.zeros_like(want[p]) for p in PLANES}
        for r in (0, 1):
            s.set_row_bands(16, r, 2)
            s.render_raw(GBUFFER)
            assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,0,0>"
            got = s.read_gbuffer_raw()
            assert_planes_equal(got, want, rows=owner == r, what=r)
            for p in PLANES:
                whole[p][owner == r] = got[p][owner == r]
        assert_planes_equal(whole, want)
        s.set_row_bands(16, 0, 1)
        s.render_raw(GBUFFER)
        assert_planes_equal(s.read_gbuffer_raw(), want)


def test_pick_pixel_and_the_mirror(nthreads):
    sc = scenes.get("sponza-sibenik")
    w, h = 320, 180
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        s.render_raw(GBUFFER)
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,0,0>"
        planes = s.read_gbuffer_raw()
        rng = np.random.RandomState(7)
        pixels = [(int(rng.randint(0, w)), int(rng.randint(0, h))) for _ in range(64)] + [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]

        def expected(x, y):
            e = np.zeros(1, _lib.GBUFFER_PIXEL_DTYPE)
            e["normal"], e["t"] = planes["geometry"][y, x]["normal"], planes["geometry"][y, x]["t"]
            for f in ("instance", "tri", "u", "v"):
                e[f] = planes["ids"][y, x][f]
            e["albedo"] = planes["albedo"][y, x]
            return e

        out = np.zeros(1, _lib.GBUFFER_PIXEL_DTYPE)
        for x, y in pixels:
            assert s.hip.crt_pick_pixel(x, y, out.ctypes.data) == 0
            assert out.tobytes() == expected(x, y).tobytes(), (x, y)
        assert sum(1 for x, y in pixels if planes["ids"][y, x]["instance"] >= 0) >= 16
        for x, y in ((-1, 0), (w, 0), (0, -1), (0, h), (w, h)):
            assert s.hip.crt_pick_pixel(x, y, out.ctypes.data) == _lib.CRT_E_OUT_OF_RANGE, (x, y)
        assert s.hip.crt_pick_pixel(0, 0, None) == _lib.CRT_E_BAD_ARGUMENT
        # Renderer::SetGBuffer / MapGBuffer / PickPixel through crth_* and the driver
        s.render(gbuffer=True)
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,0,0>"
        assert_planes_equal(s.read_gbuffer(), planes)
        for x, y in pixels:
            assert s.pick(x, y).tobytes() == expected(x, y).tobytes(), (x, y)
        with pytest.raises(_lib.CrtError):
            s.pick(w, 0)
        s.render(shadows=True, postprocess=True, gbuffer=True)             # ... and the session is still usable
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<1,0,0>"
        assert_planes_equal(s.read_gbuffer(), planes)
        s.render()
        assert s.last_kernel() == "crt_trace_kernel<0,0,0,0,0>"
        assert_planes_equal(s.read_gbuffer(), planes)


def test_refusals_change_nothing(monkeypatch):
    sc = scenes.get("tiny")
    w, h = 160, 96
    out = np.zeros(1, _lib.GBUFFER_PIXEL_DTYPE)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        s.render_raw(0)
        plain = s.read_output()
        # no G-buffer frame yet
        for plane in range(3):
            assert read_rc(s, plane) == _lib.CRT_E_BAD_ARGUMENT and not s.hip.crt_gbuffer_device_ptr(plane)
        assert s.hip.crt_pick_pixel(1, 1, out.ctypes.data) == _lib.CRT_E_BAD_ARGUMENT
        s.render_raw(GBUFFER)
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,0,0>"
        planes = s.read_gbuffer_raw()
        # unknown plane, wrong size
        buf = np.empty(w * h * 16, np.uint8)
        assert s.hip.crt_read_gbuffer(3, buf.ctypes.data, buf.size) == _lib.CRT_E_BAD_ARGUMENT
        assert s.hip.crt_read_gbuffer(-1, buf.ctypes.data, buf.size) == _lib.CRT_E_BAD_ARGUMENT
        assert s.hip.crt_read_gbuffer(2, buf.ctypes.data, buf.size) == _lib.CRT_E_BAD_ARGUMENT
        assert s.hip.crt_read_gbuffer(0, buf.ctypes.data, buf.size - 16) == _lib.CRT_E_BAD_ARGUMENT
        assert not s.hip.crt_gbuffer_device_ptr(3)
        for flags in (GBUFFER | SSAA2, GBUFFER | SSAA4, GBUFFER | STAMPS, GBUFFER | MIX3, GBUFFER | COUNT, GBUFFER | COUNT | SHADOWS):
            assert raw_rc(s, flags) == _lib.CRT_E_UNSUPPORTED, flags
            assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,0,0>"        # nothing was launched
            assert_planes_equal(s.read_gbuffer_raw(), planes, what=flags)
            s.render_raw(0)
            assert s.last_kernel() == "crt_trace_kernel<0,0,0,0,0>"
            assert np.array_equal(bits(s.read_output()), bits(plain)), flags
            assert_planes_equal(s.read_gbuffer_raw(), planes, what=flags)
            s.render_raw(GBUFFER)
        # a resize drops the planes; a resize the library ignores (below 16) does not
        s.resize(8, 8)
        assert_planes_equal(s.read_gbuffer_raw(), planes)
        s.resize(200, 120)
        for plane in range(3):
            assert read_rc(s, plane) == _lib.CRT_E_BAD_ARGUMENT and not s.hip.crt_gbuffer_device_ptr(plane)
        assert s.hip.crt_pick_pixel(1, 1, out.ctypes.data) == _lib.CRT_E_BAD_ARGUMENT
        s.resize(w, h)
        assert read_rc(s) == _lib.CRT_E_BAD_ARGUMENT
        s.render_raw(GBUFFER)
        assert_planes_equal(s.read_gbuffer_raw(), planes)
    # the opt-in kernel forms are not extended (CRT_KERNEL is read by crt_init)
    for form in ("wavefront", "refill", "block", "ldstop"):
        monkeypatch.setenv("CRT_KERNEL", form)
        with driver.Session(w, h, device=0) as s:
            s.load_scene(sc)
            s.render_raw(0)
            kern, before = s.last_kernel(), s.read_output()
            assert not kern.startswith("crt_trace_kernel") and "gbuffer" not in kern, (form, kern)
            assert raw_rc(s, GBUFFER) == _lib.CRT_E_UNSUPPORTED, form
            assert raw_rc(s, GBUFFER | ASYNC) == _lib.CRT_E_UNSUPPORTED, form
            assert s.last_kernel() == kern
            assert read_rc(s) == _lib.CRT_E_BAD_ARGUMENT
            s.render_raw(0)
            assert np.array_equal(bits(s.read_output()), bits(before)), form
    monkeypatch.delenv("CRT_KERNEL")
    # several devices: refused by the dispatcher before the slot rotation advances
    with driver.Session(w, h, devices=[0, 0]) as s:
        s.load_scene(sc)
        s.render_raw(0)
        kern = s.last_kernel()
        assert kern == "crt_trace_kernel<0,0,0,0,0>"
        assert np.array_equal(bits(s.read_output()), bits(plain))
        assert raw_rc(s, GBUFFER) == _lib.CRT_E_UNSUPPORTED
        assert raw_rc(s, GBUFFER | ASYNC) == _lib.CRT_E_UNSUPPORTED
        assert read_rc(s) == _lib.CRT_E_BAD_ARGUMENT and not s.hip.crt_gbuffer_device_ptr(0)
        for _ in range(4):
            s.render_raw(ASYNC)
        assert np.array_equal(bits(s.read_output()), bits(plain))
        s.render_raw(0)
        assert s.last_kernel() == kern
        assert np.array_equal(bits(s.read_output()), bits(plain))


def test_full_size_frame():
    """multi-1M at 1920x1080, the headline view: no CPU oracle at this size -- the session's own records over its own rays"""
    sc = scenes.get("multi-1M")
    w, h = 1920, 1080
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        s.render_raw(0)
        plain = s.read_output()
        s.render_raw(GBUFFER | WRITE_RAYS)
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,0,0>", s.last_kernel()
        got = s.read_gbuffer_raw()
        assert np.array_equal(bits(s.read_output()), bits(plain))
        rec = own_records(s)
        assert_ids_are_records(got, rec)
        hit = got["ids"]["instance"] >= 0
        share = float(hit.mean())
        print(f"multi-1M 1920x1080: {share:.4f} of the pixels hit")
        assert 0.20 <= share <= 0.45
        # misses are the miss record; hits carry a unit normal and an opaque albedo
        assert (got["albedo"][~hit] == 0).all() and (got["geometry"]["t"][~hit] == gbuffer_ref.MISS_T).all() and (got["geometry"]["normal"][~hit] == 0).all()
        n = got["geometry"]["normal"][hit].astype(np.float64)
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-5
        assert ((got["albedo"][hit] >> 24) == 0xFF).all()
        # frames in flight at full size end on the same planes
        for _ in range(5):
            s.render_raw(ASYNC | GBUFFER)
        assert_planes_equal(s.read_gbuffer_raw(), got)
