"""The root pre-test of the camera bounce on the device (crt_device.h: root_pretest_misses -- the exact root step once per surviving instance and
wave, behind the staged per-lane loop): the uncounted Trace kernels, which take it, against the counted kernels, which do not, and against the
oracle, which has no cull at all -- bit for bit, with the kernel that ran checked by name for every frame.

Scene `tiny`'s meshes as 8, 16, 17, 64 and 65 small instances (65 with CRT_TLAS=0: two 64-chunks, no wave test and no pre-test -- the same
frames all the same) plus, in every scene, one instance of a one-triangle mesh (its root is a leaf: never cleared), at 64x64, 72x40 and 203x117
(partial tiles at the edges: waves that take neither test). The instances are placed on the CPU from the arenas so that tile rays graze a
root child box: the far corner ray of a chosen tile passes the first child box of instance k at 0.999 or 1.001 of the angle at which the box's
nearest corner touches it. Flags 0, shadow rays, refraction, SSAA 2 and 4, the G-buffer (Frames.flag_sets), and SSAA and the G-buffer with shadow
rays -- the kernels with shadow rays that take the pre-test (shadowed_forms); frames in flight, row bands and split tiles; cameras inside a root child box, on a box face and beyond the cull's range; a frame whose middle column has NaN directions.
Not vacuous: in every scene the restatement (tests/root_pretest_ref.py) finds a full tile and an instance that the sphere cull keeps for its lanes
and the pre-test clears for some of them and keeps for others."""
import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import oracle_lib
import root_pretest_ref as ref
import wave_cull_ref
import gbuffer_ref
from test_gpu_camera_cull import ASYNC, COUNT, GBUFFER, SHADOWS, SSAA2, SSAA4, Frames, _one_triangle_mesh, _scene, _special_cameras
from test_gpu_ssaa import resolve
from test_gpu_wave_cull import _matrices, _spheres
from util import bits

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(64, 64), (72, 40), (203, 117)]
GRAZE = (0.999, 1.001)


def _first_child_corners(arenas, k):
    """the eight corners of instance k's first root child box, in world space relative to the instance's translation (float64)"""
    inst = arenas["instances"][k]
    node = arenas["nodes"][int(arenas["roots"][inst["meshIndex"]])]
    kid = arenas["nodes"][int(node["leftFirst"])]
    lo, hi = kid["min"].astype(np.float64), kid["max"].astype(np.float64)
    fwd = np.linalg.inv(np.ascontiguousarray(inst["inv"], F).astype(np.float64))
    pts = np.array([[hi[0] if c & 1 else lo[0], hi[1] if c & 2 else lo[1], hi[2] if c & 4 else lo[2]] for c in range(8)])
    return pts @ fwd[:3, :3]


def grazing_scene(n, w, h, nthreads, tmp_path):
    """n - 1 instances whose first root child box grazes the far corner ray of a tile of the w x h frame, and one single-leaf instance"""
    ms = _matrices(n)
    probe = _scene(f"root-pretest-probe-{n}", [scenes.Instance(k % 2, 0xFFFF, m) for k, m in enumerate(ms)])
    with driver.Session(w, h, host_only=True) as s:
        s.load_scene(probe)
        a = s.arenas()
        iv, ip, pos = s.camera()
        rays = np.asarray(oracle_lib.Oracle(a, nthreads=nthreads).raygen(w, h, iv, ip), np.float64).reshape(h, w, 3)
        corners = [_first_child_corners(a, k) for k in range(n)]
    tx, ty = w // 8, h // 8
    insts = []
    for k, m in enumerate(ms):
        i, j = (k * 5 + 1) % tx, (k * 3 + k // tx) % ty
        axis, far = rays[8 * j, 8 * i], rays[8 * j + 7, 8 * i + 7]
        side = far - (far @ axis) * axis
        side /= np.linalg.norm(side)
        theta = np.arccos(np.clip(axis @ far, -1, 1))
        x = 9.0 + 1.7 * (k % 11)

        def nearest_angle(sdisp):                      # the smallest angle from the axis, in the (axis, side) plane's sense, of the box's corners
            p = x * axis + sdisp * side + corners[k]
            return np.min(np.arctan2(p @ side, p @ axis))
        lo_s, hi_s = 0.0, x                            # nearest_angle grows with the displacement along `side`: bisect for GRAZE x theta
        for _ in range(60):
            mid = 0.5 * (lo_s + hi_s)
            lo_s, hi_s = (mid, hi_s) if nearest_angle(mid) < theta * GRAZE[k % 2] else (lo_s, mid)
        m = m.copy(); m[3, :3] = (pos.astype(np.float64) + x * axis + hi_s * side).astype(F)
        insts.append(scenes.Instance(k % 2, 0xFFFF, m))
    insts[3] = scenes.Instance(2, 0xFFFF, scenes._trs(1.5, (0.2, 1.0, 0.1), 0.8, (1.0, 3.0, 2.0)))       # the one-triangle mesh: its root is a leaf
    return _scene(f"root-pretest-{n}-{w}x{h}", insts, [_one_triangle_mesh(tmp_path)])


def shadowed_forms(f, what):
    """Frames.flag_sets' shadow frame runs a kernel that takes no wave test, and its G-buffer frame one the pre-test's policy leaves out; these are the
    kernels with shadow rays that do take the pre-test: supersampled (against the resolved oracle frame and the counted kernel) and with the
    first-hit planes (colour and planes against the oracle)."""
    s = f.s
    for k, flag in ((2, SSAA2), (4, SSAA4)):
        got = f.render(flag | SHADOWS, "crt_trace_ssaa_kernel<0,1,0,0>")
        assert np.array_equal(bits(got), bits(resolve(f.oracle(k, shadows=True), k))), (what, "ssaa + shadows", k)
        assert np.array_equal(bits(got), bits(f.render(flag | SHADOWS | COUNT, "crt_trace_ssaa_kernel<1,1,0,0>"))), (what, "ssaa + shadows, counted", k)
    got = f.render(GBUFFER | SHADOWS, "crt_trace_gbuffer_kernel<1,0,0>")
    assert np.array_equal(bits(got), bits(f.oracle(shadows=True))), (what, "gbuffer + shadows colour")
    iv, ip, pos = s.camera()
    want = gbuffer_ref.reference_planes(s.arenas(), f.orc, f.orc.raygen(s.width, s.height, iv, ip), pos)
    planes = s.read_gbuffer_raw()
    for p in ("geometry", "ids", "albedo"):
        assert np.array_equal(np.ascontiguousarray(planes[p]).view(np.uint32), np.ascontiguousarray(want[p]).view(np.uint32)), (what, "gbuffer + shadows", p)


def assert_mixed_wave(s, orc, w, h):
    """some full tile and instance: the sphere cull keeps the instance for lanes the pre-test clears AND for lanes it keeps"""
    a = s.arenas()
    iv, ip, pos = s.camera()
    d = np.asarray(orc.raygen(w, h, iv, ip), F)
    o = np.asarray(pos, F)
    clears = ref.frame_clears(a, o, d.reshape(-1, 3)).reshape(h, w, -1)
    assert not clears[..., 3].any()                                                     # the single-leaf instance
    inner = [k for k in range(len(a["instances"])) if ref.instance_terms(a, k)[1] is not None]
    sub = dict(a); sub["instances"] = a["instances"][inner]
    sph = _spheres(sub)
    cf = np.array([c for c, _ in sph], np.float64).astype(F)[None]
    wr = np.array([r for _, r in sph], F)[None]
    th, tw = h // 8, w // 8
    tiles = d[:th * 8, :tw * 8].reshape(th, 8, tw, 8, 3).transpose(0, 2, 1, 3, 4).reshape(th * tw, 64, 3)
    kept = ~wave_cull_ref.lane_culls(np.tile(o, (th * tw, 1)), tiles, np.tile(cf, (th * tw, 1, 1)), np.tile(wr, (th * tw, 1)))
    cl = clears[:th * 8, :tw * 8][..., inner].reshape(th, 8, tw, 8, -1).transpose(0, 2, 1, 3, 4).reshape(th * tw, 64, -1)
    mixed = (kept & cl).any(1) & (kept & ~cl).any(1)
    assert mixed.any(), "no wave in which the pre-test clears an instance for some lanes and keeps it for others"
    return int(mixed.sum())


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n", [8, 16, 17, 64, 65])
def test_grazing_boxes_every_flag_set(n, w, h, monkeypatch, nthreads, tmp_path):
    if n > 64:
        monkeypatch.setenv("CRT_TLAS", "0")                                   # read by crt_init: the chunked loop, 64 + 1
    sc = grazing_scene(n, w, h, nthreads, tmp_path)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        assert len(s.arenas()["instances"]) == n
        f = Frames(s, sc, nthreads)
        assert_mixed_wave(s, f.orc, w, h)
        f.flag_sets(f"{n} grazing boxes, {w}x{h}")
        shadowed_forms(f, f"{n} grazing boxes, {w}x{h}")


@pytest.mark.parametrize("w,h", SIZES[1:])
def test_special_cameras_and_nan_directions(w, h, nthreads, tmp_path):
    sc = grazing_scene(16, w, h, nthreads, tmp_path)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        f = Frames(s, sc, nthreads)
        cams, scene_lim = _special_cameras(s)                                # inside instance 0's first root child box, on its face, at and beyond the range
        for what, pos, front in cams:
            s.set_camera(np.asarray(pos, F), np.asarray(front, F))
            f.plain(what=what)
            assert (np.linalg.norm(s.camera()[2].astype(np.float64)) > scene_lim) == (what == "beyond the range")
        # RayGen with invProj = identity and invView = one row: dir = normalize((2 cx, 0, 0)) -- +-x, and NaN where cx == 0
        iv = np.zeros((4, 4), F); iv[0, 0] = 2.0
        ip = np.eye(4, dtype=F)
        pos = np.array([-30.0, 7.0, 2.0], F)
        s.resize(64, 64)
        dirs = f.orc.raygen(64, 64, iv.reshape(16), ip.reshape(16))
        assert np.isnan(dirs[:, 32]).all() and not np.isnan(dirs[:, :32]).any() and not np.isnan(dirs[:, 33:]).any()
        want = f.orc.trace(dirs, pos, sc.sun_angle)[0]
        frames = []
        for flags, kernel in ((0, "crt_trace_kernel<0,0,0,0,0>"), (COUNT, "crt_trace_kernel<1,0,0,0,0>")):
            s.render_raw(flags, view=(iv.reshape(16), ip.reshape(16), pos))
            assert s.last_kernel() == kernel
            frames.append(s.read_output())
        assert np.array_equal(bits(frames[0]), bits(frames[1]))
        assert np.array_equal(bits(frames[0]), bits(want))


def test_row_bands_split_tiles_and_frames_in_flight(monkeypatch, nthreads, tmp_path):
    monkeypatch.setenv("CRT_FRAMES_IN_FLIGHT", "3")
    w, h = 72, 40
    sc = grazing_scene(16, w, h, nthreads, tmp_path)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        f = Frames(s, sc, nthreads)
        ref_frame = f.plain()
        for _ in range(3):                      # later frames run on lists built from the first one's costs: quadrant waves of split tiles
            assert np.array_equal(bits(f.render(0, "crt_trace_kernel<0,0,0,0,0>")), bits(ref_frame))
        s.set_row_bands(16, 1, 2)
        part = f.render(0, "crt_trace_kernel<0,0,0,0,0>")
        own = np.array([_lib.hip().crt_row_owner(y, 16, 2) == 1 for y in range(s.height)])
        assert own.any() and np.array_equal(bits(part[own]), bits(ref_frame[own]))
        s.set_row_bands(16, 0, 1)
        # frames in flight: a camera that moves every frame, each ASYNC frame against the synchronous frame of the same camera
        cams = [((0.5 + 0.7 * k, 7.0 - 0.4 * k, 16.0 - k), scenes._normalize((0.05 * k, -0.3, -1.0))) for k in range(5)]
        got = []
        for pos, front in cams:
            s.set_camera(pos, front)
            s.render_raw(ASYNC)
            assert s.last_kernel() == "crt_trace_kernel<0,0,0,0,0>"
            s.sync()
            got.append(s.read_output())
        for k, (pos, front) in enumerate(cams):
            s.set_camera(pos, front)
            assert np.array_equal(bits(got[k]), bits(f.plain(what=f"camera {k}"))), k
