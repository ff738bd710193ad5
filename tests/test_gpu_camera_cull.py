"""The camera bounce's staged instance cull on the device (staged_candidate_mask, crt_device.h): the uncounted Trace kernels, which
take it, against the counted kernels, which do not (CRT_RENDER_COUNTERS: candidate_mask in every lane, as before), and against the
oracle, which has no cull at all -- bit for bit, with the kernel that ran checked by name for every frame.

Frames of 64x36 and 72x40 pixels (the second leaves partial tiles at both edges: fewer active lanes than instances to stage);
scenes of 1, 3, 16, 17 and 65 instances (65 with CRT_TLAS=0: a second 64-chunk whose staging is rewritten), rotated, non-uniformly
scaled and mirrored instances, a single-leaf mesh (never culled); cameras inside an instance's sphere, on a box face, at 0.95 of the
cull's proven range and beyond it (the all-never table), and one looking down an axis (d.x == 0 exactly in the middle column)."""
import ctypes as C

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import gbuffer_ref
import oracle_lib
from test_gpu_cull_bound import _child_boxes, _cull_range, _nonuniform
from test_gpu_ssaa import resolve
from util import bits

pytestmark = pytest.mark.gpu

POST, ASYNC, COUNT, SHADOWS, UNORM8, REFRACT, SSAA2, SSAA4, GBUFFER = 1, 4, 8, 32, 64, 256, 2048, 4096, 8192
SIZES = [(64, 36), (72, 40)]


def _instances(n, nmesh=2):
    """n instances on a grid in front of the default camera: every third one non-uniformly scaled, every fourth mirrored"""
    out = []
    per_row = int(np.ceil(np.sqrt(n)))
    for k in range(n):
        t = ((k % per_row - (per_row - 1) / 2.0) * 6.5, 1.0 + (k % 3), -(k // per_row) * 6.5)
        axis = (0.3 + 0.1 * (k % 4), 1.0, 0.2 * (k % 5) - 0.4)
        if k % 3 == 1:
            m = _nonuniform(0.6 + 0.1 * (k % 4), 1.4, 0.8, axis, 0.37 * k, t)
        else:
            m = scenes._trs(0.5 + 0.15 * (k % 5), axis, 0.37 * k, t)
        if k % 4 == 2:
            m = m.copy(); m[0, :3] = -m[0, :3]                  # mirrored: negative determinant
        out.append(scenes.Instance(k % nmesh, 0xFFFF, m.astype(np.float32)))
    return out


def _scene(name, insts, extra_meshes=()):
    base = scenes.get("tiny")
    return scenes.Scene(name, base.dir, base.skybox, list(base.meshes) + list(extra_meshes), insts, (0.5, 7.0, 16.0), scenes._normalize((0.0, -0.3, -1.0)))


def _one_triangle_mesh(tmp):
    one = scenes.Mesh(np.array([[-2, -2, 0], [2, -2, 0.1], [0, 2, 0.2]], np.float32), np.zeros((3, 2), np.float32),
                      np.tile([0, 0, 1], (3, 1)).astype(np.float32), np.array([[0, 1, 2]], np.int32), np.zeros(1, np.int32))
    return scenes._write_mesh(str(tmp), "one", one, [((0.8, 0.6, 0.4), None)])


class Frames:
    """one session + oracle; every check renders the uncounted frame, names its kernel and compares bits"""

    def __init__(self, s, sc, nthreads):
        self.s, self.sc = s, sc
        self.orc = oracle_lib.Oracle(s.arenas(), nthreads=nthreads)

    def oracle(self, k=1, **opts):
        iv, ip, pos = self.s.camera()
        return self.orc.trace(self.orc.raygen(k * self.s.width, k * self.s.height, iv, ip), pos, self.sc.sun_angle, **opts)[0]

    def render(self, flags, kernel):
        self.s.render_raw(flags)
        assert self.s.last_kernel() == kernel, (self.s.last_kernel(), kernel)
        return self.s.read_output()

    def plain(self, tlas=0, what=""):
        ref = self.oracle()
        got = self.render(0, f"crt_trace_kernel<0,0,0,{tlas},0>")
        cnt = self.render(COUNT, f"crt_trace_kernel<1,0,0,{tlas},0>")
        assert np.array_equal(bits(got), bits(cnt)), (what, "uncounted != counted")
        assert np.array_equal(bits(got), bits(ref)), (what, "uncounted != oracle")
        return ref

    def flag_sets(self, what=""):
        s = self.s
        ref = self.plain(what=what)
        for flag, kern, opts in ((SHADOWS, "1,0,0", {"shadows": True}), (REFRACT, "0,0,1", {"refraction": True})):
            want = self.oracle(**opts)
            got = self.render(flag, f"crt_trace_kernel<0,0,{kern}>")
            assert np.array_equal(bits(got), bits(self.render(flag | COUNT, f"crt_trace_kernel<1,0,{kern}>"))), (what, flag)
            assert np.array_equal(bits(got), bits(want)), (what, flag)
        for k, flag in ((2, SSAA2), (4, SSAA4)):
            got = self.render(flag, "crt_trace_ssaa_kernel<0,0,0,0>")
            assert np.array_equal(bits(got), bits(resolve(self.oracle(k), k))), (what, "ssaa", k)
        got = self.render(GBUFFER, "crt_trace_gbuffer_kernel<0,0,0>")
        assert np.array_equal(bits(got), bits(ref)), (what, "gbuffer colour")
        iv, ip, pos = s.camera()
        want = gbuffer_ref.reference_planes(s.arenas(), self.orc, self.orc.raygen(s.width, s.height, iv, ip), pos)
        planes = s.read_gbuffer_raw()
        for p in ("geometry", "ids", "albedo"):
            assert np.array_equal(np.ascontiguousarray(planes[p]).view(np.uint32), np.ascontiguousarray(want[p]).view(np.uint32)), (what, p)
        got = self.render(UNORM8 | POST, "crt_trace_kernel<0,0,0,0,0>")
        assert np.array_equal(bits(got), bits(self.render(UNORM8 | POST | COUNT, "crt_trace_kernel<1,0,0,0,0>"))), (what, "unorm8|post")


def _special_cameras(s):
    """(name, position, front): inside instance 0's sphere, on a face of one of its root child boxes, at 0.95 of the smallest O_i, beyond it"""
    a = s.arenas()
    inst = a["instances"][0]
    fwd = np.linalg.inv(inst["inv"].astype(np.float64))
    k0, _ = _child_boxes(a, int(inst["meshIndex"]))
    lo, hi = k0["min"].astype(np.float64), k0["max"].astype(np.float64)
    centre = (np.append((lo + hi) / 2, 1.0) @ fwd)[:3]
    face = (np.append([hi[0], (lo[1] + hi[1]) / 2, (lo[2] + hi[2]) / 2], 1.0) @ fwd)[:3]
    lim, scene_lim, reach, _ = _cull_range(s, len(a["instances"]))
    assert scene_lim > 0
    out = np.array([0.3, 0.5, 0.8]); out /= np.linalg.norm(out)
    look = scenes._normalize(tuple(centre - out))
    return [("inside a sphere", centre + 0.05 * (face - centre), scenes._normalize((0.2, -0.1, -1.0))),
            ("on a box face", face, scenes._normalize(tuple(centre - face + np.array([0.0, 0.3, 0.0])))),
            ("0.95 of the range", out * 0.95 * scene_lim, scenes._normalize(tuple(-out))),
            ("beyond the range", out * 2.0 * scene_lim, scenes._normalize(tuple(-out))),
            ("near, oblique", centre + out * 9.0, look)], scene_lim


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["tiny", "cornell-1k"])
def test_stock_scenes_every_flag_set(name, w, h, nthreads):
    sc = scenes.get(name)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        Frames(s, sc, nthreads).flag_sets(name)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n", [16, 17])
def test_transformed_instances_and_a_single_leaf_mesh(n, w, h, tmp_path, nthreads):
    insts = _instances(n)
    insts[5] = scenes.Instance(2, 0xFFFF, scenes._trs(1.5, (0.2, 1.0, 0.1), 0.8, (1.0, 3.0, 2.0)))       # the one-triangle mesh: its root is a leaf
    sc = _scene(f"camera-cull-{n}", insts, [_one_triangle_mesh(tmp_path)])
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        a = s.arenas()
        assert len(a["instances"]) == n and a["nodes"]["triCount"][a["roots"][2]] == 1
        lim = _cull_range(s, n)[0]
        assert lim[5] == 0.0 and (lim > 0).sum() == n - 1          # the single-leaf instance is never culled, the others are cullable
        f = Frames(s, sc, nthreads)
        f.flag_sets(f"{n} instances")
        cams, scene_lim = _special_cameras(s)
        for what, pos, front in cams:
            s.set_camera(np.asarray(pos, np.float32), np.asarray(front, np.float32))
            f.plain(what=what)
            assert (np.linalg.norm(s.camera()[2].astype(np.float64)) > scene_lim) == (what == "beyond the range")
        # looking down -z: every ray of the middle column of an even-sized frame has d.x == 0 exactly
        s.set_camera((0.0, 2.0, 20.0), (0.0, 0.0, -1.0))
        iv, ip, pos = s.camera()
        assert (f.orc.raygen(w, h, iv, ip)[:, w // 2, 0] == 0.0).all()
        f.flag_sets("axis")


@pytest.mark.parametrize("w,h", SIZES)
def test_second_chunk_restages_and_the_tree_keeps_its_kernel(w, h, monkeypatch, nthreads):
    sc = _scene("camera-cull-65", _instances(65))
    monkeypatch.setenv("CRT_TLAS", "0")                                       # read by crt_init: 65 instances in the chunked loop, 64 + 1
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        f = Frames(s, sc, nthreads)
        ref = f.plain(what="65 linear")
        for what, pos, front in _special_cameras(s)[0][:2]:
            s.set_camera(np.asarray(pos, np.float32), np.asarray(front, np.float32))
            f.plain(what="65 linear, " + what)
    monkeypatch.setenv("CRT_TLAS", "1")
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        f = Frames(s, sc, nthreads)
        assert np.array_equal(bits(f.plain(tlas=1, what="65 tree")), bits(ref))


def test_row_bands_and_split_tiles(nthreads):
    sc = _scene("camera-cull-16", _instances(16))
    with driver.Session(72, 40, device=0) as s:
        s.load_scene(sc)
        f = Frames(s, sc, nthreads)
        ref = f.plain()
        for _ in range(3):                      # later frames run on lists built from the first one's costs: quadrant waves of split tiles
            assert np.array_equal(bits(f.render(0, "crt_trace_kernel<0,0,0,0,0>")), bits(ref))
        s.set_row_bands(16, 1, 2)
        part = f.render(0, "crt_trace_kernel<0,0,0,0,0>")
        own = np.array([_lib.hip().crt_row_owner(y, 16, 2) == 1 for y in range(s.height)])
        assert own.any() and np.array_equal(bits(part[own]), bits(ref[own]))
        s.set_row_bands(16, 0, 1)
        assert np.array_equal(bits(f.render(0, "crt_trace_kernel<0,0,0,0,0>")), bits(ref))


def test_frames_in_flight_with_a_moving_camera_and_an_instance_edit(monkeypatch, nthreads):
    """Six ASYNC frames over three slots, the camera moving every frame and instance 3 re-uploaded between frames 2 and 3: each frame,
    read back after crt_sync, is the synchronous frame of the same camera and instances."""
    monkeypatch.setenv("CRT_FRAMES_IN_FLIGHT", "3")
    insts = _instances(16)
    sc = _scene("camera-cull-16", insts)
    cams = [((0.5 + 0.7 * k, 7.0 - 0.4 * k, 16.0 - k), scenes._normalize((0.05 * k, -0.3, -1.0))) for k in range(6)]
    moved = insts[3].matrix.copy(); moved[3, :3] += np.array([1.2, 0.6, -0.9], np.float32)
    with driver.Session(72, 40, device=0) as s:
        s.load_scene(sc)
        got = []
        for k, (pos, front) in enumerate(cams):
            if k == 3:
                p, keep = _lib.fptr(moved)
                s.h.crth_set_mesh_matrix(3, p)
                s.render(postprocess=False, pipelined=True)                  # the mirrored Renderer uploads the dirty range before its frame
            s.set_camera(pos, front)
            s.render_raw(ASYNC)
            assert s.last_kernel() == "crt_trace_kernel<0,0,0,0,0>"
            s.sync()
            got.append(s.read_output())
        orc_after = oracle_lib.Oracle(s.arenas(), nthreads=nthreads)
        for k, (pos, front) in enumerate(cams[3:], 3):
            s.set_camera(pos, front)
            s.render_raw(0)
            sync_frame = s.read_output()
            assert np.array_equal(bits(got[k]), bits(sync_frame)), k
            iv, ip, p3 = s.camera()
            assert np.array_equal(bits(sync_frame), bits(orc_after.trace(orc_after.raygen(72, 40, iv, ip), p3, sc.sun_angle)[0])), k
    with driver.Session(72, 40, device=0) as s:                              # frames 0..2: the scene before the edit
        s.load_scene(sc)
        for k, (pos, front) in enumerate(cams[:3]):
            s.set_camera(pos, front)
            s.render_raw(0)
            assert np.array_equal(bits(got[k]), bits(s.read_output())), k
        assert not np.array_equal(bits(got[2]), bits(got[3]))
