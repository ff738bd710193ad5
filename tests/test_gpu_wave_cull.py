"""The wave test of the staged instance cull on the device (crt_device.h: wave_cone, cone_rejects -- one test per instance and wave against the
tile's ray cone, in front of the per-lane loop): the uncounted Trace kernels, which take it, against the counted kernels, which do not, and
against the oracle, which has no cull at all -- bit for bit, with the kernel that ran checked by name for every frame.

Scene `tiny`'s meshes as 16, 17 and 65 small instances (65 with CRT_TLAS=0: two 64-chunks, which take no wave test -- the same frames all the same) at 64x64, 72x40 and 203x117 (partial tiles at
the edges: waves that take no wave test). The instances are placed so that their cull spheres graze tile cones: the cone of a tile has its
axis on the tile's first pixel and reaches to the opposite corner's ray; instance k sits on the far side of that corner ray, its sphere's
centre at 0.98, 0.999, 1.001 or 1.02 of the angle at which the sphere touches the cone -- just inside and just outside.
Flags 0, shadow rays, refraction, SSAA 2 and 4, the G-buffer (Frames.flag_sets of tests/test_gpu_camera_cull.py); frames in flight, row
bands and split tiles; cameras far beyond the cull's range and inside an instance's sphere; a frame whose middle column has NaN directions."""
import os
import sys

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import gbuffer_ref
import oracle_lib
from test_gpu_camera_cull import ASYNC, COUNT, Frames, _scene, _special_cameras
from util import bits

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from count_box_pretest import table_sphere      # noqa: E402  (fl(c), w) of crt_instances.h, restated

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (72, 40), (203, 117)]
GRAZE = (0.98, 0.999, 1.001, 1.02)


def _spheres(arenas):
    """the table's (c, w) of every instance, from the arenas (float64 centre, float32 radius)"""
    out = []
    for inst in arenas["instances"]:
        node = arenas["nodes"][int(arenas["roots"][inst["meshIndex"]])]
        assert node["triCount"] == 0
        kids = arenas["nodes"][int(node["leftFirst"]):int(node["leftFirst"]) + 2]
        fwd = np.linalg.inv(np.ascontiguousarray(inst["inv"], np.float32).astype(np.float64))
        lo = np.minimum(kids[0]["min"], kids[1]["min"]).astype(np.float64)
        hi = np.maximum(kids[0]["max"], kids[1]["max"]).astype(np.float64)
        c, _, w = table_sphere(lo, hi, fwd)
        out.append((c, float(w)))
    return out


def _matrices(n):
    return [scenes._trs(0.08 + 0.03 * (k % 5), (0.3 + 0.1 * (k % 4), 1.0, 0.2 * (k % 5) - 0.4), 0.37 * k, (0.0, 0.0, 0.0)).astype(np.float32) for k in range(n)]


def grazing_scene(n, w, h, nthreads):
    """n instances whose cull spheres graze the cones of tiles spread over the w x h frame of _scene's camera"""
    ms = _matrices(n)
    probe = _scene(f"wave-cull-probe-{n}", [scenes.Instance(k % 2, 0xFFFF, m) for k, m in enumerate(ms)])
    with driver.Session(w, h, host_only=True) as s:
        s.load_scene(probe)
        a = s.arenas()
        iv, ip, pos = s.camera()
        rays = np.asarray(oracle_lib.Oracle(a, nthreads=nthreads).raygen(w, h, iv, ip), np.float64).reshape(h, w, 3)
        spheres = _spheres(a)                  # at the origin: the centre's offset from the translation, and w
    tx, ty = w // 8, h // 8
    insts = []
    for k, m in enumerate(ms):
        i, j = (k * 5 + 1) % tx, (k * 3 + k // tx) % ty
        axis, far = rays[8 * j, 8 * i], rays[8 * j + 7, 8 * i + 7]
        side = far - (far @ axis) * axis
        side /= np.linalg.norm(side)
        theta = np.arccos(np.clip(axis @ far, -1, 1))
        off, wk = spheres[k]
        x = 9.0 + 1.7 * (k % 11)
        psi = np.arcsin(np.sqrt(1.0201 * wk * wk + 4e-6 * x * x) / x)
        ang = (theta + psi) * GRAZE[k % 4]
        centre = pos.astype(np.float64) + (np.cos(ang) * axis + np.sin(ang) * side) * x
        m = m.copy(); m[3, :3] = (centre - off).astype(np.float32)
        insts.append(scenes.Instance(k % 2, 0xFFFF, m))
    return _scene(f"wave-cull-{n}-{w}x{h}", insts)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n", [16, 17, 65])
def test_grazing_instances_every_flag_set(n, w, h, monkeypatch, nthreads):
    if n > 64:
        monkeypatch.setenv("CRT_TLAS", "0")                                   # read by crt_init: the chunked loop, 64 + 1
    sc = grazing_scene(n, w, h, nthreads)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        assert len(s.arenas()["instances"]) == n
        f = Frames(s, sc, nthreads)
        # not vacuous: of each grazing class (0.98, 0.999, 1.001, 1.02) some instance is the first hit of pixels of the oracle's frame, so a
        # wrongly rejected one changes the frame
        iv, ip, pos = s.camera()
        ids = np.ascontiguousarray(gbuffer_ref.reference_planes(s.arenas(), f.orc, f.orc.raygen(w, h, iv, ip), pos)["ids"]).view(np.uint32).reshape(-1, 4)[:, 0]
        seen = np.unique(ids[ids != 0xFFFFFFFF])
        assert all((seen % 4 == g).any() for g in range(4)), seen
        f.flag_sets(f"{n} grazing instances, {w}x{h}")


@pytest.mark.parametrize("w,h", SIZES[1:])
def test_special_cameras_and_nan_directions(w, h, nthreads):
    sc = grazing_scene(16, w, h, nthreads)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        f = Frames(s, sc, nthreads)
        cams, scene_lim = _special_cameras(s)
        for what, pos, front in cams:
            s.set_camera(np.asarray(pos, np.float32), np.asarray(front, np.float32))
            f.plain(what=what)
            assert (np.linalg.norm(s.camera()[2].astype(np.float64)) > scene_lim) == (what == "beyond the range")
        # RayGen with invProj = identity and invView = one row: dir = normalize((2 cx, 0, 0)) -- +-x, and NaN where cx == 0
        iv = np.zeros((4, 4), np.float32); iv[0, 0] = 2.0
        ip = np.eye(4, dtype=np.float32)
        pos = np.array([-30.0, 7.0, 2.0], np.float32)
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


def test_row_bands_split_tiles_and_frames_in_flight(monkeypatch, nthreads):
    monkeypatch.setenv("CRT_FRAMES_IN_FLIGHT", "3")
    w, h = 72, 40
    sc = grazing_scene(16, w, h, nthreads)
    with driver.Session(w, h, device=0) as s:
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
