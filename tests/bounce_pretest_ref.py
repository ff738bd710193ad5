"""What the tests of the reflection bounce's root pre-test (crt_device.h: bounce_pretest_mask) share, all of it on the CPU: the scene -- small
instances over a reflecting floor, placed so that rays reflected off the floor graze root child boxes -- and the per-wave view of the pre-test
from the restatements of tools/count_bounce_pretest.py (the bounce ray, the cull, the root step with one origin per lane).

The floor is an instance with the identity transform (the bounce ray starts in the hit instance's object space, hazard H6: here that is world space) of
a slightly wavy grid (a flat one has boxes without volume, which upstream's slab test never enters). Instance 0 is the floor, instance 3 a
one-triangle mesh (its root is a leaf: never cleared), every other one an instance of scene `tiny`'s two meshes, scaled to a few tenths of a unit."""
import os
import sys

import numpy as np

from clraytracer_amd import driver, scenes
import oracle_lib
from test_gpu_camera_cull import _one_triangle_mesh, _scene
from test_gpu_wave_cull import _matrices

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import count_bounce_pretest as tool  # noqa: E402

F = np.float32
GRAZE = (-1e-3, 1e-3)            # the reflected ray passes the box's extreme corner this far (x the distance along the ray) inside or outside


def _floor_mesh(tmp):
    g = scenes._grid((-40, 0, 24), (80, 0, 0), (0, 0, -80), 8, 8, (0, 1, 0))
    g.pos[:, 1] = (0.05 * np.sin(1.3 * g.pos[:, 0]) * np.cos(0.7 * g.pos[:, 2])).astype(F)
    return scenes._write_mesh(str(tmp), "floor", g, [((0.7, 0.7, 0.75), None)])


def _child_corners(arenas, mesh, m):
    """the eight corners of the first root child box of mesh `mesh` under the linear part of m (row vectors), float64"""
    node = arenas["nodes"][int(arenas["roots"][mesh])]
    kid = arenas["nodes"][int(node["leftFirst"])]
    lo, hi = kid["min"].astype(np.float64), kid["max"].astype(np.float64)
    pts = np.array([[hi[0] if c & 1 else lo[0], hi[1] if c & 2 else lo[1], hi[2] if c & 4 else lo[2]] for c in range(8)])
    return pts @ np.asarray(m, np.float64)[:3, :3]


def bounce_of_frame(arenas, orc, w, h, iv, ip, pos):
    """(alive, o', d') of the w x h frame: tool.bounce_rays on the oracle's primary hits"""
    rays = np.ascontiguousarray(orc.raygen(w, h, iv, ip), F).reshape(-1, 3)
    cam = np.asarray(pos, F)
    hits, _ = orc.closest_hits(np.broadcast_to(cam, rays.shape), rays)
    return tool.bounce_rays(arenas, cam, rays, hits)


def floor_scene(n, w, h, nthreads, tmp_path):
    """n instances: the floor, the one-triangle mesh and n - 2 small ones, each with the extreme corner of its first root child box on a ray the
    floor reflects (of pixels spread over the frame), GRAZE inside or outside"""
    meshes = [_floor_mesh(tmp_path), _one_triangle_mesh(tmp_path)]           # meshes 2 and 3 behind `tiny`'s two
    floor = scenes.Instance(2, 0xFFFF, np.eye(4, dtype=F))
    with driver.Session(w, h, host_only=True) as s:
        s.load_scene(_scene(f"bounce-pretest-probe-{w}x{h}", [floor], meshes))
        a = s.arenas()
        iv, ip, pos = s.camera()
        alive, o1, d1 = bounce_of_frame(a, oracle_lib.Oracle(a, nthreads=nthreads), w, h, iv, ip, pos)
        ms = _matrices(n)
        corners = [_child_corners(a, k % 2, ms[k]) for k in range(n)]
    assert alive.sum() >= n, "the floor fills too little of the frame"
    o1, d1 = o1.astype(np.float64), d1.astype(np.float64)
    insts, small = [], 0
    for k in range(n):
        if k == 0:
            insts.append(floor); continue
        if k == 3:
            insts.append(scenes.Instance(3, 0xFFFF, scenes._trs(1.5, (0.2, 1.0, 0.1), 0.8, (1.0, 3.0, 2.0)))); continue
        r = (small + 1) * len(o1) // (n - 1)                                # a reflected ray: the pixels spread over the floor's part of the frame
        small += 1
        x = 2.5 + 0.45 * (k % 7)
        side = np.cross(d1[r], (0.3 + 0.1 * (k % 3), 1.0, 0.2))
        side /= np.linalg.norm(side)
        c = corners[k][np.argmin(corners[k] @ side)]                         # the box lies on the +side side of this corner
        m = ms[k].copy(); m[3, :3] = (o1[r] + x * d1[r] - c + GRAZE[k % 2] * x * side).astype(F)
        insts.append(scenes.Instance(k % 2, 0xFFFF, m))
    return _scene(f"bounce-pretest-{n}-{w}x{h}", insts, meshes)


def wave_view(arenas, orc, w, h, iv, ip, pos):
    """(alive, o', d', sphere, useful) of the frame's bounce rays: tool.instance_masks' (rays, instances) masks -- the entries candidate_mask lets
    through and those of them the pre-test keeps"""
    alive, o1, d1 = bounce_of_frame(arenas, orc, w, h, iv, ip, pos)
    sph, use = tool.instance_masks(arenas, o1, d1)
    return alive, o1, d1, sph, use


def mixed_waves(alive, sph, use, w, h):
    """how many full 8 x 8 tiles hold a small instance (not the floor, whose boxes every bounce ray starts in) that the cull keeps for lanes the
    pre-test clears AND for lanes it keeps"""
    sph, use = sph[:, 1:], use[:, 1:]
    nI = sph.shape[1]
    th, tw = h // 8, w // 8

    def tiles(rows):
        frame = np.zeros((h * w, nI), bool)
        frame[alive] = rows
        return frame.reshape(h, w, nI)[:th * 8, :tw * 8].reshape(th, 8, tw, 8, nI).transpose(0, 2, 1, 3, 4).reshape(th * tw, 64, nI)
    cleared, kept = tiles(sph & ~use), tiles(use)
    return int((cleared.any(1) & kept.any(1)).any(1).sum())
