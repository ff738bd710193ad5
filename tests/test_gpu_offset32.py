"""32-bit record offsets on scalar bases (TR_OFFSET32, crt_device.h: pair_record, tri_hot_record, tri_cold_record, big_leaf_count,
instance_record) on the device: the uncounted kernels, which take them, against the counted kernels, which keep the 64-bit addresses, and
against the oracle -- frames bit for bit, the counted launch's work counters equal to the oracle's, the kernel that ran checked by name.

The scenes are built by hand so that a wrong offset shows:
  pool ends   one mesh at offset 0 of the triangle and node pools and one at their far end: its last triangle is slot triCap - 1, its last
              sibling pair the nodes nodeCap - 2 and nodeCap - 1, i.e. pair record nodeCap / 2 - 1, the highest a valid scene can name
              (an inner node needs both children below the node count). The nodes in between are filled with unreferenced leaf nodes: the
              node pool must be valid throughout, so this one test uploads the whole node array (77 MB).
  leaf sizes  leaves of 1, 2, 127, 128 and 200 triangles (the last two through bigLeaf) side by side, a few pixels each, so that lanes of
              one 8 x 8 tile stand in leaves of different sizes; the triangles of a leaf are stacked and the LAST one is the nearest, with
              materials alternating, so a leaf whose count or whose record addresses are wrong shades another triangle. And the same
              with every leaf of one triangle.
  instances   7, 8, 64 and 65 small instances on a grid, a few pixels each: lanes of one tile enter different instances in the same step
              (load_instance's divergent path) and hit different ones (shade_bounce's). Synchronous and with frames in flight.
  row bands   the leaf-size scene as rank 1 of 2.
Frames of 64 x 64 and 72 x 40 (partial tiles at both edges), 128 x 72 for the instance grids. Every non-vacuity claim above is asserted on the oracle's hit records."""
import ctypes as C
import functools

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import deep_stack_ref as ds
import gbuffer_ref
import oracle_lib
from test_gpu_ssaa import resolve
from util import bits

pytestmark = pytest.mark.gpu

ASYNC, COUNT, SHADOWS, REFRACT, SSAA2, GBUFFER = 4, 8, 32, 256, 2048, 8192
TRI_CAP = NODE_CAP = 2 * 1200000          # CRT_MAX_TRIANGLES * 2 (tests/test_offset32_cpu.py reads them from the sources)
SUN = scenes.get("tiny").sun_angle
CAMERA = ((0.2, 0.1, -20.0), (0.0, 0.0, 1.0))          # a 1.6-unit cell is about 5 pixels of a 64 x 64 frame, 3 of a 72 x 40 one
GRID_CAMERA = ((0.2, 0.1, -27.0), (0.0, 0.0, 1.0))     # the instance grids: a pitch of 2.2 units is about 6 pixels of a 128 x 72 frame
MIXED = (1, 2, 127, 128, 2, 200, 1, 127)   # leaf sizes of the mixed mesh: 128 and 200 go through bigLeaf
ONES = (1,) * 8


def half(x):
    return np.asarray(x, np.float16).view(np.uint16)


def grid_mesh(counts, cell, cols=4, depth=0.4):
    """(tris, leaves): leaf j covers cell (j % cols, j // cols) of a grid in the xy plane centred on the origin; its triangles are stacked
    along z, each nearer to a camera on the -z side than the one before. leaves = [(first, count)]"""
    total = sum(counts)
    tris = np.zeros(total, _lib.TRI_DTYPE)
    leaves, k = [], 0
    rows = (len(counts) + cols - 1) // cols
    for j, n in enumerate(counts):
        x0, y0 = (j % cols - cols / 2.0) * cell, (j // cols - rows / 2.0) * cell
        leaves.append((k, n))
        for i in range(n):
            z = -depth * (i + 1) / n
            tris["v0"][k] = (x0, y0, z); tris["v1"][k] = (x0 + cell, y0, z + 0.01); tris["v2"][k] = (x0 + 0.5 * cell, y0 + cell, z + 0.02)
            tris["uv"][k] = half([0, 0, 1, 0, 0.5, 1])
            tris["mat"][k] = (i + j) % 2
            tris["n"][k] = half([0, 0, -1] * 3)
            k += 1
    c = (tris["v0"] + tris["v1"] + tris["v2"]) * np.float32(0.333333)
    tris["cx"], tris["cy"], tris["cz"] = c[:, 0], c[:, 1], c[:, 2]
    return tris, leaves


def build_nodes(tris, leaves, node_base, tri_base):
    """a median-split tree over `leaves` in their order: the root at node_base, every sibling pair adjacent and behind its parent"""
    assert len(leaves) >= 2
    out = [None]

    def box(ls):
        v = np.concatenate([tris[f][a:a + n] for a, n in ls for f in ("v0", "v1", "v2")])
        return v.min(0), v.max(0)

    def fill(idx, ls):
        lo, hi = box(ls)
        if len(ls) == 1:
            out[idx] = (lo, hi, tri_base + ls[0][0], ls[0][1])
            return
        l = len(out)
        out.extend([None, None])
        out[idx] = (lo, hi, node_base + l, 0)
        fill(l, ls[:len(ls) // 2]); fill(l + 1, ls[len(ls) // 2:])

    fill(0, leaves)
    nodes = np.zeros(len(out), _lib.NODE_DTYPE)
    for i, (lo, hi, lf, tc) in enumerate(out):
        nodes["min"][i], nodes["max"][i], nodes["leftFirst"][i], nodes["triCount"][i] = lo, hi, lf, tc
    return nodes


def instance_records(placements):
    """placements: [(mesh, angle about z, translation)] -> INSTANCE_DTYPE records (inverse transforms, row-vector convention)"""
    inst = np.zeros(len(placements), _lib.INSTANCE_DTYPE)
    for k, (mesh, angle, t) in enumerate(placements):
        f = np.eye(4)
        f[0, 0], f[0, 1], f[1, 0], f[1, 1] = np.cos(angle), np.sin(angle), -np.sin(angle), np.cos(angle)
        f[3, :3] = t
        inst["inv"][k] = np.linalg.inv(f).astype(np.float32)
        inst["meshIndex"][k], inst["materialStart"][k] = mesh, 0
    return inst


def assemble(meshes, placements, far_last=False):
    """the arenas of `meshes` = [(tris, leaves)] packed from offset 0 (far_last: the last one at the far end of both pools, the node
    pool valid in between) and the (tri_base, count) spans to upload"""
    a = dict(ds._tiny_arenas())
    spans, node_parts, roots = [], [], []
    tri_at = node_at = 0
    for m, (tris, leaves) in enumerate(meshes):
        n_nodes = 2 * len(leaves) - 1
        if far_last and m == len(meshes) - 1:
            tri_at, node_far = TRI_CAP - len(tris), NODE_CAP - n_nodes
            filler = np.zeros(node_far - node_at, _lib.NODE_DTYPE)
            filler["triCount"] = 1                         # unreferenced leaf nodes: valid, never visited
            node_parts.append(filler)
            node_at = node_far
        nodes = build_nodes(tris, leaves, node_at, tri_at)
        roots.append(node_at)
        spans.append((tri_at, tris))
        node_parts.append(nodes)
        tri_at += len(tris)
        node_at += len(nodes)
        if node_at % 2:                                    # the next mesh's pairs keep this one's parity: no two share a pair record
            pad = np.zeros(1, _lib.NODE_DTYPE); pad["triCount"] = 1
            node_parts.append(pad); node_at += 1
    all_tris = np.zeros(max(first + len(t) for first, t in spans), _lib.TRI_DTYPE)
    for first, t in spans:
        all_tris[first:first + len(t)] = t
    a.update(tris=all_tris, nodes=np.concatenate(node_parts), roots=np.array(roots, np.uint32), instances=instance_records(placements))
    for v in a.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return a, spans


@functools.lru_cache(maxsize=None)
def scene(name):
    """(arenas, spans) by name; computed once, never modified"""
    if name == "pool-ends":
        near, far = grid_mesh(MIXED, 1.6), grid_mesh(MIXED[::-1], 1.6)
        return assemble([near, far], [(0, 0.0, (-4.0, 0.3, 0.0)), (1, 0.3, (4.0, -0.2, 1.0)), (1, 1.1, (0.0, 5.0, 2.0)), (0, 2.0, (0.5, -5.0, 3.0))], far_last=True)
    if name in ("mixed", "ones"):
        m = grid_mesh(MIXED if name == "mixed" else ONES, 1.6)
        return assemble([m, grid_mesh((2, 1) if name == "mixed" else (1, 1), 1.6, cols=2)], [(0, 0.0, (-3.5, 2.0, 0.0)), (0, 0.7, (3.5, -2.0, 1.0)), (1, 0.2, (0.0, 0.0, 2.0))])
    n = int(name)
    small = [grid_mesh((1, 2), 0.8, cols=2), grid_mesh((3, 1, 1), 0.8, cols=3)]
    per_row = int(np.ceil(np.sqrt(n)))
    return assemble(small, [(k % 2, 0.4 * k, ((k % per_row - (per_row - 1) / 2.0) * 2.2, (k // per_row - (per_row - 1) / 2.0) * 2.2, 0.1 * (k % 7))) for k in range(n)])


@functools.lru_cache(maxsize=None)
def reference(name, w, h, camera=CAMERA, what="plain"):
    """the oracle's frame and work counters (or first-hit planes, or hit records) of a scene from a camera: computed once, never modified"""
    a = scene(name)[0]
    orc = oracle_lib.Oracle(a, nthreads=16)
    iv, ip, pos = ds.camera_of(w, h, camera)
    if what == "hi":
        return orc.trace(orc.raygen(2 * w, 2 * h, iv, ip), pos, SUN)
    rays = orc.raygen(w, h, iv, ip)
    if what == "planes":
        return gbuffer_ref.reference_planes(a, orc, rays, pos)
    if what == "hits":
        d = rays.reshape(-1, 3)
        return orc.closest_hits(np.tile(np.asarray(pos, np.float32), (len(d), 1)), d)[0]
    return orc.trace(rays, pos, SUN, shadows=what == "shadows", refraction=what == "refraction")


def full_tiles(x, w, h):
    """per-pixel values as (tiles, 64) over the frame's full 8 x 8 tiles"""
    th, tw = h // 8, w // 8
    return np.asarray(x).reshape(h, w)[:th * 8, :tw * 8].reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(th * tw, 64)


def leaf_sizes_per_pixel(name, w, h):
    """the triangle count of the leaf each pixel's closest hit lies in (0: a miss)"""
    a = scene(name)[0]
    hits = reference(name, w, h, what="hits")
    size_of = np.zeros(len(a["tris"]), np.int64)
    leafs = a["nodes"][a["nodes"]["triCount"] > 0]
    for first, n in zip(leafs["leftFirst"], leafs["triCount"]):
        size_of[first:first + n] = np.maximum(size_of[first:first + n], n)
    return np.where(hits["instance"] >= 0, size_of[hits["tri"]], 0), hits


def session(w, h, name, monkeypatch, in_flight=None):
    monkeypatch.delenv("CRT_KERNEL", raising=False)
    monkeypatch.delenv("CRT_TLAS", raising=False)
    if in_flight:
        monkeypatch.setenv("CRT_FRAMES_IN_FLIGHT", str(in_flight))
    s = driver.Session(w, h, device=0)
    s.load_scene(scenes.get("tiny"))                        # materials, textures, skybox
    a, spans = scene(name)
    hip = s.hip
    for first, tris in spans:
        t = np.array(tris)
        assert hip.crt_upload_triangles(t.ctypes.data, first * t.itemsize, t.nbytes) == 0
    roots, nodes, inst = np.array(a["roots"]), np.array(a["nodes"]), np.array(a["instances"])
    assert hip.crt_upload_bvh_roots(roots.ctypes.data, 0, len(roots)) == 0
    assert hip.crt_upload_bvh_nodes(nodes.ctypes.data, 0, nodes.nbytes) == 0
    assert hip.crt_upload_instances(inst.ctypes.data, 0, len(inst)) == 0
    return s, len(inst)


def frame(s, ni, flags, camera=CAMERA):
    args, iv, ip, _ = ds.frame_args(s, ni, SUN, camera)
    assert ds.render(s, args, iv, ip, flags) == 0
    return s.last_kernel()


def check_plain(s, ni, name, w, h, camera=CAMERA):
    """uncounted == counted == oracle, counters == oracle's; returns the kernel's instance-tree digit"""
    ref, st = reference(name, w, h, camera)
    k0 = frame(s, ni, 0, camera)
    got = s.read_output()
    k1 = frame(s, ni, COUNT, camera)
    cnt = s.read_output()
    assert k0.startswith("crt_trace_kernel<0,0,0,") and k1 == k0.replace("<0,", "<1,", 1), (k0, k1)
    assert np.array_equal(bits(got), bits(cnt)), (name, "uncounted != counted")
    assert np.array_equal(bits(got), bits(ref)), (name, "uncounted != oracle")
    assert s.counters() == st, name
    return k0.split(",")[3]


def check_flag_sets(s, ni, name, w, h):
    tlas = check_plain(s, ni, name, w, h)
    for flag, what, kern in ((SHADOWS, "shadows", f"1,{tlas},0"), (REFRACT, "refraction", f"0,{tlas},1")):
        ref, st = reference(name, w, h, what=what)
        assert frame(s, ni, flag) == f"crt_trace_kernel<0,0,{kern}>"
        got = s.read_output()
        assert frame(s, ni, flag | COUNT) == f"crt_trace_kernel<1,0,{kern}>"
        assert np.array_equal(bits(got), bits(s.read_output())), (name, what, "uncounted != counted")
        assert np.array_equal(bits(got), bits(ref)), (name, what)
        assert s.counters() == st, (name, what)
    hi, st = reference(name, w, h, what="hi")
    assert frame(s, ni, SSAA2) == f"crt_trace_ssaa_kernel<0,0,{tlas},0>"
    got = s.read_output()
    assert frame(s, ni, SSAA2 | COUNT) == f"crt_trace_ssaa_kernel<1,0,{tlas},0>"
    assert np.array_equal(bits(got), bits(s.read_output())) and np.array_equal(bits(got), bits(resolve(hi, 2))), (name, "ssaa")
    assert s.counters() == st, (name, "ssaa")
    assert frame(s, ni, GBUFFER) == f"crt_trace_gbuffer_kernel<0,{tlas},0>"
    assert np.array_equal(bits(s.read_output()), bits(reference(name, w, h)[0])), (name, "gbuffer colour")
    planes, want = s.read_gbuffer_raw(), reference(name, w, h, what="planes")
    for p in ("geometry", "ids", "albedo"):
        assert np.array_equal(np.ascontiguousarray(planes[p]).view(np.uint32), np.ascontiguousarray(want[p]).view(np.uint32)), (name, p)


def check_device_queries(s, ni, name, w, h):
    """the queries on device buffers take the option too: closest hits of the frame's rays against the oracle's records"""
    iv, ip, pos = ds.camera_of(w, h, CAMERA)
    orc = oracle_lib.Oracle(scene(name)[0], nthreads=16)
    d = orc.raygen(w, h, iv, ip).reshape(-1, 3)
    o = np.tile(np.asarray(pos, np.float32), (len(d), 1))
    got = ds.records(ds.trace_rays(s, ni, ds.dev(o), ds.dev(d)))
    want = reference(name, w, h, what="hits")
    hit = want["instance"] >= 0
    assert hit.sum() > 100 and np.array_equal(got["instance"], want["instance"])
    for f in ("t", "u", "v", "tri"):
        assert np.array_equal(got[f][hit].view(np.uint32), want[f][hit].view(np.uint32)), (name, f)


def test_meshes_at_both_ends_of_the_pools(monkeypatch):
    w, h = 64, 64
    a = scene("pool-ends")[0]
    # the scene is what it says: the far mesh's last triangle and last sibling pair are the pools' last, the near mesh starts at 0
    assert len(a["tris"]) == TRI_CAP and len(a["nodes"]) == NODE_CAP and list(a["roots"])[0] == 0
    inner = a["nodes"][a["nodes"]["triCount"] == 0]
    assert inner["leftFirst"].max() == NODE_CAP - 2 and (inner["leftFirst"].max() >> 1) == NODE_CAP // 2 - 1 and inner["leftFirst"].min() == 1
    hits = reference("pool-ends", w, h, what="hits")
    seen = hits["tri"][hits["instance"] >= 0]
    assert (seen == TRI_CAP - 1).any() and (seen < 600).any() and (seen > TRI_CAP - 600).any()      # the last slot is the nearest triangle of its leaf
    assert set(np.unique(hits["instance"])) >= {0, 1, 2, 3}
    s, ni = session(w, h, "pool-ends", monkeypatch)
    with s:
        check_flag_sets(s, ni, "pool-ends", w, h)
        check_device_queries(s, ni, "pool-ends", w, h)


@pytest.mark.parametrize("w,h", [(64, 64), (72, 40)])
@pytest.mark.parametrize("name", ["mixed", "ones"])
def test_leaf_sizes_mixed_inside_a_tile(name, w, h, monkeypatch):
    sizes, hits = leaf_sizes_per_pixel(name, w, h)
    tiles = full_tiles(sizes, w, h)
    if name == "mixed":
        assert set(np.unique(sizes)) >= {1, 2, 127, 128, 200}
        assert any(len(set(t[t > 0])) >= 3 and (t >= 128).any() and (t == 127).any() for t in tiles), "no tile mixes three leaf sizes around the bigLeaf escape"
        assert any((t == 1).any() and (t >= 128).any() for t in tiles)
    else:
        assert set(np.unique(sizes)) == {0, 1} and (tiles == 1).any(1).sum() >= 4
    s, ni = session(w, h, name, monkeypatch)
    with s:
        check_flag_sets(s, ni, name, w, h)
        if (w, h) == (64, 64):
            check_device_queries(s, ni, name, w, h)


@pytest.mark.parametrize("n", [7, 8, 64, 65])
def test_lanes_of_a_tile_enter_different_instances(n, monkeypatch):
    w, h = 128, 72
    name = str(n)
    camera = GRID_CAMERA
    hits = reference(name, w, h, camera, "hits")
    tiles = full_tiles(hits["instance"], w, h)
    assert any(len(set(t[t >= 0])) >= 3 for t in tiles), "no tile whose lanes hit three different instances"
    assert len(set(hits["instance"][hits["instance"] >= 0])) >= min(n, 40)
    # every reference before the session: its camera comes from a host-only session, and the host mirror holds one session at a time
    moved = [((camera[0][0] + 0.9 * k, camera[0][1] - 0.6 * k, camera[0][2] + k), (0.03 * k, -0.02 * k, 1.0)) for k in range(1, 3)]
    ref = reference(name, w, h, camera)[0]
    moved_refs = [reference(name, w, h, cam)[0] for cam in moved]
    s, ni = session(w, h, name, monkeypatch, in_flight=3)
    with s:
        assert ni == n
        tlas = check_plain(s, ni, name, w, h, camera)
        # frames in flight: three submitted back to back on three slots, then one at a time from moved cameras
        for _ in range(3):
            assert frame(s, ni, ASYNC, camera) == f"crt_trace_kernel<0,0,0,{tlas},0>"
        s.sync()
        assert np.array_equal(bits(s.read_output()), bits(ref)), (n, "in flight")
        for k, (cam, want) in enumerate(zip(moved, moved_refs)):
            assert frame(s, ni, ASYNC, cam) == f"crt_trace_kernel<0,0,0,{tlas},0>"
            s.sync()
            assert np.array_equal(bits(s.read_output()), bits(want)), (n, "in flight, camera", k)


def test_row_bands(monkeypatch):
    w, h = 72, 40
    ref = reference("mixed", w, h)[0]
    s, ni = session(w, h, "mixed", monkeypatch)
    with s:
        check_plain(s, ni, "mixed", w, h)
        s.set_row_bands(16, 1, 2)
        assert frame(s, ni, 0) == "crt_trace_kernel<0,0,0,0,0>"
        part = s.read_output()
        own = np.array([_lib.hip().crt_row_owner(y, 16, 2) == 1 for y in range(h)])
        assert own.any() and not own.all() and np.array_equal(bits(part[own]), bits(ref[own]))
        s.set_row_bands(16, 0, 1)
        assert frame(s, ni, 0) == "crt_trace_kernel<0,0,0,0,0>"
        assert np.array_equal(bits(s.read_output()), bits(ref))
