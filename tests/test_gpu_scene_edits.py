"""Scene edits in a live session, on the GPU: a mesh pushed after frames were rendered, a mesh's triangles and nodes overwritten in place,
texels written in pieces, one material record replaced, all of it against frames in flight and in seeded sequences. Every other GPU test
loads its scene once; these render from pools that changed under a session that had already rendered.

The criterion is the suite's: raw frames bit for bit, work counters equal and query records byte for byte against oracle_lib.Oracle on the
arenas the session now describes -- Session.arenas() for edits through the mirror, tests/scene_edit_ref.py's composed arenas for edits through
the C-ABI (tests/test_scene_edits_cpu.py pins those helpers without a GPU). No tolerance anywhere. Frames are 96 x 64 (one ragged 113 x 70).

What an edit can leave stale, and the case that looks at it:
    root references in the slots' and the ray queries' instance records, the tree-top table's share per mesh    (a) append
    per-instance cull bounds and the instance tree over cached root boxes                                        (b) grow / shrink
    the big-leaf table, the node high-water mark                                                                 (b) leaves / smaller tree
    a texel word made from bytes that were replaced (crt_upload_texels redid whole texels from the span's first
    byte only: the texel a span ENDS in kept its old word -- found by (c) overwrite and (c) pieces[shuffled], fixed) (c)
    frames in flight over a pool being overwritten                                                               (e)"""
import ctypes as C
import itertools

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import ao_ref
import gbuffer_ref
import oracle_lib
import scene_edit_ref as E
import shade_ref
import texel_ref as T
from util import bits

pytestmark = pytest.mark.gpu

ASYNC, COUNT, SHADOWS, READBACK, REFRACTION, GBUFFER = E.ASYNC, E.COUNT, E.SHADOWS, E.READBACK, E.REFRACTION, E.GBUFFER
W, H = E.W, E.H
KERNEL_OF = {None: "crt_trace_kernel<", "ldstop": "crt_trace_ldstop_kernel<"}
SUN = -1.96
AO_RADIUS, AO_BIAS = 16.0, 1e-3


def set_env(monkeypatch, kernel=None, tlas=None):
    for k, v in (("CRT_KERNEL", kernel), ("CRT_TLAS", tlas), ("CRT_RAYS_GRID", None)):
        monkeypatch.delenv(k, raising=False)
        if v is not None:
            monkeypatch.setenv(k, v)                            # read by crt_init


def expected(a, s, nthreads, flags=0, view=None, sun=SUN):
    """the oracle's (frame, counters) for arenas `a` under the session's camera (or `view`) and size"""
    iv, ip, pos = view if view is not None else s.camera()
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    return orc.trace(orc.raygen(s.width, s.height, iv, ip), pos, sun, shadows=bool(flags & SHADOWS), refraction=bool(flags & REFRACTION))


def check_frame(s, a, nthreads, flags=COUNT, view=None, what=""):
    """one frame with `flags`: its bits and (when counted) its counters are the oracle's on `a`; -> the frame"""
    s.render_raw(flags, sun_angle=SUN, view=view)
    got = s.read_output()
    want, st = expected(a, s, nthreads, flags, view)
    differ = int((bits(got) != bits(want)).any(axis=2).sum())
    assert differ == 0, (what, flags, f"{differ} of {got.shape[0] * got.shape[1]} pixels differ from the oracle")
    if flags & COUNT:
        cnt = s.counters()
        assert cnt == st, (what, {k: (cnt[k], st[k]) for k in st if cnt[k] != st[k]})
    return got


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")


def render_rc(s, flags):
    a, iv, ip = s.trace_args(SUN)
    fp = C.POINTER(C.c_float)
    return s.hip.crt_render(C.byref(a), iv.ctypes.data_as(fp), ip.ctypes.data_as(fp), int(flags))


def downloaded(hip, a):
    """the device's reference-layout pools over the extent of arenas `a`"""
    t, n, r = np.zeros(len(a["tris"]), _lib.TRI_DTYPE), np.zeros(len(a["nodes"]), _lib.NODE_DTYPE), np.zeros(len(a["roots"]), np.uint32)
    assert hip.crt_download_triangles(t.ctypes.data, 0, t.nbytes) == 0 and hip.crt_download_bvh_nodes(n.ctypes.data, 0, n.nbytes) == 0
    assert hip.crt_download_bvh_roots(r.ctypes.data, 0, len(r)) == 0
    return t, n, r


# ------------------------------------------------------------------------------------------------
# (a) append through the mirror
# ------------------------------------------------------------------------------------------------
def check_queries(s, a, sc, nthreads):
    """trace_rays (closest, occluded), shade_rays (radiance, surface) and trace_ao (8 samples) over one 256-ray batch: these read root references
    through slot tables of their own (the ray queries' context), not a frame slot's"""
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    o, d = E.query_batch(a, sc.camera_pos)
    rec, _ = orc.closest_hits(o, d)
    on_b = int((a["instances"]["meshIndex"][np.maximum(rec["instance"], 0)] == 1)[rec["instance"] >= 0].sum())
    assert len(o) == 256 and on_b >= 64, on_b                                # at least a quarter of the batch ends on the appended mesh
    to, td = dev(o), dev(d)
    assert s.trace_rays(to, td).numpy().tobytes() == rec.tobytes()
    assert np.array_equal(s.trace_rays(to, td, mode="occluded").cpu().numpy(), rec["instance"] >= 0)
    rad, surf = s.shade_rays(to, td, sun_angle=SUN, surface=True)
    assert shade_ref.same_surface(surf.numpy(), shade_ref.surface(a, orc, o, d))
    assert np.array_equal(bits(rad.cpu().numpy()), bits(shade_ref.radiance(orc, o, d, SUN)))
    # ambient occlusion at the batch's hit points (a miss: the camera with a zero normal, which traces nothing)
    geometry, _, _ = gbuffer_ref.planes_from_records(a, rec)
    hit = (rec["instance"] >= 0) & ~(rec["t"] > gbuffer_ref.INF_MINUS_ONE)
    P = (o + d * rec["t"][:, None]).astype(np.float32)
    n = np.ascontiguousarray(geometry["normal"], np.float32).copy()
    P[~hit], n[~hit] = np.asarray(sc.camera_pos, np.float32), 0.0
    par = {"samples": 8, "radius": AO_RADIUS, "bias": AO_BIAS, "seed": 0}
    ro, rd, w = ao_ref.rays(P, n, np.arange(len(P), dtype=np.uint32), par, ao_ref.table())
    arec, _ = orc.closest_hits(np.repeat(ro, 8, axis=0), rd.reshape(-1, 3))
    assert np.isfinite(arec["u"]).all() and np.isfinite(arec["v"]).all()     # the precondition of "occluded = the unbounded record's t < radius"
    occ = ((arec["instance"] >= 0) & (arec["t"] < np.float32(AO_RADIUS))).reshape(len(P), 8)
    assert 0.02 <= occ[hit].mean() <= 0.98
    got = s.trace_ao(dev(P), dev(n), 8, radius=AO_RADIUS, bias=AO_BIAS, seed=0).cpu().numpy()
    assert np.array_equal(bits(got), bits(ao_ref.compose(w, occ)))


def append_case(monkeypatch, nthreads, build, tlas, kernel, devices=None):
    sc = scenes.get("tiny")
    set_env(monkeypatch, kernel, tlas)
    refused = kernel == "ldstop" and tlas == "1"                             # the instance tree belongs to the default kernel (test_gpu_variants.py)
    where = {"devices": devices} if devices else {"device": 0}
    with driver.Session(W, H, **where) as s:
        ha = E.begin_scene(s, sc, sc.meshes[:1], device_bvh_build=build)
        E.register(s, [(ha[0], sc.instances[0]), (ha[0], sc.instances[2])])
        a1 = s.arenas()
        assert len(a1["roots"]) == 1 and len(a1["instances"]) == 2
        if refused:
            assert render_rc(s, 0) == _lib.CRT_E_UNSUPPORTED
        else:
            # 1. the scene before the append: one synchronous frame and two in flight
            first = check_frame(s, a1, nthreads, 0, what="before the append")
            s.render_raw(ASYNC, sun_angle=SUN); s.render_raw(ASYNC, sun_angle=SUN)
            assert np.array_equal(bits(s.read_output()), bits(first))
            s.render_raw(ASYNC, sun_angle=SUN); s.render_raw(ASYNC, sun_angle=SUN)
        # 2. the second push, with two frames still in flight
        hb = E.append_meshes(s, sc.meshes[1:])
        handles = ha + hb
        E.register(s, [(handles[i.mesh], i) for i in sc.instances])
        a2 = s.arenas()
        assert len(a2["roots"]) == 2 and len(a2["instances"]) == 3 and len(a2["tris"]) == 2 * len(a1["tris"])
        if refused:
            assert render_rc(s, 0) == _lib.CRT_E_UNSUPPORTED and s.last_kernel() == ""
            return
        got = check_frame(s, a2, nthreads, COUNT, what="after the append")
        assert not np.array_equal(bits(got), bits(first))
        if devices:
            return
        assert s.last_kernel().startswith(KERNEL_OF[kernel]), s.last_kernel()
        if kernel is None:
            assert s.last_kernel() == "crt_trace_kernel<1,0,0,%s,0>" % tlas
        s.render_raw(ASYNC, sun_angle=SUN); s.render_raw(ASYNC, sun_angle=SUN)
        assert np.array_equal(bits(s.read_output()), bits(got))
        # 4. the host arenas after the second push are the device's pools (with the device build they were read back from them)
        t, n, r = downloaded(s.hip, a2)
        assert t.tobytes() == a2["tris"].tobytes() and n.tobytes() == a2["nodes"].tobytes() and np.array_equal(r, a2["roots"])
        # 5. the queries
        check_queries(s, a2, sc, nthreads)
    # 3. ... and a session that loaded both meshes in one push renders the same bits
    with driver.Session(W, H, device=0) as s:
        s.load_scene(sc, device_bvh_build=build)
        s.render_raw(0, sun_angle=SUN)
        assert np.array_equal(bits(s.read_output()), bits(got))


@pytest.mark.parametrize("kernel", [None, "ldstop"], ids=["default", "ldstop"])
@pytest.mark.parametrize("tlas", ["0", "1"], ids=["linear", "tree"])
@pytest.mark.parametrize("build", [False, True], ids=["host-build", "device-build"])
def test_mesh_appended_after_frames_were_rendered(monkeypatch, nthreads, build, tlas, kernel):
    append_case(monkeypatch, nthreads, build, tlas, kernel)


def test_mesh_appended_to_a_session_of_two_devices(monkeypatch, nthreads):
    append_case(monkeypatch, nthreads, False, None, None, devices=[0, 0])


# ------------------------------------------------------------------------------------------------
# (b) replace in place through the C-ABI
# ------------------------------------------------------------------------------------------------
def open_tiny(monkeypatch, tlas=None, kernel=None, size=(W, H)):
    """a session on "tiny" loaded in one push, whose arenas are scene_edit_ref.tiny_reference()'s (so its prepared variants apply)"""
    set_env(monkeypatch, kernel, tlas)
    sc, base, infos, cam = E.tiny_reference()
    s = driver.Session(size[0], size[1], device=0)
    try:
        s.load_scene(sc)
        a = s.arenas()
        for k in ("tris", "nodes", "roots", "instances", "materials", "textures", "texels"):
            assert a[k].tobytes() == base[k].tobytes(), k
    except Exception:
        s.close()
        raise
    return s, sc, base


def grow_view(size=(W, H)):
    return E.camera_of(size, E.GROW_CAMERA[0], scenes._normalize(E.GROW_CAMERA[1]))


@pytest.mark.parametrize("tlas", ["0", "1"], ids=["linear", "tree"])
def test_mesh_grows_in_place_and_shrinks_back(monkeypatch, nthreads, tlas):
    variants, (mesh, t1, f1) = E.tiny_variants()
    far, far_ragged = grow_view(), grow_view(E.RAGGED)                          # (a host-only session each: before the device session opens, there is one at a time)
    s, sc, base = open_tiny(monkeypatch, tlas)
    with s:
        grown = E.replace_mesh(base, mesh, t1, f1, variants["grown"])
        # the far view is the one that needs the instance's bound to follow: by the oracle's records, at least 5 % of its primary rays end on the
        # grown mesh outside the box the bound was made from
        orc = oracle_lib.Oracle(grown, nthreads=nthreads)
        d = orc.raygen(W, H, far[0], far[1]).reshape(-1, 3); o = np.tile(far[2], (len(d), 1))
        share = E.between_boxes(grown, orc.closest_hits(o, d)[0], o, d, 1, E.root_box(base, mesh))
        print(f"CRT_TLAS={tlas}: {share:.3f} of the far view's rays end between the old and the new root box")
        assert share >= 0.05
        before = [check_frame(s, base, nthreads, COUNT, view=v, what="before") for v in (None, far)]
        assert s.last_kernel() == "crt_trace_kernel<1,0,0,%s,0>" % tlas
        # 1. growth
        assert E.upload_mesh(s.hip, mesh, t1, f1, variants["grown"]) == [0, 0, 0]
        after = [check_frame(s, grown, nthreads, COUNT, view=v, what="grown") for v in (None, far)]
        assert not np.array_equal(bits(after[1]), bits(before[1]))
        s.resize(*E.RAGGED)
        check_frame(s, grown, nthreads, COUNT, view=far_ragged, what="grown, ragged")
        s.resize(W, H)
        check_frame(s, grown, nthreads, SHADOWS | COUNT, view=far, what="grown, shadows")
        # 2. shrink back: the original content over the grown one
        assert E.upload_mesh(s.hip, mesh, t1, f1, variants["original"]) == [0, 0, 0]
        shrunk = E.replace_mesh(grown, mesh, t1, f1, variants["original"])
        for v, b in zip((None, far), before):
            assert np.array_equal(bits(check_frame(s, shrunk, nthreads, COUNT, view=v, what="shrunk")), bits(b))


def test_big_leaves_at_the_same_first_triangle(monkeypatch, nthreads):
    """200, 100, 300, 127, 150 triangles in one leaf at the same leftFirst: the count of 128 and more lives in the big-leaf table, which is written
    and never cleared; the triangle-test counter is what would show a stale one"""
    variants, (mesh, t1, f1) = E.tiny_variants()
    s, sc, base = open_tiny(monkeypatch)
    with s:
        cur = base
        rng = np.random.default_rng(9)
        for c in E.LEAF_COUNTS:
            placed = variants["leaf%d" % c]
            assert E.upload_mesh(s.hip, mesh, t1, f1, placed) == [0, 0, 0]
            cur = E.replace_mesh(cur, mesh, t1, f1, placed)
            check_frame(s, cur, nthreads, COUNT, what=f"leaf of {c}")
            o = np.tile(np.asarray(s.camera()[2], np.float32), (64, 1)); d = rng.normal(size=(64, 3)).astype(np.float32)
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            got = s.query_hits(o, d)
            ref, st = oracle_lib.Oracle(cur, nthreads=nthreads).closest_hits(o, d)
            cnt = s.counters()
            assert got.tobytes() == ref.tobytes() and cnt == st, (c, cnt["triTests"], st["triTests"])
            assert st["triTests"] >= 64 * c                                   # every ray tests the whole leaf (no box test in front of a leaf root)


def test_smaller_tree_over_a_larger_one(monkeypatch, nthreads):
    """the node upload is shorter than what it replaces: stale nodes stay above it, below the high-water mark the relayout judges"""
    variants, (mesh, t1, f1) = E.tiny_variants()
    s, sc, base = open_tiny(monkeypatch)
    with s:
        placed = variants["small"]
        assert len(placed[1]) < len(base["nodes"]) - f1 and len(placed[0]) < len(base["tris"]) - t1
        assert E.upload_mesh(s.hip, mesh, t1, f1, placed) == [0, 0, 0]
        small = E.replace_mesh(base, mesh, t1, f1, placed)
        assert len(small["nodes"]) == len(base["nodes"])
        t, n, r = downloaded(s.hip, small)
        assert t.tobytes() == small["tris"].tobytes() and n.tobytes() == small["nodes"].tobytes() and np.array_equal(r, small["roots"])
        got = check_frame(s, small, nthreads, COUNT, what="smaller tree")
        assert not np.array_equal(bits(got), bits(expected(base, s, nthreads)[0]))
        # and a larger one over the smaller again
        assert E.upload_mesh(s.hip, mesh, t1, f1, variants["grown"]) == [0, 0, 0]
        check_frame(s, E.replace_mesh(small, mesh, t1, f1, variants["grown"]), nthreads, COUNT, what="larger over smaller")


def test_upload_order_does_not_matter(monkeypatch, nthreads):
    """triangles, nodes and roots of a replacement in all six orders, each from a freshly loaded session: an intermediate call may refuse
    (CRT_E_BAD_ARGUMENT: roots over nodes that are not consistent yet), the last one may not, and the frames agree"""
    variants, (mesh, t1, f1) = E.tiny_variants()
    frames = {}
    for order in ("".join(p) for p in itertools.permutations("tnr")):
        s, sc, base = open_tiny(monkeypatch)
        with s:
            rcs = E.upload_mesh(s.hip, mesh, t1, f1, variants["grown"], order)
            assert rcs[2] == 0 and all(rc in (0, _lib.CRT_E_BAD_ARGUMENT) for rc in rcs[:2]), (order, rcs)
            frames[order] = check_frame(s, E.replace_mesh(base, mesh, t1, f1, variants["grown"]), nthreads, COUNT, what=order)
    assert len(frames) == 6 and all(np.array_equal(bits(f), bits(frames["tnr"])) for f in frames.values())


# ------------------------------------------------------------------------------------------------
# (c) texels in pieces
# ------------------------------------------------------------------------------------------------
def open_target(monkeypatch, tmp_path):
    set_env(monkeypatch)
    s = driver.Session(W, H, device=0)
    try:
        s.load_scene(T.target_scene(tmp_path, (64, 32)))
        a = E.copy_arenas(s.arenas())
    except Exception:
        s.close()
        raise
    assert 2000 <= len(a["texels"]) // 3 <= 5000                             # a few thousand texels
    return s, a


def target_frame(s, a, nthreads, what):
    """a G-buffer frame of the target: the frame is the oracle's, the albedo plane the reference's, word for word; -> (frame, albedo plane)"""
    frame = check_frame(s, a, nthreads, GBUFFER, view=T.TARGET_VIEW, what=what)
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    want = gbuffer_ref.reference_planes(a, orc, orc.raygen(W, H, *T.TARGET_VIEW[:2]), T.TARGET_VIEW[2])
    got = s.read_gbuffer_raw()["albedo"]
    wrong = int((got != want["albedo"]).sum())
    assert wrong == 0, (what, f"{wrong} albedo words differ from the reference's")
    return frame, got


def target_records(a, nthreads):
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    d = orc.raygen(W, H, *T.TARGET_VIEW[:2]).reshape(-1, 3)
    return orc.closest_hits(np.tile(T.TARGET_VIEW[2], (len(d), 1)), d)[0]


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_texel_pool_uploaded_in_pieces(monkeypatch, tmp_path, nthreads, order):
    s, a = open_target(monkeypatch, tmp_path)
    with s:
        pool = np.ascontiguousarray(a["texels"], np.uint8)
        assert s.hip.crt_upload_texels(pool.ctypes.data, 0, len(pool)) == 0      # the session that uploaded the pool in one call
        frame, albedo = target_frame(s, a, nthreads, "one call")
        g = T.decode_albedo(albedo)
        assert (g[0] >= 1).all()                                                 # every pixel reads a coded texel of one of the three maps
    s, a2 = open_target(monkeypatch, tmp_path)
    with s:
        assert a2["texels"].tobytes() == pool.tobytes()
        junk = np.ascontiguousarray(pool ^ np.uint8(0xA5))
        junk[:6] = pool[:6]
        assert s.hip.crt_upload_texels(junk.ctypes.data, 0, len(junk)) == 0
        scrambled, _ = target_frame(s, E.splice_texels(a, 0, junk), nthreads, "scrambled")
        assert not np.array_equal(bits(scrambled), bits(frame))
        pieces = E.texel_pieces(len(pool), seed=17)
        assert any(o % 3 == 1 for o, _ in pieces) and any(o % 3 == 2 for o, _ in pieces) and any(n < 3 and o // 3 == (o + n - 1) // 3 for o, n in pieces)
        if order == "shuffled":
            pieces = [pieces[i] for i in np.random.default_rng(18).permutation(len(pieces))]
        E.upload_texels(s.hip, pool, pieces)
        got_frame, got_albedo = target_frame(s, a, nthreads, f"{len(pieces)} pieces, {order}")
        assert np.array_equal(bits(got_frame), bits(frame)) and np.array_equal(got_albedo, albedo)
        for x, y in zip(T.decode_albedo(got_albedo), g):
            assert np.array_equal(x, y)


def test_texel_overwrite_that_starts_and_ends_inside_texels(monkeypatch, tmp_path, nthreads):
    """[3k + 1, 3m + 2): texel k keeps its first byte, texel m its last; both are texels the frame reads"""
    s, a = open_target(monkeypatch, tmp_path)
    with s:
        idx = E.albedo_pool_index(a, target_records(a, nthreads))
        first_map = int(a["textures"][int(a["materials"][1]["albedo"])]["offset"])
        read = np.unique(idx[(idx >= first_map) & (idx < first_map + 35)])
        assert len(read) >= 20                                                   # the 7 x 5 map is read all over
        k, m = int(read[3]), int(read[-4])
        before, albedo0 = target_frame(s, a, nthreads, "before")
        data = np.random.default_rng(21).integers(1, 255, 3 * m + 2 - (3 * k + 1), dtype=np.uint8)
        pool = np.ascontiguousarray(a["texels"], np.uint8)
        data[0] = pool[3 * k + 1] ^ 0x40; data[-1] = pool[3 * m + 1] ^ 0x40; data[-2] = pool[3 * m] ^ 0x20     # the end texels do change
        assert s.hip.crt_upload_texels(data.ctypes.data, 3 * k + 1, len(data)) == 0
        b = E.splice_texels(a, 3 * k + 1, data)
        assert b["texels"][3 * k] == pool[3 * k] and b["texels"][3 * m + 2] == pool[3 * m + 2] and len(b["texels"]) == len(pool)
        after, albedo1 = target_frame(s, b, nthreads, "after the overwrite")
        for texel in (k, m):                                                     # the mixed texels are on screen and their words changed
            px = idx.reshape(H, W) == texel
            assert px.any() and (albedo1[px] != albedo0[px]).all(), texel
        assert np.array_equal(albedo1[idx.reshape(H, W) < k], albedo0[idx.reshape(H, W) < k])


def test_texture_table_moved_to_a_copy_and_to_another_map(monkeypatch, tmp_path, nthreads):
    s, a = open_target(monkeypatch, tmp_path)
    with s:
        tex = int(a["materials"][1]["albedo"])                                   # the 7 x 5 map of material 0 of the mesh
        other = int(a["materials"][3]["albedo"])                                 # the 16 x 4 map
        tx = a["textures"]
        assert (tx[tex]["width"], tx[tex]["height"]) == (7, 5) and (tx[other]["width"], tx[other]["height"]) == (16, 4)
        before, albedo0 = target_frame(s, a, nthreads, "before")
        pool = np.ascontiguousarray(a["texels"], np.uint8)
        copy = np.ascontiguousarray(pool[3 * int(tx[tex]["offset"]):3 * (int(tx[tex]["offset"]) + 35)])
        assert s.hip.crt_upload_texels(copy.ctypes.data, len(pool), len(copy)) == 0
        # 3. the same map at another place in the pool: nothing changes
        b = E.move_texture(E.splice_texels(a, len(pool), copy), tex, len(pool) // 3)
        assert s.hip.crt_upload_texture_table(b["textures"].ctypes.data, len(b["textures"])) == 0
        moved, albedo1 = target_frame(s, b, nthreads, "moved to the copy")
        assert np.array_equal(bits(moved), bits(before)) and np.array_equal(albedo1, albedo0)
        # 4. another map's texels under this map's size
        c = E.move_texture(b, tex, int(tx[other]["offset"]))
        assert s.hip.crt_upload_texture_table(c["textures"].ctypes.data, len(c["textures"])) == 0
        swapped, albedo2 = target_frame(s, c, nthreads, "moved to another map")
        tags0, tags2 = T.decode_albedo(albedo0)[0], T.decode_albedo(albedo2)[0]
        assert (tags0 == 1).sum() >= 500 and (tags2[tags0 == 1] == 3).all()      # what read the 7 x 5 map (tag 1) reads the 16 x 4 map (tag 3)
        assert np.array_equal(albedo2[tags0 != 1], albedo0[tags0 != 1])


# ------------------------------------------------------------------------------------------------
# (d) one material record
# ------------------------------------------------------------------------------------------------
def test_one_material_record_in_the_middle_of_the_table(monkeypatch, nthreads):
    s, sc, base = open_tiny(monkeypatch)
    with s:
        k = 3                                                                    # materials: 0 the default, 1-2 of mesh 0, 3-4 of mesh 1
        assert int(base["num_materials"]) == 5 and base["materials"][k]["albedo"] == 4
        orc = oracle_lib.Oracle(base, nthreads=nthreads)
        iv, ip, pos = s.camera()
        d = orc.raygen(W, H, iv, ip).reshape(-1, 3)
        material = E.hit_material(base, orc.closest_hits(np.tile(pos, (len(d), 1)), d)[0]).reshape(H, W)
        assert all((material == j).sum() >= 20 for j in (k - 1, k, k + 1))        # all three are on screen
        check_frame(s, base, nthreads, GBUFFER, what="before")
        albedo0 = s.read_gbuffer_raw()["albedo"]
        edited, record = E.replace_material(base, k, 0x0040C0FF, 3)              # another colour, and mesh 0's map
        assert s.hip.crt_upload_materials(record.ctypes.data, k, 1) == 0
        check_frame(s, edited, nthreads, GBUFFER, what="after")
        albedo1 = s.read_gbuffer_raw()["albedo"]
        want = gbuffer_ref.reference_planes(edited, oracle_lib.Oracle(edited, nthreads=nthreads), d.reshape(H, W, 3), pos)["albedo"]
        assert np.array_equal(albedo1, want)
        for j in (k - 1, k + 1):                                                 # the neighbours shade as before
            assert np.array_equal(albedo1[material == j], albedo0[material == j]), j
        assert (albedo1[material == k] != albedo0[material == k]).mean() > 0.9
        check_frame(s, edited, nthreads, COUNT, what="after, counted")


# ------------------------------------------------------------------------------------------------
# (e) order against frames in flight
# ------------------------------------------------------------------------------------------------
def host_frame(s):
    ptr, n = C.c_void_p(), C.c_size_t()
    assert s.hip.crt_map_host_frame(C.byref(ptr), C.byref(n)) == 0 and n.value == W * H * 16
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(H, W, 4)).copy()


@pytest.mark.parametrize("edit", ["mesh", "texels"])
def test_edit_is_ordered_against_frames_in_flight(monkeypatch, nthreads, edit):
    """frames submitted before an upload show the old scene, frames submitted after it the new one, with nothing waited for in between"""
    variants, (mesh, t1, f1) = E.tiny_variants()
    s, sc, base = open_tiny(monkeypatch)
    with s:
        if edit == "mesh":
            new = E.replace_mesh(base, mesh, t1, f1, variants["grown"])
        else:
            first = int(base["textures"][3]["offset"])                           # most of mesh 0's 64 x 64 map
            data = np.random.default_rng(23).integers(0, 256, 3 * 4000 + 1, dtype=np.uint8)
            new = E.splice_texels(base, 3 * first + 1, data)
        old_want, new_want = expected(base, s, nthreads)[0], expected(new, s, nthreads)[0]
        assert not np.array_equal(bits(old_want), bits(new_want))
        for _ in range(4):                                                       # warm the slots
            s.render_raw(ASYNC, sun_angle=SUN)
        s.render_raw(ASYNC | READBACK, sun_angle=SUN)
        s.render_raw(ASYNC, sun_angle=SUN)
        if edit == "mesh":
            assert E.upload_mesh(s.hip, mesh, t1, f1, variants["grown"]) == [0, 0, 0]
        else:
            assert s.hip.crt_upload_texels(data.ctypes.data, 3 * first + 1, len(data)) == 0
        s.render_raw(ASYNC, sun_angle=SUN)
        old_got = host_frame(s)                                                  # the READBACK frame submitted before the edit (its slot is not reused yet)
        s.render_raw(ASYNC | READBACK, sun_angle=SUN)
        s.sync()
        assert np.array_equal(bits(s.read_output()), bits(new_want))
        assert np.array_equal(bits(host_frame(s)), bits(new_want))
        assert np.array_equal(bits(old_got), bits(old_want))


# ------------------------------------------------------------------------------------------------
# (f) seeded edit sequences
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", E.FUZZ_SEEDS)
def test_seeded_edit_sequences(monkeypatch, nthreads, seed):
    """frames of random flags, instance moves, material records, texel overwrites, mesh replacements and queries in a seeded order; after every
    frame that is read, pixels and counters are the oracle's for the state the session is in now (tests/test_gpu_state_fuzz.py's rule)"""
    variants, where = E.tiny_variants()
    placed = [variants[k] for k in E.FUZZ_VARIANTS]
    s, sc, base = open_tiny(monkeypatch)
    with s:
        fz = E.EditFuzz(seed, base, sc, placed, *where)
        cache, seen = {}, {}
        for step, op, arg in fz:
            seen[op] = seen.get(op, 0) + 1
            if op == "frame":
                flags, times = arg
                for _ in range(times):                                           # the same frame once or a few times (slot rotation when ASYNC)
                    s.render_raw(flags, sun_angle=SUN)
                got = s.read_output()
                key = (fz.key(), flags & (SHADOWS | REFRACTION))
                if key not in cache:
                    cache[key] = expected(fz.a, s, nthreads, flags)
                want, st = cache[key]
                assert np.array_equal(bits(got), bits(want)), (seed, step, flags)
                if flags & COUNT:
                    assert s.counters() == st, (seed, step, flags)
            elif op == "instance":
                p, keep = _lib.fptr(arg)
                s.h.crth_set_mesh_matrix(1, p)
                s.render(sun_angle=SUN)                                          # the mirrored Renderer uploads the dirty range
                fz.set_instances(s.arenas()["instances"])
            elif op == "material":
                k, record = arg
                assert s.hip.crt_upload_materials(record.ctypes.data, k, 1) == 0, (seed, step)
            elif op == "texels":
                off, data = arg
                assert s.hip.crt_upload_texels(data.ctypes.data, off, len(data)) == 0, (seed, step)
            elif op == "mesh":
                assert E.upload_mesh(s.hip, *where, placed[arg]) == [0, 0, 0], (seed, step)
            else:
                o = np.tile(np.asarray(s.camera()[2], np.float32), (len(arg), 1))
                got = s.query_hits(o, arg)
                ref, st = oracle_lib.Oracle(fz.a, nthreads=nthreads).closest_hits(o, arg)
                assert got.tobytes() == ref.tobytes() and s.counters() == st, (seed, step)
        assert seen.get("frame", 0) >= 10 and all(seen.get(op, 0) >= 2 for op in E.EDIT_OPS), seen
