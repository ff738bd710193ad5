"""Scene edits without a GPU (tests/scene_edit_ref.py): a scene pushed in two parts describes the scene pushed in one, and the helpers
that compose "the arenas after an edit" for tests/test_gpu_scene_edits.py reach the oracle as a from-scratch build of the same final
content does. Also the conditions the GPU cases rest on -- the share of rays through the region a grown mesh reaches, the share of a query
batch on the appended mesh, the pieces of a texel pool, the counts of the seeded edit sequences -- asserted where no device is needed."""
import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import oracle_lib
import scene_edit_ref as E
import texel_ref as T
from test_bvh import check_invariants
from util import bits, seeded_rays


def frame(a, cam, size, sun, nthreads, **kw):
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    iv, ip, pos = cam
    return orc.trace(orc.raygen(size[0], size[1], iv, ip), pos, sun, **kw)


# ------------------------------------------------------------------------------------------------
# 1. two pushes describe the same scene as one
# ------------------------------------------------------------------------------------------------
def two_pushes(sc, size=(E.W, E.H)):
    """-> (arenas, mesh infos, CPU_RayCast records of the 256 seeded rays) of: sky, mesh A, push; mesh B, push again, PushTexturesToGPU"""
    with driver.Session(size[0], size[1], host_only=True) as s:
        ha = E.begin_scene(s, sc, sc.meshes[:1])
        first = E.copy_arenas(s.arenas())
        hb = E.append_meshes(s, sc.meshes[1:])
        handles = ha + hb
        E.register(s, [(handles[i.mesh], i) for i in sc.instances])
        a = E.copy_arenas(s.arenas())
        o, d = seeded_rays(a, sc.camera_pos, 256, seed=5)
        return a, first, tuple(E.mesh_info(s, m) for m in handles), s.cpu_raycast(o, d)


def test_two_pushes_describe_the_scene_of_one(nthreads):
    sc, x, infos_x, cam = E.tiny_reference()
    y, first, infos_y, cast_y = two_pushes(sc)
    assert infos_y == infos_x
    # the first push's triangles and nodes are where they were
    assert y["tris"][:len(first["tris"])].tobytes() == first["tris"].tobytes() and y["nodes"][:len(first["nodes"])].tobytes() == first["nodes"].tobytes()
    assert len(first["roots"]) == 1 and len(y["roots"]) == 2 and y["roots"][0] == first["roots"][0]
    for k in ("instances", "materials", "textures", "texels"):
        assert y[k].tobytes() == x[k].tobytes(), k                       # (node numbering may differ between the two; these may not)
    counts = [i[0] for i in infos_y]
    check_invariants(y["nodes"], y["roots"], y["tris"], counts)
    # the rebase: every leaf of B indexes triangles at or beyond A's count
    b_nodes = y["nodes"][int(y["roots"][1]):]
    leaves = b_nodes[b_nodes["triCount"] > 0]
    assert len(leaves) > 1 and (leaves["leftFirst"] >= counts[0]).all() and (leaves["leftFirst"] + leaves["triCount"] <= sum(counts)).all()
    for size in ((E.W, E.H), E.RAGGED):
        cam_s = E.tiny_reference(size)[3]
        fx, sx = frame(x, cam_s, size, sc.sun_angle, nthreads)
        fy, sy = frame(y, cam_s, size, sc.sun_angle, nthreads)
        assert np.array_equal(bits(fx), bits(fy)) and sx == sy and sx["hits"] > 0, size
    with driver.Session(E.W, E.H, host_only=True) as s:
        s.load_scene(sc)
        o, d = seeded_rays(y, sc.camera_pos, 256, seed=5)
        cast_x = s.cpu_raycast(o, d)
    assert cast_x.tobytes() == cast_y.tobytes() and (cast_x["distance"] < 1e4).sum() >= 64


# ------------------------------------------------------------------------------------------------
# 2. the helpers' arenas against a from-scratch build of the same final content
# ------------------------------------------------------------------------------------------------
def from_scratch(a, infos, new_tris):
    """mesh 0's triangles and `new_tris` as mesh 1, built in one oracle_lib.build_bvh"""
    n0 = infos[0][0]
    tris = np.concatenate([a["tris"][:n0], new_tris])
    t, n, r, _ = oracle_lib.build_bvh(tris, [n0, len(new_tris)])
    b = E.copy_arenas(a)
    b.update(tris=t, nodes=n, roots=r)
    return b


@pytest.mark.parametrize("name", ["grown", "small"])
def test_replaced_mesh_is_the_mesh_built_from_scratch(name, nthreads):
    sc, a, infos, cam = E.tiny_reference()
    variants, (mesh, t1, f1) = E.tiny_variants()
    placed = variants[name]
    got = E.replace_mesh(a, mesh, t1, f1, placed)
    assert len(got["tris"]) >= len(a["tris"]) and len(got["nodes"]) >= len(a["nodes"])       # a shorter replacement leaves the old tail in the pool
    if name == "small":
        assert len(placed[1]) < len(a["nodes"]) - f1 and got["nodes"][f1 + len(placed[1]):].tobytes() == a["nodes"][f1 + len(placed[1]):].tobytes()
    src = E.grown(a["tris"][t1:], E.GROW) if name == "grown" else np.array(a["tris"][t1:][::3][:E.SMALL])
    want = from_scratch(a, infos, src)
    for c in (cam, E.camera_of((E.W, E.H), E.GROW_CAMERA[0], scenes._normalize(E.GROW_CAMERA[1]))):
        fg, sg = frame(got, c, (E.W, E.H), sc.sun_angle, nthreads)
        fw, sw = frame(want, c, (E.W, E.H), sc.sun_angle, nthreads)
        assert np.array_equal(bits(fg), bits(fw)) and sg["hits"] == sw["hits"] > 0
    base, _ = frame(a, cam, (E.W, E.H), sc.sun_angle, nthreads)
    assert not np.array_equal(bits(base), bits(frame(got, cam, (E.W, E.H), sc.sun_angle, nthreads)[0]))


@pytest.mark.parametrize("count", E.LEAF_COUNTS)
def test_leaf_mesh_is_its_triangles(count, nthreads):
    """a one-leaf mesh against the pools written out by hand (mesh 0's triangles and nodes, the leaf's triangles, one node over all of them): the
    same frame, and `count` triangle tests per ray that reaches the leaf. (Not against a built tree over the same triangles: a leaf root is tested
    without any box test, hazard H3, so the two legitimately differ.)"""
    sc, a, infos, cam = E.tiny_reference()
    variants, (mesh, t1, f1) = E.tiny_variants()
    placed = variants["leaf%d" % count]
    assert len(placed[0]) == count and len(placed[1]) == 1
    got = E.replace_mesh(a, mesh, t1, f1, placed)
    leaf = np.zeros(1, _lib.NODE_DTYPE)
    pts = np.concatenate([placed[0][k] for k in ("v0", "v1", "v2")])
    leaf[0] = (pts.min(0), t1, pts.max(0), count)
    want = dict(a, tris=np.concatenate([a["tris"][:t1], placed[0]]), nodes=np.concatenate([a["nodes"][:f1], leaf]), roots=np.array([0, f1], np.uint32))
    fg, sg = frame(got, cam, (E.W, E.H), sc.sun_angle, nthreads)
    fw, sw = frame(want, cam, (E.W, E.H), sc.sun_angle, nthreads)
    assert np.array_equal(bits(fg), bits(fw)) and sg == sw and sg["hits"] > 0
    o = np.tile(np.asarray(cam[2], np.float32), (4, 1)); d = np.tile(np.asarray(sc.camera_front, np.float32), (4, 1))
    only = E.copy_arenas(got); only["instances"] = got["instances"][1:2]
    _, st = oracle_lib.Oracle(only, nthreads=1).closest_hits(o, d)
    assert st["triTests"] == 4 * count


def test_growth_view_sees_the_region_between_the_boxes(nthreads):
    sc, a, infos, cam = E.tiny_reference()
    variants, (mesh, t1, f1) = E.tiny_variants()
    old = E.root_box(a, mesh)
    g = E.replace_mesh(a, mesh, t1, f1, variants["grown"])
    new = E.root_box(g, mesh)
    ratio = (new[1] - new[0]) / (old[1] - old[0])
    assert np.allclose(ratio, E.GROW, rtol=1e-5)
    iv, ip, pos = E.camera_of((E.W, E.H), E.GROW_CAMERA[0], scenes._normalize(E.GROW_CAMERA[1]))
    orc = oracle_lib.Oracle(g, nthreads=nthreads)
    d = orc.raygen(E.W, E.H, iv, ip).reshape(-1, 3); o = np.tile(pos, (len(d), 1))
    rec, _ = orc.closest_hits(o, d)
    share = E.between_boxes(g, rec, o, d, 1, old)
    print(f"{share:.3f} of the primary rays hit the grown mesh outside its earlier root box")
    assert share >= 0.05


def test_spliced_texels_and_tables_are_the_ones_built_from_scratch(tmp_path, nthreads):
    with driver.Session(E.W, E.H, host_only=True) as s:
        s.load_scene(T.target_scene(tmp_path, (64, 32)))
        a = E.copy_arenas(s.arenas())
    pool = a["texels"].tobytes()
    rng = np.random.default_rng(3)
    k, m = 2060, 2075
    data = rng.integers(1, 255, 3 * m + 2 - (3 * k + 1), dtype=np.uint8)
    got = E.splice_texels(a, 3 * k + 1, data)
    want = dict(a); want["texels"] = np.frombuffer(pool[:3 * k + 1] + data.tobytes() + pool[3 * m + 2:], np.uint8)
    assert got["texels"].tobytes() == want["texels"].tobytes() and len(got["texels"]) == len(pool)
    tail = E.splice_texels(a, len(pool), pool[-30:])
    assert tail["texels"].tobytes() == pool + pool[-30:]
    moved = E.move_texture(a, 3, 7, 5, 2)
    assert tuple(moved["textures"][3]) == (5, 2, 7, 0) and moved["textures"][4] == a["textures"][4] and a["textures"]["offset"][3] != 7
    mats, record = E.replace_material(a, 2, 0x00112233, 4)
    table = np.array(a["materials"]); table[2] = (0x00112233, table[2]["specularColor"], 4, table[2]["specular"], table[2]["shininess"], table[2]["roughness"])
    assert mats["materials"].tobytes() == table.tobytes() and record.tobytes() == table[2:3].tobytes() and record.nbytes == 16
    view = T.TARGET_VIEW
    for b, w_ in ((got, want), (mats, dict(a, materials=table))):
        fb, _ = frame(b, view, (E.W, E.H), -1.96, nthreads)
        fw, _ = frame(w_, view, (E.W, E.H), -1.96, nthreads)
        assert np.array_equal(bits(fb), bits(fw)) and not np.array_equal(bits(fb), bits(frame(a, view, (E.W, E.H), -1.96, nthreads)[0]))


def test_texel_pieces_cover_the_pool_with_the_offsets_asked_for():
    for seed in (1, 2, 3):
        pieces = E.texel_pieces(6456, seed)
        assert pieces[0][0] == 0 and all(a_[0] + a_[1] == b_[0] for a_, b_ in zip(pieces, pieces[1:])) and sum(pieces[-1]) == 6456
        assert {n for _, n in pieces[:-1]} <= set(E.PIECE_SIZES)
        assert any(o % 3 == 1 for o, _ in pieces) and any(o % 3 == 2 for o, _ in pieces)
        assert any(n < 3 and o // 3 == (o + n - 1) // 3 for o, n in pieces)


@pytest.mark.parametrize("seed", E.FUZZ_SEEDS)
def test_edit_sequences_hold_enough_of_everything(seed):
    sc, a, infos, cam = E.tiny_reference()
    variants, where = E.tiny_variants()
    fz = E.EditFuzz(seed, a, sc, [variants[k] for k in E.FUZZ_VARIANTS], *where)
    ops = [op for _, op, _ in fz]
    assert len(ops) == E.FUZZ_STEPS and ops.count("frame") >= 10 and ops.count("query") >= 1
    for op in E.EDIT_OPS:
        assert ops.count(op) >= 2, (seed, op, ops)
