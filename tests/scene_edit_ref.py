"""Scene edits in a live session: what the session describes after its content changed. No tests in here; tests/test_scene_edits_cpu.py pins
these helpers without a GPU and tests/test_gpu_scene_edits.py renders from the edited pools.

    begin_scene / append_meshes / register    the mirror's call order cut in two: a mesh (with its materials and maps) imported and pushed
                                              after the first PushMeshesToGPU / PushTexturesToGPU
    mesh_info / mesh_nodes                    where a mesh lies in the arenas
    built_mesh / leaf_mesh                    a replacement tree at a chosen triangle start and first node (oracle_lib.build_bvh; one leaf)
    replace_mesh / splice_texels / replace_material / move_texture
                                              the arenas after an edit made through the C-ABI: the device pools, stale tails included
    upload_mesh                               the three uploads of a replacement in a chosen order
    grown / between_boxes                     a mesh scaled about its origin, and the share of rays whose hit lies between two root boxes
    texel_pieces                              seeded pieces of a texel pool with the offsets the relayout has to survive
    EditFuzz                                  the seeded edit sequence of the GPU fuzz, replayable without a GPU

The criterion everywhere: frames bit for bit, counters equal, records byte for byte against oracle_lib.Oracle on these arenas."""
import functools
import hashlib

import numpy as np

from clraytracer_amd import _lib
import oracle_lib
from test_traversal_independent import matmul_xyz

POST, ASYNC, COUNT, SHADOWS, READBACK, REFRACTION, GBUFFER = 1, 4, 8, 32, 128, 256, 8192
W, H = 96, 64
RAGGED = (113, 70)
TRI, NODE = _lib.TRI_DTYPE.itemsize, _lib.NODE_DTYPE.itemsize


def copy_arenas(a):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}


# ------------------------------------------------------------------------------------------------
# the mirror's call order, cut in two
# ------------------------------------------------------------------------------------------------
def begin_scene(s, sc, meshes, device_bvh_build=False):
    """driver.Session.load_scene up to the instances, with only `meshes` (paths) imported: -> their handles"""
    h = s.h
    h.crth_set_device_bvh_build(1 if device_bvh_build else 0)
    h.crth_set_asset_root((sc.asset_root or "").encode())
    h.crth_prepare_meshes()
    tex = h.crth_import_texture(sc.skybox.encode())
    s._check("ImportTexture(skybox)")
    assert tex == 2, tex
    handles = append_meshes(s, meshes)
    s.set_camera(sc.camera_pos, sc.camera_front)
    s.scene = sc
    return handles


def append_meshes(s, meshes):
    """ImportMesh (materials and maps arrive with it), PushMeshesToGPU, PushTexturesToGPU"""
    handles = []
    for path in meshes:
        handles.append(s.h.crth_import_mesh(path.encode()))
        s._check(f"ImportMesh({path})")
    s.h.crth_push_meshes()
    s.h.crth_push_textures()
    s._check("PushMeshesToGPU/PushTexturesToGPU")
    return handles


def register(s, instances):
    """the instance table from scratch: [(mesh handle, scenes.Instance)]"""
    s.h.crth_clear_instances()
    s.h.crth_begin_instances()
    for mesh, inst in instances:
        p, keep = _lib.fptr(inst.matrix)
        s.h.crth_register_instance(int(mesh), int(inst.material), p)
    s.h.crth_end_instances()
    s._check("RegisterMeshInstance")


def mesh_info(s, mesh):
    """(triangles, first triangle, first material, materials) of an imported mesh"""
    info = np.zeros(4, np.uint32)
    s.h.crth_mesh_info(int(mesh), info.ctypes.data)
    return tuple(int(x) for x in info)


def mesh_nodes(a, mesh):
    """(first node, node count) of mesh `mesh` in arenas whose meshes were built one after the other"""
    roots = [int(r) for r in a["roots"]] + [len(a["nodes"])]
    return roots[mesh], roots[mesh + 1] - roots[mesh]


@functools.lru_cache(maxsize=None)
def tiny_reference(size=(W, H)):
    """(scene, arenas, mesh infos, (invView, invProj, cameraPos)) of "tiny" loaded in one push, at the frame size: computed once, read-only"""
    from clraytracer_amd import driver, scenes
    sc = scenes.get("tiny")
    with driver.Session(size[0], size[1], host_only=True) as s:
        s.load_scene(sc)
        a = copy_arenas(s.arenas())
        infos = tuple(mesh_info(s, m) for m in range(len(sc.meshes)))
        cam = s.camera()
    for v in list(a.values()) + list(cam):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc, a, infos, cam


@functools.lru_cache(maxsize=None)
def tiny_variants():
    """placed_variants of tiny_reference(): (name -> placed, (mesh, first triangle, first node)), computed once"""
    sc, a, infos, cam = tiny_reference()
    return placed_variants(a, infos)


def query_batch(a, cam_pos):
    """the 256 rays of the query cases (util.seeded_rays): by the oracle 93 of them end on instance 1 of "tiny" (asserted where used)"""
    from util import seeded_rays
    return seeded_rays(a, cam_pos, 256, seed=6)


def camera_of(size, pos, front):
    """(invView, invProj, cameraPos) the mirror's camera gives for a frame size, position and direction. Opens a host-only session: the mirror
    holds one session at a time, so never call this while another one is open."""
    from clraytracer_amd import driver
    with driver.Session(size[0], size[1], host_only=True) as s:
        s.set_camera(pos, front)
        return s.camera()


MESH = 1                                     # the mesh of "tiny" the C-ABI edits replace: the last one, so a larger replacement grows into free pool
GROW = 10.0                                  # (b)1: the replacement's root box is ten times the original's extent
# (b)1's view: from far enough back that the grown mesh is in front of the camera, not around it (a ray never enters a box it starts in)
GROW_CAMERA = ((4.0, 12.0, 60.0), (0.0, -0.1, -1.0))
# (b)3: either side of the 128 at which a leaf's count moves from its reference into the big-leaf table; the last one a big leaf smaller than
# an earlier big leaf, which a table entry that is only ever raised would get wrong
LEAF_COUNTS = (200, 100, 300, 127, 150)
SMALL = 150                                  # (b)4: triangles of the smaller tree


def placed_variants(a, infos):
    """name -> (triangles, nodes, root) placed over MESH of the arenas `a`: its own content, GROW times as large, a smaller tree, leaves"""
    n1, t1, _, _ = infos[MESH]
    f1, _ = mesh_nodes(a, MESH)
    orig = np.array(a["tris"][t1:t1 + n1])
    out = {"original": (orig, np.array(a["nodes"][f1:]), f1),
           "grown": built_mesh(grown(orig, GROW), t1, f1),
           "small": built_mesh(orig[::3][:SMALL], t1, f1)}
    for c in LEAF_COUNTS:
        out["leaf%d" % c] = leaf_mesh(orig[::max(1, n1 // c)][:c] if c <= n1 // 2 else orig[:c], t1, f1)
    return out, (MESH, t1, f1)


# ------------------------------------------------------------------------------------------------
# replacement trees
# ------------------------------------------------------------------------------------------------
def built_mesh(tris, tri_start, first_node):
    """oracle_lib.build_bvh of one mesh, placed: (reordered triangles, nodes with absolute child indices and leaves rebased to tri_start, root)"""
    t, n, r, used = oracle_lib.build_bvh(tris, [len(tris)], counter_start=first_node)
    n = n[first_node:].copy()
    leaf = n["triCount"] > 0
    n["leftFirst"][leaf] += np.uint32(tri_start)
    assert int(r[0]) == first_node and used == len(n)
    return t, n, int(r[0])


def leaf_mesh(tris, tri_start, first_node):
    """a mesh that is one leaf: the root holds every triangle (hazard H3: tested without a box test)"""
    t = np.ascontiguousarray(tris).copy()
    n = np.zeros(1, _lib.NODE_DTYPE)
    pts = np.concatenate([t["v0"], t["v1"], t["v2"]])
    n["min"][0], n["max"][0] = pts.min(0), pts.max(0)
    n["leftFirst"][0], n["triCount"][0] = tri_start, len(t)
    return t, n, first_node


def grown(tris, k):
    """every vertex k times as far from the mesh's origin; attributes kept"""
    t = np.ascontiguousarray(tris).copy()
    for f in ("v0", "v1", "v2"):
        t[f] = t[f] * np.float32(k)
    return t


def _overlay(pool, first, part):
    """`part` written at `first` into a copy of `pool`, which grows if it has to: what the device pool holds after the upload (a shorter
    replacement leaves the old tail in place)"""
    out = np.zeros(max(len(pool), first + len(part)), pool.dtype)
    out[:len(pool)] = pool
    out[first:first + len(part)] = part
    return out


def replace_mesh(a, mesh, tri_start, first_node, placed):
    """arenas after `placed` = (triangles, nodes, root) was uploaded over mesh `mesh`"""
    t, n, root = placed
    b = copy_arenas(a)
    b["tris"] = _overlay(a["tris"], tri_start, t)
    b["nodes"] = _overlay(a["nodes"], first_node, n)
    b["roots"] = np.array(a["roots"], np.uint32)
    b["roots"][mesh] = root
    return b


def upload_mesh(hip, mesh, tri_start, first_node, placed, order="tnr"):
    """crt_upload_triangles / _bvh_nodes / _bvh_roots of `placed` in `order` (a permutation of "tnr"): -> the three return codes in call order"""
    t, n, root = placed
    t, n, r = np.ascontiguousarray(t), np.ascontiguousarray(n), np.array([root], np.uint32)
    calls = {"t": lambda: hip.crt_upload_triangles(t.ctypes.data, tri_start * TRI, t.nbytes),
             "n": lambda: hip.crt_upload_bvh_nodes(n.ctypes.data, first_node * NODE, n.nbytes),
             "r": lambda: hip.crt_upload_bvh_roots(r.ctypes.data, mesh, 1)}
    assert sorted(order) == ["n", "r", "t"]
    return [calls[c]() for c in order]


def root_box(a, mesh):
    """the box an entering ray is tested against: around the root's two children (the root's own for a leaf)"""
    nd = a["nodes"][int(a["roots"][mesh])]
    if nd["triCount"] > 0:
        return np.array(nd["min"], np.float64), np.array(nd["max"], np.float64)
    kids = a["nodes"][int(nd["leftFirst"]):int(nd["leftFirst"]) + 2]
    return kids["min"].min(0).astype(np.float64), kids["max"].max(0).astype(np.float64)


def between_boxes(a, rec, origins, dirs, instance, inner):
    """the share of the rays whose closest hit `rec` (the oracle's, on arenas `a`) is on `instance` at an object-space point outside the box
    `inner` = (min, max): rays that pass through the region a grown mesh reaches and its earlier root box did not"""
    sel = np.flatnonzero(rec["instance"] == instance)
    if len(sel) == 0:
        return 0.0
    p = (origins[sel].astype(np.float64) + dirs[sel].astype(np.float64) * rec["t"][sel, None]).astype(np.float32)
    q = matmul_xyz(np.ascontiguousarray(a["instances"][instance]["inv"], np.float32), p, 1.0).astype(np.float64)
    outside = ((q < inner[0]) | (q > inner[1])).any(axis=1)
    return float(outside.sum()) / len(rec)


# ------------------------------------------------------------------------------------------------
# texels, textures, materials
# ------------------------------------------------------------------------------------------------
def splice_texels(a, offset, data):
    """arenas after crt_upload_texels(data, offset, len(data))"""
    b = copy_arenas(a)
    b["texels"] = _overlay(np.ascontiguousarray(a["texels"], np.uint8), int(offset), np.frombuffer(bytes(data), np.uint8))
    return b


def replace_material(a, k, color, albedo):
    """arenas after material k got another colour and another albedo texture: -> (arenas, the 16-byte record to upload)"""
    b = copy_arenas(a)
    b["materials"] = np.array(a["materials"])
    b["materials"]["color"][k], b["materials"]["albedo"][k] = color, albedo
    if k >= int(b["num_materials"]):
        b["num_materials"] = k + 1
    return b, np.ascontiguousarray(b["materials"][k:k + 1])


def move_texture(a, tex, offset, width=None, height=None):
    """arenas after the texture table was uploaded again with textures[tex] at another texel offset (and size)"""
    b = copy_arenas(a)
    b["textures"] = np.array(a["textures"])
    b["textures"]["offset"][tex] = offset
    if width is not None:
        b["textures"]["width"][tex], b["textures"]["height"][tex] = width, height
    return b


PIECE_SIZES = (1, 2, 3, 4, 5, 7, 64, 257)


def texel_pieces(nbytes, seed):
    """[(offset, size)] covering [0, nbytes) in ascending order, sizes drawn from PIECE_SIZES (the last one cut to fit). The draw is repeated
    until a piece begins at offset % 3 == 1, another at == 2, and one of fewer than 3 bytes lies inside a single texel."""
    rng = np.random.default_rng(seed)
    while True:
        out, at = [], 0
        while at < nbytes:
            n = min(int(rng.choice(PIECE_SIZES)), nbytes - at)
            out.append((at, n))
            at += n
        starts = {o % 3 for o, _ in out}
        inside = any(n < 3 and o // 3 == (o + n - 1) // 3 for o, n in out)
        if {1, 2} <= starts and inside:
            return out


def upload_texels(hip, pool, pieces):
    """crt_upload_texels of every piece of the bytes `pool`; every call must succeed"""
    pool = np.ascontiguousarray(pool, np.uint8)
    for off, n in pieces:
        assert hip.crt_upload_texels(pool[off:off + n].ctypes.data, off, n) == 0, (off, n)


def albedo_pool_index(a, rec):
    """the pool index SampleTexture reads for every closest-hit record (-1: a miss), with the arithmetic of gbuffer_ref.planes_from_records"""
    from test_shading_independent import F, half, to_int
    import gbuffer_ref
    idx = np.full(len(rec), -1, np.int64)
    shaded = np.flatnonzero((rec["instance"] >= 0) & ~(rec["t"] > gbuffer_ref.INF_MINUS_ONE))
    if len(shaded) == 0:
        return idx
    hr = rec[shaded]
    inst = a["instances"][hr["instance"]]
    tri = a["tris"][hr["tri"]]
    mat = a["materials"][np.minimum(inst["materialStart"].astype(np.int64) + tri["mat"].astype(np.int64), 255)]
    uu, vv = hr["u"].astype(np.float32), hr["v"].astype(np.float32)
    bx = (F(1.0) - uu) - vv
    uvh = half(tri["uv"])
    uv = (uvh[:, 0:2] * bx[:, None] + uvh[:, 2:4] * uu[:, None]) + uvh[:, 4:6] * vv[:, None]
    tx = a["textures"][np.minimum(mat["albedo"].astype(np.int64), 31)]
    uvf = uv - np.floor(uv)
    us = to_int(tx["width"].astype(np.float32) * uvf[:, 0])
    vs = to_int(tx["height"].astype(np.float32) * uvf[:, 1])
    n = (len(a["texels"]) + 2) // 3
    idx[shaded] = np.clip(vs * tx["width"].astype(np.int64) + tx["offset"].astype(np.int64) + us, 0, n - 1)
    return idx


def hit_material(a, rec):
    """the material index of every closest-hit record (-1: a miss): kernel_main.cl:229"""
    out = np.full(len(rec), -1, np.int64)
    hit = np.flatnonzero(rec["instance"] >= 0)
    inst = a["instances"][rec["instance"][hit]]
    out[hit] = np.minimum(inst["materialStart"].astype(np.int64) + a["tris"][rec["tri"][hit]]["mat"].astype(np.int64), 255)
    return out


# ------------------------------------------------------------------------------------------------
# the seeded edit sequence
# ------------------------------------------------------------------------------------------------
FUZZ_SEEDS = (31, 32)
FUZZ_STEPS = 40
FUZZ_OPS = ("frame", "frame", "frame", "instance", "material", "texels", "mesh", "query")
EDIT_OPS = ("instance", "material", "texels", "mesh")
FUZZ_VARIANTS = ("original", "grown", "leaf200")  # of placed_variants: the mesh-replace operation draws among these three


class EditFuzz:
    """The sequence of one seed over the "tiny" scene, as a list of steps the GPU test applies and whose expected arenas this class composes.
    Everything random is drawn here, so the CPU test can replay a seed (count its frames and edits) without a device.

    base: the arenas of the loaded scene; variants: three placed replacements of mesh 1 (see tests: original, grown, one leaf)."""

    def __init__(self, seed, base, sc, variants, mesh, tri_start, first_node, steps=FUZZ_STEPS):
        self.rng = np.random.default_rng(seed)
        self.a = copy_arenas(base)
        self.sc, self.variants, self.where = sc, variants, (mesh, tri_start, first_node)
        self.steps = steps
        self.texel_bytes = len(base["texels"])
        self.num_materials = int(base["num_materials"])
        self.num_textures = int(base["num_textures"])

    def __iter__(self):
        rng = self.rng
        for step in range(self.steps):
            op = str(rng.choice(FUZZ_OPS))
            if op == "frame":
                flags = 0
                for f, p in ((SHADOWS, 0.3), (COUNT, 0.5), (ASYNC, 0.5), (REFRACTION, 0.3)):
                    if rng.random() < p:
                        flags |= f
                yield step, op, (flags, int(rng.integers(1, 4)))
            elif op == "instance":
                m = self.sc.instances[1].matrix.copy()
                m[3, :3] += rng.uniform(-1.5, 1.5, 3).astype(np.float32)
                yield step, op, m
            elif op == "material":
                k = int(rng.integers(1, self.num_materials))
                color = int(rng.integers(0, 1 << 24))
                albedo = int(rng.integers(0, self.num_textures))
                self.a, record = replace_material(self.a, k, color, albedo)
                yield step, op, (k, record)
            elif op == "texels":
                # [3k + 1, 3m + 2): both end texels keep some of their bytes
                k = int(rng.integers(2, self.texel_bytes // 3 - 40))
                m = k + int(rng.integers(1, 32))
                data = rng.integers(0, 256, 3 * m + 2 - (3 * k + 1), dtype=np.uint8)
                self.a = splice_texels(self.a, 3 * k + 1, data)
                yield step, op, (3 * k + 1, data)
            elif op == "mesh":
                v = int(rng.integers(len(self.variants)))
                mesh, tri_start, first_node = self.where
                self.a = replace_mesh(self.a, mesh, tri_start, first_node, self.variants[v])
                yield step, op, v
            else:
                d = rng.normal(size=(64, 3)).astype(np.float32)
                d /= np.linalg.norm(d, axis=1, keepdims=True)
                yield step, op, d

    def set_instances(self, instances):
        """after an instance move: the session's own table (the mirror computes the inverse transform)"""
        self.a["instances"] = np.array(instances)

    def key(self):
        """a digest of everything the oracle reads: the cache key of the expected frames"""
        h = hashlib.sha1()
        for k in ("tris", "nodes", "roots", "materials", "textures", "texels", "instances"):
            h.update(np.ascontiguousarray(self.a[k]).tobytes())
        return h.hexdigest()
