"""Deep traversal stacks for everything that owns a stack (hazard H2; CrtStackT, csrc/crt_device.h): the scene, the rays, the ambient-occlusion
points and the depth probe that tests/test_query_deep_stack_cpu.py (conditions, no GPU) and tests/test_gpu_query_deep_stack.py /
tests/test_gpu_deep_stack.py (the kernels) share. A helper, no test.

Scene: test_gpu_deep_stack.caterpillar(levels) as ONE mesh under three instances -- at the world origin, 60 behind it and 90 to its right --
with the materials, textures and sky of `tiny`. A ray along +z descends a tree to its last level pushing every leaf on the way: levels - 1
entries before the first pop, whatever the kernel keeps in LDS (kLds = 15, 16, 18, 19 or 20), around upstream's 32 slots from 34 levels on and
into the 250-pop cap at 300.
Rays: 321 (five whole 64-ray chunks and a last one of a single ray, so that the spill ballot runs with 63 lanes inactive) seeded by `levels`:
descending rays, rays that point away (k % 8 == 3: a miss with an empty stack) and rays that graze the trees from the side (k % 8 == 5: a few
boxes only) in every chunk -- the mixed waves the per-wave ballot exists for. A ray that hits the last level's triangle has its answer before
the first pop, whatever the stack then returns; the edge rays (k % 8 == 1, k % 16 == 6) find theirs in a chosen slot, and the rays of
k % 8 == 7 start inside the nested boxes, where the inclusive rule differs from upstream's."""
import ctypes as C
import functools

import numpy as np

from clraytracer_amd import _lib, driver, scenes
import oracle_lib

LEVELS = (16, 17, 18, 19, 20, 21, 22, 33, 34, 48, 300)     # pushes 15 .. 21: one below, at and above every kLds (15, 16, 18, 19, 20); the wrap; the cap
N_RAYS = 321
TRANSLATIONS = ((0.0, 0.0, 0.0), (0.0, 0.0, 60.0), (90.0, 0.0, 0.0))
CAMERA = ((0.3, 0.2, -40.0), (0.0, 0.0, 1.0))
# A camera left of the first tree that looks along the edge rays' direction: its pixels' rays cross the triangles' slanted edge at every depth, so
# what they hit is decided by one stack entry each (from CAMERA every ray that hits at all hits the last level's triangle before its first pop)
EDGE_CAMERA = ((-45.0, 0.0, -40.0), (0.15, -0.15, 1.0))
# The frame whose pixels' ambient occlusion walks deep stacks: a fourth tree BEHIND the camera of CAMERA, seen from its shallow side by a
# camera that looks back at it; the normals of its hit points face the camera, so their sample rays run along +z down the three trees in front.
AO_TRANSLATIONS = TRANSLATIONS + ((0.0, 0.0, -150.0),)
AO_CAMERA = ((10.0, 0.2, -20.0), (0.0, 0.0, -1.0))
POISON = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def _tiny_arenas():
    with driver.Session(64, 48, host_only=True) as s:
        s.load_scene(scenes.get("tiny"))
        return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}


def instances():
    inst = np.zeros(len(AO_TRANSLATIONS), _lib.INSTANCE_DTYPE)
    for k, t in enumerate(AO_TRANSLATIONS):
        m = np.eye(4, dtype=np.float32)
        m[3, :3] = -np.asarray(t, np.float32)                # inverseTransform of a translation, row-vector convention
        inst["inv"][k] = m
    inst["meshIndex"], inst["materialStart"] = 0, 0
    return inst


@functools.lru_cache(maxsize=None)
def scene(levels, n_instances=3):
    """the arenas dict for the oracle: tiny's materials, textures and texels around the caterpillar and its instances; never modified"""
    from test_gpu_deep_stack import caterpillar             # (here: that module uses this one for its deep frames)
    a = dict(_tiny_arenas())
    tris, nodes = caterpillar(levels)
    a.update(tris=tris, nodes=nodes, roots=np.zeros(1, np.uint32), instances=instances()[:n_instances])
    for v in a.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return a


def upload(s, a):
    """triangles, roots, nodes and instances of `a` into the live session `s` (after load_scene("tiny")), as test_gpu_deep_stack does it"""
    hip = s.hip
    tris, nodes, roots, inst = (np.array(a[k]) for k in ("tris", "nodes", "roots", "instances"))
    assert hip.crt_upload_triangles(tris.ctypes.data, 0, tris.nbytes) == 0
    assert hip.crt_upload_bvh_roots(roots.ctypes.data, 0, len(roots)) == 0
    assert hip.crt_upload_bvh_nodes(nodes.ctypes.data, 0, nodes.nbytes) == 0
    assert hip.crt_upload_instances(inst.ctypes.data, 0, len(inst)) == 0
    return len(inst)


def tlas_nodes(s):
    b, r, n = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    _lib.check(s.hip.crt_debug_tlas_stats(C.byref(b), C.byref(r), C.byref(n)), "crt_debug_tlas_stats")
    return int(n.value)


def deepest_z(levels):
    """z of the last level's triangle (caterpillar: the one closest to the camera), which is the near face of every nested box"""
    return 100.0 - min(0.75, 90.0 / levels) * (levels - 1)


@functools.lru_cache(maxsize=None)
def rays(levels, n=N_RAYS):
    """(origins, dirs) float32, read-only; directions are not unit vectors (hazard H6: t is in units of their length)"""
    rng = np.random.RandomState(levels)
    o = rng.uniform((-70.0, -40.0, -45.0), (130.0, 40.0, -35.0), size=(n, 3))
    d = np.stack([rng.choice((-0.15, 0.15), n), rng.choice((-0.15, 0.15), n), np.ones(n)], 1)
    k = np.arange(n)
    away, side = k % 8 == 3, k % 8 == 5
    d[away, 2] = -1.0
    o[side] = np.stack([np.full(n, -200.0), rng.uniform(-30.0, 30.0, n), rng.uniform(60.0, 100.0, n)], 1)[side]
    d[side] = np.stack([np.ones(n), np.zeros(n), rng.uniform(-0.05, 0.05, n)], 1)[side]
    # edge rays: inside every box but beside the triangles until they cross the slanted left edge between levels j + 1 and j, so their
    # closest hit is T_j -- found by popping the entries above it and decided by stack slot j % 32 alone; j runs over the top (up to 32) entries from 12 up
    edge = np.flatnonzero((k % 8 == 1) | (k % 16 == 6))
    step = min(0.75, 90.0 / levels)
    for m, r in enumerate(edge):
        lowest = max(12, levels - 33)                        # (what lies 32 entries below the top has been overwritten: the slot index wraps)
        j = lowest + m % (levels - 1 - lowest)
        u = 0.3 + 0.4 * rng.uniform()
        tx, ty, tz = TRANSLATIONS[(0, 2)[m % 2]]
        zc = 100.0 - step * j + 0.2 * u - 0.5 * step + tz
        z0 = o[r, 2]
        o[r, 0], o[r, 1] = -60.0 + 60.0 * u + tx - 0.15 * (zc - z0), -60.0 + 120.0 * u + ty + 0.15 * (zc - z0)
        d[r] = (0.15, -0.15, 1.0)
    o[k % 8 == 7, 2] = deepest_z(levels) + 0.25             # inside every nested box of the first tree (or beside it): upstream's rule skips them, the inclusive one descends
    o[-1], d[-1] = (0.3, 0.2, -40.0), (0.15, -0.15, 1.0)    # the last chunk's only ray descends
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    o.setflags(write=False); d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def ao_points(levels, n=N_RAYS):
    """(P, normals): a 20 x 16 grid in front of the trees (and one point more: a ragged last chunk) looking along +z, every seventh normal zero,
    every sixteenth point inside the trees' nested boxes (behind the last level's triangle), where the inclusive rule differs from upstream's"""
    gx, gy = np.meshgrid(np.linspace(-60.0, 140.0, 20), np.linspace(-45.0, 45.0, 16))
    P = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -38.0)], 1)
    P = np.concatenate([P, [[3.0, 1.0, -41.0]]])[:n].astype(np.float32)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (len(P), 1))
    nrm[6::7] = 0.0
    P[9::16, 2] = deepest_z(levels) + 0.25
    P.setflags(write=False); nrm.setflags(write=False)
    return P, nrm


@functools.lru_cache(maxsize=None)
def camera_of(w, h, camera=CAMERA):
    """(invView, invProj, cameraPos) of a w x h session looking from `camera`, by the host mirror"""
    with driver.Session(w, h, host_only=True) as s:
        s.load_scene(scenes.get("tiny"))
        s.set_camera(camera[0], scenes._normalize(camera[1]))
        return s.camera()


def ao_frame_items(levels, w, h, nthreads=None):
    """(P, n, k) of ao_ref.frame_items for the oracle's planes of the w x h frame of the four-instance scene from AO_CAMERA, and the planes"""
    import ao_ref
    import gbuffer_ref
    iv, ip, pos = camera_of(w, h, AO_CAMERA)
    a = scene(levels, 4)
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    rays = orc.raygen(w, h, iv, ip)
    planes = gbuffer_ref.reference_planes(a, orc, rays, pos)
    return ao_ref.frame_items(planes, rays, pos), planes


def chunk_depths(orc, o, d, chunk=64):
    """maxStack of every `chunk` rays, by the oracle on slices"""
    return [orc.closest_hits(o[k:k + chunk], d[k:k + chunk])[1]["maxStack"] for k in range(0, len(o), chunk)]


def ray_depths(orc, o, d):
    """maxStack of every ray, by the oracle on one-ray slices"""
    return np.array(chunk_depths(orc, o, d, 1))


def oracle(levels, nthreads=None, n_instances=3):
    return oracle_lib.Oracle(scene(levels, n_instances), nthreads=nthreads)


# ---- the C-ABI calls of a session whose geometry was uploaded by hand (the host mirror still counts tiny's instances) ----
def dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def trace_rays(s, ni, to, td, tmax=None, occluded=False, inclusive=False, n=None, tail=0):
    """crt_trace_rays on device tensors: records (_lib.RAYHIT_DTYPE) or occlusion bytes of the first n rays, and the `tail` sentinel rows behind them"""
    import torch
    n = len(to) if n is None else n
    batch = _lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), tmax.data_ptr() if tmax is not None else None, 3, 3, n)
    mode = (_lib.CRT_RAYS_OCCLUDED if occluded else _lib.CRT_RAYS_CLOSEST) | (_lib.CRT_RAYS_INCLUSIVE if inclusive else 0)
    if occluded:
        out = torch.full((n + tail,), 0xA5, dtype=torch.uint8, device="cuda:0")
    else:
        out = torch.full((n + tail, 5), POISON, dtype=torch.int32, device="cuda:0")
    _lib.check(s.hip.crt_trace_rays(C.byref(batch), ni, mode, out.data_ptr(), _stream()), "crt_trace_rays")
    return out


def records(out, n=None):
    x = out if isinstance(out, np.ndarray) else out.cpu().numpy()
    return np.ascontiguousarray(x[:len(x) if n is None else n]).view(_lib.RAYHIT_DTYPE).reshape(-1)


def shade_rays(s, ni, to, td, sun_angle, radiance=True, surface=True):
    import torch
    n = len(to)
    batch = _lib.CrtRayBatch(to.data_ptr(), td.data_ptr(), None, 3, 3, n)
    par = _lib.CrtShadeParams(float(sun_angle), 0)
    rad = torch.full((n, 4), POISON, dtype=torch.int32, device="cuda:0") if radiance else None
    rec = torch.full((n, 12), POISON, dtype=torch.int32, device="cuda:0") if surface else None
    _lib.check(s.hip.crt_shade_rays(C.byref(batch), C.byref(par), ni, rad.data_ptr() if radiance else None, rec.data_ptr() if surface else None, _stream()),
               "crt_shade_rays")
    return (rad.cpu().numpy().view(np.float32) if radiance else None,
            rec.cpu().numpy().view(_lib.SURFACE_HIT_DTYPE).reshape(-1) if surface else None)


def trace_ao(s, ni, tp, tn, par, inclusive=False):
    import torch
    n = len(tp)
    pts = _lib.CrtAoPoints(tp.data_ptr(), tn.data_ptr(), 3, 3, n)
    cp = _lib.CrtAoParams(int(par["samples"]), float(par["radius"]), float(par["bias"]), int(par["seed"]), _lib.CRT_AO_INCLUSIVE if inclusive else 0, 0.0, 0.0)
    out = torch.full((n,), POISON, dtype=torch.int32, device="cuda:0")
    _lib.check(s.hip.crt_trace_ao(C.byref(pts), C.byref(cp), ni, out.data_ptr(), _stream()), "crt_trace_ao")
    return out.cpu().numpy().view(np.float32)


def frame_args(s, ni, sun_angle, camera=CAMERA):
    """(CrtTraceArgs, invView, invProj, cameraPos) of a frame of the uploaded scene from `camera`"""
    s.set_camera(camera[0], scenes._normalize(camera[1]))
    iv, ip, pos = s.camera()
    args = _lib.CrtTraceArgs()
    args.cameraPos[0], args.cameraPos[1], args.cameraPos[2] = [float(x) for x in pos]
    args.time, args.numMeshes, args.sunAngle = 0.0, ni, float(sun_angle)
    return args, iv, ip, pos


def render(s, args, iv, ip, flags):
    fp = C.POINTER(C.c_float)
    return s.hip.crt_render(C.byref(args), iv.ctypes.data_as(fp), ip.ctypes.data_as(fp), int(flags))
