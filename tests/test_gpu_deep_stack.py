"""Hazard H2: upstream's traversal stack is `int nodesToVisit[32]` with no overflow check (kernel_main.cl:126,154).
The oracle pins the undefined overflow as "slot index wraps modulo 32"; the HIP path keeps 20 slots in LDS and the
other 12 in a per-workgroup overflow area (CrtStack, crt_device.h) and must reproduce exactly that -- including a hand-built 48-level caterpillar
tree whose rays push 47 far children before the first pop, and the 250-pop cap on a tree deeper than the cap.
Every Trace kernel form walks them (CRT_KERNEL: the megakernel, wavefront, ldstop with 15 slots per wave, refill with 18 and block with 18
beside their parked rows), and the default form's other instantiations walk the three-instance scene of tests/deep_stack_ref.py at every
level count around their own LDS boundary: with the instance tree (16 slots, 15 with shadow rays), with the first-hit planes, 2 x 2
supersampled and with refraction."""
import ctypes as C
import functools

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import deep_stack_ref as ds
import gbuffer_ref
import oracle_lib
from util import bits

pytestmark = pytest.mark.gpu
COUNT, ASYNC, SHADOWS, REFRACT, SSAA2, GBUFFER = 8, 4, 32, 256, 2048, 8192
# crt_debug_last_kernel of a frame by kernel form: c = counted, s = shadow rays
KERNELS = {"megakernel": "crt_trace_kernel<{c},0,{s},0,0>", "wavefront": "crt_primary_kernel<{c}>+crt_wavefront_scan_kernel+crt_bounce_kernel<{c}>",
           "ldstop": "crt_trace_ldstop_kernel<{c}>", "refill": "crt_trace_refill_kernel<{c},0>", "block": "crt_trace_block_kernel<{c},0>"}


def half(x):
    return np.asarray(x, np.float16).view(np.uint16)


def caterpillar(levels, reverse=False):
    """Level k holds one leaf triangle T_k; inner node N_k = {inner N_{k+1} (near for a +z ray), leaf T_k (far)}.
    Deeper triangles are closer to the camera, so a ray descends all the way down pushing every leaf on the way."""
    tris = np.zeros(levels, _lib.TRI_DTYPE)
    for k in range(levels):
        step = min(0.75, 90.0 / levels)                     # every level stays in front of the camera
        z = 100.0 - step * k
        s = 60.0                                            # big enough that every level covers the view
        if reverse:
            z = 100.0 - step * (levels - 1 - k)
        tris["v0"][k] = (-s, -s, z); tris["v1"][k] = (s, -s, z + 0.1); tris["v2"][k] = (0.0, s, z + 0.2)
        tris["uv"][k] = half([0, 0, 1, 0, 0.5, 1])
        tris["mat"][k] = k % 2
        tris["n"][k] = half([0, 0, -1] * 3)
    for k in range(levels):
        c = (tris["v0"][k] + tris["v1"][k] + tris["v2"][k]) * np.float32(0.333333)
        tris["cx"][k], tris["cy"][k], tris["cz"][k] = c
    nodes = np.zeros(2 * levels - 1, _lib.NODE_DTYPE)

    def tri_box(k0, k1):
        v = np.concatenate([tris[f][k0:k1] for f in ("v0", "v1", "v2")])
        return v.min(0), v.max(0)

    # node 0 = root N_0; pair k at (2k+1, 2k+2) = (N_{k+1} or the last leaf, leaf T_k)
    lo, hi = tri_box(0, levels)
    nodes["min"][0], nodes["max"][0], nodes["leftFirst"][0], nodes["triCount"][0] = lo, hi, 1, 0
    for k in range(levels - 1):
        a, b = 2 * k + 1, 2 * k + 2
        lo, hi = tri_box(k + 1, levels)
        if k + 1 == levels - 1:                              # deepest level: both children are leaves
            nodes["min"][a], nodes["max"][a], nodes["leftFirst"][a], nodes["triCount"][a] = lo, hi, levels - 1, 1
        else:
            nodes["min"][a], nodes["max"][a], nodes["leftFirst"][a], nodes["triCount"][a] = lo, hi, 2 * (k + 1) + 1, 0
        lo, hi = tri_box(k, k + 1)
        nodes["min"][b], nodes["max"][b], nodes["leftFirst"][b], nodes["triCount"][b] = lo, hi, k, 1
    return tris, nodes


@pytest.fixture(params=["megakernel", "wavefront", "ldstop", "refill", "block"])
def structure(request, monkeypatch):
    """CRT_KERNEL (read by crt_init): the default megakernel or the one-launch-per-bounce form, which share CrtStack (20 LDS slots), the
    four-wave form with the tree tops in LDS, whose waves keep 15 slots in LDS and index the overflow area by wave (CrtStackTop), and the two
    compaction forms, which park the pixel index and energy (refill, CrtStackT<2>) or the ray list (block, CrtStackT<CRT_BLOCK_TILES>) in the
    stack's last LDS rows and own an overflow block per block of tiles."""
    monkeypatch.delenv("CRT_TLAS", raising=False)
    if request.param != "megakernel":
        monkeypatch.setenv("CRT_KERNEL", request.param)
    else:
        monkeypatch.delenv("CRT_KERNEL", raising=False)
    return request.param


# (16 .. 19 and 21 levels: with 20 and 22, one level count that just fills and one that first spills the 15, 18 and 20 LDS slots of the kernel forms)
@pytest.mark.parametrize("levels,reverse", [(20, False), (22, False), (31, False), (34, False), (48, False), (48, True), (300, False),
                                            (16, False), (17, False), (18, False), (19, False), (21, False)])
def test_hand_built_deep_tree_matches_oracle(levels, reverse, structure, nthreads):
    sc = scenes.get("tiny")
    hip = _lib.hip()
    W, H = (640, 368) if levels == 48 else (96, 64)      # 48 levels: thousands of waves deep in the overflow slots at once
    with driver.Session(W, H, device=0) as s:
        s.load_scene(sc)                                     # materials, textures, skybox
        a = dict(s.arenas())
        tris, nodes = caterpillar(levels, reverse)
        roots = np.zeros(1, np.uint32)
        inst = np.zeros(1, _lib.INSTANCE_DTYPE)
        inst["inv"][0] = np.eye(4, dtype=np.float32)
        inst["meshIndex"], inst["materialStart"] = 0, 0
        assert hip.crt_upload_triangles(tris.ctypes.data, 0, tris.nbytes) == 0
        assert hip.crt_upload_bvh_roots(roots.ctypes.data, 0, 1) == 0
        assert hip.crt_upload_bvh_nodes(nodes.ctypes.data, 0, nodes.nbytes) == 0
        assert hip.crt_upload_instances(inst.ctypes.data, 0, 1) == 0
        a.update(tris=tris, nodes=nodes, roots=roots, instances=inst)
        orc = oracle_lib.Oracle(a, nthreads=nthreads)
        s.set_camera((0.3, 0.2, -40.0), scenes._normalize((0.0, 0.0, 1.0)))
        iv, ip, pos = s.camera()
        args = _lib.CrtTraceArgs()
        args.cameraPos[0], args.cameraPos[1], args.cameraPos[2] = [float(x) for x in pos]
        args.time, args.numMeshes, args.sunAngle = 0.0, 1, float(sc.sun_angle)
        fp = C.POINTER(C.c_float)
        ref, st = orc.trace(orc.raygen(W, H, iv, ip), pos, sc.sun_angle)
        for flags in ((8, 0, 4, 4) if structure != "megakernel" else (8, 0, 4, 4, 8 | 32)):   # shadow rays: default kernel only
            assert hip.crt_render(C.byref(args), iv.ctypes.data_as(fp), ip.ctypes.data_as(fp), flags) == 0
            assert s.last_kernel() == KERNELS[structure].format(c=int(flags & 8 != 0), s=int(flags & 32 != 0)), (structure, flags)
            if flags & 32:
                ref, st = orc.trace(orc.raygen(W, H, iv, ip), pos, sc.sun_angle, shadows=True)
            assert np.array_equal(bits(s.read_output()), bits(ref)), (levels, flags)
            if flags & 8:
                assert s.counters() == st, (levels, flags)
        if not reverse:
            assert st["maxStack"] == min(levels - 1, 249) or levels > 250
        if levels in (34, 48) and not reverse:
            assert st["stackOverflows"] > 0
        if levels == 300:
            assert st["capHits"] > 0


# ---- the default form's other instantiations on the three-instance scene (tests/deep_stack_ref.py; its conditions: tests/test_query_deep_stack_cpu.py) ----
W, H = 96, 64
SUN = scenes.get("tiny").sun_angle


@functools.lru_cache(maxsize=None)
def frames(levels):
    """the oracle's frames (and their work counters) of the W x H view of deep_stack_ref.EDGE_CAMERA: computed once, never modified"""
    a = ds.scene(levels)
    orc = oracle_lib.Oracle(a, nthreads=16)
    iv, ip, pos = ds.camera_of(W, H, ds.EDGE_CAMERA)
    rays = orc.raygen(W, H, iv, ip)
    out = {"plain": orc.trace(rays, pos, SUN), "shadows": orc.trace(rays, pos, SUN, shadows=True), "refraction": orc.trace(rays, pos, SUN, refraction=True),
           "hi": orc.trace(orc.raygen(2 * W, 2 * H, iv, ip), pos, SUN), "planes": gbuffer_ref.reference_planes(a, orc, rays, pos)}
    assert out["plain"][1]["maxStack"] == out["hi"][1]["maxStack"] == levels - 1
    assert not np.array_equal(bits(out["refraction"][0]), bits(out["plain"][0]))      # the trees' materials are translucent
    return out


def default_session(monkeypatch, tlas):
    monkeypatch.delenv("CRT_KERNEL", raising=False)
    monkeypatch.setenv("CRT_TLAS", tlas)
    s = driver.Session(W, H, device=0)
    s.load_scene(scenes.get("tiny"))
    return s


def upload_and_aim(s, levels, tlas):
    ni = ds.upload(s, ds.scene(levels))
    if tlas == "1":
        assert ds.tlas_nodes(s) > 0
    args, iv, ip, pos = ds.frame_args(s, ni, SUN, ds.EDGE_CAMERA)
    want = ds.camera_of(W, H, ds.EDGE_CAMERA)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip((iv, ip, pos), want))
    return args, iv, ip


@pytest.mark.parametrize("tlas", ["0", "1"])
def test_three_instances_with_and_without_the_instance_tree(monkeypatch, tlas):
    wants = {levels: frames(levels) for levels in ds.LEVELS}      # before the session: the host mirror holds one session at a time
    with default_session(monkeypatch, tlas) as s:
        for levels in ds.LEVELS:
            want = wants[levels]
            args, iv, ip = upload_and_aim(s, levels, tlas)
            for flags in (COUNT, 0, ASYNC, ASYNC, COUNT | SHADOWS, SHADOWS):
                ref, st = want["shadows" if flags & SHADOWS else "plain"]
                assert ds.render(s, args, iv, ip, flags) == 0
                assert s.last_kernel() == f"crt_trace_kernel<{int(flags & COUNT != 0)},0,{int(flags & SHADOWS != 0)},{tlas},0>", (levels, flags)
                assert np.array_equal(bits(s.read_output()), bits(ref)), (levels, flags)
                if flags & COUNT:
                    assert s.counters() == st, (levels, flags)


@pytest.mark.parametrize("form", ["wavefront", "ldstop", "refill", "block"])
def test_three_instances_through_the_other_kernel_forms(monkeypatch, form):
    """the same frames through the opt-in forms: their pixels need what the spilled entries hold, which the one-tree frames above do not"""
    wants = {levels: frames(levels) for levels in ds.LEVELS}
    monkeypatch.setenv("CRT_KERNEL", form)
    monkeypatch.delenv("CRT_TLAS", raising=False)
    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get("tiny"))
        for levels in ds.LEVELS:
            ref, st = wants[levels]["plain"]
            args, iv, ip = upload_and_aim(s, levels, "0")
            for flags in (COUNT, 0, ASYNC, ASYNC):
                assert ds.render(s, args, iv, ip, flags) == 0
                assert s.last_kernel() == KERNELS[form].format(c=int(flags & COUNT != 0), s=0), (levels, flags)
                assert np.array_equal(bits(s.read_output()), bits(ref)), (levels, flags)
                if flags & COUNT:
                    assert s.counters() == st, (levels, flags)


@pytest.mark.parametrize("tlas", ["0", "1"])
def test_gbuffer_frames_of_deep_trees(monkeypatch, tlas):
    wants = {levels: frames(levels) for levels in ds.LEVELS}
    with default_session(monkeypatch, tlas) as s:
        for levels in ds.LEVELS:
            want = wants[levels]
            args, iv, ip = upload_and_aim(s, levels, tlas)
            for flags in (GBUFFER, GBUFFER | SHADOWS):
                assert ds.render(s, args, iv, ip, flags) == 0
                assert s.last_kernel() == f"crt_trace_gbuffer_kernel<{int(flags & SHADOWS != 0)},{tlas},0>", (levels, flags)
                got = s.read_gbuffer_raw()
                for p in ("geometry", "ids", "albedo"):
                    assert np.array_equal(np.ascontiguousarray(got[p]).view(np.uint32), np.ascontiguousarray(want["planes"][p]).view(np.uint32)), (levels, flags, p)
                assert np.array_equal(bits(s.read_output()), bits(want["shadows" if flags & SHADOWS else "plain"][0])), (levels, flags)


@pytest.mark.parametrize("tlas", ["0", "1"])
def test_supersampled_frames_of_deep_trees(monkeypatch, tlas):
    from test_gpu_ssaa import resolve
    wants = {levels: frames(levels) for levels in ds.LEVELS}
    with default_session(monkeypatch, tlas) as s:
        for levels in ds.LEVELS:
            hi, st = wants[levels]["hi"]
            args, iv, ip = upload_and_aim(s, levels, tlas)
            for flags in (SSAA2 | COUNT, SSAA2):
                assert ds.render(s, args, iv, ip, flags) == 0
                assert s.last_kernel() == f"crt_trace_ssaa_kernel<{int(flags & COUNT != 0)},0,{tlas},0>", (levels, flags)
                assert np.array_equal(bits(s.read_output()), bits(resolve(hi, 2))), (levels, flags)
                if flags & COUNT:
                    assert s.counters() == st, levels


@pytest.mark.parametrize("tlas", ["0", "1"])
def test_refraction_frames_of_deep_trees(monkeypatch, tlas):
    wants = {levels: frames(levels) for levels in ds.LEVELS}
    with default_session(monkeypatch, tlas) as s:
        for levels in ds.LEVELS:
            ref, st = wants[levels]["refraction"]
            args, iv, ip = upload_and_aim(s, levels, tlas)
            for flags in (REFRACT | COUNT, REFRACT):
                assert ds.render(s, args, iv, ip, flags) == 0
                assert s.last_kernel() == f"crt_trace_kernel<{int(flags & COUNT != 0)},0,0,{tlas},1>", (levels, flags)
                assert np.array_equal(bits(s.read_output()), bits(ref)), (levels, flags)
                if flags & COUNT:
                    assert s.counters() == st, levels
