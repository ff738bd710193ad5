"""The staged cull terms of the camera bounce (staged_candidate_mask, crt_device.h) live in the wave's stack rows 0..5 until the mask
is read; the traversal behind them must find an empty stack. tests/test_gpu_deep_stack.py's hand-built caterpillar trees push 19 and
249 far children before the first pop -- through every staged row, into the overflow block and around the 32-slot wrap -- in the
uncounted kernel, plain and with shadow rays (whose stack has one row fewer), against the oracle bit for bit."""
import ctypes as C

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import oracle_lib
from test_gpu_deep_stack import caterpillar
from util import bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("levels", [20, 300])
def test_deep_trees_through_the_uncounted_kernel(levels, nthreads):
    sc = scenes.get("tiny")
    hip = _lib.hip()
    W, H = 72, 40
    with driver.Session(W, H, device=0) as s:
        s.load_scene(sc)
        a = dict(s.arenas())
        tris, nodes = caterpillar(levels)
        roots = np.zeros(1, np.uint32)
        inst = np.zeros(1, _lib.INSTANCE_DTYPE)
        inst["inv"][0] = np.eye(4, dtype=np.float32)
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
        rays = orc.raygen(W, H, iv, ip)
        for flags, kernel, opts in ((0, "crt_trace_kernel<0,0,0,0,0>", {}), (32, "crt_trace_kernel<0,0,1,0,0>", {"shadows": True})):
            ref, st = orc.trace(rays, pos, sc.sun_angle, **opts)
            assert st["maxStack"] == min(levels - 1, 249) or levels > 250
            assert hip.crt_render(C.byref(args), iv.ctypes.data_as(fp), ip.ctypes.data_as(fp), flags) == 0
            assert s.last_kernel() == kernel
            assert np.array_equal(bits(s.read_output()), bits(ref)), (levels, flags)
