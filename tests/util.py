"""Shared helpers for the parity tests."""
import importlib.util
import os
import re

import numpy as np

# tools/ is no package: the resource compile (one per process, memoised there) and the tool's line format are imported by path
_spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "kernel_resources.py"))
_kernel_resources = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_kernel_resources)
kernel_resources, kernel_resource_rows, resource_line = _kernel_resources.kernel_resources, _kernel_resources.kernel_resource_rows, _kernel_resources.resource_line
HIP_UNITS = _kernel_resources.HIP_UNITS


def unit_sources(unit):
    """`unit` (a path below the repository) and every in-tree file it includes by #include "...", transitively: what the compiler reads of this
    repository when it builds the unit, as sorted absolute paths. A source scan that reads these follows code that moves into a shared header."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seen, todo = set(), [os.path.join(root, unit)]
    while todo:
        path = os.path.normpath(todo.pop())
        if path in seen:
            continue
        assert path.startswith(root + os.sep) and os.path.isfile(path), path
        seen.add(path)
        todo += [os.path.join(os.path.dirname(path), inc) for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M)]
    return sorted(seen)


def seeded_rays(scene_arenas, cam_pos, n, seed):
    """n world-space rays: half from the camera towards the scene, half random origins/directions."""
    rng = np.random.RandomState(seed)
    tris = scene_arenas["tris"]
    inst = scene_arenas["instances"]
    # aim at random triangle centroids pushed through a random instance transform (approximate world
    # positions are good enough: we only need rays that hit things)
    k = rng.randint(0, len(tris), size=n)
    target = (tris["v0"][k] + tris["v1"][k] + tris["v2"][k]) / 3.0
    ii = rng.randint(0, len(inst), size=n)
    inv = inst["inv"][ii].astype(np.float64)
    fwd = np.linalg.inv(inv)
    tw = np.einsum("ni,nij->nj", np.concatenate([target.astype(np.float64), np.ones((n, 1))], 1), fwd)[:, :3]
    origins = np.tile(np.asarray(cam_pos, np.float64), (n, 1))
    half = n // 2
    origins[half:] = tw[half:] + rng.normal(size=(n - half, 3)) * 8.0 + np.array([0, 6.0, 0])
    d = tw + rng.normal(size=(n, 3)) * 0.05 - origins
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return origins.astype(np.float32), d.astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def live_resources():
    """Device buffers, pinned buffers, events and streams libcrt_hip.so holds right now (crt_debug_live_resources; needs no session)."""
    import ctypes as C
    from clraytracer_amd import _lib
    n = C.c_uint64(0)
    _lib.check(_lib.hip().crt_debug_live_resources(C.byref(n)), "crt_debug_live_resources")
    return int(n.value)
