"""crt_shade_rays without a GPU: the ABI (the call, the two structs and their sizes in the headers and both ctypes tables, the refusal before
crt_init) and the
numpy restatement the GPU tests compare the surface records with (tests/shade_ref.py), pinned two ways: the albedo sampled again from a
record's own (material, texU, texV) is its `albedo` field, and shading bounce 0 from the records reproduces the oracle's primary-only
frame bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import gbuffer_ref
import oracle_lib
import shade_ref
from util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORC_EXT_PRIMARY_ONLY = 4                  # oracle/crt_oracle.h


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_headers_declare_the_call_and_the_struct_sizes():
    api, types, host, debug = header("crt_api.h"), header("crt_types.h"), header("crt_host.h"), header("crt_debug.h")
    assert ("int crt_shade_rays(const CrtRayBatch* rays, const CrtShadeParams* params, uint32_t numInstances, float* radiance, "
            "CrtSurfaceHit* surface, void* stream);") in api
    assert "int crt_debug_shade_stats(uint64_t out[3]);" in debug
    assert "int crth_shade_rays(const CrtRayBatch* rays, const CrtShadeParams* params, float* radiance, CrtSurfaceHit* surface, void* stream);" in host
    assert re.search(r"typedef struct CrtSurfaceHit \{\s*float normal\[3\];\s*float t;\s*int32_t instance;[^}]*uint32_t triIndex;\s*float u, v;\s*"
                     r"uint32_t albedo;[^}]*uint32_t material;[^}]*float texU, texV;[^}]*\} CrtSurfaceHit;", types)
    assert re.search(r"typedef struct CrtShadeParams \{\s*float sunAngle;[^}]*uint32_t flags;[^}]*\} CrtShadeParams;", types)
    assert re.search(r"static_assert\(sizeof\(CrtSurfaceHit\) == 48,", types)
    assert re.search(r"static_assert\(sizeof\(CrtShadeParams\) == 8,", types)


def test_bindings_and_dtypes():
    for n in ("crt_shade_rays", "crt_debug_shade_stats"):
        assert n in _lib.HIP_API and hasattr(_lib.hip(), n), n
    assert "crth_shade_rays" in _lib.HOST_API and hasattr(_lib.host(), "crth_shade_rays")
    s, p = _lib.SURFACE_HIT_DTYPE, _lib.GBUFFER_PIXEL_DTYPE
    assert s.itemsize == 48 and C.sizeof(_lib.CrtShadeParams) == 8
    # the first 36 bytes are the G-buffer pixel, field for field
    assert [(f, s.fields[f][0], s.fields[f][1]) for f in p.names] == [(f, p.fields[f][0], p.fields[f][1]) for f in p.names]
    assert [s.fields[f][1] for f in ("material", "texU", "texV")] == [36, 40, 44]
    import inspect
    sig = inspect.signature(driver.Session.shade_rays).parameters
    assert [k for k in sig] == ["self", "origins", "dirs", "tmax", "sun_angle", "radiance", "surface"]
    assert sig["tmax"].default is None and sig["sun_angle"].default is None and sig["radiance"].default is True and sig["surface"].default is False


def test_the_call_refuses_before_init():
    hip = _lib.hip()
    # no crt_init has been made in this process (tests/test_abi.py relies on the same)
    buf = np.zeros(64 * 12, np.float32)
    batch = _lib.CrtRayBatch(buf.ctypes.data, buf.ctypes.data, None, 3, 3, 64)
    par = _lib.CrtShadeParams(0.5, 0)
    assert hip.crt_shade_rays(C.byref(batch), C.byref(par), 1, buf.ctypes.data, buf.ctypes.data, None) == _lib.CRT_E_NOT_INITIALIZED
    assert hip.crt_shade_rays(None, None, 1, None, None, None) == _lib.CRT_E_NOT_INITIALIZED
    assert hip.crt_debug_shade_stats((C.c_uint64 * 3)()) == _lib.CRT_E_NOT_INITIALIZED
    with driver.Session(64, 48, host_only=True) as s:
        s.load_scene(scenes.get("tiny"))
        assert s.h.crth_shade_rays(C.byref(batch), C.byref(par), buf.ctypes.data, None, None) == 0
        assert s.h.crth_last_error() == _lib.CRT_E_NOT_INITIALIZED
        s.h.crth_clear_error()


@pytest.mark.parametrize("name,w,h", [("tiny", 131, 67), ("cornell-1k", 160, 96)])
def test_the_restatement_is_pinned(name, w, h, nthreads):
    sc = scenes.get(name)
    with driver.Session(w, h, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        iv, ip, pos = s.camera()
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    rays = orc.raygen(w, h, iv, ip)
    surf = shade_ref.surface(a, orc, pos, rays.reshape(-1, 3))
    hit = surf["instance"] >= 0
    assert int(hit.sum()) >= 500 and not hit.all()          # both kinds of record are exercised
    # 1. the albedo of every hit, sampled again from the record's own material index and uv
    again = shade_ref.resample_albedo(a, surf[hit])
    print(f"{name} {w}x{h}: {int((again == surf['albedo'][hit]).sum())} of {int(hit.sum())} albedos reproduced")
    assert np.array_equal(again, surf["albedo"][hit])
    assert (surf["material"][hit] < 256).all() and np.isfinite(surf["texU"][hit]).all() and np.isfinite(surf["texV"][hit]).all()
    # a miss is the miss record, all twelve words
    assert shade_ref.same_surface(surf[~hit], np.full(int((~hit).sum()), shade_ref.MISS))
    # 2. bounce 0 shaded from the records is the oracle's primary-only frame
    got, shaded = gbuffer_ref.shade_primary(a, shade_ref.planes_of(surf, h, w), rays, pos, sc.sun_angle)
    ref = np.zeros((h, w, 4), np.float32)
    args = oracle_lib.CrtTraceArgs()
    args.cameraPos[0], args.cameraPos[1], args.cameraPos[2] = [float(x) for x in pos]
    args.time = 0.0; args.numMeshes = orc.s.numInstances; args.sunAngle = float(sc.sun_angle)
    st = oracle_lib.OrcStats()
    oracle_lib.lib().orc_trace_ex(C.byref(orc.s), C.byref(args), rays.ctypes.data, w, h, 0, h, ref.ctypes.data, C.byref(st), nthreads, ORC_EXT_PRIMARY_ONLY)
    equal = (bits(got) == bits(ref[..., :3])).all(axis=2)
    print(f"{name} {w}x{h}: {int((equal & shaded).sum())} of {int(shaded.sum())} hit pixels bit-equal")
    assert np.array_equal(shaded.reshape(-1), hit) and int(shaded.sum()) == st.as_dict()["hits"]
    assert (equal | ~shaded).all()
    # radiance of the reference: one oracle call per origin, the same as the oracle's frame of these rays
    frame, _ = orc.trace(rays, pos, sc.sun_angle)
    rad = shade_ref.radiance(orc, pos, rays.reshape(-1, 3), sc.sun_angle)
    assert np.array_equal(bits(rad), bits(frame.reshape(-1, 4)))
    # ... and under a bound: kept hits keep their radiance, cut rays have the sky's, which no instance changes
    tmax = np.where(np.arange(w * h) % 2 == 0, surf["t"] * np.float32(2.0), surf["t"] * np.float32(0.5)).astype(np.float32)
    brad, kept = shade_ref.bounded_radiance(a, orc, pos, rays.reshape(-1, 3), sc.sun_angle, tmax, nthreads)
    assert np.array_equal(kept, hit & (np.arange(w * h) % 2 == 0))
    assert np.array_equal(bits(brad[kept]), bits(rad[kept])) and np.array_equal(bits(brad[~hit]), bits(rad[~hit]))
