"""The inclusive box test of the device queries (CRT_RAYS_INCLUSIVE / CRT_AO_INCLUSIVE, include/crt_api.h), the part that needs no GPU: the
numpy reference (tests/inclusive_ref.py) against the all-triangles search of oracle/brute_force.c on rays that start on surfaces, the bound
rule on the inclusive records, the ABI before crt_init, and a
physics check of the inclusive AO on a scene whose answer is known.
Under upstream's rule (kernel_main.cl:115, tnear > 0) a ray from a surface sees a fraction of the scene; under the inclusive rule it must see
what the search sees."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import ao_ref
import inclusive_ref as ir
import oracle_lib
import trace_rays_ref as rr
from test_abi import declared
from test_brute_force import brute_force
from util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# scene -> (camera grid, the number of surface rays it gives)
SURFACE_SETS = {"tiny": ((256, 144), 4550), "cornell-1k": ((256, 144), 10474), "sponza-sibenik": ((128, 72), 9170),
                "nanosuit-demo": ((96, 54), 1642), "multi-1M": ((48, 27), 454)}


def load(name, nthreads):
    """arenas, camera, per-mesh (triangle start, triangle count) and an oracle of scene `name`"""
    with driver.Session(64, 48, host_only=True) as s:
        s.load_scene(scenes.get(name))
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        cam = s.camera()
        nmesh = s.h.crth_num_meshes()
        info = np.zeros((nmesh, 4), np.uint32)
        for m in range(nmesh):
            s.h.crth_mesh_info(m, info[m].ctypes.data)
    return a, cam, np.ascontiguousarray(info[:, 1]), np.ascontiguousarray(info[:, 0]), oracle_lib.Oracle(a, nthreads=nthreads)


@pytest.mark.parametrize("name", list(SURFACE_SETS))
def test_inclusive_reference_sees_what_the_all_triangles_search_sees(name, nthreads):
    (w, h), count = SURFACE_SETS[name]
    a, (iv, ip, pos), mesh_start, mesh_count, orc = load(name, nthreads)
    o, d = ir.surface_rays(a, orc, iv, ip, pos, w, h)
    assert len(o) == count
    up, _ = ir.closest_hits(a, o, d, inclusive=False)
    inc, st = ir.closest_hits(a, o, d)
    bf = brute_force(a, mesh_start, mesh_count, o, d, nthreads)
    hit_bf, hit_inc = bf["instance"] >= 0, inc["instance"] >= 0
    same = (inc["instance"] == bf["instance"]) & (inc["tri"] == bf["tri"])
    for f in ("t", "u", "v"):
        same &= bits(inc[f]) == bits(bf[f])
    same |= ~hit_bf & ~hit_inc                                   # a miss on both sides
    tied = hit_bf & (bf["ties"] > 0)
    comparable = ~tied
    wrong = comparable & ~same
    nearer = wrong & hit_bf & hit_inc & (inc["t"] < bf["t"])
    share_up, share_inc, share_bf = float((up["instance"] >= 0).mean()), float(hit_inc.mean()), float(hit_bf.mean())
    print(f"{name}: {len(o)} surface rays; hit share upstream {share_up:.3f}, inclusive {share_inc:.3f}, all-triangles {share_bf:.3f}; "
          f"{int(wrong.sum())} of {int(comparable.sum())} comparable records differ ({int(nearer.sum())} nearer than the search's); {int(tied.sum())} tied; "
          f"cap hits {st['capHits']}, stack overflows {st['stackOverflows']}, max stack {st['maxStack']}, pops/ray {st['pops'] / len(o):.1f}")
    assert st["capHits"] == 0
    assert tied.sum() <= 0.01 * len(o)
    # the traversal tests a subset of the search's triangles: where the search finds nothing, so does it
    assert not (~hit_bf & hit_inc).any()
    assert wrong.sum() <= max(2, int(2e-3 * comparable.sum()))  # tests/test_brute_force.py's bound for grazing differences
    assert not nearer.any()
    assert share_inc > share_up


@functools.lru_cache(maxsize=None)
def query_set(name):
    """arenas, the 4099 rays of ir.query_rays and their unbounded inclusive records: computed once, never modified"""
    a, (iv, ip, pos), _, _, orc = load(name, 8)
    o, d = ir.query_rays(a, orc, iv, ip, pos, name)
    ref, st = ir.closest_hits(a, o, d)
    assert st["capHits"] == 0
    for x in (o, d, ref):
        x.setflags(write=False)
    return a, o, d, ref


@pytest.mark.parametrize("name", ["tiny", "cornell-1k"])
def test_bounds_filter_the_unbounded_inclusive_records(name):
    a, o, d, ref = query_set(name)
    assert len(o) == 4099
    finite = np.isfinite(ref["u"]) & np.isfinite(ref["v"])       # the filter's precondition (include/crt_api.h)
    hits = ref["instance"] >= 0
    assert finite.sum() >= 4000 and hits.sum() >= 1000                 # (the 1999 surface rays alone hit on more than half)
    for fam, (tmax, kept) in rr.tmax_families(ref).items():
        got, _ = ir.closest_hits(a, o, d, tmax)
        want = rr.filtered(ref, tmax)
        assert rr.same_records(got[finite], want[finite]), fam
        assert np.array_equal((want["instance"] >= 0)[finite], (hits if kept else np.zeros_like(hits))[finite]), fam


def test_abi_declares_the_flags_and_the_calls_refuse_before_init():
    header = open(os.path.join(ROOT, "include", "crt_api.h")).read()
    assert int(re.search(r"CRT_RAYS_INCLUSIVE\s*=\s*(\w+)", header).group(1), 0) == 0x100 == _lib.CRT_RAYS_INCLUSIVE
    assert int(re.search(r"CRT_AO_INCLUSIVE\s*=\s*(\w+)", header).group(1), 0) == 4 == _lib.CRT_AO_INCLUSIVE
    assert _lib.CRT_AO_INCLUSIVE != 2 and not (_lib.CRT_AO_INCLUSIVE & _lib.CRT_AO_FILTER)
    assert {"crt_trace_rays", "crt_trace_ao", "crt_frame_ao"} <= set(declared("crt_api.h", "crt_"))
    hip = _lib.hip()
    # no crt_init has been made in this process (tests/test_abi.py relies on the same)
    buf = np.zeros(64 * 5, np.float32)
    batch = _lib.CrtRayBatch(buf.ctypes.data, buf.ctypes.data, None, 3, 3, 64)
    for mode in (_lib.CRT_RAYS_INCLUSIVE, _lib.CRT_RAYS_INCLUSIVE | _lib.CRT_RAYS_OCCLUDED):
        assert hip.crt_trace_rays(C.byref(batch), 1, mode, buf.ctypes.data, None) == _lib.CRT_E_NOT_INITIALIZED
    pts = _lib.CrtAoPoints(buf.ctypes.data, buf.ctypes.data, 3, 3, 64)
    par = _lib.CrtAoParams(8, 1.0, 1e-3, 0, _lib.CRT_AO_INCLUSIVE, 0.0, 0.0)
    assert hip.crt_trace_ao(C.byref(pts), C.byref(par), 1, buf.ctypes.data, None) == _lib.CRT_E_NOT_INITIALIZED
    assert hip.crt_frame_ao(C.byref(par), None) == _lib.CRT_E_NOT_INITIALIZED


def _corner_mesh_scene(tmp_path):
    """The floor and the wall of tests/test_ao_cpu.py (_corner_scene: a 6 x 6 floor through the origin, normal +y, a 6 x 3 wall standing on it in
    the plane z = 0, normal +z, leaning by 0.002 rad) as ONE mesh with one instance: every sample ray of a point on the floor starts inside
    the mesh's boxes."""
    d = str(tmp_path)
    sky = os.path.join(d, "sky.ppm")
    scenes.write_ppm(sky, scenes._skybox(64, 32))
    lean = 0.002
    Rx = np.array([[1, 0, 0], [0, np.cos(lean), -np.sin(lean)], [0, np.sin(lean), np.cos(lean)]])
    m = scenes.Mesh.concat([scenes._grid((-3, 0, 3), (6, 0, 0), (0, 0, -6), 6, 6, (0, 1, 0)), scenes._grid((-3, 0, 0), (6, 0, 0), (0, 3, 0), 6, 3, (0, 0, 1))])
    m.pos = (m.pos.astype(np.float64) @ Rx.T).astype(np.float32)
    m.nrm = (m.nrm.astype(np.float64) @ Rx.T).astype(np.float32)
    obj = scenes._write_mesh(d, "corner", m, [((0.7, 0.7, 0.7), None)])
    sc = scenes.Scene("ao-corner-one-mesh", d, sky, [obj], [scenes.Instance(0, 0xFFFF, np.eye(4, dtype=np.float32))], (0.0, 1.0, 3.0), (0.0, 0.0, -1.0))
    with driver.Session(64, 48, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
    return a, Rx


def _composed_ao(a, P, n, k, par, inclusive):
    """ao_ref.compose over the reference's bounded records (tmax = R) under the given rule"""
    o, d, w = ao_ref.rays(P, n, k, par, ao_ref.table())
    N = par["samples"]
    rec, st = ir.closest_hits(a, np.repeat(o, N, axis=0), d.reshape(-1, 3), np.full(len(o) * N, par["radius"], np.float32), inclusive=inclusive)
    assert st["capHits"] == 0
    occ = (rec["instance"] >= 0).reshape(len(o), N)
    return ao_ref.compose(w, occ), occ


K0, COUNT = 1000, 256


def test_inclusive_ao_of_one_mesh_foot_of_a_wall_and_open_floor(tmp_path):
    """A point on the floor 0.02 in front of a perpendicular wall of the SAME mesh, both reaching farther than R = 1: the wall covers the half
    of the hemisphere behind its plane, cosine-weighted share 1/2, minus the sliver of rays that leave the radius before they arrive:
    analytically 0.51 (tests/test_ao_cpu.py measures 0.5099 on the two-mesh scene under upstream's rule). 256 items x 64 samples = 16,384
    sample rays: a standard error of 0.5 / sqrt(16384) = 0.0039; the bound is five of them, 0.02. A point 1.1 in front of the wall sees
    nothing within R: exactly 1."""
    a, R = _corner_mesh_scene(tmp_path)
    k = np.arange(K0, K0 + COUNT, dtype=np.uint32)
    n = np.tile((np.array([0.0, 1.0, 0.0]) @ R.T).astype(np.float32), (COUNT, 1))
    par = {"samples": 64, "radius": 1.0, "bias": 1e-3, "seed": 0}
    foot = np.tile((np.array([0.3, 0.0, 0.02]) @ R.T).astype(np.float32), (COUNT, 1))
    ao, occ = _composed_ao(a, foot, n, k, par, True)
    mean = float(ao.astype(np.float64).mean())
    up, occ_up = _composed_ao(a, foot, n, k, par, False)
    print(f"one-mesh corner, foot of the wall: inclusive mean AO {mean:.6f} ({occ.mean():.4f} of the sample rays occluded); "
          f"upstream's rule on the same scene: mean AO {float(up.astype(np.float64).mean()):.6f} ({occ_up.mean():.4f} occluded)")
    assert abs(mean - 0.51) <= 0.02
    open_floor = np.tile((np.array([0.3, 0.0, 1.1]) @ R.T).astype(np.float32), (COUNT, 1))
    ao, occ = _composed_ao(a, open_floor, n, k, par, True)
    assert not occ.any() and np.array_equal(ao, np.ones(COUNT, np.float32))
