"""Ray queries on device buffers (crt_trace_rays), the part that needs no GPU: the ABI, the resource lines of crt_rays_kernel, the numpy
reference of the bounded loop (tests/trace_rays_ref.py) against the C oracle, and the argument checks of Session.trace_rays.
Reference: kernel_main.cl:124-160, 189-217 started with besthit.distance = the bound (include/crt_api.h, crt_trace_rays)."""
import ctypes as C

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import oracle_lib
import trace_rays_ref as rr
from test_abi import declared
from util import kernel_resources, resource_line, seeded_rays


def test_abi_declares_and_exports_the_ray_queries():
    assert "crt_trace_rays" in declared("crt_api.h", "crt_") and "crt_debug_rays_stats" in declared("crt_debug.h", "crt_")
    assert "crth_trace_rays" in declared("crt_host.h", "crth_")
    hip, host = C.CDLL(_lib.HIP_SO), C.CDLL(_lib.HOST_SO, mode=C.RTLD_GLOBAL)
    assert hasattr(hip, "crt_trace_rays") and hasattr(hip, "crt_debug_rays_stats") and hasattr(host, "crth_trace_rays")
    assert C.sizeof(_lib.CrtRayBatch) == 40
    assert (_lib.CRT_RAYS_CLOSEST, _lib.CRT_RAYS_OCCLUDED) == (0, 1)


def test_trace_rays_without_a_session_is_refused():
    # no crt_init has been made in this process (tests/test_abi.py relies on the same)
    batch = _lib.CrtRayBatch(None, None, None, 3, 3, 64)
    assert _lib.hip().crt_trace_rays(C.byref(batch), 1, 0, None, None) == _lib.CRT_E_NOT_INITIALIZED
    assert _lib.hip().crt_debug_rays_stats((C.c_uint64 * 3)()) == _lib.CRT_E_NOT_INITIALIZED


def test_the_four_ray_kernels_fit_the_plain_kernels_budget():
    """no scratch, at most 64 VGPRs, 8 waves per SIMD, the 5 KiB stack in LDS: the traversal of the plain Trace kernels without their shading"""
    rows = {n: r for n, r in kernel_resources().items() if n.startswith("crt_rays_kernel<")}
    for n, r in sorted(rows.items()):
        print(resource_line(n, r))
    assert sorted(rows) == ["crt_rays_kernel<false, false>", "crt_rays_kernel<false, true>", "crt_rays_kernel<true, false>", "crt_rays_kernel<true, true>"]
    for n, r in rows.items():
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["Occupancy"] == 8 and r["LDS Size"] <= 5120, resource_line(n, r)


@pytest.mark.parametrize("name", ["tiny", "cornell-1k"])
def test_bounded_reference_is_the_filtered_oracle_record(name, nthreads):
    """The numpy loop started at the bound == "the oracle's unbounded record if its t < tmax, else the miss record", bit for bit and on every
    ray, for the ten families of bounds the GPU tests use; unbounded it IS the oracle's record."""
    sc = scenes.get(name)
    with driver.Session(64, 48, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
    o, d = seeded_rays(a, sc.camera_pos, 2048, seed=11)
    ref, _ = oracle_lib.Oracle(a, nthreads=nthreads).closest_hits(o, d)
    hits = ref["instance"] >= 0
    print(f"{name}: {int(hits.sum())} of {len(ref)} reference rays hit")
    assert int(hits.sum()) >= 1900 and not any(np.isnan(ref[k]).any() for k in ("t", "u", "v"))      # the preconditions of the filter
    assert rr.same_records(rr.bounded_closest_hits(a, o, d, np.full(len(o), np.inf, np.float32)), ref)
    assert rr.same_records(rr.bounded_closest_hits(a, o, d, None), ref)
    for fam, (tmax, kept) in rr.tmax_families(ref).items():
        want = rr.filtered(ref, tmax)
        assert np.array_equal(want["instance"] >= 0, hits if kept else np.zeros_like(hits)), fam
        assert rr.same_records(rr.bounded_closest_hits(a, o, d, tmax), want), fam


def test_session_refuses_tensors_it_cannot_hand_to_the_device():
    import torch
    with driver.Session(64, 48, host_only=True) as s:
        s.load_scene(scenes.get("tiny"))
        good = torch.zeros(8, 3, dtype=torch.float32)
        with pytest.raises(ValueError):
            s.trace_rays(torch.zeros(8, 3, dtype=torch.float64), good)
        with pytest.raises(ValueError):
            s.trace_rays(good, torch.zeros(3, 8, dtype=torch.float32).T)
        with pytest.raises(ValueError):
            s.trace_rays(good, good, tmax=torch.zeros(8, dtype=torch.float64))
        with pytest.raises(ValueError):
            s.trace_rays(good, good, mode="nearest")
        with pytest.raises(ValueError):                      # CPU tensors: not the session's device (and no call into the library)
            s.trace_rays(good, good)
        assert s.h.crth_last_error() == 0
