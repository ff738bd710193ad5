"""CRT_RENDER_SSAA2 / SSAA4 and Renderer::SetSupersampling: k x k ordered-grid supersampling resolved in the Trace kernel
(crt_trace_ssaa_kernel). By definition the SSAA frame at W x H is the plain frame at kW x kH -- the same invView / invProj -- with
each k x k block summed in a fixed order (horizontal pairs, then vertical pairs, log2(k) times) and scaled by 1/k^2. `resolve`
restates that order in numpy, so every pixel is checked bit for bit against the oracle's kW x kH frame or our own."""
import ctypes as C

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import oracle_lib
from util import bits

pytestmark = pytest.mark.gpu

POST, WRITE_RAYS, ASYNC, COUNT, STAMPS, SHADOWS, UNORM8, READBACK, REFRACT, FXAA, MIX3 = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024
SSAA2, SSAA4 = 2048, 4096
SS = {2: SSAA2, 4: SSAA4}


def resolve(hi, k):
    h, w = hi.shape[0] // k, hi.shape[1] // k
    s = np.ascontiguousarray(hi, np.float32).reshape(h, k, w, k, hi.shape[2])
    for _ in range(k.bit_length() - 1):
        s = s[:, :, :, 0::2] + s[:, :, :, 1::2]
        s = s[:, 0::2] + s[:, 1::2]
    return s.reshape(h, w, hi.shape[2]) * np.float32(1.0 / (k * k))


def assert_post_close(got, want):
    """PostProcess (powf) against the oracle: the tolerance of the existing stage tests."""
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.nanmax(d) <= 2e-5
    assert (d > 2e-5).sum() <= 0.002 * d.size


def raw_rc(s, flags, view=None):
    a, iv, ip = s.trace_args()
    fp = C.POINTER(C.c_float)
    return s.hip.crt_render(C.byref(a), iv.ctypes.data_as(fp), ip.ctypes.data_as(fp), int(flags))


def oracle_hi(s, sc, k, nthreads, **opts):
    iv, ip, pos = s.camera()
    orc = oracle_lib.Oracle(s.arenas(), nthreads=nthreads)
    hi, st = orc.trace(orc.raygen(k * s.width, k * s.height, iv, ip), pos, sc.sun_angle, **opts)
    return orc, hi, st


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name,w,h", [("tiny", 200, 120), ("tiny", 16, 16), ("cornell-1k", 333, 187)])
def test_ssaa_frame_is_the_resolved_oracle_frame(name, w, h, k, nthreads):
    sc = scenes.get(name)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        orc, hi, st = oracle_hi(s, sc, k, nthreads)
        want = resolve(hi, k)
        s.render_raw(SS[k])
        assert s.last_kernel() == "crt_trace_ssaa_kernel<0,0,0,0>", s.last_kernel()
        got = s.read_output()
        assert got.shape == (h, w, 4)
        assert np.array_equal(bits(got), bits(want))
        assert (got[..., 3] == 1.0).all()
        # counters: every subsample ray, equal to the oracle's kW x kH frame field by field
        s.render_raw(SS[k] | COUNT)
        assert s.last_kernel() == "crt_trace_ssaa_kernel<1,0,0,0>"
        assert np.array_equal(bits(s.read_output()), bits(want))
        assert s.counters() == st
        assert st["primary"] == k * k * w * h
        # the stages behind Trace run on the resolved frame at output coordinates
        s.render_raw(SS[k] | UNORM8)
        assert np.array_equal(bits(s.read_output()), bits(orc.quantize_unorm8(want)))
        s.render_raw(SS[k] | POST)
        assert_post_close(s.read_output(), orc.postprocess(want))
        s.render_raw(SS[k] | POST | UNORM8)
        got = s.read_output()
        want_pu = orc.quantize_unorm8(orc.postprocess(orc.quantize_unorm8(want)))
        d = np.abs(got.astype(np.float64) - want_pu.astype(np.float64))
        assert np.array_equal(np.isnan(got), np.isnan(want_pu)) and np.nanmax(d) <= 1.0 / 255.0 + 1e-6
        assert (d > 2e-5).sum() <= 0.002 * d.size
        s.render_raw(SS[k] | FXAA)
        assert np.array_equal(bits(s.read_output()), bits(orc.fxaa(want)))
        s.render_raw(SS[k] | FXAA | POST)
        assert_post_close(s.read_output(), orc.postprocess(orc.fxaa(want)))
        # the plain frame is unchanged behind it
        s.render_raw(0)
        assert s.last_kernel() == "crt_trace_kernel<0,0,0,0,0>"
        plain, _ = orc.trace(orc.raygen(w, h, *s.camera()[:2]), s.camera()[2], sc.sun_angle)
        assert np.array_equal(bits(s.read_output()), bits(plain))


@pytest.mark.parametrize("opt,flag,kern", [("shadows", SHADOWS, "crt_trace_ssaa_kernel<1,1,0,0>"), ("refraction", REFRACT, "crt_trace_ssaa_kernel<1,0,0,1>")])
def test_ssaa_with_shadows_and_refraction(opt, flag, kern, nthreads):
    sc = scenes.get("cornell-1k")
    w, h, k = 160, 96, 2
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        orc, hi, st = oracle_hi(s, sc, k, nthreads, **{opt: True})
        s.render_raw(SSAA2 | COUNT | flag)
        assert s.last_kernel() == kern
        assert np.array_equal(bits(s.read_output()), bits(resolve(hi, k)))
        assert s.counters() == st


def test_ssaa_with_the_instance_tree():
    """401 instances: the TLAS instantiation, against our own plain kW x kH frame (same per-pixel code) and its counters."""
    tiny = scenes.get("tiny")
    w, h = 96, 64
    with driver.Session(4 * w, 4 * h, device=0) as s:
        s.load_scene(tiny)
        s.h.crth_begin_instances()
        for i in range(len(tiny.instances), 401):
            m = scenes._trs(0.6 + 0.1 * (i % 5), (0.3, 1.0, 0.2), 0.37 * i, (float((i % 21) - 10) * 6.0, float((i // 21) - 9) * 6.0, -float(i % 7) * 2.0))
            pm, keep = _lib.fptr(m)
            s.h.crth_register_instance(i % 2, 0xFFFF, pm)
        s.h.crth_end_instances()
        s.set_camera((0.0, 0.0, 23.0 * 6.0), scenes._normalize((0.0, 0.0, -1.0)))
        view = s.camera()
        hi = {}
        for k in (4, 2):
            s.resize(k * w, k * h)
            s.render_raw(COUNT, view=view)
            assert s.last_kernel() == "crt_trace_kernel<1,0,0,1,0>"
            hi[k] = (s.read_output(), s.counters())
        s.resize(w, h)
        for k in (2, 4):
            s.render_raw(SS[k] | COUNT, view=view)
            assert s.last_kernel() == "crt_trace_ssaa_kernel<1,0,1,0>", s.last_kernel()
            assert np.array_equal(bits(s.read_output()), bits(resolve(hi[k][0], k)))
            assert s.counters() == hi[k][1]
            s.render_raw(SS[k], view=view)
            assert s.last_kernel() == "crt_trace_ssaa_kernel<0,0,1,0>"
            assert np.array_equal(bits(s.read_output()), bits(resolve(hi[k][0], k)))


def test_full_size_ssaa_equals_the_resolved_4k_frame():
    """multi-1M: the same 3840x2160 ray set as a plain frame, as SSAA2 at 1920x1080 and as SSAA4 at 960x540 (explicit matrices of the
    3840x2160 camera; test_gpu_config5 pins the plain 4K frame to the oracle)."""
    sc = scenes.get("multi-1M")
    with driver.Session(3840, 2160, device=0) as s:
        s.load_scene(sc)
        view = s.camera()
        s.render_raw(0, view=view)
        full = s.read_output()
        for k, (w, h) in ((2, (1920, 1080)), (4, (960, 540))):
            s.resize(w, h)
            s.render_raw(SS[k], view=view)
            assert np.array_equal(bits(s.read_output()), bits(resolve(full, k))), k


def test_frames_in_flight_interleave_factors(monkeypatch, nthreads):
    monkeypatch.setenv("CRT_FEEDBACK_ASYNC", "1")         # feedback launch lists on frames in flight too (read by crt_init)
    sc = scenes.get("tiny")
    w, h = 256, 144
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        iv, ip, pos = s.camera()
        orc = oracle_lib.Oracle(s.arenas(), nthreads=nthreads)
        plain, _ = orc.trace(orc.raygen(w, h, iv, ip), pos, sc.sun_angle)
        r2 = resolve(orc.trace(orc.raygen(2 * w, 2 * h, iv, ip), pos, sc.sun_angle)[0], 2)
        r4 = resolve(orc.trace(orc.raygen(4 * w, 4 * h, iv, ip), pos, sc.sun_angle)[0], 4)
        variants = [(0, plain), (SSAA2, r2), (SSAA4, r4), (SSAA2 | UNORM8, orc.pack_unorm8(orc.quantize_unorm8(r2)))]
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        seq = [variants[i % 4] for i in range(13)]
        for start in range(0, len(seq), 3):                  # three frames in flight (the default slots), then their host copies
            batch = seq[start:start + 3]
            for flags, _ in batch:
                s.render_raw(ASYNC | READBACK | flags)
            for back, (flags, want) in enumerate(reversed(batch)):
                assert s.hip.crt_map_host_frame_back(back, C.byref(ptr), C.byref(nbytes)) == 0
                if flags & UNORM8:
                    host = np.frombuffer((C.c_char * nbytes.value).from_address(ptr.value), np.uint8).reshape(h, w, 4)
                    assert np.array_equal(host, want), (start, flags)
                else:
                    host = np.frombuffer((C.c_char * nbytes.value).from_address(ptr.value), np.float32).reshape(h, w, 4)
                    assert np.array_equal(bits(host), bits(want)), (start, flags)
        # synchronous frames after factor switches on slot 0 (its feedback lists restart for each grid)
        for flags, want in ((SSAA4, r4), (SSAA2, r2), (SSAA4, r4), (0, plain)):
            s.render_raw(flags)
            assert np.array_equal(bits(s.read_output()), bits(want)), flags


def test_row_bands_and_multi_device_sessions():
    sc = scenes.get("cornell-1k")
    w, h = 200, 120                                        # 7.5 bands of 16 rows: a partial band at the bottom
    hip = _lib.hip()
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        s.render_raw(SSAA2)
        one = s.read_output()
        s.render_raw(SSAA2 | UNORM8)
        one8 = s.read_output()
        for n in (2, 3):
            owner = np.array([hip.crt_row_owner(y, 16, n) for y in range(h)])
            for r in range(n):
                s.set_row_bands(16, r, n)
                s.render_raw(SSAA4 if r == 0 else SSAA2)   # a factor switch between bands of the same slot
                s.render_raw(SSAA2)
                assert np.array_equal(bits(s.read_output()[owner == r]), bits(one[owner == r])), (n, r)
        s.set_row_bands(16, 0, 1)
    for n in (2, 3):
        with driver.Session(w, h, devices=[0] * n) as s:
            s.load_scene(sc)
            s.render_raw(SSAA2)
            assert np.array_equal(bits(s.read_output()), bits(one)), n
            s.render_raw(SSAA2 | UNORM8)                    # RGBA8 gather
            assert s.last_gather()[1] == 4
            assert np.array_equal(bits(s.read_output()), bits(one8)), n
            for _ in range(4):
                s.render_raw(ASYNC | SSAA2)
            assert np.array_equal(bits(s.read_output()), bits(one)), n


def test_refusals_change_nothing(monkeypatch):
    sc = scenes.get("tiny")
    w, h = 160, 96
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        s.render_raw(SSAA2)
        ref = s.read_output()
        for flags, rc in ((SSAA2 | SSAA4, -2), (SSAA2 | STAMPS, -5), (SSAA4 | WRITE_RAYS, -5), (SSAA2 | MIX3, -5)):
            assert raw_rc(s, flags) == rc, flags
            s.render_raw(SSAA2)
            assert np.array_equal(bits(s.read_output()), bits(ref)), flags
        # virtual frame above 7680 x 4320: 4 x 1928 x 4 x 1080 > 33,177,600
        s.resize(1928, 1080)
        assert raw_rc(s, SSAA4) == -5
        assert raw_rc(s, SSAA2 | ASYNC) == 0            # 3856 x 2160 is within the cap
        s.sync()
        s.resize(w, h)
        s.render_raw(SSAA2)
        assert np.array_equal(bits(s.read_output()), bits(ref))
    # the opt-in kernel forms are not extended (CRT_KERNEL is read by crt_init)
    monkeypatch.setenv("CRT_KERNEL", "wavefront")
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        assert raw_rc(s, SSAA2) == -5
        s.render_raw(0)
    monkeypatch.delenv("CRT_KERNEL")
    with driver.Session(w, h, devices=[0, 0]) as s:
        s.load_scene(sc)
        assert raw_rc(s, SSAA2 | SSAA4) == -2
        assert raw_rc(s, SSAA2 | MIX3) == -5
        s.render_raw(SSAA2)
        assert np.array_equal(bits(s.read_output()), bits(ref))


def test_mirror_set_supersampling():
    sc = scenes.get("tiny")
    with driver.Session(160, 96, device=0) as s:
        s.load_scene(sc)
        s.render_raw(SSAA2)
        raw2 = s.read_output()
        s.render_raw(SSAA4)
        raw4 = s.read_output()
        s.render(ssaa=2)
        assert s.last_kernel() == "crt_trace_ssaa_kernel<0,0,0,0>"
        assert np.array_equal(bits(s.output()), bits(raw2))
        s.render(ssaa=4)
        assert np.array_equal(bits(s.output()), bits(raw4))
        # factor 3 is rejected and the previous factor stays in force
        s.h.crth_clear_error()
        s.h.crth_set_supersampling(3)
        assert s.h.crth_last_error() == -2
        s.h.crth_clear_error()
        assert s.h.crth_render(C.c_float(sc.sun_angle)) != 0
        assert np.array_equal(bits(s.output()), bits(raw4))
        with pytest.raises(ValueError):
            s.render(ssaa=3)
        s.render()
        assert s.last_kernel() == "crt_trace_kernel<0,0,0,0,0>"
