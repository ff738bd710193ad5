"""Whatever a session creates on the device -- buffers, pinned buffers, events, streams -- is held by an owner (csrc/crt_own.h) and released
when the session's State goes: crt_debug_live_resources counts them, and after close() the count is 0 again, whichever lazily made
buffers the session touched, whichever kernel form it ran, also after an init that was refused half way and on every device of a
multi-device session. Sessions are one per process and every earlier test closes its own, so each test starts from 0."""
import ctypes as C

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
from util import live_resources, seeded_rays

pytestmark = pytest.mark.gpu

W, H = 64, 48
POST, WRITE_RAYS, ASYNC, COUNTERS, STAMPS, UNORM8, READBACK, FXAA, MIX3, GBUFFER = 1, 2, 4, 8, 16, 64, 128, 512, 1024, 8192


@pytest.fixture(autouse=True)
def plain_environment(monkeypatch):
    monkeypatch.delenv("CRT_KERNEL", raising=False)
    monkeypatch.setenv("CRT_FRAMES_IN_FLIGHT", "3")


def test_shutdown_releases_everything_a_session_made():
    """Every lazily made owner touched once: the count is above 0 while the session is open and exactly 0 after close(), twice."""
    import torch
    assert live_resources() == 0
    sc = scenes.get("cornell-1k")
    hip = _lib.hip()
    s = driver.Session(W, H, device=0)
    base = live_resources()
    assert base > 0
    s.load_scene(sc, device_bvh_build=True)                    # buildTris, buildCtlHost, buildBuf
    s.render_raw(0)                                            # a synchronous frame (lists, ovf)
    for _ in range(4):                                         # frames in flight: slots 1 and 2
        s.render_raw(ASYNC)
    s.sync()
    s.render_raw(FXAA)                                         # aux
    s.render_raw(UNORM8 | READBACK)                            # packBuf, hostBuf, copied
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    assert hip.crt_map_host_frame(C.byref(ptr), C.byref(nbytes)) == 0 and nbytes.value == W * H * 4
    assert s.read_output_rgba8().shape == (H, W, 4)            # queryBuf
    s.render_raw(GBUFFER)                                      # gbuf
    s.render_raw(COUNTERS)
    assert s.counters()["rays"] > 0
    s.render_raw(STAMPS)                                       # stamps
    s.render_raw(MIX3)                                         # mixOrder
    s.render_raw(WRITE_RAYS)
    assert s.read_rays().shape == (H, W, 3)
    o, d = seeded_rays(s.arenas(), sc.camera_pos, 100, 1)
    assert len(s.query_hits(o, d)) == 100                      # queryBuf
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    hits = s.trace_rays(to, td, mode="closest")                # the query context: stream, tables, ctl, raysDone
    occ = s.trace_rays(to, td, mode="occluded")
    torch.cuda.synchronize(dev)
    assert len(hits) == 100 and occ.shape == (100,)
    ghz = C.c_double(0)
    assert hip.crt_debug_measure_clock(200, C.byref(ghz)) == 0 and ghz.value > 0
    s.resize(80, 64)
    s.render_raw(0)
    assert s.read_output().shape == (64, 80, 4)
    assert live_resources() > base                             # the lazily made ones were counted
    s.close()
    assert live_resources() == 0
    with driver.Session(W, H, device=0) as s2:
        s2.load_scene(scenes.get("tiny"))
        s2.render_raw(0)
        assert live_resources() >= base                        # what a fresh session starts with, plus this frame's lists
    assert live_resources() == 0


@pytest.mark.parametrize("form", ["wavefront", "refill", "block", "ldstop"])
def test_every_kernel_form_releases_its_queues(monkeypatch, form):
    """blockQueue, wfCount and the LdsTop sizing of the overflow area belong to the opt-in forms."""
    assert live_resources() == 0
    monkeypatch.setenv("CRT_KERNEL", form)
    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get("tiny"))
        s.render_raw(0)
        s.render_raw(COUNTERS)
        assert s.counters()["rays"] > 0
        assert live_resources() > 0
    assert live_resources() == 0


def test_refused_init_frees_the_half_built_state(monkeypatch):
    """CRT_KERNEL is read after the frame slots and the pools exist: a refused name leaves a half-built State, which is freed whole."""
    assert live_resources() == 0
    monkeypatch.setenv("CRT_KERNEL", "nonsense")
    with pytest.raises(driver.CrtError):
        driver.Session(W, H, device=0)
    assert live_resources() == 0
    monkeypatch.delenv("CRT_KERNEL")
    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get("tiny"))
        s.render_raw(0)
        assert np.isfinite(s.read_output()).all() and live_resources() > 0
    assert live_resources() == 0


def test_several_devices_release_everything():
    """Two device states on one GPU (the rehearsal of the multi-device tests): every device's byte frame (RGBA8 gather) and the primary's
    FXAA buffer, the secondary allocating from its worker thread."""
    assert live_resources() == 0
    with driver.Session(W, H, devices=[0, 0]) as s:
        s.load_scene(scenes.get("tiny"))
        s.render_raw(UNORM8)
        assert s.last_gather()[1] == 4
        s.render_raw(FXAA)
        assert s.read_output().shape == (H, W, 4)
        assert live_resources() > 0
    assert live_resources() == 0
