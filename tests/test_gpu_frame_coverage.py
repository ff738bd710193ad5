"""Every frame kernel must write every pixel it owns, every frame. Nothing clears a slot's output buffer (nor its byte frame, its G-buffer
planes or its pinned host frame), so a tile that a frame never writes keeps whatever the frame before left there -- and a test that renders
one view twice cannot see it. Here every checked frame is rendered over a *poison* frame in the same slot that differs from the expected
frame at EVERY pixel (asserted: 0 equal pixels), so a dropped tile shows the poison; a COUNT frame of the same state catches a doubled one
(its counters would exceed the oracle's).

  poison A   the same view with PostProcess: the view did not move, the next sort uses the plain costs (the steady-state lists)
  poison B   another view (VIEW_B: up into the sky from in front of the scene) with PostProcess: the view moved, the next sort goes through
             crt_cost_spread_kernel
  stages     the other view with the SAME stage flags, so the byte frame and the host frame are poisoned too. (PostProcess alone is the
             exception: its vignette writes black on row 0 and column 0 whatever the input, so no PostProcess frame can differ from another
             there; its poison is the other view without PostProcess.)

Frame sizes (scene `tiny`): 203x117 = 26x15 tiles (partial right and bottom tiles; the second round of tile rows lacks XCD 7), 72x72 = 9x9
tiles (the second round belongs to XCD 0 alone), 64x20 = 8x3 tiles (five XCDs own nothing)."""
import ctypes as C

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import gbuffer_ref
import launch_lists_ref as ll
import oracle_lib
from test_gpu_ssaa import resolve
from util import bits

pytestmark = pytest.mark.gpu

POST, ASYNC, COUNT, UNORM8, READBACK, FXAA, SSAA2, GBUFFER = 1, 4, 8, 64, 128, 512, 2048, 8192
SIZES = ((203, 117), (72, 72), (64, 20))
VIEW_B = ((0.0, 3.0, 25.0), (0.0, 0.6, -1.0))           # camera position, front
FORM_ENV = ("CRT_KERNEL", "CRT_SPLIT", "CRT_SPLIT_BETA", "CRT_FEEDBACK", "CRT_FEEDBACK_ASYNC", "CRT_FRAMES_IN_FLIGHT", "CRT_COST_SPREAD", "CRT_TLAS")


def equal_pixels(a, b):
    """pixels whose r, g and b all have the same bits in both frames"""
    return int((bits(a)[..., :3] == bits(b)[..., :3]).all(-1).sum())


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Rig:
    """One session on `tiny` with its oracle frames: `want` (the session camera's frame), counters `stats`, and the other view."""

    def __init__(self, s, nthreads):
        self.s, self.sc = s, scenes.get("tiny")
        s.load_scene(self.sc)
        self.arenas = s.arenas()
        self.orc = oracle_lib.Oracle(self.arenas, nthreads=nthreads)
        self.view_a = s.camera()
        s.set_camera(VIEW_B[0], scenes._normalize(VIEW_B[1]))
        self.view_b = s.camera()
        s.set_camera(self.sc.camera_pos, self.sc.camera_front)
        self.want, self.stats = self.trace(self.view_a)

    def trace(self, view, k=1):
        iv, ip, pos = view
        return self.orc.trace(self.orc.raygen(k * self.s.width, k * self.s.height, iv, ip), pos, self.sc.sun_angle)

    def poison(self, flags, moved, want=None):
        """Render the poison frame and trust it only if it differs from the frame expected next at every pixel"""
        self.s.render_raw(flags, view=self.view_b if moved else None)
        got = self.s.read_output()
        assert equal_pixels(got, self.want if want is None else want) == 0, (flags, moved)
        return got

    def check(self, flags=0):
        self.s.render_raw(flags)
        assert np.array_equal(bits(self.s.read_output()), bits(self.want)), flags

    def check_counters(self):
        self.s.render_raw(COUNT)
        assert self.s.counters() == self.stats
        assert np.array_equal(bits(self.s.read_output()), bits(self.want))

    def slots_per_xcd(self, tiles_per_entry=1):
        tiles_x = ((self.s.width + 7) // 8 + tiles_per_entry - 1) // tiles_per_entry
        return (((self.s.height + 7) // 8 + 7) // 8) * tiles_x

    def split_counts(self, S=None):
        """the live lists of slot 0 cover every tile exactly once; -> split tiles per XCD"""
        order, length, slots = self.s.read_launch_lists()
        assert S is None or slots == S, (slots, S)
        return [n for n, _ in ll.check_structure(order, length, slots)]


@pytest.fixture
def clean_env(monkeypatch):
    for name in FORM_ENV:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("regime", ["no-split", "default", "split-everything"])
@pytest.mark.parametrize("size", SIZES, ids=lambda wh: "%dx%d" % wh)
def test_default_form_covers_every_pixel(size, regime, clean_env, nthreads):
    """Synchronous frames of the default kernel on its feedback lists: first frame (identity order: the SSAA poison before it is another
    tile grid), steady state after poison A, the spread sort after poison B. CRT_SPLIT=0: no tile is ever split; CRT_SPLIT_BETA=1e-6: every
    owned tile with a cost is heavier than the threshold, so tiles are split up to the cap."""
    if regime == "no-split":
        clean_env.setenv("CRT_SPLIT", "0")
    elif regime == "split-everything":
        clean_env.setenv("CRT_SPLIT_BETA", "1e-6")
    with driver.Session(*size, device=0) as s:
        r = Rig(s, nthreads)
        S = r.slots_per_xcd()
        seen = []
        r.poison(POST | SSAA2, True)
        for moved in (None, False, False, True):
            if moved is not None:
                r.poison(POST, moved)
            r.check()
            assert s.last_kernel() == "crt_trace_kernel<0,0,0,0,0>"
            seen.append(r.split_counts(S))
            r.check_counters()
            seen.append(r.split_counts(S))
        print(f"tiny {size[0]}x{size[1]} {regime}: split tiles per XCD after each frame: {seen}")
        if regime == "no-split":
            assert max(max(n) for n in seen) == 0
        elif regime == "split-everything":
            assert all(max(n) >= 1 for n in seen), seen
            assert max(max(n) for n in seen) <= min(S, ll.MAX_SPLIT)


@pytest.mark.parametrize("size", SIZES, ids=lambda wh: "%dx%d" % wh)
def test_without_feedback_lists(size, clean_env, nthreads):
    clean_env.setenv("CRT_FEEDBACK", "0")
    with driver.Session(*size, device=0) as s:
        r = Rig(s, nthreads)
        for moved in (False, True, False):
            r.poison(POST, moved)
            r.check()
            with pytest.raises(driver.CrtError):
                s.read_launch_lists()
            assert s.hip.crt_debug_read_launch_lists(None, 0, np.zeros(8, np.uint32).ctypes.data, C.byref(C.c_int()), C.byref(C.c_int())) == _lib.CRT_E_UNSUPPORTED
            r.check_counters()
        frames_in_flight(r)


def host_frame(s, back):
    ptr, n = C.c_void_p(), C.c_size_t()
    assert s.hip.crt_map_host_frame_back(back, C.byref(ptr), C.byref(n)) == 0 and n.value == s.width * s.height * 16
    return np.frombuffer((C.c_char * n.value).from_address(ptr.value), np.float32).reshape(s.height, s.width, 4).copy()


def frames_in_flight(r, rounds=3):
    """Three frames in flight, one per slot: each slot gets its own poison (read back from the slot's pinned host frame), then its own
    checked frame; poison A and poison B alternate, so later rounds run on lists sorted with and without the spread."""
    s = r.s
    for k in range(rounds):
        moved = bool(k & 1)
        for _ in range(3):
            s.render_raw(ASYNC | READBACK | POST, view=r.view_b if moved else None)
        for back in range(3):
            assert equal_pixels(host_frame(s, back), r.want) == 0, (k, back)
        for _ in range(3):
            s.render_raw(ASYNC | READBACK)
        for back in range(3):
            assert np.array_equal(bits(host_frame(s, back)), bits(r.want)), (k, back)
        assert np.array_equal(bits(s.read_output()), bits(r.want)), k
    s.sync()


@pytest.mark.parametrize("size", SIZES, ids=lambda wh: "%dx%d" % wh)
def test_frames_in_flight_on_feedback_lists(size, clean_env, nthreads):
    clean_env.setenv("CRT_FEEDBACK_ASYNC", "1")
    clean_env.setenv("CRT_FRAMES_IN_FLIGHT", "3")
    with driver.Session(*size, device=0) as s:
        r = Rig(s, nthreads)
        frames_in_flight(r, rounds=4)
        r.split_counts(r.slots_per_xcd())                 # slot 0's lists after its frames in flight
        r.poison(POST, True)
        r.check()
        r.check_counters()


KERNEL_OF = {"refill": "crt_trace_refill_kernel<", "block": "crt_trace_block_kernel<", "wavefront": "crt_primary_kernel<", "ldstop": "crt_trace_ldstop_kernel<"}


@pytest.mark.parametrize("form", ["refill", "block", "wavefront", "ldstop"])
@pytest.mark.parametrize("size", SIZES, ids=lambda wh: "%dx%d" % wh)
def test_opt_in_forms_cover_every_pixel(size, form, clean_env, nthreads):
    clean_env.setenv("CRT_KERNEL", form)
    with driver.Session(*size, device=0) as s:
        r = Rig(s, nthreads)
        for moved in (False, True, False, True):
            r.poison(POST, moved)
            assert s.last_kernel().startswith(KERNEL_OF[form])
            r.check()
            assert s.last_kernel().startswith(KERNEL_OF[form]), s.last_kernel()
            if form in ("refill", "block"):                  # their list entries are blocks of tiles and are never split
                assert max(r.split_counts()) == 0
            else:
                with pytest.raises(driver.CrtError):
                    s.read_launch_lists()
            r.check_counters()


def assert_stage(got, want, post, unorm, what):
    """the comparison of tests/test_gpu_flag_matrix.py, tolerances unchanged"""
    if post:                                                 # powf: 2e-5; through the RGBA8 store that can move a value by one code
        tol = (1.0 / 255.0 + 1e-6) if unorm else 2e-5
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.nanmax(d) <= tol, (what, float(np.nanmax(d)))
        assert (d > 2e-5).sum() <= 0.002 * d.size, (what, int((d > 2e-5).sum()))
    else:
        assert np.array_equal(bits(got), bits(want)), what


@pytest.mark.parametrize("form", ["default", "wavefront"], ids=["fused", "own-launches"])
@pytest.mark.parametrize("size", SIZES, ids=lambda wh: "%dx%d" % wh)
def test_per_pixel_stages_cover_every_pixel(size, form, clean_env, nthreads):
    """The stages behind Trace, fused into the Trace (or FXAA) kernel's epilogue by the default form and run as launches of their own
    behind the wavefront form, against the oracle composition."""
    if form != "default":
        clean_env.setenv("CRT_KERNEL", form)
    with driver.Session(*size, device=0) as s:
        r = Rig(s, nthreads)
        orc, W, H = r.orc, s.width, s.height
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        for flags in (POST, UNORM8, FXAA, UNORM8 | READBACK):
            def compose(frame):
                if flags & UNORM8:
                    frame = orc.quantize_unorm8(frame)
                if flags & FXAA:
                    frame = orc.fxaa(frame)
                if flags & POST:
                    frame = orc.postprocess(frame)
                return frame
            want = compose(r.want)
            for k in range(2):                               # twice: the second check runs on lists sorted from stage frames
                poison = r.poison(flags & ~POST, True, want)
                if flags & POST:                             # compared within 2e-5: the poison must be farther than that from every pixel
                    far = np.abs(poison[..., :3].astype(np.float64) - want[..., :3].astype(np.float64)).max(-1)
                    assert far.min() > 2e-5, float(far.min())
                if flags & READBACK:                         # the byte frame in pinned host memory is poisoned too
                    assert s.hip.crt_map_host_frame(C.byref(ptr), C.byref(nbytes)) == 0 and nbytes.value == W * H * 4
                    host = np.frombuffer((C.c_char * nbytes.value).from_address(ptr.value), np.uint8).reshape(H, W, 4)
                    assert int((host[..., :3] == orc.pack_unorm8(want)[..., :3]).all(-1).sum()) == 0
                    assert int((s.read_output_rgba8()[..., :3] == orc.pack_unorm8(want)[..., :3]).all(-1).sum()) == 0
                s.render_raw(flags)
                got = s.read_output()
                assert_stage(got, want, flags & POST, flags & UNORM8, (flags, k))
                if flags & UNORM8:
                    assert np.array_equal(s.read_output_rgba8(), orc.pack_unorm8(want)), (flags, k)
                if flags & READBACK:
                    assert s.hip.crt_map_host_frame(C.byref(ptr), C.byref(nbytes)) == 0 and nbytes.value == W * H * 4
                    host = np.frombuffer((C.c_char * nbytes.value).from_address(ptr.value), np.uint8).reshape(H, W, 4)
                    assert np.array_equal(host, orc.pack_unorm8(want)), (flags, k)


@pytest.mark.parametrize("size", SIZES, ids=lambda wh: "%dx%d" % wh)
def test_ssaa_and_gbuffer_frames_cover_every_pixel(size, clean_env, nthreads):
    with driver.Session(*size, device=0) as s:
        r = Rig(s, nthreads)
        want2 = resolve(r.trace(r.view_a, 2)[0], 2)
        for moved in (True, False):
            r.poison(SSAA2 | POST, moved, want2)
            s.render_raw(SSAA2)
            assert s.last_kernel() == "crt_trace_ssaa_kernel<0,0,0,0>"
            assert np.array_equal(bits(s.read_output()), bits(want2)), moved
            r.split_counts()
        iv, ip, pos = r.view_a
        planes = gbuffer_ref.reference_planes(r.arenas, r.orc, r.orc.raygen(s.width, s.height, iv, ip), pos)
        hit = planes["ids"]["instance"] >= 0
        assert hit.any() and not hit.all()
        for k in range(2):
            r.poison(GBUFFER | POST, True)
            stale = s.read_gbuffer_raw()
            # the other view sees none of this view's surfaces: wherever this view hits something the ids and the geometry are poisoned
            # (a pixel of sky holds the same miss record in every frame and cannot be)
            assert not (words(stale["ids"]).reshape(*hit.shape, 4) == words(planes["ids"]).reshape(*hit.shape, 4)).all(-1)[hit].any()
            assert not (words(stale["geometry"]).reshape(*hit.shape, 4) == words(planes["geometry"]).reshape(*hit.shape, 4)).all(-1)[hit].any()
            s.render_raw(GBUFFER)
            assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,0,0>"
            assert np.array_equal(bits(s.read_output()), bits(r.want)), k
            got = s.read_gbuffer_raw()
            for p in ("geometry", "ids", "albedo"):
                assert np.array_equal(words(got[p]), words(planes[p])), (p, k)
            r.split_counts(r.slots_per_xcd())


@pytest.mark.parametrize("size", SIZES, ids=lambda wh: "%dx%d" % wh)
def test_row_bands_leave_the_other_rows_alone(size, clean_env, nthreads):
    """A rank renders the bands it owns and nothing else: its rows are the full frame's, every other row still holds the poison's bits."""
    with driver.Session(*size, device=0) as s:
        r = Rig(s, nthreads)
        for rank, n in ((1, 2), (0, 3), (2, 3)):
            own = np.array([s.hip.crt_row_owner(y, 16, n) == rank for y in range(s.height)])
            for moved in (True, False):
                s.set_row_bands(16, 0, 1)
                poison = r.poison(POST, moved)
                s.set_row_bands(16, rank, n)
                assert s.owned_rows() == int(own.sum())
                s.render_raw(0)
                got = s.read_output()
                assert np.array_equal(bits(got[own]), bits(r.want[own])), (rank, n, moved)
                assert np.array_equal(bits(got[~own]), bits(poison[~own])), (rank, n, moved)
                if own.any():
                    r.split_counts()
        s.set_row_bands(16, 0, 1)
        r.poison(POST, True)
        r.check()
