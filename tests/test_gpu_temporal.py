"""crtt_accumulate / Session.accumulate on the GPU against the numpy restatement of the definition (tests/temporal_ref.py): every pixel of all
four planes of `next`, bit for bit (util.bits), none exempt; the outputs start as NaN poison whose payload differs from word to word, and the
inputs are checked to be untouched. Shapes that break tiles and the clamp's halo (1 x 1, 5 x 3, 33 x 9, 70 x 37, 257 x 19), hand-made camera
pairs (identical, a sub-pixel pan, pans over every border, a translation, a previous camera behind the surface, a NaN in toScreen), every flag
combination, both layouts of the current frame, a reset, both forms of each measured kernel choice, a history with N of 0, 1 and maxHistory
and non-finite colours and moments over guides with pixels that are no hit, a ping-ponged sequence, and a Session on rendered frames."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clraytracer_amd import _lib, driver, scenes

if not os.path.exists(getattr(_lib, "TEMPORAL_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import temporal_ref as ref
from util import bits

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (5, 3), (33, 9), (70, 37), (257, 19)]                 # (width, height)
PAIRS = list(ref.camera_pairs(8, 8))
BOTH = ref.MATCH_INSTANCE | ref.CLAMP
PARAMS = dict(alpha=0.2, moments_alpha=0.3, max_history=32.0, depth_tol=0.05, normal_cos=0.9)
PLANES = ("color", "moments", "geometry", "instance")


@functools.lru_cache(maxsize=None)
def inputs(w, h):
    """the hand-made frame (guides, noisy colour with NaNs) and previous history of one shape: made once, never modified"""
    planes, color = ref.guides(h, w, seed=w), ref.noisy_color(h, w, seed=w)
    hist = ref.history_content(h, w, None, seed=w)
    for a in (*planes.values(), color, *(hist[k] for k in PLANES)):
        a.setflags(write=False)
    return planes, color, hist


def frozen(hist):
    for k in PLANES:
        if hist[k] is not None:
            hist[k].setflags(write=False)
    return hist


@functools.lru_cache(maxsize=None)
def reference(w, h, pair, flags, reset=False):
    planes, color, hist = inputs(w, h)
    cur, prev_cam = ref.camera_pairs(w, h)[pair]
    prev = None if reset else dict(hist, camera=prev_cam)
    return frozen(ref.accumulate(color, planes["geometry"], planes["ids"]["instance"].astype(np.int32), cur, prev=prev, flags=flags, **PARAMS))


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")


def camera_struct(cam):
    c = _lib.CrttCamera()
    c.pos[:], c.toRay[:], c.toScreen[:] = [float(v) for v in cam["pos"]], [float(v) for v in cam["toRay"].reshape(-1)], [float(v) for v in cam["toScreen"].reshape(-1)]
    assert np.array_equal(bits(np.array(c.toScreen[:], np.float32)), bits(cam["toScreen"].reshape(-1)))          # NaNs included
    return c


class History:
    """one set of history planes on the device: poison (what `next` holds before a call) or a copy of host planes"""

    def __init__(self, w, h, salt=None, host=None, instance=True):
        import torch
        self.w, self.h = w, h
        if host is None:
            words = lambda n, s: torch.arange(n, dtype=torch.int32, device="cuda:0") + (0x7FC00000 + s)
            self.t = {k: words(h * w * 4, salt + 0x100 * i).view(torch.float32).reshape(h, w, 4) for i, k in enumerate(PLANES[:3])}
            self.t["instance"] = words(h * w, salt + 0x300).reshape(h, w) if instance else None
        else:
            self.t = {k: dev(host[k]) for k in PLANES[:3]}
            self.t["instance"] = dev(host["instance"]) if instance else None

    def struct(self, cam):
        return _lib.CrttHistory(*[self.t[k].data_ptr() if self.t[k] is not None else None for k in PLANES], camera_struct(cam))

    def host(self):
        return {k: (self.t[k].cpu().numpy() if self.t[k] is not None else None) for k in PLANES}


class Buffers:
    """One shape's inputs on the device, the current frame under either layout; call() runs crtt_accumulate on torch's current stream."""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.planes, self.color, self.hist = inputs(w, h)
        self.t_color = dev(self.color)
        self.t_planes = {k: dev(v.view(np.int32) if v.dtype.fields is None else v.view(np.int32).reshape(h, w, 4)) for k, v in self.planes.items()}
        self.records = ref.surface_records(self.planes)
        self.t_records = dev(self.records)
        self.prev = History(w, h, host=self.hist)

    def frame(self, layout, cam, ids=True):
        f = _lib.CrttFrame(self.w, self.h, self.t_color.data_ptr(), layout, None, None, camera_struct(cam))
        if layout == _lib.CRTT_GUIDES_SURFACE:
            f.geometry = self.t_records.data_ptr()
        else:
            f.geometry = self.t_planes["geometry"].data_ptr()
            f.ids = self.t_planes["ids"].data_ptr() if ids else None
        return f

    def call(self, layout, pair, flags, reset=False, instance=True, prev=None, nxt=None, cams=None, params=PARAMS):
        import torch
        cur, prev_cam = cams or ref.camera_pairs(self.w, self.h)[pair]
        f = self.frame(layout, cur, ids=instance)
        nxt = History(self.w, self.h, salt=0x77, instance=instance) if nxt is None else nxt
        p = _lib.CrttParams(flags, params["alpha"], params["moments_alpha"], params["max_history"], params["depth_tol"], params["normal_cos"])
        lib = _lib.temporal()
        rc = lib.crtt_accumulate(C.byref(f), None if reset else C.byref((prev or self.prev).struct(prev_cam)), C.byref(nxt.struct(cur)), C.byref(p),
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.crtt_error_string(rc)
        return nxt

    def inputs_untouched(self):
        assert np.array_equal(bits(self.t_color.cpu().numpy()), bits(self.color))
        for k, v in self.planes.items():
            assert np.array_equal(self.t_planes[k].cpu().numpy().reshape(-1), v.view(np.int32).reshape(-1)), k
        assert np.array_equal(self.t_records.cpu().numpy(), self.records)
        got = self.prev.host()
        for k in PLANES[:3]:
            assert np.array_equal(bits(got[k]), bits(self.hist[k])), k
        assert np.array_equal(got["instance"], self.hist["instance"])


def same(got, want, instance=True):
    got = got.host() if isinstance(got, History) else got
    for k in PLANES[:3]:
        differ = (bits(got[k]) != bits(want[k])).any(axis=-1)
        assert not differ.any(), f"{k}: {int(differ.sum())} of {differ.size} pixels differ, the first at (y, x) = {tuple(np.argwhere(differ)[0])}"
    if instance:
        differ = got["instance"] != want["instance"]
        assert not differ.any(), f"instance: {int(differ.sum())} of {differ.size} pixels differ, the first at (y, x) = {tuple(np.argwhere(differ)[0])}"


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_shape_and_camera_pair_matches_the_reference(shape, pair):
    w, h = shape
    b = Buffers(w, h)
    want = reference(w, h, pair, BOTH)
    same(b.call(_lib.CRTT_GUIDES_PLANES, pair, BOTH), want)
    same(b.call(_lib.CRTT_GUIDES_SURFACE, pair, BOTH), want)
    b.inputs_untouched()


@pytest.mark.parametrize("flags", range(4))
@pytest.mark.parametrize("pair", ["sub-pixel pan", "translation"])
def test_every_flag_combination_and_a_reset(pair, flags):
    w, h = 70, 37
    b = Buffers(w, h)
    want = reference(w, h, pair, flags)
    same(b.call(_lib.CRTT_GUIDES_PLANES, pair, flags), want)
    same(b.call(_lib.CRTT_GUIDES_SURFACE, pair, flags), want)
    if flags:
        base = reference(w, h, pair, 0)
        assert not np.array_equal(bits(want["color"]), bits(base["color"]))                # the flag is seen
    # prev == NULL: the frame itself, whatever the flags
    reset = reference(w, h, pair, flags, reset=True)
    same(b.call(_lib.CRTT_GUIDES_PLANES, pair, flags, reset=True), reset)
    same(b.call(_lib.CRTT_GUIDES_SURFACE, pair, flags, reset=True), reset)
    assert np.array_equal(bits(reset["color"]), bits(b.color))
    if not flags & ref.MATCH_INSTANCE:
        # without instance planes (and, under the planes layout, without ids): the other three planes are the same
        same(b.call(_lib.CRTT_GUIDES_PLANES, pair, flags, instance=False, prev=History(w, h, host=b.hist, instance=False)), want, instance=False)
        same(b.call(_lib.CRTT_GUIDES_SURFACE, pair, flags, instance=False, prev=History(w, h, host=b.hist, instance=False)), want, instance=False)
    b.inputs_untouched()


def test_the_history_content_and_the_guides_are_not_degenerate():
    """what the cases above fetch from: N of 0, 1 and maxHistory, non-finite colours and moments, pixels that are no hit, far and NaN t"""
    planes, color, hist = inputs(70, 37)
    N = hist["moments"][..., 2]
    for v in (0.0, 0.5, 1.0, 32.0):
        assert (N == v).any(), v
    assert np.isnan(N).any() and np.isnan(hist["color"]).any() and np.isinf(hist["color"]).any() and not np.isfinite(hist["moments"][..., :2]).all()
    t = planes["geometry"][..., 3]
    assert (t == 99999.0).any() and (t == 99998.5).any() and np.isnan(t).any() and np.isnan(color).any()
    got = reference(70, 37, "sub-pixel pan", 0)["moments"][..., 2]
    assert (got == 32.0).any() and (got == 2.0).any() and (got == 1.0).any() and (got == 0.0).any()      # capped, grown, lost and no hit


@pytest.mark.parametrize("clamp_taps", ["l1", "lds"])
@pytest.mark.parametrize("taps", ["all", "gated"])
@pytest.mark.parametrize("shape", [(70, 37), (257, 19), (5, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_forms_of_each_kernel_choice(monkeypatch, shape, taps, clamp_taps):
    """CRTT_TAPS and CRTT_CLAMP_TAPS choose among the kernel's forms: the same bits whichever runs."""
    monkeypatch.setenv("CRTT_TAPS", taps)
    monkeypatch.setenv("CRTT_CLAMP_TAPS", clamp_taps)
    w, h = shape
    b = Buffers(w, h)
    for pair in ("sub-pixel pan", "pan left", "pan down", "translation"):
        for flags in (BOTH, ref.CLAMP, 0):
            want = reference(w, h, pair, flags)
            same(b.call(_lib.CRTT_GUIDES_PLANES, pair, flags), want)
            same(b.call(_lib.CRTT_GUIDES_SURFACE, pair, flags), want)
    b.inputs_untouched()


def test_three_frames_ping_ponged_through_two_sets_on_another_stream():
    import torch
    w, h = 70, 37
    b = Buffers(w, h)
    planes = b.planes
    inst = planes["ids"]["instance"].astype(np.int32)
    px = 2.0 * np.tan(0.5) / w
    cams = [ref.pinhole(w, h), ref.pinhole(w, h, yaw=0.4 * px), ref.pinhole(w, h, pos=(0.3, 0.0, 0.0), yaw=1.7 * px, pitch=-0.6 * px)]
    params = dict(PARAMS, max_history=2.0)
    want, hist = [], None
    for cam in cams:                                                         # the same frame three times: what moves is the camera
        hist = ref.accumulate(b.color, planes["geometry"], inst, cam, prev=hist, flags=BOTH, **params)
        want.append(hist)
    sets = [History(w, h, salt=0x1000), History(w, h, salt=0x2000)]
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())                            # the uploads were made on the current stream
    got = []
    with torch.cuda.stream(side):
        for i, cam in enumerate(cams):
            layout = _lib.CRTT_GUIDES_SURFACE if i == 1 else _lib.CRTT_GUIDES_PLANES
            b.call(layout, None, BOTH, reset=i == 0, prev=sets[(i + 1) % 2], nxt=sets[i % 2], cams=(cam, cams[i - 1]), params=params)
            got.append({k: v.clone() for k, v in sets[i % 2].t.items()})
    side.synchronize()
    for g, wnt in zip(got, want):
        same({k: v.cpu().numpy() for k, v in g.items()}, wnt)
    N = want[2]["moments"][..., 2]
    assert (N == 2.0).any() and (N == 1.0).any()
    b.inputs_untouched()


# ---- through Session, on rendered frames ------------------------------------------------------------------------------------------------------
def frame_inputs(s, w, h):
    g = s.read_gbuffer_raw()
    geometry = np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1).astype(np.float32)
    return s.read_output(), geometry, g["ids"]["instance"].astype(np.int32), ref.camera_from_struct(_lib.crtt_camera(*s.camera(), w, h))


def test_session_accumulates_rendered_frames_and_hands_them_to_denoise():
    import torch
    w, h = ref.SESSION_SIZE
    sc = scenes.get("tiny")
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        hist = driver.TemporalHistory(s, match_instance=True)
        with pytest.raises(ValueError, match="none has been rendered"):
            s.accumulate(hist)
        s.render()
        with pytest.raises(ValueError, match="without gbuffer"):
            s.accumulate(hist)
        s.render(gbuffer=True)
        first_in = frame_inputs(s, w, h)
        color, moments = s.accumulate(hist)
        assert color.shape == (h, w, 4) and moments.shape == (h, w, 4) and color.dtype == torch.float32 and hist.frames == 1
        want1 = ref.accumulate(*first_in)
        same({k: getattr(hist, k).cpu().numpy() for k in PLANES}, want1)
        hit = first_in[1][..., 3] <= 99998.0
        assert 0.0 < hit.mean() < 1.0
        # an unmoved camera: every hit pixel has N == 2
        color, moments = s.accumulate(hist, clamp=True, alpha=0.25)
        want_still = ref.accumulate(*first_in, prev=want1, flags=BOTH, alpha=0.25)
        same({k: getattr(hist, k).cpu().numpy() for k in PLANES}, want_still)
        N = moments.cpu().numpy()[..., 2]
        assert (N[hit] == 2.0).all() and (N[~hit] == 0.0).all() and hist.frames == 2
        # the camera moves: history is kept where the surface was seen before and lost elsewhere
        s.set_camera(*ref.session_second_camera(sc))
        s.render(gbuffer=True)
        second_in = frame_inputs(s, w, h)
        noisy = (second_in[0] + np.random.RandomState(3).normal(0, 0.3, second_in[0].shape) * np.array([1, 1, 1, 0])).astype(np.float32)
        t_noisy = dev(noisy)
        kw = {k: v for k, v in ref.SESSION_MOVED_PARAMS.items() if k != "flags"}          # (the history was made with match_instance=True)
        color, moments = s.accumulate(hist, t_noisy, **kw)
        want_moved = ref.accumulate(noisy, *second_in[1:], prev=want_still, **ref.SESSION_MOVED_PARAMS)
        same({k: getattr(hist, k).cpu().numpy() for k in PLANES}, want_moved)
        hit2 = second_in[1][..., 3] <= 99998.0
        N = moments.cpu().numpy()[..., 2]
        assert (N[hit2] == 2.0).mean() >= 0.05 and (N[hit2] == 1.0).mean() >= 0.05
        assert np.array_equal(bits(t_noisy.cpu().numpy()), bits(noisy))
        # camera=: the matrices given are the ones used; reset=: the frame itself
        again = s.accumulate(hist, t_noisy, camera=s.camera(), reset=True)[0]
        assert np.array_equal(bits(again.cpu().numpy()), bits(noisy)) and hist.frames == 1
        # the result is a valid color= for Session.denoise
        out = s.denoise(color, iterations=2)
        assert out.shape == (h, w, 4) and bool(torch.isfinite(out).all())
        # refusals of the wrapper
        with pytest.raises(ValueError, match="TemporalHistory"):
            s.accumulate(None)
        with pytest.raises(ValueError):
            s.accumulate(hist, t_noisy[:-1])
        with pytest.raises(driver.CrtError, match="bad argument"):
            s.accumulate(hist, alpha=0.0)
        with pytest.raises(driver.CrtError, match="bad argument"):
            s.accumulate(hist, color)                                       # the history's own plane as the frame: next would alias it
        s.resize(96, 64)
        with pytest.raises(ValueError, match="TemporalHistory"):
            s.accumulate(hist)
