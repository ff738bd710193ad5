"""crtu_upsample / Session.upsample on the GPU against the numpy restatement of the definition (tests/upsample_ref.py): every pixel of `out` and
`outState`, bit for bit (util.bits), none exempt; `out` and `outState` start as poison whose payload differs from word to word, and the inputs are
checked to be untouched. Full frames that break tiles and leave partial low tiles (1 x 1, 2 x 2, 5 x 3, 33 x 9, 70 x 37, 257 x 19), factors 2 and 4,
offsets (0, 0), (1, 1) and (F-1, 0) (the refusal where one does not fit the frame), 1 and 4 channels, both guide layouts, every flag combination,
both tap forms (CRTU_TAPS), outState NULL and given, the unguided stops, a depthTol of 0, guides with depth and normal edges, two instances,
scattered sky, a NaN t and a tile wholly sky, albedo bytes of 0, NaN and infinite low samples, a side stream, and a Session on `tiny` under both
guide sources."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clraytracer_amd import _lib, driver, scenes

if not os.path.exists(getattr(_lib, "UPSAMPLE_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import upsample_ref as ref
from util import bits

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (2, 2), (5, 3), (33, 9), (70, 37), (257, 19)]         # (width, height) of the full frame
BOTH = ref.MATCH_INSTANCE | ref.MODULATE
WRITE_RAYS = 2


def offsets(factor):
    return [(0, 0), (1, 1), (factor - 1, 0)]


def flag_sets(channels):
    return range(4) if channels == 4 else (0, ref.MATCH_INSTANCE)       # CRTU_MODULATE takes four channels


@functools.lru_cache(maxsize=None)
def guides(w, h):
    """the hand-made guides of one shape: made once, never modified. ref.guides() has a depth edge, a normal edge, two instances, scattered pixels
    that are no hit (a miss, a far t, a NaN t) and albedo bytes of 0; here the second tile of the first tile row becomes sky as a whole (where the
    frame has one)."""
    planes = ref.guides(h, w, seed=w)
    if w >= 64 and h >= 8:
        planes["geometry"][0:8, 32:64] = (0.0, 0.0, 0.0, 99999.0)
        planes["ids"]["instance"][0:8, 32:64] = -1
        planes["albedo"][0:8, 32:64] = 0
    for a in planes.values():
        a.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=None)
def low_image(w, h, factor, offset, channels):
    v = ref.low_image(w, h, factor, offset, channels, seed=w)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def reference(w, h, factor, offset, channels, flags, **kw):
    planes = guides(w, h)
    out, state = ref.upsample(low_image(w, h, factor, offset, channels), planes["geometry"], planes["ids"]["instance"].astype(np.int32), planes["albedo"],
                              factor, offset, flags, **dict(ref.DEFAULTS, **kw))
    out.setflags(write=False); state.setflags(write=False)
    return out, state


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")


def poison(shape, salt, dtype="float32"):
    """NaNs (or, as int32, large words) whose payload differs from word to word: what out and outState hold before a call"""
    import torch
    t = torch.arange(int(np.prod(shape)), dtype=torch.int32, device="cuda:0") + (0x7FC00000 + salt)
    return (t.view(torch.float32) if dtype == "float32" else t).reshape(shape)


class Buffers:
    """One shape's guides on the device, under either layout, and every low image asked for; call() runs crtu_upsample on torch's current
    stream into poisoned buffers."""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.planes = guides(w, h)
        self.t_planes = {k: dev(v.view(np.int32) if v.dtype.fields is None else v.view(np.int32).reshape(h, w, 4)) for k, v in self.planes.items()}
        self.records = ref.surface_records(self.planes)
        self.t_records = dev(self.records)
        self.lows = {}

    def low(self, factor, offset, channels):
        key = (factor, offset, channels)
        if key not in self.lows:
            host = low_image(self.w, self.h, factor, offset, channels)
            self.lows[key] = (host, dev(host))
        return self.lows[key][1]

    def raw(self, layout, factor, offset, channels, flags, low, state=True, depth_tol=0.05, normal_cos=0.9):
        """(rc, out, outState)"""
        import torch
        f = _lib.CrtuFrame(self.w, self.h, layout, None, None, None)
        if layout == _lib.CRTU_GUIDES_SURFACE:
            f.geometry = self.t_records.data_ptr()
        else:
            f.geometry = self.t_planes["geometry"].data_ptr()
            f.ids = self.t_planes["ids"].data_ptr() if flags & ref.MATCH_INSTANCE else None      # a plane no flag needs may be NULL
            f.albedo = self.t_planes["albedo"].data_ptr() if flags & ref.MODULATE else None
        l = _lib.CrtuLow(low.data_ptr(), channels, factor, offset[0], offset[1])
        p = _lib.CrtuParams(flags, depth_tol, normal_cos)
        out = poison((self.h, self.w, 4) if channels == 4 else (self.h, self.w), 0x77)
        st = poison((self.h, self.w), 0x3000, "int32") if state else None
        rc = _lib.upsample().crtu_upsample(C.byref(f), C.byref(l), C.byref(p), out.data_ptr(), st.data_ptr() if state else None,
                                           torch.cuda.current_stream().cuda_stream)
        return rc, out, st

    def call(self, layout, factor, offset, channels, flags, state=True, **kw):
        rc, out, st = self.raw(layout, factor, offset, channels, flags, self.low(factor, offset, channels), state, **kw)
        assert rc == 0, _lib.upsample().crtu_error_string(rc)
        return out, st

    def inputs_untouched(self):
        for k, v in self.planes.items():
            assert np.array_equal(self.t_planes[k].cpu().numpy().reshape(-1), v.view(np.int32).reshape(-1)), k
        assert np.array_equal(self.t_records.cpu().numpy(), self.records)
        for host, device in self.lows.values():
            assert np.array_equal(bits(device.cpu().numpy()), bits(host))


def same(got, want, what=""):
    """got: (out, outState or None) tensors; want: the reference's pair"""
    for name, g, w in (("out", got[0], want[0]), ("outState", got[1], want[1])):
        if g is None:
            continue
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        differ = (g.view(np.uint32) != w) if name == "outState" else (bits(g) != bits(w))
        differ = differ.any(axis=-1) if differ.ndim == 3 else differ
        assert not differ.any(), f"{what} {name}: {int(differ.sum())} of {differ.size} pixels differ, the first at (y, x) = {tuple(np.argwhere(differ)[0])}"


LAYOUTS = (_lib.CRTU_GUIDES_PLANES, _lib.CRTU_GUIDES_SURFACE)


@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_shape_offset_channel_count_layout_flag_and_tap_form_matches_the_reference(monkeypatch, shape, factor):
    w, h = shape
    b = Buffers(w, h)
    ran = 0
    for offset in offsets(factor):
        fits = offset[0] < w and offset[1] < h
        for channels in (1, 4):
            for flags in flag_sets(channels):
                if not fits:
                    for layout in LAYOUTS:                                  # no sample would lie in the frame: refused, nothing written
                        rc, out, st = b.raw(layout, factor, offset, channels, flags, dev(np.zeros(16, np.float32)))
                        assert rc == _lib.CRTU_E_BAD_ARGUMENT
                        assert np.array_equal(out.cpu().numpy().view(np.int32), poison(out.shape, 0x77).cpu().numpy().view(np.int32))
                    continue
                want = reference(w, h, factor, offset, channels, flags)
                for taps in ("l1", "lds"):
                    monkeypatch.setenv("CRTU_TAPS", taps)
                    for layout in LAYOUTS:
                        for state in (True, False):
                            same(b.call(layout, factor, offset, channels, flags, state), want, f"{offset} {channels} ch, flags {flags}, {taps}, layout {layout}:")
                            ran += 1
    assert ran >= 24 * (1 if (w, h) == (1, 1) else 2)                       # (0, 0) fits every frame, (1, 1) all but 1 x 1
    b.inputs_untouched()


def test_the_inputs_are_not_degenerate():
    """what the cases above upsample: pixels that are no hit (a miss, a far t, a NaN t), a tile wholly sky beside tiles that are not, both
    instances, albedo bytes of 0, NaN and infinite samples, and all three states in the result; each flag is seen"""
    planes = guides(70, 37)
    t = planes["geometry"][..., 3]
    hit = t <= 99998.0
    assert (t == 99999.0).any() and (t == 99998.5).any() and np.isnan(t).any()
    assert not hit[0:8, 32:64].any() and hit[0:8, 0:32].any() and hit[8:16, 32:64].any()
    assert {3, 7} <= set(np.unique(planes["ids"]["instance"][hit]))
    assert (((planes["albedo"] >> 8) & 255) == 0)[hit].any()
    for factor in (2, 4):
        for channels in (1, 4):
            low = low_image(70, 37, factor, (0, 0), channels)
            assert np.isnan(low).any() and np.isposinf(low).any() and np.isneginf(low).any()
            out, state = reference(70, 37, factor, (0, 0), channels, 0)
            assert {ref.INTERPOLATED, ref.NEAREST} <= set(np.unique(state)) and (state == ref.INTERPOLATED).mean() > 0.5
            assert not np.array_equal(bits(out), bits(reference(70, 37, factor, (0, 0), channels, ref.MATCH_INSTANCE)[0]))
        assert not np.array_equal(bits(reference(70, 37, factor, (0, 0), 4, 0)[0]), bits(reference(70, 37, factor, (0, 0), 4, ref.MODULATE)[0]))
    assert (reference(70, 37, 4, (1, 1), 4, 0, depth_tol=0.0)[1] == ref.NEAREST).mean() > 0.5


@pytest.mark.parametrize("taps", ["l1", "lds"])
@pytest.mark.parametrize("stops", [ref.UNGUIDED, dict(depth_tol=0.0), dict(depth_tol=float("inf")), dict(normal_cos=2.0)],
                         ids=["unguided", "depthTol 0", "depthTol inf", "normalCos 2"])
def test_the_unguided_stops_a_depth_tolerance_of_zero_and_stops_nothing_passes(monkeypatch, stops, taps):
    monkeypatch.setenv("CRTU_TAPS", taps)
    stops = dict(stops)
    for w, h in ((70, 37), (33, 9)):
        b = Buffers(w, h)
        for factor in (2, 4):
            for offset in offsets(factor):
                for channels, flags in ((1, ref.MATCH_INSTANCE), (4, ref.MODULATE), (4, BOTH), (1, 0)):
                    want = reference(w, h, factor, offset, channels, flags, **stops)
                    same(b.call(_lib.CRTU_GUIDES_PLANES, factor, offset, channels, flags, **stops), want)
                    same(b.call(_lib.CRTU_GUIDES_SURFACE, factor, offset, channels, flags, **stops), want)
        b.inputs_untouched()


@pytest.mark.parametrize("taps", ["l1", "lds"])
def test_an_image_with_nothing_finite_gives_empty_and_zeros(monkeypatch, taps):
    import torch
    monkeypatch.setenv("CRTU_TAPS", taps)
    w, h = 70, 37
    b = Buffers(w, h)
    for factor in (2, 4):
        lw, lh = ref.low_size(w, h, factor, (1, 0))
        for channels, fill in ((1, float("nan")), (4, float("inf")), (4, float("nan"))):
            low = torch.full((lh, lw, 4) if channels == 4 else (lh, lw), fill, device="cuda:0")
            rc, out, st = b.raw(_lib.CRTU_GUIDES_PLANES, factor, (1, 0), channels, BOTH if channels == 4 else ref.MATCH_INSTANCE, low=low)
            assert rc == 0
            assert (out.cpu().numpy().view(np.uint32) == 0).all() and (st.cpu().numpy() == ref.EMPTY).all()


def test_on_another_stream_and_back_to_back():
    import torch
    w, h = 70, 37
    b = Buffers(w, h)
    for key in ((2, (0, 0), 4), (4, (1, 1), 1), (4, (3, 0), 4)):
        b.low(*key)
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())                                    # the uploads were made on the current stream
    with torch.cuda.stream(side):
        first = b.call(_lib.CRTU_GUIDES_PLANES, 2, (0, 0), 4, BOTH)
        second = b.call(_lib.CRTU_GUIDES_SURFACE, 4, (1, 1), 1, ref.MATCH_INSTANCE)
        third = b.call(_lib.CRTU_GUIDES_PLANES, 4, (3, 0), 4, 0, state=False)
    side.synchronize()
    same(first, reference(w, h, 2, (0, 0), 4, BOTH))
    same(second, reference(w, h, 4, (1, 1), 1, ref.MATCH_INSTANCE))
    same(third, reference(w, h, 4, (3, 0), 4, 0))
    b.inputs_untouched()


# ---- through Session, on a rendered frame -----------------------------------------------------------------------------------------------------
SW, SH = 112, 72


def test_session_upsamples_under_both_guide_sources():
    import torch
    sc = scenes.get("tiny")
    with driver.Session(SW, SH, device=0) as s:
        s.load_scene(sc)
        s.render_raw(WRITE_RAYS)
        dirs = s.read_rays().reshape(-1, 3)
        _, _, pos = s.camera()
        hits = s.shade_rays(dev(np.asarray(pos, np.float32)), dev(dirs), radiance=False, surface=True)
        some = np.zeros(ref.low_size(SW, SH, 2)[::-1], np.float32)
        with pytest.raises(ValueError, match="render_raw"):
            s.upsample(some)
        s.render(gbuffer=True)
        g = s.read_gbuffer_raw()
        geometry = np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1).astype(np.float32)
        inst, albedo = g["ids"]["instance"].astype(np.int32), g["albedo"]
        hit = geometry[..., 3] <= 99998.0
        assert 0.0 < hit.mean() < 1.0                                               # the frame shows the scene and sky around it
        reference_of = lambda low, **kw: ref.upsample(low, geometry, inst, albedo, **kw)
        # the defaults, from a numpy array: factor 2, no offset, one channel
        low1 = ref.low_image(SW, SH, 2, (0, 0), 1, seed=1)
        got = s.upsample(low1)
        same((got, None), reference_of(low1, **ref.DEFAULTS))
        assert got.shape == (SH, SW) and got.dtype == torch.float32 and got.device == torch.device("cuda", 0)
        # every option, a device tensor, the state plane
        low4 = ref.low_image(SW, SH, 4, (3, 1), 4, seed=2)
        t_low4 = dev(low4)
        opts = dict(factor=4, offset=(3, 1), depth_tol=0.1, normal_cos=0.5)
        got = s.upsample(t_low4, match_instance=True, modulate=True, return_state=True, **opts)
        same(got, reference_of(low4, flags=BOTH, **opts))
        assert got[0].shape == (SH, SW, 4) and got[1].shape == (SH, SW) and got[1].dtype == torch.int32
        assert np.array_equal(bits(t_low4.cpu().numpy()), bits(low4))
        # surface=: the records of the frame's own rays guide as the planes do; on a side stream
        side = torch.cuda.Stream(device="cuda:0")
        side.wait_stream(torch.cuda.current_stream())
        got = s.upsample(t_low4, surface=hits, match_instance=True, return_state=True, stream=side, **opts)
        side.synchronize()
        same(got, reference_of(low4, flags=ref.MATCH_INSTANCE, **opts))
        # an image that is a small-integer function of the instance comes out exactly where it was interpolated, under the instance match
        full = ((inst % 5) + 1).astype(np.float32)
        for factor, offset in ((2, (1, 1)), (4, (0, 2))):
            ys, xs = ref.sample_pixels(SW, SH, factor, offset)
            out, state = s.upsample(np.ascontiguousarray(full[np.ix_(ys, xs)]), factor=factor, offset=offset, match_instance=True, return_state=True)
            out, state = out.cpu().numpy(), state.cpu().numpy()
            exact = hit & (state == ref.INTERPOLATED)
            assert exact.sum() > 0.5 * hit.sum() and np.array_equal(bits(out)[exact], bits(full)[exact])


def test_session_refusals():
    import torch
    sc = scenes.get("tiny")
    with driver.Session(SW, SH, device=0) as s:
        s.load_scene(sc)
        good = torch.zeros((SH // 2, SW // 2), device="cuda:0")
        with pytest.raises(ValueError, match="none has been rendered"):
            s.upsample(good)
        s.render()
        with pytest.raises(ValueError, match="without gbuffer"):
            s.upsample(good)
        s.render(gbuffer=True)
        for bad in (good.cpu(), good.double(), good[:-1], good[:, :-1], torch.zeros((SH // 2, SW // 2, 3), device="cuda:0"), good.t(),
                    torch.zeros((SH, SW), device="cuda:0"), np.zeros((SH // 2, SW // 2), np.float64), None):
            with pytest.raises(ValueError):
                s.upsample(bad)
        hits = s.shade_rays(torch.zeros(3, device="cuda:0"), torch.ones((5, 3), device="cuda:0"), radiance=False, surface=True)
        with pytest.raises(ValueError, match="records"):
            s.upsample(good, surface=hits)                                  # 5 records for 112 x 72 pixels
        for kw in (dict(factor=3), dict(factor=8), dict(offset=(2, 0)), dict(offset=(0, -1)), dict(depth_tol=-1.0), dict(normal_cos=float("nan")),
                   dict(modulate=True)):
            with pytest.raises(driver.CrtError, match="bad argument"):
                s.upsample(good, **kw)
        with pytest.raises(ValueError, match="stream"):
            s.upsample(good, stream=0)
        assert s.upsample(good).shape == (SH, SW)
        s.set_row_bands(16, 1, 2)
        with pytest.raises(ValueError, match="row bands"):
            s.upsample(good)
        s.set_row_bands(16, 0, 1)
        s.resize(96, 64)
        with pytest.raises(ValueError):
            s.upsample(good)
