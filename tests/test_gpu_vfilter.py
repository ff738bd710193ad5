"""crtv_filter / Session.filter_variance on the GPU against the numpy restatement of the definition (tests/vfilter_ref.py): every pixel of `out`
and `outVariance`, bit for bit (util.bits), none exempt; `out`, `outVariance` and `scratch` start as NaN poison whose payload differs from word to
word, and the inputs are checked to be untouched. Shapes that break tiles and the 7 x 7, 5 x 5 and 3 x 3 windows (1 x 1, 5 x 3, 33 x 9, 70 x 37,
257 x 19), 1..5 passes, all four flag combinations, both guide layouts, every threshold between the taps from LDS and through L1 and both forms of
the estimate, outVariance NULL and given, a minHistory of 0, above every N and in between, guides with depth and normal edges, sky and a tile
wholly sky, non-finite colours, variances and moments, a negative variance, infinite variances, a luminance stop of zero, a side stream, and a Session on `tiny`."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clraytracer_amd import _lib, driver, scenes

if not os.path.exists(getattr(_lib, "VFILTER_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import vfilter_ref as ref
from util import bits

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (5, 3), (33, 9), (70, 37), (257, 19)]                 # (width, height)
BOTH = ref.DEMODULATE | ref.MATCH_INSTANCE
PARAMS = dict(depth_tol=0.05, normal_cos=0.9, luma_sigma=4.0, luma_floor=1e-4)
ABOVE_EVERY_N = 100.0                                                   # moments_content()'s N reach 32
WRITE_RAYS = 2


@functools.lru_cache(maxsize=None)
def inputs(w, h):
    """the hand-made guides, noisy colour and moments of one shape: made once, never modified. ref.guides() has a depth edge, a normal edge, two
    instances and scattered pixels that are no hit; here the second tile of the first tile row becomes sky as a whole (where the frame has one)."""
    planes, color = ref.guides(h, w, seed=w), ref.noisy_color(h, w, seed=w)
    if w >= 64 and h >= 8:
        planes["geometry"][0:8, 32:64] = (0.0, 0.0, 0.0, 99999.0)
        planes["ids"]["instance"][0:8, 32:64] = -1
        planes["albedo"][0:8, 32:64] = 0
    if w * h > 8:
        color[h // 2, w // 3, 2] = np.inf
    moments = ref.moments_content(color, planes["geometry"], seed=w)
    for a in (*planes.values(), color, moments):
        a.setflags(write=False)
    return planes, color, moments


@functools.lru_cache(maxsize=None)
def reference(w, h, iterations, flags, min_history, **kw):
    planes, color, moments = inputs(w, h)
    out, variance = ref.filter(color, moments, planes["geometry"], planes["ids"]["instance"].astype(np.int32), planes["albedo"], iterations=iterations,
                               flags=flags, min_history=min_history, **dict(PARAMS, **kw))
    out.setflags(write=False); variance.setflags(write=False)
    return out, variance


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")


def poison(shape, salt):
    """a float32 tensor of NaNs whose payload differs from word to word: what out, outVariance and scratch hold before a call"""
    import torch
    return (torch.arange(int(np.prod(shape)), dtype=torch.int32, device="cuda:0") + (0x7FC00000 + salt)).view(torch.float32).reshape(shape)


class Buffers:
    """One shape's inputs on the device, under either guide layout; call() runs crtv_filter on torch's current stream into poisoned buffers."""

    def __init__(self, w, h, moments=None):
        self.w, self.h = w, h
        self.planes, self.color, self.moments = inputs(w, h)
        if moments is not None:
            self.moments = moments
        self.t_color, self.t_moments = dev(self.color), dev(self.moments)
        self.t_planes = {k: dev(v.view(np.int32) if v.dtype.fields is None else v.view(np.int32).reshape(h, w, 4)) for k, v in self.planes.items()}
        self.records = ref.surface_records(self.planes)
        self.t_records = dev(self.records)
        self.scratch = poison((h, w, 4), 0x1000)

    def call(self, layout, iterations, flags, min_history, variance=True, **kw):
        import torch
        f = _lib.CrtvFrame(self.w, self.h, self.t_color.data_ptr(), self.t_moments.data_ptr(), layout, None, None, None)
        if layout == _lib.CRTV_GUIDES_SURFACE:
            f.geometry = self.t_records.data_ptr()
        else:
            f.geometry = self.t_planes["geometry"].data_ptr()
            f.ids = self.t_planes["ids"].data_ptr() if flags & ref.MATCH_INSTANCE else None      # a plane no flag needs may be NULL
            f.albedo = self.t_planes["albedo"].data_ptr() if flags & ref.DEMODULATE else None
        q = dict(PARAMS, **kw)
        p = _lib.CrtvParams(iterations, flags, q["depth_tol"], q["normal_cos"], q["luma_sigma"], q["luma_floor"], min_history)
        out = poison((self.h, self.w, 4), 0x77)
        var = poison((self.h, self.w), 0x3000) if variance else None
        lib = _lib.vfilter()
        assert lib.crtv_scratch_bytes(self.w, self.h, iterations) == self.w * self.h * 16
        rc = lib.crtv_filter(C.byref(f), C.byref(p), out.data_ptr(), var.data_ptr() if variance else None, self.scratch.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.crtv_error_string(rc)
        return out, var

    def inputs_untouched(self):
        assert np.array_equal(bits(self.t_color.cpu().numpy()), bits(self.color))
        assert np.array_equal(bits(self.t_moments.cpu().numpy()), bits(self.moments))
        for k, v in self.planes.items():
            assert np.array_equal(self.t_planes[k].cpu().numpy().reshape(-1), v.view(np.int32).reshape(-1)), k
        assert np.array_equal(self.t_records.cpu().numpy(), self.records)


def same(got, want):
    """got: (out, variance or None) tensors; want: the reference's pair"""
    for name, g, w in (("out", got[0], want[0]), ("outVariance", got[1], want[1])):
        if g is None:
            continue
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        differ = bits(g) != bits(w)
        differ = differ.any(axis=-1) if differ.ndim == 3 else differ
        assert not differ.any(), f"{name}: {int(differ.sum())} of {differ.size} pixels differ, the first at (y, x) = {tuple(np.argwhere(differ)[0])}"


@pytest.mark.parametrize("iterations", range(1, 6))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_shape_and_pass_count_matches_the_reference(shape, iterations):
    w, h = shape
    b = Buffers(w, h)
    want = reference(w, h, iterations, BOTH, 4.0)
    same(b.call(_lib.CRTV_GUIDES_PLANES, iterations, BOTH, 4.0), want)
    same(b.call(_lib.CRTV_GUIDES_SURFACE, iterations, BOTH, 4.0), want)
    b.inputs_untouched()


@pytest.mark.parametrize("min_history", [0.0, 4.0, ABOVE_EVERY_N], ids=["temporal", "mixed", "spatial"])
@pytest.mark.parametrize("flags", range(4))
def test_every_flag_combination_and_estimate_with_and_without_the_variance_plane(flags, min_history):
    w, h = 70, 37
    b = Buffers(w, h)
    want = reference(w, h, 5, flags, min_history)
    same(b.call(_lib.CRTV_GUIDES_PLANES, 5, flags, min_history), want)
    same(b.call(_lib.CRTV_GUIDES_SURFACE, 5, flags, min_history, variance=False), want)
    same(b.call(_lib.CRTV_GUIDES_PLANES, 2, flags, min_history, variance=False), reference(w, h, 2, flags, min_history))
    same(b.call(_lib.CRTV_GUIDES_SURFACE, 2, flags, min_history), reference(w, h, 2, flags, min_history))
    b.inputs_untouched()
    if flags:
        assert not np.array_equal(bits(want[0]), bits(reference(w, h, 5, 0, min_history)[0]))          # the flag is seen
    if min_history:
        assert not np.array_equal(bits(want[0]), bits(reference(w, h, 5, flags, 0.0)[0]))              # and so is the estimate


def test_the_inputs_are_not_degenerate():
    """what the cases above filter: N of 0, 1 and 32 and NaN, non-finite colours, variances and moments, a negative variance, pixels that are no
    hit (a miss, a far t, a NaN t), a tile wholly sky beside tiles that are not, and both estimates in use under the mixed minHistory"""
    planes, color, moments = inputs(70, 37)
    N = moments[..., 2]
    hit = planes["geometry"][..., 3] <= 99998.0
    for v in (0.0, 1.0, 32.0):
        assert (N[hit] == v).any(), v
    assert np.isnan(N).any() and np.isnan(color).any() and np.isinf(color).any()
    assert np.isnan(moments[..., 0]).any() and np.isinf(moments[..., 0]).any() and np.isnan(moments[..., 1]).any() and np.isinf(moments[..., 1]).any()
    assert np.isnan(moments[..., 3]).any() and (moments[..., 3] == 0).any()
    assert (moments[..., 3] < 0).any()
    t = planes["geometry"][..., 3]
    assert (t == 99999.0).any() and (t == 99998.5).any() and np.isnan(t).any()
    assert not hit[0:8, 32:64].any() and hit[0:8, 0:32].any() and hit[8:16, 32:64].any()
    assert (hit & (N >= 4.0)).sum() > 100 and (hit & ~(N >= 4.0)).sum() > 100
    out, variance = reference(70, 37, 5, BOTH, 4.0)
    assert np.isfinite(out[hit]).mean() > 0.95 and (variance[hit] > 0).mean() > 0.9 and np.isfinite(variance[hit]).mean() > 0.95


@pytest.mark.parametrize("estimate_taps", ["l1", "lds"])
@pytest.mark.parametrize("stage_max_step", ["0", "1", "2", "4"])
@pytest.mark.parametrize("shape", [(70, 37), (257, 19), (5, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_tap_forms_at_every_step_that_has_two(monkeypatch, shape, stage_max_step, estimate_taps):
    """CRTV_STAGE_MAX_STEP moves the threshold between a pass's taps from LDS and through L1 / L2, CRTV_ESTIMATE_TAPS chooses the estimate's: the
    same bits wherever they stand."""
    monkeypatch.setenv("CRTV_STAGE_MAX_STEP", stage_max_step)
    monkeypatch.setenv("CRTV_ESTIMATE_TAPS", estimate_taps)
    w, h = shape
    b = Buffers(w, h)
    for flags, min_history in ((BOTH, 4.0), (ref.DEMODULATE, ABOVE_EVERY_N), (0, 0.0)):
        want = reference(w, h, 5, flags, min_history)
        same(b.call(_lib.CRTV_GUIDES_PLANES, 5, flags, min_history), want)
        same(b.call(_lib.CRTV_GUIDES_SURFACE, 5, flags, min_history), want)
    b.inputs_untouched()


@pytest.mark.parametrize("stage_max_step", ["0", "4"])
def test_a_luminance_stop_of_zero_keeps_every_tap_out(monkeypatch, stage_max_step):
    """lumaFloor = 0 over a variance of 0: sd = 0, xl is x / 0 = inf or 0 / 0 = NaN, and no tap but the centre counts"""
    monkeypatch.setenv("CRTV_STAGE_MAX_STEP", stage_max_step)
    w, h = 70, 37
    planes, color, moments = inputs(w, h)
    zero = moments.copy()
    zero[..., 3] = 0.0
    zero[..., 2] = 32.0
    b = Buffers(w, h, moments=zero)
    hit = planes["geometry"][..., 3] <= 99998.0
    for layout in (_lib.CRTV_GUIDES_PLANES, _lib.CRTV_GUIDES_SURFACE):
        want = ref.filter(color, zero, planes["geometry"], planes["ids"]["instance"].astype(np.int32), planes["albedo"], iterations=3, flags=0,
                          min_history=4.0, **dict(PARAMS, luma_floor=0.0))
        same(b.call(layout, 3, 0, 4.0, luma_floor=0.0), want)
        finite = hit & np.isfinite(color[..., :3]).all(axis=-1)
        assert np.abs(want[0][finite] - color[finite]).max() <= 1e-6 * np.abs(color[finite]).max() and (want[1] == 0).all()
    b.inputs_untouched()


def test_infinite_variances_spread_as_the_definition_says():
    """one +inf variance (temporal) and one +inf m2 (spatial): sd is infinite around them, xl = 0 and every tap that passes the geometry counts
    with w = k; the variance of what they reach is +inf"""
    w, h = 70, 37
    planes, color, _ = inputs(w, h)
    moments = ref.moments_content(color, planes["geometry"], seed=w, infinite=True)
    b = Buffers(w, h, moments=moments)
    for iterations, flags in ((1, BOTH), (3, ref.DEMODULATE), (5, 0)):
        want = ref.filter(color, moments, planes["geometry"], planes["ids"]["instance"].astype(np.int32), planes["albedo"], iterations=iterations,
                          flags=flags, min_history=4.0, **PARAMS)
        assert np.isinf(want[1]).sum() >= 2 * iterations and not np.isnan(want[1][np.isfinite(moments).all(axis=-1)]).any()
        same(b.call(_lib.CRTV_GUIDES_PLANES, iterations, flags, 4.0), want)
        same(b.call(_lib.CRTV_GUIDES_SURFACE, iterations, flags, 4.0), want)
    b.inputs_untouched()


def test_on_another_stream_and_back_to_back_with_one_scratch():
    import torch
    w, h = 70, 37
    b = Buffers(w, h)
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())                                    # the uploads were made on the current stream
    with torch.cuda.stream(side):
        first = b.call(_lib.CRTV_GUIDES_PLANES, 4, BOTH, 4.0)
        second = b.call(_lib.CRTV_GUIDES_SURFACE, 3, ref.DEMODULATE, ABOVE_EVERY_N)    # the same scratch, an odd pass count behind an even one
        third = b.call(_lib.CRTV_GUIDES_PLANES, 1, 0, 0.0, variance=False)
    side.synchronize()
    same(first, reference(w, h, 4, BOTH, 4.0))
    same(second, reference(w, h, 3, ref.DEMODULATE, ABOVE_EVERY_N))
    same(third, reference(w, h, 1, 0, 0.0))
    b.inputs_untouched()


# ---- through Session, on a rendered frame -----------------------------------------------------------------------------------------------------
SW, SH = 112, 72


def test_session_filters_what_accumulate_returns():
    import torch
    sc = scenes.get("tiny")
    with driver.Session(SW, SH, device=0) as s:
        s.load_scene(sc)
        s.render_raw(WRITE_RAYS)
        dirs = s.read_rays().reshape(-1, 3)
        _, _, pos = s.camera()
        hits = s.shade_rays(dev(np.asarray(pos, np.float32)), dev(dirs), radiance=False, surface=True)
        good = torch.zeros((SH, SW, 4), device="cuda:0")
        with pytest.raises(ValueError, match="render_raw"):
            s.filter_variance(good, good.clone())
        s.render(gbuffer=True)
        frame = s.read_output()
        g = s.read_gbuffer_raw()
        geometry = np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1).astype(np.float32)
        hit = geometry[..., 3] <= 99998.0
        assert 0.0 < hit.mean() < 1.0                                               # the frame shows the scene and sky around it
        hist = driver.TemporalHistory(s)
        for seed in (3, 4):                                                         # two noisy frames of an unmoved camera: N = 2
            noisy = (frame + np.random.RandomState(seed).normal(0, 0.3, frame.shape) * np.array([1, 1, 1, 0])).astype(np.float32)
            color, moments = s.accumulate(hist, dev(noisy))
        h_color, h_moments = color.cpu().numpy(), moments.cpu().numpy()
        assert (h_moments[..., 2][hit] == 2.0).all() and (h_moments[..., 3][hit] > 0).mean() > 0.9
        reference_of = lambda **kw: ref.filter(h_color, h_moments, geometry, g["ids"]["instance"].astype(np.int32), g["albedo"], **kw)
        # the defaults: N = 2 is below min_history = 4, so the estimate is the spatial one
        got = s.filter_variance(color, moments)
        want = reference_of(iterations=4, flags=ref.DEMODULATE, **ref.DEFAULTS)
        same((got, None), want)
        assert got.shape == (SH, SW, 4) and got.dtype == torch.float32 and got.device == color.device
        assert np.abs(want[0] - frame)[hit][:, :3].mean() < np.abs(h_color - frame)[hit][:, :3].mean()      # and it denoises: closer to the clean frame
        # every option, and the variance
        opts = dict(iterations=5, depth_tol=0.1, normal_cos=0.5, luma_sigma=2.0, luma_floor=0.01, min_history=2)
        got = s.filter_variance(color, moments, demodulate=False, match_instance=True, return_variance=True, **opts)
        want = reference_of(flags=ref.MATCH_INSTANCE, **opts)
        same(got, want)
        assert got[1].shape == (SH, SW) and got[1].dtype == torch.float32
        # surface=: the records of the frame's own rays guide as the planes do; out= is the tensor returned
        mine = torch.full((SH, SW, 4), float("nan"), device="cuda:0")
        got = s.filter_variance(color, moments, surface=hits, out=mine, return_variance=True, match_instance=True)
        assert got[0] is mine
        same(got, reference_of(iterations=4, flags=BOTH, **ref.DEFAULTS))
        assert np.array_equal(bits(color.cpu().numpy()), bits(h_color)) and np.array_equal(bits(moments.cpu().numpy()), bits(h_moments))


def test_session_refusals():
    import torch
    sc = scenes.get("tiny")
    with driver.Session(SW, SH, device=0) as s:
        s.load_scene(sc)
        good, m = torch.zeros((SH, SW, 4), device="cuda:0"), torch.zeros((SH, SW, 4), device="cuda:0")
        with pytest.raises(ValueError, match="none has been rendered"):
            s.filter_variance(good, m)
        s.render()
        with pytest.raises(ValueError, match="without gbuffer"):
            s.filter_variance(good, m)
        s.render(gbuffer=True)
        for bad in (good.cpu(), good.double(), good[:, :, :3], good[:-1], good.permute(1, 0, 2), np.zeros((SH, SW, 4), np.float32)):
            with pytest.raises(ValueError):
                s.filter_variance(bad, m)
            with pytest.raises(ValueError):
                s.filter_variance(good, bad)
            with pytest.raises(ValueError):
                s.filter_variance(good, m, out=bad)
        with pytest.raises(ValueError):
            s.filter_variance(None, m)                                     # there is no frame form: the moments belong to a colour tensor
        hits = s.shade_rays(torch.zeros(3, device="cuda:0"), torch.ones((5, 3), device="cuda:0"), radiance=False, surface=True)
        with pytest.raises(ValueError, match="records"):
            s.filter_variance(good, m, surface=hits)                       # 5 records for 112 x 72 pixels
        for kw in (dict(iterations=6), dict(iterations=0), dict(out=good), dict(out=m), dict(luma_sigma=-1.0), dict(min_history=float("nan"))):
            with pytest.raises(driver.CrtError, match="bad argument"):
                s.filter_variance(good, m, **kw)
        s.filter_variance(good, m)
        s.set_row_bands(16, 1, 2)
        with pytest.raises(ValueError, match="row bands"):
            s.filter_variance(good, m)
        s.set_row_bands(16, 0, 1)
        s.resize(96, 64)
        with pytest.raises(ValueError):
            s.filter_variance(good, m)
    with driver.Session(SW, SH, devices=[0, 0]) as s:
        s.load_scene(sc)
        s.render()
        with pytest.raises(ValueError, match="several devices"):
            s.filter_variance(good, m)
