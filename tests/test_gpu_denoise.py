"""crtd_denoise / Session.denoise on the GPU against the numpy restatement of the definition (tests/denoise_ref.py): every pixel of every case,
bit for bit (util.bits), none exempt. Shapes that break tiles and halos (1 x 1, 5 x 3, 33 x 9, 70 x 37, 257 x 19: at steps 16 and 32 the taps
leave a 37-row frame on both sides), 1..6 passes, every flag combination, both guide layouts, both tap forms of the kernel at every step that
has two, guides with pixels that are no hit, depth and normal edges, two instances, albedo bytes 0 and 255, NaN colours and NaN distances."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clraytracer_amd import _lib, driver, scenes

if not os.path.exists(_lib.DENOISE_SO):
    import __graft_entry__
    __graft_entry__.build()

import ctypes as C

import denoise_ref as ref
from util import bits

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (5, 3), (33, 9), (70, 37), (257, 19)]                 # (width, height)
ALL = ref.DEMODULATE | ref.MATCH_INSTANCE | ref.LUMA_STOP
TOL = dict(depth_tol=0.05, normal_cos=0.9, luma_tol=0.35)
WRITE_RAYS = 2


@functools.lru_cache(maxsize=None)
def inputs(w, h):
    """the hand-made guides and the noisy colour of one shape: made once, never modified"""
    planes, color = ref.guides(h, w, seed=w), ref.noisy_color(h, w, seed=w)
    for a in (*planes.values(), color):
        a.setflags(write=False)
    return planes, color


@functools.lru_cache(maxsize=None)
def reference(w, h, iterations, flags):
    planes, color = inputs(w, h)
    out = ref.denoise(color, planes["geometry"], planes["ids"]["instance"], planes["albedo"], iterations=iterations, flags=flags, **TOL)
    out.setflags(write=False)
    return out


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")


def poison(h, w, salt):
    """an (h, w, 4) float32 tensor of NaNs whose payload differs from word to word: what out and scratch hold before a call"""
    import torch
    return (torch.arange(h * w * 4, dtype=torch.int32, device="cuda:0") + (0x7FC00000 + salt)).view(torch.float32).reshape(h, w, 4)


class Buffers:
    """One shape's inputs on the device, under either guide layout; call() runs crtd_denoise on torch's current stream into poisoned buffers."""

    def __init__(self, w, h, planes=None, color=None):
        self.w, self.h = w, h
        self.planes, self.color = (planes, color) if planes is not None else inputs(w, h)
        self.t_color = dev(self.color)
        self.t_planes = {k: dev(v.view(np.int32) if v.dtype.fields is None else v.view(np.int32).reshape(h, w, 4)) for k, v in self.planes.items()}
        self.records = ref.surface_records(self.planes)
        self.t_records = dev(self.records)
        self.scratch = poison(h, w, 0x1000)

    def call(self, layout, iterations, flags, out=None, scratch=True):
        import torch
        f = _lib.CrtdFrame(self.w, self.h, self.t_color.data_ptr(), layout, None, None, None)
        if layout == _lib.CRTD_GUIDES_SURFACE:
            f.geometry = self.t_records.data_ptr()
        else:
            f.geometry = self.t_planes["geometry"].data_ptr()
            f.ids = self.t_planes["ids"].data_ptr() if flags & ref.MATCH_INSTANCE else None      # a plane no flag needs may be NULL
            f.albedo = self.t_planes["albedo"].data_ptr() if flags & ref.DEMODULATE else None
        p = _lib.CrtdParams(iterations, flags, TOL["depth_tol"], TOL["normal_cos"], TOL["luma_tol"])
        out = poison(self.h, self.w, 0x77) if out is None else out
        lib = _lib.denoise()
        assert lib.crtd_scratch_bytes(self.w, self.h, iterations) == (0 if iterations == 1 else self.w * self.h * 16)
        rc = lib.crtd_denoise(C.byref(f), C.byref(p), out.data_ptr(), self.scratch.data_ptr() if scratch and iterations > 1 else None,
                              torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.crtd_error_string(rc)
        return out

    def inputs_untouched(self):
        assert np.array_equal(bits(self.t_color.cpu().numpy()), bits(self.color))
        for k, v in self.planes.items():
            assert np.array_equal(self.t_planes[k].cpu().numpy().reshape(-1), v.view(np.int32).reshape(-1)), k
        assert np.array_equal(self.t_records.cpu().numpy(), self.records)


def same(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    differ = bits(got) != bits(want)
    assert not differ.any(), f"{int(differ.any(axis=-1).sum())} of {differ.shape[0] * differ.shape[1]} pixels differ, the first at (y, x) = {tuple(np.argwhere(differ.any(axis=-1))[0])}"


@pytest.mark.parametrize("iterations", range(1, 7))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_shape_and_pass_count_matches_the_reference(shape, iterations):
    w, h = shape
    b = Buffers(w, h)
    want = reference(w, h, iterations, ALL)
    planes_out = b.call(_lib.CRTD_GUIDES_PLANES, iterations, ALL)
    surface_out = b.call(_lib.CRTD_GUIDES_SURFACE, iterations, ALL)
    same(planes_out, want)
    same(surface_out, want)
    b.inputs_untouched()


@pytest.mark.parametrize("flags", range(8))
def test_every_flag_combination(flags):
    w, h = 70, 37
    b = Buffers(w, h)
    want = reference(w, h, 5, flags)
    same(b.call(_lib.CRTD_GUIDES_PLANES, 5, flags), want)
    same(b.call(_lib.CRTD_GUIDES_SURFACE, 5, flags), want)
    b.inputs_untouched()
    if flags:
        assert not np.array_equal(bits(want), bits(reference(w, h, 5, 0)))          # the flag is seen


@pytest.mark.parametrize("stage_max_step", ["0", "1", "2", "4"])
@pytest.mark.parametrize("shape", [(70, 37), (257, 19), (5, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_tap_forms_at_every_step_that_has_two(monkeypatch, shape, stage_max_step):
    """CRTD_STAGE_MAX_STEP moves the threshold between the taps from LDS and the taps through L1 / L2: the same bits wherever it stands."""
    monkeypatch.setenv("CRTD_STAGE_MAX_STEP", stage_max_step)
    w, h = shape
    b = Buffers(w, h)
    for flags in (ALL, ref.DEMODULATE):
        want = reference(w, h, 6, flags)
        same(b.call(_lib.CRTD_GUIDES_PLANES, 6, flags), want)
        same(b.call(_lib.CRTD_GUIDES_SURFACE, 6, flags), want)
    b.inputs_untouched()


def test_on_another_stream_and_back_to_back_with_one_scratch():
    import torch
    w, h = 70, 37
    b = Buffers(w, h)
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())                                    # the uploads were made on the current stream
    with torch.cuda.stream(side):
        first = b.call(_lib.CRTD_GUIDES_PLANES, 4, ALL)
        second = b.call(_lib.CRTD_GUIDES_SURFACE, 3, ref.DEMODULATE)                 # the same scratch, an odd pass count behind an even one
        third = b.call(_lib.CRTD_GUIDES_PLANES, 1, 0, scratch=False)                 # one pass needs none
    side.synchronize()
    same(first, reference(w, h, 4, ALL))
    same(second, reference(w, h, 3, ref.DEMODULATE))
    same(third, reference(w, h, 1, 0))
    b.inputs_untouched()


# ---- through Session, on a rendered frame -----------------------------------------------------------------------------------------------------
SW, SH = 112, 72


def frame_reference(s, color, **kw):
    g = s.read_gbuffer_raw()
    geometry = np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1)
    return ref.denoise(color, geometry, g["ids"]["instance"], g["albedo"], **kw)


def test_session_frame_tensor_and_surface_forms():
    import torch
    sc = scenes.get("tiny")
    with driver.Session(SW, SH, device=0) as s:
        s.load_scene(sc)
        # the frame's own rays and their surface records, then the G-buffer frame itself
        s.render_raw(WRITE_RAYS)
        dirs = s.read_rays().reshape(-1, 3)
        _, _, pos = s.camera()
        hits = s.shade_rays(dev(np.asarray(pos, np.float32)), dev(dirs), radiance=False, surface=True)
        with pytest.raises(ValueError, match="render_raw"):
            s.denoise()
        s.render(gbuffer=True)
        frame = s.read_output()
        assert 0.0 < (s.read_gbuffer_raw()["geometry"]["t"] <= 99998.0).mean() < 1.0  # the frame shows the scene and sky around it
        # frame form, defaults and every option
        same(s.denoise(), frame_reference(s, frame, iterations=4, flags=ref.DEMODULATE, depth_tol=0.05, normal_cos=0.9))
        same(s.denoise(iterations=6, depth_tol=0.1, normal_cos=0.5, luma_tol=0.25, demodulate=False, match_instance=True),
             frame_reference(s, frame, iterations=6, flags=ref.MATCH_INSTANCE | ref.LUMA_STOP, depth_tol=0.1, normal_cos=0.5, luma_tol=0.25))
        assert np.array_equal(bits(s.read_output()), bits(frame))
        # tensor form: seeded noise on the frame
        noisy = (frame + np.random.RandomState(3).normal(0, 0.3, frame.shape) * np.array([1, 1, 1, 0])).astype(np.float32)
        t_noisy = dev(noisy)
        want = frame_reference(s, noisy, iterations=3, flags=ref.DEMODULATE, depth_tol=0.05, normal_cos=0.9)
        got = s.denoise(t_noisy, iterations=3)
        same(got, want)
        assert got.shape == (SH, SW, 4) and got.dtype == torch.float32 and got.device == t_noisy.device
        hit = s.read_gbuffer_raw()["geometry"]["t"] <= 99998.0
        assert np.abs(want - frame)[hit][:, :3].mean() < np.abs(noisy - frame)[hit][:, :3].mean()      # and it denoises: closer to the clean frame
        # surface=: the records of the frame's own rays guide as the planes do
        mine = torch.full((SH, SW, 4), float("nan"), device="cuda:0")
        assert s.denoise(t_noisy, iterations=3, surface=hits, out=mine) is mine
        same(mine, want)
        same(s.denoise(t_noisy, iterations=5, surface=hits, match_instance=True), s.denoise(t_noisy, iterations=5, match_instance=True).cpu().numpy())
        assert np.array_equal(bits(t_noisy.cpu().numpy()), bits(noisy))


def test_session_refusals():
    import torch
    sc = scenes.get("tiny")
    with driver.Session(SW, SH, device=0) as s:
        s.load_scene(sc)
        with pytest.raises(ValueError, match="none has been rendered"):
            s.denoise()
        s.render()
        with pytest.raises(ValueError, match="without gbuffer"):
            s.denoise()
        s.render(gbuffer=True)
        good = torch.zeros((SH, SW, 4), device="cuda:0")
        for bad in (good.cpu(), good.double(), good[:, :, :3], good[:-1], good.permute(1, 0, 2), np.zeros((SH, SW, 4), np.float32)):
            with pytest.raises(ValueError):
                s.denoise(bad)
            with pytest.raises(ValueError):
                s.denoise(good, out=bad)
        hits = s.shade_rays(torch.zeros(3, device="cuda:0"), torch.ones((5, 3), device="cuda:0"), radiance=False, surface=True)
        with pytest.raises(ValueError, match="records"):
            s.denoise(good, surface=hits)                          # 5 records for 112 x 72 pixels
        with pytest.raises(ValueError):
            s.denoise(surface=hits)                                # surface= guides a colour tensor
        with pytest.raises(driver.CrtError, match="bad argument"):
            s.denoise(good, iterations=7)
        with pytest.raises(driver.CrtError, match="bad argument"):
            s.denoise(good, out=good)
        s.denoise(good)
        s.set_row_bands(16, 1, 2)
        with pytest.raises(ValueError, match="row bands"):
            s.denoise()
        s.set_row_bands(16, 0, 1)
        s.render(gbuffer=True)
        s.denoise()
        s.resize(96, 64)
        with pytest.raises(ValueError, match="none has been rendered"):
            s.denoise()
    with driver.Session(SW, SH, devices=[0, 0]) as s:
        s.load_scene(sc)
        s.render()
        with pytest.raises(ValueError, match="several devices"):
            s.denoise()
