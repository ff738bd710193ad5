"""crtp_present, crtp_view and Session.present / Session.view on the GPU.

Frame equivalence: on the plain colour of a frame, present() gives what render_raw stores under the same POSTPROCESS / UNORM8 / FXAA flags, floats
and RGBA8 bytes, bit for bit -- the chain on device buffers ends where the frame path ends. Against tests/present_ref.py: the forms without
PostProcess bit for bit on HDR random images (NaN, +-Inf, negatives, values above 1) and on patterns that drive FXAA to its +-8 clamp and to the
edge clamps; the forms with PostProcess under the rule of tests/test_gpu_flag_matrix.py (powf on the device and on the host differ in the last
place). Views: every mode under both guide layouts. The chain end to end, and one call behind a held stream.

Where a value is a NaN the comparison is of the NaN pattern, not of the payload: IEEE 754 leaves the sign and payload of a NaN an operation
GENERATES (inf - inf, inf * 0) to the hardware -- x86 makes 0xFFC00000, gfx950 0x7FC00000 -- so the oracle on the host and the kernel differ
there by construction. Every value that is no NaN is compared in every bit, and so is every byte (a NaN packs to 0 on both)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clraytracer_amd import _lib, driver, scenes

if not os.path.exists(getattr(_lib, "PRESENT_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import present_ref as ref
import test_gpu_upsample as gu
from stream_hold import Hold
from util import bits

pytestmark = pytest.mark.gpu
GUARD = 64
POST, UNORM8, FXAA, WRITE_RAYS = 1, 64, 512, 2          # crt_render's flags
AO = dict(radius=16.0, bias=1e-3)                       # tests/test_gpu_ao.py: the radius at which `tiny` occludes a share of the sample rays


def render_flags(f):
    """crt_render's flags for the CRTP_* set f"""
    return (POST if f & ref.POST else 0) | (UNORM8 if f & ref.UNORM8 else 0) | (FXAA if f & ref.FXAA else 0)


def kwargs(f):
    return dict(postprocess=bool(f & ref.POST), unorm8=bool(f & ref.UNORM8), fxaa=bool(f & ref.FXAA), heal=bool(f & ref.HEAL))


def same(got, want, what=""):
    """every bit, except that a NaN equals any NaN (see the module's docstring)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: the NaN patterns differ at {int((gn != wn).sum())} values"
    differ = (bits(got) != bits(want)) & ~gn
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} values differ, the first at {tuple(int(i[0]) for i in np.nonzero(differ))}"


def guarded_out(h, w):
    """a poisoned (h, w, 4) float image with GUARD poisoned words behind it, and the whole allocation"""
    whole = gu.poison((h * w * 4 + GUARD,), 0x500)
    return whole[:h * w * 4].reshape(h, w, 4), whole


def guard_intact(whole, words):
    tail = (np.arange(words, words + GUARD, dtype=np.int64) + (0x7FC00000 + 0x500)).astype(np.uint32)
    assert np.array_equal(whole.cpu().numpy().view(np.uint32)[words:], tail), "the words behind the output were written"


def raw_present(color, flags, ao=None, strength=1.0, exposure=1.0):
    """crtp_present itself on device tensors of any size: (float image, bytes) as numpy, outputs poisoned and guarded"""
    import torch
    h, w = color.shape[:2]
    out, whole = guarded_out(h, w)
    packed = gu.poison((h, w), 0x600, "int32")
    p = _lib.CrtpPresent(w, h, color.data_ptr(), ao.data_ptr() if ao is not None else None, strength, exposure, flags)
    lib = _lib.present()
    rc = lib.crtp_present(C.byref(p), out.data_ptr(), packed.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.crtp_error_string(rc)
    guard_intact(whole, h * w * 4)
    return out.cpu().numpy(), packed.cpu().numpy().view(np.uint8).reshape(h, w, 4)


# ---- frame equivalence: the test that fails without the feature --------------------------------------------------------------------------------
FRAMES = [("tiny", 200, 120), ("tiny", 16, 16), ("tiny", 33, 9), ("cornell-1k", 333, 187)]


@pytest.mark.parametrize("source", ["frame", "tensor"])
@pytest.mark.parametrize("scene,W,H", FRAMES, ids=[f"{n}-{w}x{h}" for n, w, h in FRAMES])
def test_present_of_the_plain_frame_is_the_frame_path_s_frame(scene, W, H, source):
    """33 x 9: the frame path takes no frame below 16 rows or columns (crt_init refuses it as upstream's Renderer does, Renderer.cpp:96), so there
    is no frame to be equal to: the case pins the refusal and runs the equivalence at 33 x 16, the nearest frame there is. 33 x 9 itself is
    compared against the reference in the tests below, which need no session."""
    import torch
    if H < 16:
        with pytest.raises(driver.CrtError):
            driver.Session(W, H, device=0)
        H = 16
    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get(scene))
        s.render_raw(0)
        plain = s.read_output()
        tensor = torch.from_numpy(plain.copy()).to("cuda:0")
        for f in range(8):
            s.render_raw(render_flags(f))
            want, want_bytes = s.read_output(), s.read_output_rgba8()
            if source == "frame":
                s.render_raw(0)
            out, whole = guarded_out(H, W)
            got = s.present(None if source == "frame" else tensor, out=out, **kwargs(f))
            assert got[0] is out and got[1].dtype == torch.uint8 and tuple(got[1].shape) == (H, W, 4)
            assert np.array_equal(bits(out.cpu().numpy()), bits(want)), (scene, W, H, f)
            assert np.array_equal(got[1].cpu().numpy(), want_bytes), (scene, W, H, f)
            guard_intact(whole, H * W * 4)
            if f & ref.FXAA:
                assert not np.array_equal(bits(want), bits(ref.frame_chain(plain, f & ~ref.FXAA)))     # the filter moved something
        # the other two return forms hold the same values
        only_bytes = s.present(tensor)
        only_float = s.present(tensor, bytes=False)
        both = s.present(tensor, out=torch.empty_like(tensor))
        assert only_bytes.dtype == torch.uint8 and only_float.dtype == torch.float32
        assert torch.equal(only_bytes, both[1]) and torch.equal(only_float.view(torch.int32), both[0].view(torch.int32))
        assert np.array_equal(bits(tensor.cpu().numpy()), bits(plain))                                  # the input is only read


# ---- against the reference, bit for bit: every form without PostProcess ------------------------------------------------------------------------
SIZES = [(1, 1), (3, 2), (31, 7), (33, 9), (64, 16), (200, 120)]
EXACT = [f | h for h in (0, ref.HEAL) for f in (0, ref.UNORM8, ref.FXAA, ref.UNORM8 | ref.FXAA)]


def hdr_image(w, h, seed):
    rng = np.random.RandomState(seed)
    img = rng.uniform(-0.5, 2.5, (h, w, 4)).astype(np.float32)
    img *= (rng.uniform(size=(h, w, 1)) < 0.85)                       # black pixels too
    n = w * h * 3
    flat = img[..., :3].reshape(-1).copy()
    for k, v in enumerate((np.nan, np.inf, -np.inf, -3.0, 40.0, 1.0, 0.5 / 255.0, 1.5 / 255.0)):
        flat[rng.randint(0, n, max(1, n // 97))] = v
        flat[k % n] = v if n >= 8 else flat[k % n]
    img[..., :3] = flat.reshape(h, w, 3)
    return img


def ao_plane(w, h, seed):
    rng = np.random.RandomState(seed)
    ao = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    ao[rng.uniform(size=(h, w)) < 0.02] = np.nan
    ao[0, 0] = np.inf
    return ao


@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_forms_without_postprocess_match_the_reference_in_every_bit(W, H):
    aoh = ao_plane(W, H, 3 * W + H)
    aod = gu.dev(aoh)
    images = {"hdr": hdr_image(W, H, W * 1000 + H), **ref.fxaa_patterns(W, H)}
    ran = moved = 0
    for name, host in images.items():
        color = gu.dev(host)
        for f in EXACT:
            if name != "hdr" and not f & ref.FXAA:
                continue
            for strength in (None, 0.0, 0.35, 1.0) if name == "hdr" else (None, 0.35):
                for exposure in (1.0, 1.7):
                    a = dict(ao=None) if strength is None else dict(ao=aoh, ao_strength=strength)
                    want, want_bytes = ref.present(host, f, exposure=exposure, **a)
                    got, got_bytes = raw_present(color, f, None if strength is None else aod, 1.0 if strength is None else strength, exposure)
                    what = f"{W}x{H} {name} flags {f} ao {strength} exposure {exposure}"
                    same(got, want, what)
                    assert np.array_equal(got_bytes, want_bytes), what
                    if f & ref.HEAL:
                        assert np.isfinite(got).all(), what
                    if name != "hdr" and W >= 31:
                        # a filter that is a no-op fails here: the filtered image is not the image it read
                        S = ref.source(host, f, exposure=exposure, **a)
                        assert not np.array_equal(bits(got[..., :3]), bits(S[..., :3])), what
                        moved += 1
                    ran += 1
        assert np.array_equal(bits(color.cpu().numpy()), bits(host))
    assert ran == 8 * 4 * 2 + 4 * 4 * 2 * 2 and moved == (4 * 4 * 2 * 2 if W >= 31 else 0)
    same(aod.cpu().numpy(), aoh)


def test_both_fxaa_variants_give_the_same_bits(monkeypatch):
    """CRTP_TAPS=l1|lds: the taps made again from color and ao through L1, or read from the staged tile"""
    W, H = 70, 37
    host, aoh = hdr_image(W, H, 5), ao_plane(W, H, 6)
    color, aod = gu.dev(host), gu.dev(aoh)
    for f in (ref.FXAA, ref.FXAA | ref.UNORM8 | ref.HEAL, ref.FXAA | ref.POST | ref.UNORM8):
        results = {}
        for taps in ("l1", "lds"):
            monkeypatch.setenv("CRTP_TAPS", taps)
            results[taps] = raw_present(color, f, aod, 0.35, 1.7)
        same(results["l1"][0], results["lds"][0], f"flags {f}")         # (which operand's payload a NaN result carries is the instruction's choice)
        assert np.array_equal(results["l1"][1], results["lds"][1]), f


# ---- with PostProcess: the rule of tests/test_gpu_flag_matrix.py:63-67, on the scenes' frames --------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_frame(scene, W, H):
    """the plain frame of a scene, its G-buffer planes and the frame's rays: rendered once, shared, never written"""
    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get(scene))
        s.render_raw(WRITE_RAYS)
        rays = s.read_rays().reshape(-1, 3).copy()
        s.render(gbuffer=True)
        frame = np.array(s.output(), copy=True)
        planes = {k: v.copy() for k, v in s.read_gbuffer_raw().items()}
    for a in (rays, frame, *planes.values()):
        a.setflags(write=False)
    return frame, planes, rays


def post_rule(got, want, unorm, what):
    """the NaN pattern is identical; without UNORM8 max |d| < 2e-5 (powf); with it a value may move by one code -- max |d| < 1/255 + 1e-6 -- and
    at most 0.002 of the values differ by more than 2e-5"""
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst, moved = float(np.nanmax(d)), int((d > 2e-5).sum())
    print(f"{what}: max |d| {worst:.3e}, {moved} of {d.size} values beyond 2e-5")
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert worst < ((1.0 / 255.0 + 1e-6) if unorm else 2e-5), (what, worst)
    assert moved <= 0.002 * d.size, (what, moved)


@pytest.mark.parametrize("scene,W,H", [("tiny", 200, 120), ("cornell-1k", 333, 187)])
def test_forms_with_postprocess_match_the_reference_under_the_frame_s_rule(scene, W, H):
    frame, _, _ = scene_frame(scene, W, H)
    rng = np.random.RandomState(W)
    aoh = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    color, aod = gu.dev(frame), gu.dev(aoh)
    for f in (ref.POST, ref.POST | ref.UNORM8, ref.POST | ref.FXAA, ref.POST | ref.UNORM8 | ref.FXAA, ref.POST | ref.UNORM8 | ref.FXAA | ref.HEAL):
        for strength in (None, 0.35):
            a = dict(ao=None) if strength is None else dict(ao=aoh, ao_strength=strength)
            want, want_bytes = ref.present(frame, f, **a)
            got, got_bytes = raw_present(color, f, None if strength is None else aod, 1.0 if strength is None else strength, 1.0)
            what = f"{scene} {W}x{H} flags {f} ao {strength}"
            post_rule(got, want, f & ref.UNORM8, what)
            assert (got[..., 3] == 1.0).all()
            # the bytes: those of the float result exactly; against the reference's a byte may be the neighbouring code, as rarely
            assert np.array_equal(got_bytes, ref.pack(got)), what
            db = np.abs(got_bytes.astype(np.int32) - want_bytes.astype(np.int32))
            assert db.max() <= 1 and (db > 0).sum() <= 0.002 * db.size, (what, int(db.max()), int((db > 0).sum()))


# ---- views -------------------------------------------------------------------------------------------------------------------------------------
def view_arrays(planes):
    g, ids = planes["geometry"], planes["ids"]
    return dict(normal=np.ascontiguousarray(g["normal"]), t=np.ascontiguousarray(g["t"]), instance=np.ascontiguousarray(ids["instance"]),
                tri=np.ascontiguousarray(ids["tri"]), albedo=np.ascontiguousarray(planes["albedo"]))


def check_view(got, want, what):
    f, b = (x.cpu().numpy() for x in got)
    assert np.array_equal(b, want[1]), f"{what}: {int((b != want[1]).sum())} bytes differ"
    assert np.array_equal(bits(f), bits(want[0])), what


def test_session_views_of_a_frame_under_both_layouts():
    import torch
    W, H = 200, 120
    frame, planes, rays = scene_frame("tiny", W, H)
    arrays = view_arrays(planes)
    rng = np.random.RandomState(9)
    scalar = rng.uniform(-0.2, 1.2, (H, W)).astype(np.float32)
    scalar[rng.uniform(size=(H, W)) < 0.01] = np.nan
    state = rng.randint(0, 4, (H, W)).astype(np.int32)
    state[rng.uniform(size=(H, W)) < 0.01] = 7
    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get("tiny"))
        _, _, pos = s.camera()
        hits = s.shade_rays(gu.dev(np.asarray(pos, np.float32)), gu.dev(rays), radiance=False, surface=True)
        s.render(gbuffer=True)
        assert (arrays["t"] <= 99998.0).any() and not (arrays["t"] <= 99998.0).all() and len(np.unique(arrays["instance"])) > 2
        for mode in ("normal", "depth", "instance", "triangle", "albedo"):
            want = ref.view(mode, scale=25.0, **arrays)
            assert len(np.unique(want[1].reshape(-1, 4), axis=0)) > 2, mode           # a picture, not a constant
            for kw in (dict(), dict(surface=hits)):
                out = torch.empty((H, W, 4), device="cuda:0")
                check_view(s.view(mode, scale=25.0, out=out, **kw), want, f"{mode} {sorted(kw)}")
        check_view(s.view("scalar", plane=gu.dev(scalar), lo=0.1, hi=0.9, out=torch.empty((H, W, 4), device="cuda:0")),
                   ref.view("scalar", plane=scalar, lo=0.1, hi=0.9), "scalar")
        check_view(s.view("state", plane=gu.dev(state), out=torch.empty((H, W, 4), device="cuda:0")), ref.view("state", plane=state), "state")
        only = s.view("normal")
        assert only.dtype == torch.uint8 and np.array_equal(only.cpu().numpy(), ref.view("normal", **arrays)[1])
        for bad in (lambda: s.view("colour"), lambda: s.view("scalar"), lambda: s.view("normal", plane=gu.dev(scalar)),
                    lambda: s.view("state", plane=gu.dev(scalar)), lambda: s.view("scalar", plane=gu.dev(scalar), surface=hits)):
            with pytest.raises(ValueError):
                bad()
        s.render()
        with pytest.raises(ValueError, match="without gbuffer"):
            s.view("depth")


def test_views_of_synthetic_planes_under_both_layouts():
    """a miss, a NaN t, a negative instance, a state word of 7, odd sizes: crtp_view itself on device tensors"""
    import torch
    lib = _lib.present()
    for W, H in ((33, 9), (1, 1), (70, 37)):
        rng = np.random.RandomState(W)
        n = rng.normal(size=(H, W, 3)).astype(np.float32)
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        t = rng.uniform(0.0, 60.0, (H, W)).astype(np.float32)
        inst = rng.randint(0, 9, (H, W)).astype(np.int32)
        tri = rng.randint(0, 2 ** 31, (H, W)).astype(np.uint32)
        albedo = (rng.randint(0, 2 ** 24, (H, W)).astype(np.uint32) | np.uint32(0xFF000000))
        for k, (tv, iv) in enumerate(((99999.0, -1), (np.nan, 3), (99998.0, -5), (99998.5, 2), (np.inf, 0), (-1.0, 2 ** 31 - 1))):
            y, x = divmod((k * 7) % (W * H), W)
            t[y, x], inst[y, x] = tv, iv
        records = np.zeros((H, W, 12), np.int32)
        records[..., 0:3] = n.view(np.int32); records[..., 3] = t.view(np.int32); records[..., 4] = inst; records[..., 5] = tri.view(np.int32)
        records[..., 8] = albedo.view(np.int32); records[..., 9:] = 0x55555555
        geometry = np.concatenate([n, t[..., None]], axis=-1)
        ids = np.zeros((H, W, 4), np.int32)
        ids[..., 0] = inst; ids[..., 1] = tri.view(np.int32); ids[..., 2:] = 0x33333333
        scalar = rng.uniform(-1.0, 2.0, (H, W)).astype(np.float32)
        scalar[0, 0] = np.nan
        state = rng.randint(0, 4, (H, W)).astype(np.int32)
        state[-1, -1] = 7
        dv = {k: gu.dev(v) for k, v in dict(geometry=geometry, ids=ids, albedo=albedo.view(np.int32), records=records, scalar=scalar, state=state).items()}
        arrays = dict(normal=n, t=t, instance=inst, tri=tri, albedo=albedo)
        for mode, m in ref.MODES.items():
            plane = dv["scalar"] if mode == "scalar" else dv["state"] if mode == "state" else None
            want = ref.view(mode, scale=7.5, lo=-0.5, hi=1.5, plane=scalar if mode == "scalar" else state, **arrays)
            for layout in (_lib.CRTP_GUIDES_PLANES, _lib.CRTP_GUIDES_SURFACE):
                surface = layout == _lib.CRTP_GUIDES_SURFACE
                v = _lib.CrtpView(W, H, layout, m, (dv["records"] if surface else dv["geometry"]).data_ptr(), None if surface else dv["ids"].data_ptr(),
                                  None if surface else dv["albedo"].data_ptr(), plane.data_ptr() if plane is not None else None, 7.5, -0.5, 1.5)
                out, whole = guarded_out(H, W)
                packed = gu.poison((H, W), 0x700, "int32")
                rc = lib.crtp_view(C.byref(v), out.data_ptr(), packed.data_ptr(), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, lib.crtp_error_string(rc)
                what = f"{W}x{H} {mode} layout {layout}"
                assert np.array_equal(packed.cpu().numpy().view(np.uint8).reshape(H, W, 4), want[1]), what
                assert np.array_equal(bits(out.cpu().numpy()), bits(want[0])), what
                guard_intact(whole, H * W * 4)


# ---- the chain, end to end ---------------------------------------------------------------------------------------------------------------------
def test_render_ao_at_half_resolution_upsample_present():
    W, H = 160, 96
    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get("tiny"))
        s.render(gbuffer=True)
        frame = np.array(s.output(), copy=True)
        positions, normals = s.frame_points(factor=2)
        low = s.trace_ao(positions[:, :3], normals[:, :3], 8, **AO).reshape(H // 2, W // 2)
        ao = s.upsample(low)
        got = s.present(ao=ao, ao_strength=0.8, exposure=1.25, postprocess=False, fxaa=True)
        aoh = ao.cpu().numpy()
        assert 0.0 <= aoh.min() < aoh.max() <= 1.0
        want = ref.present(frame, ref.UNORM8 | ref.FXAA, ao=aoh, ao_strength=0.8, exposure=1.25)
        assert np.array_equal(got.cpu().numpy(), want[1])
        assert not np.array_equal(want[1], ref.present(frame, ref.UNORM8 | ref.FXAA, exposure=1.25)[1])       # the AO plane shows
        # the default form ends in PostProcess: a byte may be the neighbouring code (powf), as rarely as the frame's rule has it
        got = s.present(ao=ao, ao_strength=0.8).cpu().numpy()
        want = ref.present(frame, ref.UNORM8 | ref.POST, ao=aoh, ao_strength=0.8)[1]
        db = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert db.max() <= 1 and (db > 0).sum() <= 0.002 * db.size, (int(db.max()), int((db > 0).sum()))
        assert s.frame_readers_pending() >= 0
        s.render()                                                          # waits for the readers of the frame's buffer


# ---- stream order ------------------------------------------------------------------------------------------------------------------------------
def test_present_on_a_held_stream_returns_at_once_and_is_right_afterwards():
    import torch
    W, H = 200, 120
    frame, _, _ = scene_frame("tiny", W, H)
    rng = np.random.RandomState(4)
    aoh = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    color, aod = gu.dev(frame), gu.dev(aoh)
    want = ref.present(frame, ref.UNORM8 | ref.FXAA, ao=aoh, ao_strength=0.5)
    case = "present on a held stream"
    with driver.Session(W, H, device=0) as s:
        side = torch.cuda.Stream(device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            out = torch.empty((H, W, 4), device="cuda:0")
            s.present(color, ao=aod, ao_strength=0.5, postprocess=False, fxaa=True, out=out)       # nothing allocates inside the window
        side.synchronize()
        out.fill_(-1.0)
        torch.cuda.synchronize()
        hold = Hold(side)
        with torch.cuda.stream(side):
            got = s.present(color, ao=aod, ao_strength=0.5, postprocess=False, fxaa=True, out=out)
        hold.must_be_pending(case)
        assert s.frame_readers_pending() == 0                               # the tensor form leaves nothing for a render to wait for
        hold.release()
        side.synchronize()
        same(got[0].cpu().numpy(), want[0], case)
        assert np.array_equal(got[1].cpu().numpy(), want[1]), case


def test_session_refusals():
    import torch
    sc = scenes.get("tiny")
    W, H = 160, 96
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(sc)
        for call in (lambda: s.present(), lambda: s.view("normal")):
            with pytest.raises(ValueError, match="host-only"):
                call()
    with driver.Session(W, H, device=0) as s:
        s.load_scene(sc)
        with pytest.raises(ValueError, match="no frame has been rendered"):
            s.present()
        color = torch.zeros((H, W, 4), device="cuda:0")
        for kw in (dict(ao_strength=1.5), dict(ao_strength=-0.1), dict(exposure=0.0), dict(exposure=float("nan")), dict(exposure=float("inf"))):
            with pytest.raises(driver.CrtError, match="bad argument"):
                s.present(color, **kw)
        with pytest.raises(driver.CrtError, match="bad argument"):
            s.present(color, out=color)                                     # in place is never allowed
        for bad in (dict(color=color.cpu()), dict(color=color.double()), dict(color=color[:-1]), dict(color=color, ao=torch.zeros((H, W, 1), device="cuda:0")),
                    dict(color=color, ao=torch.zeros((H, W), device="cuda:0", dtype=torch.float64)), dict(color=color, out=torch.zeros((H, W, 3), device="cuda:0"))):
            with pytest.raises(ValueError):
                s.present(**bad)
        s.render_raw(0)
        s.set_row_bands(16, 0, 2)
        with pytest.raises(ValueError, match="row bands"):
            s.present()
