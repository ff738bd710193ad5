"""crtm_accumulate / Session.accumulate(instances=) on the GPU against the numpy restatement of the definition (tests/motion_ref.py): every pixel
of all four planes of `next` and of the motion-vector plane, bit for bit (util.bits), none exempt; the outputs start as NaN poison whose payload
differs from word to word. Shapes that break tiles and the clamp's halo (1 x 1, 5 x 3, 33 x 9, 70 x 37, 257 x 19); tests/test_gpu_temporal.py's
hand-made frame and history with the instance planes remapped onto five ids, over a table with one entry of each kind -- static, moving by a
translation, moving by a rotation and a non-uniform scale, new -- and an id beyond its count; a static and a panned camera pair, every flag
combination, both layouts of the current frame, a reset; the same bits as crtt_accumulate on the same device buffers wherever nothing moves; a
ping-ponged sequence on another stream; and a Session on rendered frames of `tiny` between which an instance moves."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clraytracer_amd import _lib, driver, scenes

if not os.path.exists(getattr(_lib, "MOTION_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import motion_ref as ref
import temporal_ref
from util import bits

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (5, 3), (33, 9), (70, 37), (257, 19)]                 # (width, height)
BOTH = ref.MATCH_INSTANCE | ref.CLAMP
PARAMS = dict(alpha=0.2, moments_alpha=0.3, max_history=32.0, depth_tol=0.05, normal_cos=0.9)
PLANES = ("color", "moments", "geometry", "instance")
TABLE = ref.hand_made_table()
TABLE.setflags(write=False)


@functools.lru_cache(maxsize=None)
def inputs(w, h):
    """the hand-made frame and previous history of one shape, their instance planes on the five ids: made once, never modified"""
    planes, color, hist = ref.hand_made_inputs(h, w)
    for a in (*planes.values(), color, *(hist[k] for k in PLANES)):
        a.setflags(write=False)
    return planes, color, hist


def frozen(hist, vectors):
    for a in [hist[k] for k in PLANES if hist[k] is not None] + [vectors]:
        a.setflags(write=False)
    return hist, vectors


@functools.lru_cache(maxsize=None)
def reference(w, h, pair, flags, reset=False, table="hand-made"):
    planes, color, hist = inputs(w, h)
    cur, prev_cam = ref.camera_pairs(w, h)[pair]
    prev = None if reset else dict(hist, camera=prev_cam)
    return frozen(*ref.accumulate(color, planes["geometry"], planes["ids"]["instance"].astype(np.int32), cur, prev=prev,
                                  motions=TABLE if table == "hand-made" else None, flags=flags, **PARAMS))


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")


def camera_struct(cam):
    c = _lib.CrttCamera()
    c.pos[:], c.toRay[:], c.toScreen[:] = [float(v) for v in cam["pos"]], [float(v) for v in cam["toRay"].reshape(-1)], [float(v) for v in cam["toScreen"].reshape(-1)]
    return c


def poison_words(n, salt):
    import torch
    return torch.arange(n, dtype=torch.int32, device="cuda:0") + (0x7FC00000 + salt)


def poison(n, salt):
    """n float32 NaNs whose payload differs from word to word"""
    import torch
    return poison_words(n, salt).view(torch.float32)


class History:
    """one set of history planes on the device: poison (what `next` holds before a call) or a copy of host planes"""

    def __init__(self, w, h, salt=None, host=None):
        self.w, self.h = w, h
        if host is None:
            self.t = {k: poison(h * w * 4, salt + 0x100 * i).reshape(h, w, 4) for i, k in enumerate(PLANES[:3])}
            self.t["instance"] = poison_words(h * w, salt + 0x300).reshape(h, w)
        else:
            self.t = {k: dev(host[k]) for k in PLANES}

    def struct(self, cam):
        return _lib.CrttHistory(*[self.t[k].data_ptr() for k in PLANES], camera_struct(cam))

    def host(self):
        return {k: self.t[k].cpu().numpy() for k in PLANES}


class Buffers:
    """One shape's inputs on the device, the current frame under either layout; motion() runs crtm_accumulate and sibling() crtt_accumulate
    on torch's current stream."""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.planes, self.color, self.hist = inputs(w, h)
        self.t_color = dev(self.color)
        self.t_planes = {k: dev(v.view(np.int32) if v.dtype.fields is None else v.view(np.int32).reshape(h, w, 4)) for k, v in self.planes.items()}
        self.records = ref.surface_records(self.planes)
        self.t_records = dev(self.records)
        self.prev = History(w, h, host=self.hist)
        self.t_table = dev(TABLE.view(np.uint8))

    def frame(self, layout, cam):
        f = _lib.CrttFrame(self.w, self.h, self.t_color.data_ptr(), layout, None, None, camera_struct(cam))
        if layout == _lib.CRTT_GUIDES_SURFACE:
            f.geometry = self.t_records.data_ptr()
        else:
            f.geometry, f.ids = self.t_planes["geometry"].data_ptr(), self.t_planes["ids"].data_ptr()
        return f

    def _args(self, layout, pair, flags, reset, prev, nxt, cams, params):
        cur, prev_cam = cams or ref.camera_pairs(self.w, self.h)[pair]
        nxt = History(self.w, self.h, salt=0x77) if nxt is None else nxt
        p = _lib.CrttParams(flags, params["alpha"], params["moments_alpha"], params["max_history"], params["depth_tol"], params["normal_cos"])
        self._keep = (self.frame(layout, cur), None if reset else (prev or self.prev).struct(prev_cam), nxt.struct(cur), p)
        f, pv, nx, p = self._keep
        return nxt, (C.byref(f), None if reset else C.byref(pv), C.byref(nx), C.byref(p))

    def motion(self, layout, pair, flags, reset=False, prev=None, nxt=None, cams=None, params=PARAMS, table="hand-made", vectors=True):
        import torch
        nxt, args = self._args(layout, pair, flags, reset, prev, nxt, cams, params)
        t_table = {"hand-made": self.t_table, None: None}.get(table, table)
        t_vectors = poison(self.h * self.w * 4, 0x500).reshape(self.h, self.w, 4) if vectors is True else vectors if vectors is not False else None
        m = _lib.CrtmMotionArgs(t_table.data_ptr() if t_table is not None else None, t_table.numel() // 88 if t_table is not None else 0,
                                t_vectors.data_ptr() if t_vectors is not None else None)
        lib = _lib.motion()
        rc = lib.crtm_accumulate(*args, C.byref(m), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.crtm_error_string(rc)
        return nxt, t_vectors

    def sibling(self, layout, pair, flags, reset=False):
        import torch
        nxt, args = self._args(layout, pair, flags, reset, None, None, None, PARAMS)
        lib = _lib.temporal()
        rc = lib.crtt_accumulate(*args, torch.cuda.current_stream().cuda_stream)
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
        assert np.array_equal(self.t_table.cpu().numpy(), TABLE.view(np.uint8))


def same(got, want):
    """(History or dict, vectors tensor or array or None) against (history dict, vectors array)"""
    hist, vectors = got
    hist = hist.host() if isinstance(hist, History) else hist
    names = PLANES[:3] + (("vectors",) if vectors is not None else ())
    have = dict(hist, vectors=vectors if isinstance(vectors, np.ndarray) or vectors is None else vectors.cpu().numpy())
    for k in names:
        w = want[1] if k == "vectors" else want[0][k]
        differ = (bits(have[k]) != bits(w)).any(axis=-1)
        assert not differ.any(), f"{k}: {int(differ.sum())} of {differ.size} pixels differ, the first at (y, x) = {tuple(np.argwhere(differ)[0])}"
    differ = hist["instance"] != want[0]["instance"]
    assert not differ.any(), f"instance: {int(differ.sum())} of {differ.size} pixels differ, the first at (y, x) = {tuple(np.argwhere(differ)[0])}"


@pytest.mark.parametrize("pair", ["identical", "pan left"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_shape_matches_the_reference_under_a_static_and_a_panned_camera(shape, pair):
    """Fails against a build that reprojects every pixel through the camera alone: ids 1 and 2 move."""
    w, h = shape
    b = Buffers(w, h)
    want = reference(w, h, pair, BOTH)
    same(b.motion(_lib.CRTT_GUIDES_PLANES, pair, BOTH), want)
    same(b.motion(_lib.CRTT_GUIDES_SURFACE, pair, BOTH), want)
    b.inputs_untouched()
    if w * h > 1000:
        static = reference(w, h, pair, BOTH, table=None)
        inst = b.planes["ids"]["instance"]
        for i in (1, 2):                                                     # the moving entries are seen
            assert (bits(want[0]["color"]) != bits(static[0]["color"]))[inst == i].any() and (bits(want[1]) != bits(static[1]))[inst == i].any(), i
        assert set(np.unique(want[1][..., 3])) == {0.0, 1.0, 2.0}


@pytest.mark.parametrize("flags", range(4))
def test_every_flag_combination_and_a_reset(flags):
    w, h, pair = 70, 37, "sub-pixel pan"
    b = Buffers(w, h)
    want = reference(w, h, pair, flags)
    same(b.motion(_lib.CRTT_GUIDES_PLANES, pair, flags), want)
    same(b.motion(_lib.CRTT_GUIDES_SURFACE, pair, flags), want)
    if flags:
        assert not np.array_equal(bits(want[0]["color"]), bits(reference(w, h, pair, 0)[0]["color"]))      # the flag is seen
    # without a vectors plane the history is the same
    same((b.motion(_lib.CRTT_GUIDES_PLANES, pair, flags, vectors=False)[0], None), want)
    # prev == NULL: the frame itself and vectors of zeros, whatever the flags and the table
    reset = reference(w, h, pair, flags, reset=True)
    same(b.motion(_lib.CRTT_GUIDES_PLANES, pair, flags, reset=True), reset)
    same(b.motion(_lib.CRTT_GUIDES_SURFACE, pair, flags, reset=True), reset)
    assert np.array_equal(bits(reset[0]["color"]), bits(b.color)) and not reset[1].any()
    b.inputs_untouched()


def test_nans_in_the_history_heal():
    """The history of these cases holds NaN and infinite colours and moments and N of 0 (temporal_ref.history_content). Such a tap is selected
    away: the pixels that fetch it keep the history of their other taps, through a moving instance's reprojection as through the camera's."""
    w, h, pair = 70, 37, "sub-pixel pan"
    planes, color, hist = inputs(w, h)
    assert np.isnan(hist["color"]).any() and np.isinf(hist["color"]).any() and not np.isfinite(hist["moments"][..., :2]).all()
    b = Buffers(w, h)
    got, vectors = b.motion(_lib.CRTT_GUIDES_PLANES, pair, ref.MATCH_INSTANCE)
    same((got, vectors), reference(w, h, pair, ref.MATCH_INSTANCE))
    out, v = got.host(), vectors.cpu().numpy()
    kept = v[..., 3] == 2.0
    inst = planes["ids"]["instance"]
    fine = np.isfinite(color).all(axis=-1)
    assert (kept & (inst == 1)).any() and (kept & (inst == 2)).any()
    assert np.isfinite(out["color"][kept & fine]).all() and np.isfinite(out["moments"][kept & fine]).all() and np.isfinite(v).all()
    # and some of those pixels did have such a tap: with the bad values replaced by finite ones the result differs
    clean = {k: np.nan_to_num(hist[k], nan=0.5, posinf=0.5, neginf=0.5) if k in ("color", "moments") else hist[k] for k in PLANES}
    cur, prev_cam = ref.camera_pairs(w, h)[pair]
    other, _ = ref.accumulate(color, planes["geometry"], inst.astype(np.int32), cur, prev=dict(clean, camera=prev_cam), motions=TABLE, flags=ref.MATCH_INSTANCE, **PARAMS)
    assert ((bits(other["color"]) != bits(out["color"])).any(axis=-1) & kept & (inst >= 1) & (inst <= 2)).any()


@pytest.mark.parametrize("flags", range(4))
def test_where_nothing_moves_the_bits_are_the_siblings(flags):
    """Library against library on the same device buffers: a NULL table, and a table whose every entry is static."""
    w, h = 70, 37
    b = Buffers(w, h)
    static = ref.table([ref.motion(np.eye(4), np.eye(4))] * 5)
    assert (static["kind"] == ref.STATIC).all()
    t_static = dev(static.view(np.uint8))
    for pair in ("sub-pixel pan", "translation"):
        for layout in (_lib.CRTT_GUIDES_PLANES, _lib.CRTT_GUIDES_SURFACE):
            want = b.sibling(layout, pair, flags).host()
            for table in (None, t_static):
                got, vectors = b.motion(layout, pair, flags, table=table)
                got = got.host()
                for k in PLANES[:3]:
                    assert np.array_equal(bits(got[k]), bits(want[k])), (pair, layout, k)
                assert np.array_equal(got["instance"], want["instance"])
                assert np.array_equal(vectors.cpu().numpy()[..., 3] == 2.0, want["moments"][..., 2] > 1.0)
            reset = b.sibling(layout, pair, flags, reset=True).host()
            got = b.motion(layout, pair, flags, reset=True, table=t_static)[0].host()
            for k in PLANES[:3]:
                assert np.array_equal(bits(got[k]), bits(reset[k])), (pair, layout, k)
    assert (want["moments"][..., 2] > 1.0).any()
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
    for cam in cams:                                                         # the same frame three times: the camera moves, and ids 1 and 2
        hist, vectors = ref.accumulate(b.color, planes["geometry"], inst, cam, prev=hist, motions=TABLE, flags=BOTH, **params)
        want.append((hist, vectors))
    sets = [History(w, h, salt=0x1000), History(w, h, salt=0x2000)]
    t_vectors = [poison(h * w * 4, 0x3000 + i).reshape(h, w, 4) for i in range(3)]
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())                            # the uploads were made on the current stream
    got = []
    with torch.cuda.stream(side):
        for i, cam in enumerate(cams):
            layout = _lib.CRTT_GUIDES_SURFACE if i == 1 else _lib.CRTT_GUIDES_PLANES
            b.motion(layout, None, BOTH, reset=i == 0, prev=sets[(i + 1) % 2], nxt=sets[i % 2], cams=(cam, cams[i - 1]), params=params, vectors=t_vectors[i])
            got.append({k: v.clone() for k, v in sets[i % 2].t.items()})
    side.synchronize()
    for g, v, wnt in zip(got, t_vectors, want):
        same(({k: t.cpu().numpy() for k, t in g.items()}, v), wnt)
    N = want[2][0]["moments"][..., 2]
    assert (N == 2.0).any() and (N == 1.0).any() and (want[2][1][..., 3] == 2.0).any() and not want[0][1].any()
    b.inputs_untouched()


# ---- through Session, on rendered frames between which an instance moves --------------------------------------------------------------------
def local_colour(torch, s, w, h, records):
    """(h, w, 4) float32 on the device: each pixel's hit point in its instance's local space (0 where nothing is hit), alpha 1 -- computed from
    the frame's G-buffer, its camera and the transforms it was rendered with. A texture that travels with the surface."""
    g = s.read_gbuffer_raw()
    cam = temporal_ref.camera_from_struct(_lib.crtt_camera(*s.camera(), w, h))
    t = torch.from_numpy(g["geometry"]["t"].copy()).to("cuda:0")
    inst = torch.from_numpy(g["ids"]["instance"].astype(np.int64)).to("cuda:0")
    inv = torch.from_numpy(records["inv"].copy()).to("cuda:0")
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda:0", dtype=torch.float32), torch.arange(w, device="cuda:0", dtype=torch.float32), indexing="ij")
    d = torch.stack([xx, yy, torch.ones_like(xx)], dim=-1) @ torch.from_numpy(cam["toRay"]).to("cuda:0").T
    P = torch.from_numpy(cam["pos"]).to("cuda:0") + d / d.norm(dim=-1, keepdim=True) * t[..., None]
    hit = t <= 99998.0
    m = inv[torch.where(hit, inst, torch.zeros_like(inst))]
    local = torch.einsum("hwj,hwjk->hwk", P, m[..., :3, :3]) + m[..., 3, :3]
    color = torch.ones((h, w, 4), device="cuda:0")
    color[..., :3] = torch.where(hit[..., None], local, torch.zeros_like(local))
    geometry = np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1).astype(np.float32)
    return color.contiguous(), (color.cpu().numpy(), geometry, g["ids"]["instance"].astype(np.int32), cam)


def test_session_follows_an_instance_that_moves_between_two_rendered_frames():
    """`tiny` at 96 x 64: frame A; instance 0 moves 0.6 to the side (2.5 pixels on the screen); frame B. The colour is each pixel's hit point in
    its instance's local space, the same on the same piece of surface in both frames. With e = the largest-channel |out - colour of B| over the
    moved instance's pixels that keep their history (a correct fetch leaves the bilinear interpolation error of a smooth function; the
    camera-only one leaves (1 - a) = half the move in local units), the reference alone, on frames traced by the CPU oracle, gives:
    269 pixels, 95.9 % keep their history with instances= (median e 3.4e-3) and 25.7 % with instances=None (median e 0.291): a ratio of 1 / 85.
    The test asserts, on the reference over the read-back inputs first and then on the GPU's planes: at least half keep it with instances=, some
    with instances=None, and the first median is at most a tenth of the second. Fails against a build that reprojects through the camera alone."""
    import torch
    w, h = ref.SESSION_SIZE
    sc = scenes.get("tiny")
    k = ref.SESSION_INSTANCE
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        rec_a = s.arenas()["instances"]
        rec_b = ref.translated(rec_a, k, ref.SESSION_DELTA)
        follow, blind = driver.TemporalHistory(s, match_instance=True), driver.TemporalHistory(s, match_instance=True)
        s.render(gbuffer=True)
        color_a, in_a = local_colour(torch, s, w, h, rec_a)
        out = s.accumulate(follow, color_a, instances=rec_a, return_vectors=True)
        assert len(out) == 3 and out[2].shape == (h, w, 4) and out[2].dtype == torch.float32 and not bool(out[2].any())      # a first frame: no vectors
        assert follow.frames == 1 and np.array_equal(follow.instances, rec_a) and follow.instances is not rec_a
        s.accumulate(blind, color_a)
        want_a, _ = ref.accumulate(*in_a, flags=ref.MATCH_INSTANCE)
        same(({p: getattr(follow, p).cpu().numpy() for p in PLANES}, out[2]), (want_a, np.zeros((h, w, 4), np.float32)))
        same(({p: getattr(blind, p).cpu().numpy() for p in PLANES}, None), (want_a, None))

        s.upload_instances(rec_b[k:k + 1], first=k)
        s.render(gbuffer=True)
        color_b, in_b = local_colour(torch, s, w, h, rec_b)
        assert (in_b[2] != in_a[2]).any()                                        # the upload was seen: the instance covers other pixels
        color, moments, vectors = s.accumulate(follow, color_b, instances=rec_b["inv"], return_vectors=True)       # the (n, 4, 4) form
        color_blind, moments_blind = s.accumulate(blind, color_b)
        assert follow.frames == 2 and blind.frames == 2 and blind.instances is None and np.array_equal(follow.instances["inv"], rec_b["inv"])
        table = _lib.crtm_motions(rec_a, rec_b)
        assert list(table["kind"]) == [ref.MOVING if i == k else ref.STATIC for i in range(len(rec_a))]
        want = ref.accumulate(*in_b, prev=want_a, motions=table, flags=ref.MATCH_INSTANCE)
        want_blind = temporal_ref.accumulate(*in_b, prev=want_a, flags=ref.MATCH_INSTANCE)
        moved = in_b[2] == k

        def figures(c, m):
            e = np.abs(c[..., :3] - in_b[0][..., :3]).max(axis=-1)
            kept = moved & (m[..., 2] == 2.0)
            return float(kept.sum()) / float(moved.sum()), float(np.median(e[kept])) if kept.any() else float("nan")

        for who, (a, b_) in {"reference": (figures(want[0]["color"], want[0]["moments"]), figures(want_blind["color"], want_blind["moments"])),
                             "GPU": (figures(color.cpu().numpy(), moments.cpu().numpy()), figures(color_blind.cpu().numpy(), moments_blind.cpu().numpy()))}.items():
            print(f"{who}: {int(moved.sum())} pixels of the moved instance; with instances= {a[0]:.1%} keep their history, median e {a[1]:.3e}; "
                  f"with instances=None {b_[0]:.1%}, median e {b_[1]:.3e}; ratio 1 / {b_[1] / a[1]:.0f}")
            assert moved.sum() >= 100 and a[0] >= 0.5, who
            assert b_[0] > 0.0, who
            assert a[1] <= 0.1 * b_[1], who
        # the planes are the definition's, bit for bit, on the read-back inputs
        same(({p: getattr(follow, p).cpu().numpy() for p in PLANES}, vectors), want)
        same(({p: getattr(blind, p).cpu().numpy() for p in PLANES}, None), (want_blind, None))
        sideways = vectors.cpu().numpy()[..., 0][moved & (want[1][..., 3] == 2.0)]
        assert 1.5 < float(np.abs(sideways).mean()) < 4.0                     # a few pixels

        # what instances= refuses
        with pytest.raises(ValueError, match="previous transforms are unknown"):
            s.accumulate(blind, color_b, instances=rec_b)
        with pytest.raises(ValueError, match="instances"):
            s.accumulate(follow, color_b, instances=rec_b["inv"].astype(np.float64))
        with pytest.raises(ValueError, match="instances"):
            s.accumulate(follow, color_b, instances=np.zeros((3, 16), np.float32))
        with pytest.raises(ValueError, match="INSTANCE_DTYPE"):
            s.upload_instances(rec_b["inv"])
        assert follow.frames == 2 and blind.frames == 2                       # a refusal leaves the history as it was
        # ... and reset=True starts such a history over with them; return_vectors works without instances= too
        assert len(s.accumulate(blind, color_b, instances=rec_b, reset=True)) == 2 and blind.frames == 1 and blind.instances is not None
        c3, m3, v3 = s.accumulate(blind, color_b, return_vectors=True)
        assert v3.shape == (h, w, 4) and blind.instances is None and bool((v3[..., 3] == 2.0).any())
        # a new instance beyond the previous table has no history: the previous frame knew two instances only
        c4, m4, v4 = s.accumulate(follow, color_b, instances=rec_b, return_vectors=True)
        assert bool((m4[..., 2][torch.from_numpy(moved).to("cuda:0")] >= 2.0).any())
        follow.instances = follow.instances[:2]
        c5, m5, v5 = s.accumulate(follow, color_b, instances=rec_b, return_vectors=True)
        newcomer = torch.from_numpy(in_b[2] == 2).to("cuda:0")
        assert bool(newcomer.any()) and bool((m5[..., 2][newcomer] == 1.0).all()) and not bool(v5[newcomer].any())
        # the result is a valid input of the filters
        out = s.denoise(c5, iterations=2)
        assert out.shape == (h, w, 4) and bool(torch.isfinite(out).all())
        out = s.filter_variance(c5, m5, iterations=2)
        assert out.shape == (h, w, 4) and bool(torch.isfinite(out).all())
        s.upload_instances(rec_a)                                             # the whole table, from the first record
