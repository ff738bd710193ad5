"""libcrt_upsample.so without a GPU: the header, the ctypes table and the exports agree; the struct layouts match the header's comments;
crtu_low_size over every factor and offset; every refusal of include/crt_upsample.h is answered before anything is dereferenced or enqueued; the
numpy restatement (tests/upsample_ref.py) has the properties the upsample exists for -- a pixel that carries a sample copies it, an instance-valued
image comes out exactly under the instance match, a NaN heals, a tile whose taps all fail takes the nearest in depth, nothing finite gives zeros --
and stays inside the cap on exempt pixels on a frame of `tiny`; the kernels cross-compile for gfx950 without scratch, spills or AGPRs; the
library's source owns no HIP object, waits on nothing and copies nothing."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clraytracer_amd import _lib, driver, scenes

if not os.path.exists(getattr(_lib, "UPSAMPLE_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import gbuffer_ref
import oracle_lib
import upsample_ref as ref
from test_abi import HIP_OWNING_CALLS
from util import bits, kernel_resource_rows, resource_line, unit_sources

UPSAMPLE_DIR = os.path.join(ROOT, "clraytracer_amd", "upsample")
IMAGE_DIR = os.path.join(ROOT, "clraytracer_amd", "image")          # the headers the image libraries share, compiled into each
A = 0x10000                                      # dummy device addresses, 64 KiB apart: a refusal looks at none of them
NAMES = ["crtu_error_string", "crtu_low_size", "crtu_upsample"]


def test_header_table_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "crt_upsample.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(crtu_\w+)\s*\(", text)))
    assert names == NAMES
    assert sorted(_lib.UPSAMPLE_API) == names
    lib = _lib.upsample()
    for n in names:
        assert hasattr(lib, n), n
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.UPSAMPLE_SO], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(crtu_\w+)$", out, re.M))) == names
        assert not re.findall(r"\bcrt[dtvm]?_\w+$", out, re.M)      # no name of another library's
    for name, value in (("CRTU_OK", 0), ("CRTU_E_BAD_ARGUMENT", -2), ("CRTU_E_OUT_OF_RANGE", -3), ("CRTU_GUIDES_PLANES", 0), ("CRTU_GUIDES_SURFACE", 1),
                        ("CRTU_MATCH_INSTANCE", 1), ("CRTU_MODULATE", 2), ("CRTU_STATE_INTERPOLATED", 0), ("CRTU_STATE_NEAREST", 1),
                        ("CRTU_STATE_EMPTY", 2)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text) and getattr(_lib, name) == value, name
    assert (_lib.CRTU_E_BAD_ARGUMENT, _lib.CRTU_E_OUT_OF_RANGE) == (_lib.CRT_E_BAD_ARGUMENT, _lib.CRT_E_OUT_OF_RANGE)
    assert (_lib.CRTU_GUIDES_PLANES, _lib.CRTU_GUIDES_SURFACE) == (_lib.CRTD_GUIDES_PLANES, _lib.CRTD_GUIDES_SURFACE)
    assert (ref.MATCH_INSTANCE, ref.MODULATE) == (_lib.CRTU_MATCH_INSTANCE, _lib.CRTU_MODULATE)
    assert (ref.INTERPOLATED, ref.NEAREST, ref.EMPTY) == (_lib.CRTU_STATE_INTERPOLATED, _lib.CRTU_STATE_NEAREST, _lib.CRTU_STATE_EMPTY)


def test_struct_sizes_and_offsets_are_the_header_s():
    """The figures the header's comments state, crt_upsample.hip static_asserts and _lib mirrors. LP64: the int32 `guides` sits at 8 with 4 bytes
    of padding behind it."""
    header = open(os.path.join(ROOT, "include", "crt_upsample.h")).read()
    source = open(os.path.join(UPSAMPLE_DIR, "crt_upsample.hip")).read()
    offsets = {_lib.CrtuFrame: (40, dict(width=0, height=4, guides=8, geometry=16, ids=24, albedo=32)),
               _lib.CrtuLow: (24, dict(low=0, channels=8, factor=12, offsetX=16, offsetY=20)),
               _lib.CrtuParams: (12, dict(flags=0, depthTol=4, normalCos=8))}
    for struct, (size, fields) in offsets.items():
        assert C.sizeof(struct) == size, struct
        m = re.search(r"/\* %d bytes([^\n]*)\*/\ntypedef struct \{(?:(?!typedef).)*?\} %s;" % (size, struct.__name__), header, re.S)
        assert m, struct
        stated = {n: int(o) for n, o in re.findall(r"\b(\w+) (\d+)\b", m.group(1).split(":", 1)[1])}
        assert stated == fields, (struct, stated)                           # the comment names every field with its offset
        assert "sizeof(%s) == %d" % (struct.__name__, size) in source, struct
        assert [n for n, _ in struct._fields_] == list(fields), struct
        for name, off in fields.items():
            assert getattr(struct, name).offset == off, (struct, name)
            if off:
                assert "offsetof(%s, %s) == %d" % (struct.__name__, name, off) in source, (struct, name)


def low_size(w, h, f, ox, oy):
    lw, lh = C.c_int32(-7), C.c_int32(-7)
    rc = _lib.upsample().crtu_low_size(w, h, f, ox, oy, C.byref(lw), C.byref(lh))
    return rc, lw.value, lh.value


def test_low_size_over_every_factor_and_offset():
    for f in (2, 4):
        for ox in range(f):
            for oy in range(f):
                for w in range(1, 10):
                    for h in (1, 2, 3, 4, 5, 8, 9):
                        rc, lw, lh = low_size(w, h, f, ox, oy)
                        if ox >= w or oy >= h:
                            assert (rc, lw, lh) == (_lib.CRTU_E_BAD_ARGUMENT, -7, -7), (w, h, f, ox, oy)     # no sample lies in the frame
                            continue
                        # counted: the samples whose pixel lies in the frame
                        want = (len(range(ox, w, f)), len(range(oy, h, f)))
                        assert (rc, lw, lh) == (0, *want) and want == ref.low_size(w, h, f, (ox, oy)), (w, h, f, ox, oy)
                        assert f * (lw - 1) + ox <= w - 1 < f * lw + ox and f * (lh - 1) + oy <= h - 1 < f * lh + oy
    assert low_size(1920, 1080, 2, 0, 0) == (0, 960, 540) and low_size(1920, 1080, 4, 3, 3) == (0, 480, 270)
    assert low_size(16384, 16384, 2, 1, 1) == (0, 8192, 8192)
    for args, want in (((0, 5, 2, 0, 0), -2), ((5, -1, 2, 0, 0), -2), ((5, 5, 3, 0, 0), -2), ((5, 5, 1, 0, 0), -2), ((5, 5, 8, 0, 0), -2),
                       ((5, 5, 2, 2, 0), -2), ((5, 5, 2, 0, -1), -2), ((5, 5, 4, 0, 4), -2), ((16385, 5, 2, 0, 0), -3), ((5, 16385, 4, 1, 1), -3)):
        assert low_size(*args) == (want, -7, -7), args
    lib, n = _lib.upsample(), C.c_int32()
    assert lib.crtu_low_size(5, 5, 2, 0, 0, None, C.byref(n)) == -2 and lib.crtu_low_size(5, 5, 2, 0, 0, C.byref(n), None) == -2


def test_error_strings():
    lib = _lib.upsample()
    assert lib.crtu_error_string(0) == b"ok"
    assert lib.crtu_error_string(-2) == b"crtu: bad argument" and b"range" in lib.crtu_error_string(-3) and b"16384" in lib.crtu_error_string(-3)
    assert b"unknown" in lib.crtu_error_string(-77)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
OUT, STATE = 6 * A, 7 * A


def call(frame=None, low=None, params=None, out=OUT, state=STATE, null_frame=False, null_low=False, null_params=False):
    f = dict(width=70, height=37, guides=_lib.CRTU_GUIDES_PLANES, geometry=3 * A, ids=4 * A, albedo=5 * A)
    l = dict(low=1 * A, channels=4, factor=2, offsetX=0, offsetY=0)
    p = dict(flags=_lib.CRTU_MATCH_INSTANCE | _lib.CRTU_MODULATE, depthTol=0.05, normalCos=0.9)
    f.update(frame or {}); l.update(low or {}); p.update(params or {})
    fs, ls, ps = _lib.CrtuFrame(**f), _lib.CrtuLow(**l), _lib.CrtuParams(**p)
    return _lib.upsample().crtu_upsample(None if null_frame else C.byref(fs), None if null_low else C.byref(ls), None if null_params else C.byref(ps),
                                         out, state, None)


BAD, RANGE = _lib.CRTU_E_BAD_ARGUMENT, _lib.CRTU_E_OUT_OF_RANGE
SURFACE = dict(guides=_lib.CRTU_GUIDES_SURFACE, ids=None, albedo=None)
INPUTS = (("the low image", 1 * A), ("the geometry", 3 * A), ("the ids", 4 * A), ("the albedo", 5 * A))
NAN, INF = float("nan"), float("inf")
REFUSALS = {
    "null frame": (dict(null_frame=True), BAD),
    "null low struct": (dict(null_low=True), BAD),
    "null params": (dict(null_params=True), BAD),
    "null low image": (dict(low=dict(low=None)), BAD),
    "null geometry": (dict(frame=dict(geometry=None)), BAD),
    "null out": (dict(out=None), BAD),
    "no ids under MATCH_INSTANCE": (dict(frame=dict(ids=None)), BAD),
    "no albedo under MODULATE": (dict(frame=dict(albedo=None)), BAD),
    "ids under SURFACE": (dict(frame=dict(SURFACE, ids=4 * A)), BAD),
    "albedo under SURFACE": (dict(frame=dict(SURFACE, albedo=5 * A)), BAD),
    "unknown flag": (dict(params=dict(flags=4)), BAD),
    "unknown high flag": (dict(params=dict(flags=0x80000001)), BAD),
    "unknown guides": (dict(frame=dict(guides=2)), BAD),
    "negative guides": (dict(frame=dict(guides=-1)), BAD),
    "channels 0": (dict(low=dict(channels=0)), BAD),
    "channels 2": (dict(low=dict(channels=2)), BAD),
    "channels 3": (dict(low=dict(channels=3)), BAD),
    "channels 8": (dict(low=dict(channels=8)), BAD),
    "MODULATE with one channel": (dict(low=dict(channels=1), params=dict(flags=_lib.CRTU_MODULATE)), BAD),
    "factor 0": (dict(low=dict(factor=0)), BAD),
    "factor 1": (dict(low=dict(factor=1)), BAD),
    "factor 3": (dict(low=dict(factor=3)), BAD),
    "factor 8": (dict(low=dict(factor=8)), BAD),
    "negative factor": (dict(low=dict(factor=-2)), BAD),
    "offsetX = factor": (dict(low=dict(offsetX=2)), BAD),
    "offsetY = factor": (dict(low=dict(factor=4, offsetY=4)), BAD),
    "negative offsetX": (dict(low=dict(offsetX=-1)), BAD),
    "negative offsetY": (dict(low=dict(offsetY=-1)), BAD),
    "offsetX not below the width": (dict(frame=dict(width=1), low=dict(offsetX=1)), BAD),
    "offsetY not below the height": (dict(frame=dict(height=3), low=dict(factor=4, offsetY=3)), BAD),
    **{f"out is {b}": (dict(out=addr), BAD) for b, addr in INPUTS},
    **{f"outState is {b}": (dict(state=addr), BAD) for b, addr in INPUTS},
    "outState is out": (dict(state=OUT), BAD),
    "out is the records under SURFACE": (dict(frame=SURFACE, out=3 * A), BAD),
    "negative depthTol": (dict(params=dict(depthTol=-0.01)), BAD),
    "NaN depthTol": (dict(params=dict(depthTol=NAN)), BAD),
    "NaN normalCos": (dict(params=dict(normalCos=NAN)), BAD),
    "width 0": (dict(frame=dict(width=0)), BAD),
    "height 0": (dict(frame=dict(height=0)), BAD),
    "negative width": (dict(frame=dict(width=-5)), BAD),
    "width 16385": (dict(frame=dict(width=16385)), RANGE),
    "height 16385": (dict(frame=dict(height=16385)), RANGE),
    "width 2^31 - 1": (dict(frame=dict(width=2 ** 31 - 1)), RANGE),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_come_before_anything_is_enqueued(case):
    """Every pointer is a dummy address: a refusal that dereferenced one would fault, and one that enqueued would need a device."""
    kwargs, want = REFUSALS[case]
    assert call(**kwargs) == want, case


# ---- the reference itself, on hand-made planes ----------------------------------------------------------------------------------------------
H, W = 37, 70
OFFSETS = {2: [(0, 0), (1, 1), (1, 0)], 4: [(0, 0), (1, 1), (3, 0), (2, 3)]}


def planes(seed=0):
    p = ref.guides(H, W, seed=seed)
    return p["geometry"], p["ids"]["instance"].astype(np.int32), p["albedo"]


def flat(h, w, t=10.0):
    """one surface: every pixel a hit with the same normal and distance, one instance"""
    g = np.zeros((h, w, 4), np.float32)
    g[...] = (0.0, 1.0, 0.0, t)
    return g, np.zeros((h, w), np.int32), np.full((h, w), 0xFF808080, np.uint32)


@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("factor", [2, 4])
def test_a_pixel_that_carries_a_finite_sample_returns_it(factor, channels):
    """fx = fy = 0 there: b = (1, 0, 0, 0), the sample is tap 0 and the only tap that may count; it passes its own stops (d = 0, and the
    hand-made normals are within 4 % of unit length, so dot3(n, n) >= 0.9), v * 1 / 1 = v, and a NaN t is no hit on both sides. A sample of -0
    would come out as +0 (0 + -0): the image has none."""
    g, inst, albedo = planes()
    for offset in OFFSETS[factor]:
        low = ref.low_image(W, H, factor, offset, channels)
        for flags in (0, ref.MATCH_INSTANCE):
            out, state = ref.upsample(low, g, inst, albedo, factor, offset, flags)
            ys, xs = ref.sample_pixels(W, H, factor, offset)
            carried, st = out[np.ix_(ys, xs)], state[np.ix_(ys, xs)]
            finite = np.isfinite(low.reshape(low.shape[0], low.shape[1], -1)).all(axis=-1)
            assert finite.sum() > 20 and (~finite).sum() > 2
            assert np.array_equal(bits(carried)[finite], bits(low)[finite]) and (st[finite] == ref.INTERPOLATED).all()
            assert (st[~finite] != ref.INTERPOLATED).all()                  # its own sample is the only tap with b > 0


def instance_image(inst, channels):
    """a small-integer-valued function of the instance id: every product with a multiple of 1/16 and every sum of four is exact"""
    v = ((inst % 5) + 1).astype(np.float32)
    return v if channels == 1 else np.stack([v, v + 8, 16 - v, 2 * v], axis=-1).astype(np.float32)


@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("factor", [2, 4])
def test_an_instance_valued_image_comes_out_exactly_under_the_instance_match(factor, channels):
    g, inst, albedo = planes()
    hit = g[..., 3] <= 99998.0
    full = instance_image(inst, channels)
    for offset in OFFSETS[factor]:
        ys, xs = ref.sample_pixels(W, H, factor, offset)
        low = full[np.ix_(ys, xs)]
        out, state = ref.upsample(low, g, inst, albedo, factor, offset, ref.MATCH_INSTANCE)
        exact = hit & (state == ref.INTERPOLATED)
        assert exact.sum() > 0.5 * hit.sum()
        assert np.array_equal(bits(out)[exact], bits(full)[exact])
        # unguided, and without the match, taps of the other instance count on the edge between the two
        loose, _ = ref.upsample(low, g, inst, albedo, factor, offset, 0, **ref.UNGUIDED)
        differ = (bits(loose) != bits(full)).reshape(H, W, -1).any(axis=-1) & hit
        assert differ.any()
        edge = np.zeros((H, W), bool)
        for dy in range(-factor, factor + 1):
            for dx in range(-factor, factor + 1):
                shifted = np.roll(inst, (dy, dx), axis=(0, 1))
                edge |= (shifted != inst) & (shifted >= 0)
        assert not (differ & ~edge).any()                                   # and only there


def test_a_nan_sample_changes_no_pixel_to_nan():
    g, inst, albedo = flat(H, W)
    for factor in (2, 4):
        for channels in (1, 4):
            low = ref.low_image(W, H, factor, (0, 0), channels, specials=False)
            clean, state = ref.upsample(low, g, inst, albedo, factor)
            assert np.isfinite(clean).all() and (state == ref.INTERPOLATED).all()
            bad = low.copy()
            bad[3, 5] = np.nan
            bad[6, 2] = np.inf
            out, state = ref.upsample(bad, g, inst, albedo, factor)
            assert np.isfinite(out).all()                                   # multiplied by zero instead of selected away it would have spread
            changed = (bits(out) != bits(clean)).reshape(H, W, -1).any(axis=-1)
            reach = np.zeros((H, W), bool)
            for y, x in ((3, 5), (6, 2)):
                reach[max(0, factor * (y - 1) + 1):factor * (y + 1), max(0, factor * (x - 1) + 1):factor * (x + 1)] = True
            assert changed.any() and not (changed & ~reach).any()
            # the two pixels that carry the samples have no other tap with b > 0: the nearest surviving one in depth, which on a flat plane is tap 1
            assert state[factor * 3, factor * 5] == ref.NEAREST and state[factor * 6, factor * 2] == ref.NEAREST
            assert (state == ref.NEAREST).sum() == 2
            assert np.array_equal(bits(out[factor * 3, factor * 5]), bits(low[3, 6]))


def test_a_tile_whose_taps_all_fail_takes_the_smallest_depth_difference():
    """depthTol = 0 over distances that all differ: no tap passes but a pixel's own sample. Every other hit pixel is NEAREST, with the value of the
    existing tap whose distance is closest to its own -- found here by a loop over the pixels, not by the vectorised rule."""
    rng = np.random.RandomState(3)
    h, w, factor = 12, 20, 4
    g, inst, albedo = flat(h, w)
    g[..., 3] = rng.permutation(h * w).reshape(h, w).astype(np.float32) + 1.0       # all different, exact
    g[5, 7, 3] = 99999.0                                                    # one pixel of sky that carries no sample
    for offset in ((0, 0), (1, 2)):
        lw, lh = ref.low_size(w, h, factor, offset)
        low = rng.uniform(1, 2, (lh, lw)).astype(np.float32)
        low[1, 2] = np.nan                                                  # a sample that is no candidate
        out, state = ref.upsample(low, g, inst, albedo, factor, offset, depth_tol=0.0)
        for y in range(h):
            for x in range(w):
                X0, Y0 = (x - offset[0]) // factor, (y - offset[1]) // factor
                taps = [(X0 + (k & 1), Y0 + (k >> 1)) for k in range(4)]
                cands = [(X, Y) for X, Y in taps if 0 <= X < lw and 0 <= Y < lh and np.isfinite(low[Y, X])]
                carries = (x - offset[0]) % factor == 0 and (y - offset[1]) % factor == 0 and np.isfinite(low[Y0, X0])
                if carries:
                    assert state[y, x] == ref.INTERPOLATED and out[y, x] == low[Y0, X0]
                    continue
                assert state[y, x] == ref.NEAREST and cands, (y, x)
                if (y, x) == (5, 7):
                    X, Y = cands[0]                                         # no hit: the first candidate in tap order
                else:
                    X, Y = min(cands, key=lambda c: abs(float(g[factor * c[1] + offset[1], factor * c[0] + offset[0], 3]) - float(g[y, x, 3])))
                assert out[y, x] == low[Y, X], (y, x)
    # a tie goes to the first in tap order: a flat plane under a normal stop nothing passes
    g, inst, albedo = flat(h, w)
    low = rng.uniform(1, 2, (3, 5)).astype(np.float32)
    out, state = ref.upsample(low, g, inst, albedo, factor, (0, 0), normal_cos=2.0)
    assert (state == ref.NEAREST).all()
    assert out[1, 1] == low[0, 0] and out[5, 6] == low[1, 1] and out[11, 19] == low[2, 4] and out[3, 17] == low[0, 4]


def test_nothing_finite_gives_empty_and_zeros():
    g, inst, albedo = planes()
    for channels in (1, 4):
        for fill in (np.nan, np.inf):
            low = np.full_like(ref.low_image(W, H, 2, (1, 0), channels), fill)
            out, state = ref.upsample(low, g, inst, albedo, 2, (1, 0), ref.MATCH_INSTANCE | (ref.MODULATE if channels == 4 else 0))
            assert (state == ref.EMPTY).all() and (bits(out) == 0).all()
    # one finite sample among them: the pixels it is a tap of are not empty, every other one is
    low = np.full((10, 18, 4), np.nan, np.float32)
    low[4, 9] = (1, 2, 3, 4)
    out, state = ref.upsample(low, g, inst, albedo, 4, (0, 0))
    touched = np.zeros((H, W), bool); touched[12:20, 32:40] = True
    assert (state[~touched] == ref.EMPTY).all() and (out[~touched] == 0).all()
    assert (state[touched] != ref.EMPTY).all() and state[16, 36] == ref.INTERPOLATED
    assert all(np.array_equal(p, (1, 2, 3, 4)) for p in out[touched])       # interpolated of one tap or nearest: the sample itself


def test_modulate_multiplies_hit_pixels_by_the_albedo_and_nothing_else():
    g, inst, albedo = planes()
    hit = g[..., 3] <= 99998.0
    low = ref.low_image(W, H, 2, (0, 0), 4)
    plain, s0 = ref.upsample(low, g, inst, albedo, 2)
    mod, s1 = ref.upsample(low, g, inst, albedo, 2, flags=ref.MODULATE)
    assert np.array_equal(s0, s1) and np.array_equal(bits(plain[..., 3]), bits(mod[..., 3]))
    assert np.array_equal(bits(plain)[~hit], bits(mod)[~hit])
    assert np.array_equal(bits(mod[..., :3])[hit], bits(plain[..., :3][hit] * ref.den_of(albedo)[hit]))
    assert (bits(mod) != bits(plain)).any()


def test_every_flag_and_parameter_changes_some_pixel():
    g, inst, albedo = planes()
    low = ref.low_image(W, H, 2, (0, 0), 4)
    key = lambda r: np.concatenate([bits(r[0]).reshape(-1), r[1].reshape(-1)])
    seen = [key(ref.upsample(low, g, inst, albedo, 2))]
    for kw in (dict(flags=ref.MATCH_INSTANCE), dict(flags=ref.MODULATE), dict(depth_tol=0.0), dict(depth_tol=0.001), dict(normal_cos=0.9995),
               ref.UNGUIDED, dict(offset=(1, 1), low=ref.low_image(W, H, 2, (1, 1), 4))):
        kw = dict(kw)
        out = key(ref.upsample(kw.pop("low", low), g, inst, albedo, 2, **kw))
        assert not any(np.array_equal(out, s) for s in seen), kw
        seen.append(out)


def test_the_reference_makes_no_nan_on_the_gpu_tests_inputs():
    """The GPU tests compare bit for bit, which a NaN made by an operation would not survive (its sign differs between host and device). No tap
    with a value that is not finite counts, so `out` holds no NaN at all."""
    import test_gpu_upsample as gpu
    for w, h in gpu.SHAPES:
        for factor in (2, 4):
            for offset in gpu.offsets(factor):
                if offset[0] >= w or offset[1] >= h:
                    continue
                for channels in (1, 4):
                    for flags in range(4 if channels == 4 else 2):
                        out, _ = gpu.reference(w, h, factor, offset, channels, flags)
                        assert np.isfinite(out).all(), (w, h, factor, offset, channels, flags)


# ---- the cap on exempt pixels, on a frame of the oracle's ----------------------------------------------------------------------------------
def test_on_tiny_at_most_a_tenth_of_the_hit_pixels_is_not_interpolated(nthreads):
    """What the exact-colour checks leave out are the pixels whose state is not INTERPOLATED. On `tiny` at 160 x 96 under the oracle's G-buffer,
    factor 2 and the default stops, they are at most 10 % of the hit pixels."""
    w, h = 160, 96
    sc = scenes.get("tiny")
    with driver.Session(w, h, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        iv, ip, pos = s.camera()
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    p = gbuffer_ref.reference_planes(a, orc, orc.raygen(w, h, iv, ip), pos)
    geometry = np.concatenate([p["geometry"]["normal"], p["geometry"]["t"][..., None]], axis=-1).astype(np.float32)
    inst = p["ids"]["instance"].astype(np.int32)
    hit = geometry[..., 3] <= 99998.0
    assert 0.05 < hit.mean() < 0.95
    for offset in ((0, 0), (1, 1)):
        for flags in (0, ref.MATCH_INSTANCE):
            ys, xs = ref.sample_pixels(w, h, 2, offset)
            full = instance_image(inst, 1)
            out, state = ref.upsample(full[np.ix_(ys, xs)], geometry, inst, p["albedo"], 2, offset, flags, **ref.DEFAULTS)
            exempt = int((state != ref.INTERPOLATED).sum())
            print(f"tiny {w}x{h}, factor 2, offset {offset}, flags {flags}: {exempt} of {int(hit.sum())} hit pixels' worth are not interpolated "
                  f"({exempt / hit.sum():.2%})")
            assert exempt <= 0.10 * hit.sum()
            if flags:
                exact = hit & (state == ref.INTERPOLATED)
                assert np.array_equal(bits(out)[exact], bits(full)[exact])


# ---- the unit as the compiler sees it -------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_kernels_need_no_scratch_no_spill_and_no_agprs():
    rows = kernel_resource_rows(source=os.path.join(UPSAMPLE_DIR, "crt_upsample.hip"))
    for n, r in rows:
        print(resource_line(n, r))
    # per guide layout, channel count and factor: the taps through L1, or from (32/F + 2) x (8/F + 2) samples of 20 B + 4 B per channel in LDS
    tf = ("false", "true")
    want = {f"crtu_upsample_kernel<{s}, {c}, {f}, {st}>": ((32 // f + 2) * (8 // f + 2) * (20 + 4 * c) if st == "true" else 0)
            for s in tf for c in (1, 4) for f in (2, 4) for st in tf}
    assert sorted(n for n, _ in rows) == sorted(want)
    for n, r in rows:
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r.get("SGPRs Spill", 0) == 0 and r["AGPRs"] == 0, resource_line(n, r)
        assert r["LDS Size"] == want[n], resource_line(n, r)                     # nothing but the staged samples
        assert r["Occupancy"] >= 8, resource_line(n, r)                          # by registers every form fits eight waves per SIMD


def test_the_library_owns_no_hip_object_and_follows_the_recipe():
    sources = sorted(f for f in os.listdir(UPSAMPLE_DIR) if f.endswith((".h", ".hip", ".cpp", ".hpp")))
    assert sources == ["crt_upsample.hip"]
    # the unit and every in-tree header it includes, transitively: the shared steps of clraytracer_amd/image/ are this library's source too
    scanned = unit_sources("clraytracer_amd/upsample/crt_upsample.hip")
    assert set(scanned) == {os.path.join(UPSAMPLE_DIR, "crt_upsample.hip"), os.path.join(ROOT, "include", "crt_upsample.h"),
                            os.path.join(IMAGE_DIR, "crt_image_device.h"), os.path.join(IMAGE_DIR, "crt_image_host.h"), os.path.join(IMAGE_DIR, "crt_image_env.h")}
    launches = 0
    for path in scanned:
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        assert not re.findall(HIP_OWNING_CALLS, text), path
        assert not re.findall(r"\bhip(DeviceSynchronize|StreamSynchronize|EventSynchronize|Memcpy\w*|Memset\w*|Malloc\w*|Free\w*)\s*\(", text), path
        launches += len(re.findall(r"<<<", text))
    assert launches == 2                                                    # the two tap forms of the one launch a call makes
    if shutil.which("make"):
        p = subprocess.run(["make", "-n", "-W", "clraytracer_amd/upsample/crt_upsample.hip", _lib.UPSAMPLE_SO.replace(ROOT + os.sep, "")], cwd=ROOT,
                           stdout=subprocess.PIPE, text=True, check=True)
        makefile = open(os.path.join(ROOT, "Makefile")).read()
        flags = re.search(r"^HIPFLAGS = (.*)$", makefile, re.M).group(1).replace("$(ARCH)", "gfx950").split()
        lines = [l.split() for l in p.stdout.splitlines() if "-shared" in l.split()]
        assert len(lines) == 1 and lines[0][1:] == flags + ["-shared", "-o", "clraytracer_amd/upsample/libcrt_upsample.so", "clraytracer_amd/upsample/crt_upsample.hip"]
        assert re.search(r"^all:.*\$\(UPSAMPLE_SO\)", makefile, re.M) and re.search(r"rm -f .*\$\(UPSAMPLE_SO\)", makefile)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.upsample()" in entry
