"""libcrt_meter.so without a GPU: the header, the ctypes table and the exports agree; the struct layouts match the header's comments and the
unit's static_asserts; every refusal of include/crt_meter.h is answered with dummy addresses before anything is dereferenced or enqueued;
crtx_scratch_bytes is 0 for refused arguments and monotone otherwise; crtx_rate is numpy's; the numpy restatement (tests/meter_ref.py) agrees
with plain arithmetic -- a constant image meters to itself, the log code never exceeds log2 and falls short by at most 0.0861, the result does
not depend on the pixels' order, the binned mean lies within a bin of the exact one, an adaptation converges monotonically; every kernel
cross-compiles for gfx950 without scratch, spills or AGPRs; the unit owns no HIP object, waits on nothing, copies nothing, and its only atomics
are adds to LDS."""
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
from clraytracer_amd import _lib

if not os.path.exists(getattr(_lib, "METER_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import meter_ref as ref
from test_abi import HIP_OWNING_CALLS
from util import bits, kernel_resource_rows, resource_line, unit_sources

METER_DIR = os.path.join(ROOT, "clraytracer_amd", "meter")
IMAGE_DIR = os.path.join(ROOT, "clraytracer_amd", "image")
A = 0x10000                                      # dummy device addresses, 64 KiB apart: a refusal looks at none of them
NAMES = ["crtx_error_string", "crtx_expose", "crtx_meter", "crtx_rate", "crtx_scratch_bytes"]
BAD, RANGE = -2, -3
INF, NAN = float("inf"), float("nan")
F = np.float32


def test_header_table_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "crt_meter.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(crtx_\w+)\s*\(", text)))
    assert names == NAMES
    assert sorted(_lib.METER_API) == names
    lib = _lib.meter()
    for n in names:
        assert hasattr(lib, n), n
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.METER_SO], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(crtx_\w+)$", out, re.M))) == names
        assert not re.findall(r"\bcrt[dtvmusp]?_\w+$", out, re.M)    # no name of another library's
    for name, value in (("CRTX_OK", 0), ("CRTX_E_BAD_ARGUMENT", -2), ("CRTX_E_OUT_OF_RANGE", -3), ("CRTX_HEAL", 1), ("CRTX_ADAPT", 2),
                        ("CRTX_HIST_BINS", 256), ("CRTX_MAX_GROUPS", 2048), ("CRTX_DEFAULT_GROUPS", 128), ("CRTX_RECORD_WORDS", 264)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text) and getattr(_lib, name) == value, name
    assert re.search(r"\bCRTX_QMIN = 107 << 16\b", text) and re.search(r"\bCRTX_QMAX = 139 << 16\b", text)
    assert (_lib.CRTX_QMIN, _lib.CRTX_QMAX) == (107 << 16, 139 << 16) == (ref.QMIN, ref.QMAX)
    assert (_lib.CRTX_E_BAD_ARGUMENT, _lib.CRTX_E_OUT_OF_RANGE) == (_lib.CRT_E_BAD_ARGUMENT, _lib.CRT_E_OUT_OF_RANGE) == (BAD, RANGE)
    assert (ref.HEAL, ref.ADAPT, ref.BINS) == (_lib.CRTX_HEAL, _lib.CRTX_ADAPT, _lib.CRTX_HIST_BINS)
    assert (ref.MAX_GROUPS, ref.DEFAULT_GROUPS, ref.RECORD_WORDS) == (_lib.CRTX_MAX_GROUPS, _lib.CRTX_DEFAULT_GROUPS, _lib.CRTX_RECORD_WORDS)
    # the ends of the code are the floats the header names, and the bins cover them
    assert int(bits(F(2.0 ** -20))[0]) >> 7 == ref.QMIN and int(bits(F(2.0 ** 12))[0]) >> 7 == ref.QMAX and (ref.QMAX - 1 - ref.QMIN) >> 13 == ref.BINS - 1


def test_struct_sizes_and_offsets_are_the_header_s():
    """The figures the header's comments state, crt_meter.hip static_asserts and _lib mirrors (LP64)."""
    header = open(os.path.join(ROOT, "include", "crt_meter.h")).read()
    source = open(os.path.join(METER_DIR, "crt_meter.hip")).read()
    offsets = {_lib.CrtxResult: (32, dict(exposure=0, target=4, average=8, meanQ=12, valid=16, invalid=20, minQ=24, maxQ=28)),
               _lib.CrtxMeter: (88, dict(width=0, height=4, color=8, ao=16, aoStrength=24, flags=28, x0=32, y0=36, x1=40, y1=44, key=48, lowFraction=52,
                                         highFraction=56, minExposure=60, maxExposure=64, rateUp=68, rateDown=72, groups=76, prev=80)),
               _lib.CrtxExpose: (40, dict(width=0, height=4, color=8, ao=16, exposure=24, aoStrength=32, flags=36))}
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


SIZES = ((1, 1), (3, 2), (33, 9), (200, 120), (1920, 1080), (3840, 2160), (16384, 16384))


def test_scratch_bytes_is_zero_for_refused_arguments_and_monotone():
    lib = _lib.meter()
    for groups in (0, 1, 3, 128, _lib.CRTX_MAX_GROUPS):
        sizes = [lib.crtx_scratch_bytes(w, h, groups) for w, h in SIZES]
        assert sizes == sorted(sizes) and sizes[0] > 0, (groups, sizes)
        assert sizes == [ref.scratch_bytes(w, h, groups) for w, h in SIZES]
        assert [lib.crtx_scratch_bytes(w, h, groups) for w, h in ((0, 5), (5, 0), (-1, 5), (16385, 5), (5, 16385), (-2 ** 31, 1))] == [0] * 6
    for w, h in SIZES:
        given = [lib.crtx_scratch_bytes(w, h, g) for g in range(1, _lib.CRTX_MAX_GROUPS + 1)]
        assert given == [g * _lib.CRTX_RECORD_WORDS * 4 for g in range(1, _lib.CRTX_MAX_GROUPS + 1)]      # one record per workgroup: monotone in groups
        assert lib.crtx_scratch_bytes(w, h, 0) <= _lib.CRTX_DEFAULT_GROUPS * _lib.CRTX_RECORD_WORDS * 4
        assert [lib.crtx_scratch_bytes(w, h, g) for g in (-1, _lib.CRTX_MAX_GROUPS + 1, -2 ** 31, 2 ** 31 - 1)] == [0] * 4
    assert lib.crtx_scratch_bytes(1, 1, 0) == _lib.CRTX_RECORD_WORDS * 4 and lib.crtx_scratch_bytes(200, 120, 0) == 105 * _lib.CRTX_RECORD_WORDS * 4


def test_error_strings():
    lib = _lib.meter()
    assert lib.crtx_error_string(0) == b"ok"
    assert lib.crtx_error_string(-2) == b"crtx: bad argument" and b"range" in lib.crtx_error_string(-3) and b"16384" in lib.crtx_error_string(-3)
    assert b"unknown" in lib.crtx_error_string(-77)


def test_rate_is_numpy_s():
    lib = _lib.meter()
    for dt in (0.0, 1e-4, 1.0 / 240, 1.0 / 60, 0.033, 0.5, 3.0, 100.0):
        for tau in (1e-3, 0.05, 0.2, 0.5, 1.0, 4.0, 1e6):
            got = F(lib.crtx_rate(dt, tau))
            assert bits(got) == bits(F(1.0 - np.exp(-np.float64(dt) / np.float64(tau)))) == bits(ref.rate(dt, tau)), (dt, tau)
            assert 0.0 <= got <= 1.0
        for tau in (0.0, -0.0, -1.0, -INF):
            assert lib.crtx_rate(dt, tau) == 1.0 == ref.rate(dt, tau)
    assert lib.crtx_rate(0.0, 0.5) == 0.0 and lib.crtx_rate(1.0, INF) == 0.0


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
COLOR, AO, RESULT, HIST, SCRATCH, PREV, OUT = (i * A for i in range(1, 8))


def meter(m=None, result=RESULT, hist=HIST, scratch=SCRATCH, null=False):
    f = dict(width=70, height=37, color=COLOR, ao=AO, aoStrength=0.5, flags=3, x0=3, y0=2, x1=66, y1=30, key=0.18, lowFraction=0.1, highFraction=0.9,
             minExposure=0.01, maxExposure=100.0, rateUp=0.5, rateDown=0.25, groups=0, prev=PREV)
    f.update(m or {})
    s = _lib.CrtxMeter(**f)
    return _lib.meter().crtx_meter(None if null else C.byref(s), result, hist, scratch, None)


def expose(e=None, out=OUT, null=False):
    f = dict(width=70, height=37, color=COLOR, ao=AO, exposure=RESULT, aoStrength=0.5, flags=1)
    f.update(e or {})
    s = _lib.CrtxExpose(**f)
    return _lib.meter().crtx_expose(None if null else C.byref(s), out, None)


NUMBERS = ("aoStrength", "key", "lowFraction", "highFraction", "minExposure", "maxExposure", "rateUp", "rateDown")
REFUSALS = {
    # crtx_meter
    "meter: null struct": (meter, dict(null=True), BAD),
    "meter: null color": (meter, dict(m=dict(color=None)), BAD),
    "meter: null result": (meter, dict(result=None), BAD),
    "meter: null scratch": (meter, dict(scratch=None), BAD),
    **{f"meter: result is {n}": (meter, dict(result=a), BAD) for n, a in (("color", COLOR), ("ao", AO))},
    **{f"meter: outHist is {n}": (meter, dict(hist=a), BAD) for n, a in (("color", COLOR), ("ao", AO), ("result", RESULT), ("prev", PREV))},
    **{f"meter: scratch is {n}": (meter, dict(scratch=a), BAD) for n, a in (("color", COLOR), ("ao", AO), ("result", RESULT), ("outHist", HIST), ("prev", PREV))},
    "meter: scratch is prev and result": (meter, dict(m=dict(prev=RESULT), scratch=RESULT), BAD),
    "meter: outHist is prev without ADAPT": (meter, dict(m=dict(flags=0), hist=PREV), BAD),
    **{f"meter: flags {f}": (meter, dict(m=dict(flags=f)), BAD) for f in (4, 8, 7, 0x80000000, 0xFFFFFFFF)},
    **{f"meter: {n} {v}": (meter, dict(m={n: v}), BAD) for n in NUMBERS for v in (NAN, INF, -INF)},
    **{f"meter: aoStrength {v}": (meter, dict(m=dict(aoStrength=v)), BAD) for v in (-0.001, 1.001, 2.0)},
    "meter: aoStrength out of range without ao": (meter, dict(m=dict(ao=None, aoStrength=1.5)), BAD),
    **{f"meter: key {v}": (meter, dict(m=dict(key=v)), BAD) for v in (0.0, -0.0, -0.18)},
    **{f"meter: fractions {lo}, {hi}": (meter, dict(m=dict(lowFraction=lo, highFraction=hi)), BAD)
       for lo, hi in ((-0.01, 0.5), (0.5, 1.01), (0.6, 0.5), (1.0, 0.999), (-1.0, -0.5), (1.5, 2.0))},
    **{f"meter: exposures {lo}, {hi}": (meter, dict(m=dict(minExposure=lo, maxExposure=hi)), BAD)
       for lo, hi in ((0.0, 1.0), (-0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (-2.0, -1.0))},
    **{f"meter: {n} {v}": (meter, dict(m={n: v}), BAD) for n in ("rateUp", "rateDown") for v in (-0.001, 1.001, 7.0)},
    **{f"meter: rectangle {r}": (meter, dict(m=dict(zip(("x0", "y0", "x1", "y1"), r))), BAD)
       for r in ((5, 2, 5, 30), (3, 9, 66, 9), (6, 2, 5, 30), (3, 10, 66, 9), (-1, 2, 66, 30), (3, -1, 66, 30), (3, 2, 71, 30), (3, 2, 66, 38),
                 (70, 0, 71, 1), (0, 37, 1, 38), (-5, -5, 0, 0), (0, 0, 0, 0), (-2 ** 31, 0, 70, 37), (0, 0, 2 ** 31 - 1, 37))},
    **{f"meter: groups {g}": (meter, dict(m=dict(groups=g)), BAD) for g in (-1, _lib.CRTX_MAX_GROUPS + 1, -2 ** 31, 2 ** 31 - 1)},
    "meter: width 0": (meter, dict(m=dict(width=0)), BAD),
    "meter: height 0": (meter, dict(m=dict(height=0)), BAD),
    "meter: negative width": (meter, dict(m=dict(width=-5)), BAD),
    "meter: negative height": (meter, dict(m=dict(height=-2 ** 31)), BAD),
    "meter: width 16385": (meter, dict(m=dict(width=16385)), RANGE),
    "meter: height 16385": (meter, dict(m=dict(height=16385)), RANGE),
    "meter: width 2^31 - 1": (meter, dict(m=dict(width=2 ** 31 - 1)), RANGE),
    # crtx_expose
    "expose: null struct": (expose, dict(null=True), BAD),
    "expose: null color": (expose, dict(e=dict(color=None)), BAD),
    "expose: null record": (expose, dict(e=dict(exposure=None)), BAD),
    "expose: null out": (expose, dict(out=None), BAD),
    "expose: out is ao": (expose, dict(out=AO), BAD),
    "expose: out is the record": (expose, dict(out=RESULT), BAD),
    "expose: in place, out is the record too": (expose, dict(e=dict(color=RESULT), out=RESULT), BAD),
    **{f"expose: flags {f}": (expose, dict(e=dict(flags=f)), BAD) for f in (2, 3, 4, 0x80000000, 0xFFFFFFFF)},
    **{f"expose: aoStrength {v}": (expose, dict(e=dict(aoStrength=v)), BAD) for v in (NAN, INF, -INF, -0.001, 1.001)},
    "expose: width 0": (expose, dict(e=dict(width=0)), BAD),
    "expose: negative height": (expose, dict(e=dict(height=-3)), BAD),
    "expose: width 16385": (expose, dict(e=dict(width=16385)), RANGE),
    "expose: height 16385": (expose, dict(e=dict(height=16385)), RANGE),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_come_before_anything_is_enqueued(case):
    """Every pointer is a dummy address: a refusal that dereferenced one would fault, and one that enqueued would need a device."""
    fn, kwargs, want = REFUSALS[case]
    assert fn(**kwargs) == want, case


# ---- the reference against plain arithmetic -------------------------------------------------------------------------------------------------
def grey(l, h=9, w=33):
    """a grey image: its luminance is exactly l for a power of two l (the three weights add up to 1 in float32; the first test checks it)"""
    img = np.zeros((h, w, 4), np.float32)
    img[..., :3] = F(l)
    img[..., 3] = 1
    return img


def test_a_constant_image_meters_to_itself():
    # the luminance of a grey of value v is ((v*0.2126f + v*0.7152f) + v*0.0722f): for v a power of two that is v times the same sum for 1
    one = ref.luminance(np.ones((1, 1, 3), np.float32))[0, 0]
    assert one == 1                                                                          # (0.2126f + 0.7152f) + 0.0722f rounds to 1
    for e in (-24, -20, -19, -7, -1, 0, 1, 5, 11, 12, 14):
        img = grey(2.0 ** e)
        l = ref.luminance(img)
        assert (l == F(2.0 ** e) * one).all()
        rec, hist = ref.meter(img, key=0.18, min_exposure=2.0 ** -30, max_exposure=2.0 ** 30)
        want_q = int(ref.log_code(np.array([l[0, 0]], np.float32))[1][0])
        assert rec[3] == want_q == rec[6] == rec[7] and rec[4] == img.shape[0] * img.shape[1] and rec[5] == 0
        assert hist.sum() == rec[4] and hist[(want_q - ref.QMIN) >> 13] == rec[4]
        if -20 <= e < 12:
            assert rec[2:3].view(np.float32)[0] == F(2.0 ** e) and rec[:1].view(np.float32)[0] == F(0.18) / F(2.0 ** e)
    # with a single channel the luminance is a power of two times one weight; what counts is the statement on exact inputs: feed the code itself
    for e in range(-20, 12):
        st = dict(valid=7, invalid=0, sumQ=7 * ((e + 127) << 16), minQ=(e + 127) << 16, maxQ=(e + 127) << 16, hist=np.bincount([(e + 20) * 8] * 7, minlength=256))
        for fractions in ((0.0, 1.0),):
            rec = ref.resolve(st, key=0.18, low=fractions[0], high=fractions[1], min_exposure=2.0 ** -30, max_exposure=2.0 ** 30)
            assert rec[2:3].view(np.float32)[0] == F(2.0 ** e) and bits(rec[:1].view(np.float32)[0]) == bits(F(0.18) / F(2.0 ** e))
            assert bits(rec[1:2].view(np.float32)[0]) == bits(rec[:1].view(np.float32)[0])


def test_the_log_code_never_exceeds_log2_and_falls_short_by_at_most_0_0861():
    rng = np.random.RandomState(5)
    l = np.exp2(rng.uniform(-20, 12, 1_000_000)).astype(np.float32)
    l = l[(l >= F(2.0 ** -20)) & (l < F(2.0 ** 12))]
    valid, q = ref.log_code(l)
    assert valid.all() and (q >= ref.QMIN).all() and (q < ref.QMAX).all()
    back = ref.decode(q)
    assert (back <= l).all() and (ref.log_code(back)[1] == q).all()                        # the inverse is exact on codes
    assert (l.astype(np.float64) - back.astype(np.float64) < np.ldexp(1.0, np.frexp(l)[1] - 1 - 16)).all()      # seven mantissa bits lost
    short = np.log2(l.astype(np.float64)) - (q.astype(np.float64) / 65536 - 127)
    assert short.min() >= -2.0 ** -16 and 0.085 < short.max() <= 0.0861                    # (the code truncates: 2^-16 of slack below)
    # the clamps and the invalid values
    edge = np.array([0.0, -0.0, 1e-30, 2.0 ** -21, 2.0 ** -20, 2.0 ** 12, 3e38, np.inf, -np.inf, np.nan, -1e-30, -1.0], np.float32)
    valid, q = ref.log_code(edge)
    assert valid.tolist() == [True] * 7 + [False] * 5
    assert q[:7].tolist() == [ref.QMIN] * 5 + [ref.QMAX - 1] * 2
    assert ((q[:7] - ref.QMIN) >> 13).tolist() == [0] * 5 + [255] * 2


def noisy(h, w, seed):
    rng = np.random.RandomState(seed)
    img = np.exp2(rng.uniform(-24, 14, (h, w, 4))).astype(np.float32)
    bad = rng.uniform(size=(h, w)) < 0.05
    img[bad, 1] = rng.choice(np.array([np.nan, np.inf, -np.inf, -1e9, -0.0], np.float32), int(bad.sum()))
    return img


def test_the_result_does_not_depend_on_the_pixels_order():
    img = noisy(24, 40, 3)
    ao = np.random.RandomState(4).uniform(size=(24, 40)).astype(np.float32)
    for fractions in ((0.0, 1.0), (0.5, 0.9), (0.3, 0.3)):
        for flags in (0, ref.HEAL):
            base = ref.meter(img, None, flags, ao, 0.35, low=fractions[0], high=fractions[1])
            assert base[0][5] > 0 or flags
            for seed in range(3):
                order = np.random.RandomState(seed).permutation(24 * 40)
                got = ref.meter(img.reshape(-1, 4)[order].reshape(24, 40, 4), None, flags, ao.reshape(-1)[order].reshape(24, 40), 0.35,
                                low=fractions[0], high=fractions[1])
                assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
    # the rectangle is the same as a crop
    rect = (3, 5, 37, 20)
    a = ref.meter(img, rect, ref.HEAL, ao, 0.35, low=0.5, high=0.9)
    b = ref.meter(img[5:20, 3:37], None, ref.HEAL, ao[5:20, 3:37], 0.35, low=0.5, high=0.9)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_binned_mean_lies_within_a_bin_of_the_exact_mean():
    for seed in range(4):
        st = ref.statistics(noisy(31, 57, seed), flags=ref.HEAL)
        exact = st["sumQ"] // st["valid"]
        binned = ref.binned_mean(st["hist"], 0, st["valid"])
        assert abs(exact - binned) <= 1 << 12, (exact, binned)                              # a centre is at most half a bin from its pixels
        assert ref.ranks(st["valid"], 0.0, 1.0) == (0, st["valid"])
    # ranks: the fractions of the GPU cases, an empty window widened to one pixel, the ends
    assert ref.ranks(1000, 0.5, 0.9) == (500, 900) and ref.ranks(10, 0.3, 0.3)[1] - ref.ranks(10, 0.3, 0.3)[0] == 1
    assert ref.ranks(1, 0.3, 0.3) == (0, 1) and ref.ranks(7, 1.0, 1.0) == (6, 7) and ref.ranks(7, 0.0, 0.0) == (0, 1)
    # a trimmed mean takes the bins it names: two bins of 100 pixels, the upper half only
    hist = np.zeros(256, np.uint32); hist[10] = 100; hist[200] = 100
    assert ref.binned_mean(hist, 100, 200) == ref.QMIN + (200 << 13) + 4096 and ref.binned_mean(hist, 0, 100) == ref.QMIN + (10 << 13) + 4096
    assert ref.binned_mean(hist, 50, 150) == ref.QMIN + (105 << 13) + 4096


def test_an_adaptation_converges_monotonically_to_the_target():
    st = ref.statistics(grey(2.0 ** -3))
    for start, up, down in ((2.0 ** -6, 0.25, 0.5), (2.0 ** 7, 0.5, 0.125), (1.0, 1.0, 1.0)):
        p, seq = F(start), []
        for _ in range(200):
            rec = ref.resolve(st, prev=p, rate_up=up, rate_down=down).view(np.float32)
            target = rec[1]
            p = rec[0]
            seq.append(p)
        seq = np.array(seq, np.float32)
        step = np.diff(seq)
        assert (step >= 0).all() if start < target else (step <= 0).all()
        assert ((seq <= target).all() if start < target else (seq >= target).all())
        assert abs(float(seq[-1]) - float(target)) <= 4 * np.spacing(target), (start, seq[-1], target)     # a rate below 1 stalls a few ulps short
    # a poisoned, zero or negative record before gives the target; with no valid pixel the record before stays
    for p in (np.nan, np.inf, 0.0, -1.0):
        rec = ref.resolve(st, prev=F(p), rate_up=0.1, rate_down=0.1)
        assert rec[0] == rec[1]
    none = dict(valid=0, invalid=5, sumQ=0, minQ=0, maxQ=0, hist=np.zeros(256, np.uint32))
    assert ref.resolve(none, prev=F(3.5)).view(np.float32)[:3].tolist() == [3.5, 3.5, 0.0]
    assert ref.resolve(none, prev=F(np.nan)).view(np.float32)[:3].tolist() == [1.0, 1.0, 0.0] == ref.resolve(none).view(np.float32)[:3].tolist()


# ---- the unit as the compiler sees it -------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_kernels_need_no_scratch_no_spill_and_no_agprs():
    rows = kernel_resource_rows(source=os.path.join(METER_DIR, "crt_meter.hip"))
    for n, r in rows:
        print(resource_line(n, r))
    want = {**{f"crtx_histogram_kernel<{h}, {l}>": None for h in ("false", "true") for l in ("false", "true")},
            "crtx_resolve_kernel": None, "crtx_expose_kernel<false>": 0, "crtx_expose_kernel<true>": 0}
    assert sorted(n for n, _ in rows) == sorted(want)
    for n, r in rows:
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r.get("SGPRs Spill", 0) == 0 and r["AGPRs"] == 0, resource_line(n, r)
        assert r["Occupancy"] == 8, resource_line(n, r)
        if n.startswith("crtx_histogram_kernel"):
            assert 4 * 256 * 4 <= r["LDS Size"] <= 4 * 256 * 4 + 4 * 32, resource_line(n, r)        # four private histograms and the waves' sums
        elif want[n] is not None:
            assert r["LDS Size"] == want[n], resource_line(n, r)


def test_the_library_owns_no_hip_object_and_its_atomics_are_lds_adds():
    sources = sorted(f for f in os.listdir(METER_DIR) if f.endswith((".h", ".hip", ".cpp", ".hpp")))
    assert sources == ["crt_meter.hip"]
    scanned = unit_sources("clraytracer_amd/meter/crt_meter.hip")
    assert set(scanned) == {os.path.join(METER_DIR, "crt_meter.hip"), os.path.join(ROOT, "include", "crt_meter.h"),
                            os.path.join(IMAGE_DIR, "crt_image_device.h"), os.path.join(IMAGE_DIR, "crt_image_host.h"), os.path.join(IMAGE_DIR, "crt_image_env.h")}
    launches, adds = 0, 0
    for path in scanned:
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        assert not re.findall(HIP_OWNING_CALLS, text), path
        assert not re.findall(r"\bhip(DeviceSynchronize|StreamSynchronize|EventSynchronize|Memcpy\w*|Memset\w*|Malloc\w*|Free\w*)\s*\(", text), path
        assert not re.findall(r"__hip_atomic\w*|__atomic\w*|\bwhile\s*\(|\bvolatile\b|__threadfence\w*|\basm\b", text), path
        # every atomic is an add to `hist`, the wave's own row of the __shared__ histogram
        atomics = re.findall(r"\batomic\w*\s*\(\s*([^,]*),", text)
        assert all(a == "&hist[its]" or a == "&hist[bin]" for a in atomics), (path, atomics)
        assert len(re.findall(r"\batomic\w*", text)) == len(atomics)
        adds += len(atomics)
        launches += len(re.findall(r"<<<", text))
        if path.endswith("crt_meter.hip"):
            assert re.search(r"__shared__ uint32_t s_hist\[CRTX_WAVES\]\[CRTX_HIST_BINS\];", text) and re.search(r"uint32_t\* const hist = s_hist\[wave\];", text)
    assert adds == 3 and launches == 5          # plain: one add; leader: the leader's and the others'. histogram x 2, resolve, expose x 2
    if shutil.which("make"):
        p = subprocess.run(["make", "-n", "-W", "clraytracer_amd/meter/crt_meter.hip", _lib.METER_SO.replace(ROOT + os.sep, "")], cwd=ROOT,
                           stdout=subprocess.PIPE, text=True, check=True)
        makefile = open(os.path.join(ROOT, "Makefile")).read()
        flags = re.search(r"^HIPFLAGS = (.*)$", makefile, re.M).group(1).replace("$(ARCH)", "gfx950").split()
        lines = [l.split() for l in p.stdout.splitlines() if "-shared" in l.split()]
        assert len(lines) == 1 and lines[0][1:] == flags + ["-shared", "-o", "clraytracer_amd/meter/libcrt_meter.so", "clraytracer_amd/meter/crt_meter.hip"]
        assert re.search(r"^all:.*\$\(METER_SO\)", makefile, re.M) and re.search(r"rm -f .*\$\(METER_SO\)", makefile)
        # a change of the shared steps rebuilds the library
        p = subprocess.run(["make", "-n", "-W", "clraytracer_amd/image/crt_image_device.h", _lib.METER_SO.replace(ROOT + os.sep, "")], cwd=ROOT,
                           stdout=subprocess.PIPE, text=True, check=True)
        assert "-shared" in p.stdout
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.meter()" in entry
