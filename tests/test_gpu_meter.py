"""crtx_meter, crtx_expose and Session.meter / Session.expose on the GPU against the numpy restatement of the definition (tests/meter_ref.py):
every word of the record and of the histogram, bit for bit -- the metering is integers, so there is no tolerance. Outputs start as poison
whose payload differs from word to word and have guard words behind them, as the scratch has, so a word that was not written and a write
past the end both show; the inputs are checked to be untouched. Sizes at, below and across a tile, 105 tiles, and the size bound both ways;
groups 1, 3 (several tiles per workgroup, a partial stride), the library's choice and, where it exceeds the tiles, CRTX_MAX_GROUPS; both
CRTX_BINS forms (read by every call, so one process shows both); luminances over both clamps, one bin, two bins in alternation, invalid
pixels with and without CRTX_HEAL, no valid pixel, AO planes with non-finite values; four rectangles; four pairs of fractions; adaptation in
place. crtx_expose against the reference, in place, on a side stream, and its consequence: present(expose(color, R), exposure 1) is
present(color, exposure e) in every float and byte. A Session on `tiny` runs render -> meter -> expose -> present, and again behind a held
stream."""
import contextlib
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clraytracer_amd import _lib, driver, scenes

if not os.path.exists(getattr(_lib, "METER_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import meter_ref as ref
import present_ref
import test_gpu_upsample as gu
from stream_hold import Hold
from util import bits

pytestmark = pytest.mark.gpu
GUARD = 64                              # words behind every output and behind the scratch
SIZES = [(1, 1), (3, 2), (31, 7), (32, 8), (33, 9), (64, 16), (200, 120), (16384, 1), (1, 16384)]
FORMS = ("plain", "leader")
FRACTIONS = [(0.0, 1.0), (0.5, 0.9), (0.8, 0.983), (0.3, 0.3)]
F = np.float32
RESULT, HIST, SCRATCH = 0x100, 0x200, 0x300         # the salts of the three poisons


def word(v):
    """the uint32 word of the float32 v, as a Python int"""
    return int(np.array(v, np.float32).view(np.uint32))


def signed(w):
    """the uint32 word w as an element of an int32 tensor takes it"""
    return int(np.array(w, np.uint32).view(np.int32))


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def side_stream():
    """A HIP stream of one test's own, as a torch stream, destroyed when the test is over. torch.cuda.Stream() would take one from torch's pool,
    which lives as long as the process and keeps its place on one of the few hardware queues (tests/stream_hold.py): the tests that run later in
    the process and time streams against each other should find the queues as they were. Made through the HIP runtime the process has loaded,
    as stream_hold.Ballast makes its streams."""
    import torch
    torch.cuda.synchronize()
    with open("/proc/self/maps") as maps:
        paths = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
    runtime = C.CDLL(paths[0])
    handle = C.c_void_p()
    assert runtime.hipStreamCreateWithFlags(C.byref(handle), 1) == 0        # hipStreamNonBlocking, as torch's own side streams are
    side = torch.cuda.ExternalStream(handle.value, device="cuda:0")
    try:
        yield side
    finally:
        torch.cuda.synchronize()
        runtime.hipStreamDestroy(handle)


def guarded(words, salt):
    """`words` words of poison and GUARD more behind them"""
    return gu.poison((words + GUARD,), salt, "int32")


def written(t, words, salt, want=None, what=""):
    """the guard behind the first `words` words of t is the poison it was; with `want`, those words are `want`, bit for bit; returns them"""
    got = t.cpu().numpy().view(np.uint32)
    tail = np.arange(words, words + GUARD, dtype=np.int64) + (0x7FC00000 + salt)
    assert np.array_equal(got[words:], tail.astype(np.uint32)), f"{what}: the guard words were written"
    if want is not None:
        want = np.ascontiguousarray(want).view(np.uint32).reshape(-1)
        assert want.size == words
        differ = got[:words] != want
        assert not differ.any(), (f"{what}: {int(differ.sum())} of {words} words differ, the first at {int(np.flatnonzero(differ)[0])}: "
                                  f"got {got[:words][differ][:4]}, want {want[differ][:4]}")
    return got[:words]


def run_meter(color, w, h, *, ao=None, strength=1.0, flags=0, rect=None, groups=0, fractions=(0.0, 1.0), key=0.18, lo=2.0 ** -8, hi=2.0 ** 8,
              prev=None, up=1.0, down=1.0, result=None, hist=True, scratch=None):
    """crtx_meter itself on device tensors: (result, hist or None, scratch, scratch words), all guarded; prev: a tensor, or "result" for in place"""
    lib = _lib.meter()
    result = guarded(8, RESULT) if result is None else result
    out_hist = guarded(ref.BINS, HIST) if hist else None
    words = lib.crtx_scratch_bytes(w, h, groups) // 4
    assert words == ref.scratch_bytes(w, h, groups) // 4 > 0
    scratch = guarded(words, SCRATCH) if scratch is None else scratch
    x0, y0, x1, y1 = (0, 0, w, h) if rect is None else rect
    prev_ptr = None if prev is None else result.data_ptr() if isinstance(prev, str) else prev.data_ptr()
    m = _lib.CrtxMeter(w, h, color.data_ptr(), ao.data_ptr() if ao is not None else None, strength, flags, x0, y0, x1, y1, key, fractions[0], fractions[1],
                       lo, hi, up, down, groups, prev_ptr)
    rc = lib.crtx_meter(C.byref(m), result.data_ptr(), out_hist.data_ptr() if hist else None, scratch.data_ptr(), stream())
    assert rc == 0, lib.crtx_error_string(rc)
    return result, out_hist, scratch, words


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------------
def log_uniform(w, h, seed):
    """luminances log-uniform over 2^-24 .. 2^14 (a grey per pixel, each channel a little off it): both clamps are hit"""
    rng = np.random.RandomState(seed)
    img = (np.exp2(rng.uniform(-24, 14, (h, w, 1))) * rng.uniform(0.9, 1.1, (h, w, 4))).astype(np.float32)
    flat = img.reshape(-1, 4)
    if len(flat) >= 4:                                                      # the ends themselves, whatever the draw
        flat[0, :3], flat[1, :3], flat[2, :3], flat[3, :3] = 2.0 ** -20, 2.0 ** 12, 2.0 ** -21, 2.0 ** 13
    return img


def sprinkled(w, h, seed):
    """log_uniform with NaN, infinite, negative and -0.0f components in a tenth of the pixels"""
    rng = np.random.RandomState(seed + 1)
    img = log_uniform(w, h, seed)
    flat = img.reshape(-1, 4)
    values = np.array([np.nan, np.inf, -np.inf, -1.0, -1e30, -0.0], np.float32)
    for k in range(max(1, len(flat) // 10) if len(flat) > 1 else 0):
        i = rng.randint(0, len(flat))
        flat[i, rng.randint(0, 3)] = values[k % len(values)]
    if len(flat) >= 16:
        flat[5, :3] = -0.0                                                  # luminance -0.0f: valid, the lowest code
        flat[6, :3] = (np.inf, -np.inf, 1.0)                                # luminance NaN
        flat[7, :3] = (1.0, 2.0, -1e-3)                                     # a negative component, a positive luminance: valid
    return img


def contents(w, h):
    seed = 131 * w + h
    yy, xx = np.mgrid[0:h, 0:w]
    constant = np.full((h, w, 4), 0.5, np.float32)
    two = np.where((((xx + yy) & 1) == 0)[..., None], F(0.1), F(3.0)) * np.ones((1, 1, 4), np.float32)
    none = np.full((h, w, 4), np.nan, np.float32)
    none[(xx + yy) % 3 == 0] = -1.0
    none[(xx + yy) % 3 == 1, 1] = np.inf
    black = np.zeros((h, w, 4), np.float32)
    return {"log-uniform": log_uniform(w, h, seed), "constant": constant, "two bins": two.astype(np.float32), "sprinkled": sprinkled(w, h, seed),
            "no valid pixel": none, "black": black}


def ao_plane(w, h, seed):
    rng = np.random.RandomState(seed)
    ao = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    bad = rng.uniform(size=(h, w)) < 0.03
    ao[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf, -2.0], np.float32), int(bad.sum()))
    if w * h >= 2:
        ao.reshape(-1)[1] = np.nan
    return ao


def rectangles(w, h):
    """the whole frame, one pixel, one that crosses tile edges on all four sides where the frame has them, one row"""
    crossing = (min(17, w - 1), min(5, h - 1), max(w - 29, min(17, w - 1) + 1), max(h - 21, min(5, h - 1) + 1))
    return {"whole": None, "one pixel": (w // 2, h // 2, w // 2 + 1, h // 2 + 1), "crossing": crossing, "one row": (0, h // 2, w, h // 2 + 1)}


class Case:
    """One size's inputs on the device and the reference's statistics, computed once per (content, flags, ao, rectangle)."""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.host = contents(w, h)
        self.dev = {k: gu.dev(v) for k, v in self.host.items()}
        self.aoh = ao_plane(w, h, 7 * w + h)
        self.aod = gu.dev(self.aoh)
        self.stats = functools.lru_cache(maxsize=None)(self._stats)
        self.ran = 0

    def _stats(self, name, flags, strength, rect):
        return ref.statistics(self.host[name], rect, flags & ref.HEAL, None if strength is None else self.aoh, 1.0 if strength is None else strength)

    def check(self, name, *, flags=0, strength=None, rect=None, groups=0, fractions=(0.0, 1.0), **params):
        st = self.stats(name, flags, strength, rect)
        want = ref.resolve(st, low=fractions[0], high=fractions[1], **params)
        res, hist, scratch, words = run_meter(self.dev[name], self.w, self.h, ao=None if strength is None else self.aod,
                                              strength=1.0 if strength is None else strength, flags=flags, rect=rect, groups=groups, fractions=fractions,
                                              **{dict(min_exposure="lo", max_exposure="hi").get(k, k): v for k, v in params.items()})
        what = f"{self.w}x{self.h} {name} flags {flags} ao {strength} rect {rect} groups {groups} fractions {fractions}"
        written(res, 8, RESULT, want, what + " record")
        written(hist, ref.BINS, HIST, st["hist"], what + " histogram")
        records = written(scratch, words, SCRATCH, None, what + " scratch").reshape(-1, ref.RECORD_WORDS)
        # every word of every partial record was written, and the records add up to the histogram
        assert np.array_equal(records[:, :ref.BINS].sum(axis=0, dtype=np.uint64), st["hist"].astype(np.uint64)), what
        assert (records[:, ref.BINS + 6:] == 0).all() and int(records[:, ref.BINS].sum()) == st["valid"], what
        self.ran += 1
        return want

    def untouched(self):
        for k, v in self.host.items():
            assert np.array_equal(bits(self.dev[k].cpu().numpy()), bits(v)), k
        assert np.array_equal(bits(self.aod.cpu().numpy()), bits(self.aoh))


@functools.lru_cache(maxsize=2)
def case_of(w, h):
    return Case(w, h)


def group_counts(w, h):
    tiles = ((w + 31) // 32) * ((h + 7) // 8)
    return [1, 3, 0] + ([ref.MAX_GROUPS] if ref.MAX_GROUPS > tiles > 100 else [])


# ---- crtx_meter against the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_every_rectangle_and_group_count_matches_the_reference_in_every_word(W, H, form, monkeypatch):
    """the launch geometry: every rectangle under every group count, on the sprinkled image (heal alternating) and on the constant one"""
    monkeypatch.setenv("CRTX_BINS", form)
    c = case_of(W, H)
    k = 0
    for name in ("sprinkled", "constant"):
        for rname, rect in rectangles(W, H).items():
            for groups in group_counts(W, H):
                c.check(name, flags=ref.HEAL if k & 1 else 0, strength=(None, 0.35)[(k >> 1) & 1], rect=rect, groups=groups, fractions=FRACTIONS[k % 4])
                k += 1
    assert k >= 24
    if (W, H) == (200, 120):
        assert group_counts(W, H)[-1] == ref.MAX_GROUPS > 105
    c.untouched()


@pytest.mark.parametrize("form", FORMS + (None,))
@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_every_content_ao_strength_and_fraction_matches_the_reference_in_every_word(W, H, form, monkeypatch):
    """the values: every content with and without CRTX_HEAL, without an AO plane and with one at strengths 0, 0.35 and 1, under the four pairs
    of fractions; form None: CRTX_BINS unset, the built-in choice"""
    if form is None:
        monkeypatch.delenv("CRTX_BINS", raising=False)
    else:
        monkeypatch.setenv("CRTX_BINS", form)
    c = case_of(W, H)
    rects = rectangles(W, H)
    k = 0
    for name in c.host:
        for flags in (0, ref.HEAL):
            for strength in (None, 0.0, 0.35, 1.0):
                rect = rects["whole" if k % 3 else "crossing"]
                for fractions in FRACTIONS if form is not None else FRACTIONS[k % 4:k % 4 + 1]:
                    want = c.check(name, flags=flags, strength=strength, rect=rect, groups=group_counts(W, H)[k % 3], fractions=fractions)
                k += 1
                if name == "no valid pixel" and not flags and strength is None:      # (a negative AO value makes a negative pixel valid)
                    assert want[4] == 0 and want[5] > 0 and want[:3].view(np.float32).tolist() == [1.0, 1.0, 0.0]
                if name == "constant" and strength is None:
                    assert want[6] == want[7] == word(0.5) >> 7 and want[5] == 0
    # what the contents are for
    if W * H >= 512:
        st = c.stats("log-uniform", 0, None, None)
        assert st["hist"][0] > 0 and st["hist"][255] > 0 and st["minQ"] == ref.QMIN and st["maxQ"] == ref.QMAX - 1 and st["invalid"] == 0
        assert np.count_nonzero(c.stats("two bins", 0, None, None)["hist"]) == 2 and np.count_nonzero(c.stats("constant", 0, None, None)["hist"]) == 1
        plain, healed = c.stats("sprinkled", 0, None, None), c.stats("sprinkled", ref.HEAL, None, None)
        assert plain["invalid"] > healed["invalid"] > 0 and healed["valid"] > plain["valid"]       # a healed pixel may still be negative
        assert c.stats("sprinkled", 0, 0.35, None)["invalid"] > plain["invalid"]                   # the AO plane's own non-finite values
        assert c.stats("black", 0, None, None)["hist"][0] == W * H
    c.untouched()


# ---- adaptation -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_adaptation_in_place_follows_the_reference_s_sequence(form, monkeypatch):
    monkeypatch.setenv("CRTX_BINS", form)
    W, H = 200, 120
    c = case_of(W, H)
    st = c.stats("log-uniform", 0, None, None)
    for start, up, down in ((2.0 ** -6, 0.25, 0.75), (2.0 ** 7, 0.75, 0.125)):
        result = guarded(8, RESULT)
        result[0] = word(start)                                 # the record before: only its first word counts
        scratch, p = None, F(start)
        for step in range(5):
            want = ref.resolve(st, prev=p, rate_up=up, rate_down=down)
            _, _, scratch, words = run_meter(c.dev["log-uniform"], W, H, flags=ref.ADAPT, prev="result", up=up, down=down, result=result, hist=False,
                                             scratch=scratch, groups=3)
            got = written(result, 8, RESULT, want, f"adaptation from {start}, step {step}")
            p = got[:1].view(np.float32)[0]
        target = want[1:2].view(np.float32)[0]
        assert (start < p < target) if start < target else (start > p > target)
        written(scratch, words, SCRATCH)
    # prev in another buffer: it is read and left alone; without CRTX_ADAPT it is not looked at
    prev = guarded(8, 0x400)
    prev[0] = word(0.5)
    before = prev.cpu().numpy().copy()
    res, _, _, _ = run_meter(c.dev["log-uniform"], W, H, flags=ref.ADAPT, prev=prev, up=0.5, down=0.25, hist=False)
    written(res, 8, RESULT, ref.resolve(st, prev=F(0.5), rate_up=0.5, rate_down=0.25), "prev elsewhere")
    res, _, _, _ = run_meter(c.dev["log-uniform"], W, H, flags=0, prev=prev, up=0.5, down=0.25, hist=False)
    written(res, 8, RESULT, ref.resolve(st), "prev without ADAPT")
    assert np.array_equal(prev.cpu().numpy(), before)
    # a poisoned, zero, negative or infinite record before gives the target; so does CRTX_ADAPT without a record
    target = ref.resolve(st)
    for w in (0x7FC00123, 0, 0x80000000, word(-2.0), 0x7F800000, 0xFF800000):
        result = guarded(8, RESULT)
        result[0] = signed(w)
        run_meter(c.dev["log-uniform"], W, H, flags=ref.ADAPT, prev="result", up=0.1, down=0.1, result=result, hist=False)
        written(result, 8, RESULT, target, f"prev {w:#x}")
    res, _, _, _ = run_meter(c.dev["log-uniform"], W, H, flags=ref.ADAPT, prev=None, up=0.1, down=0.1, hist=False)
    written(res, 8, RESULT, target, "ADAPT without a record")
    # no valid pixel: the record before stays, unclamped; a poisoned one gives 1
    none = c.stats("no valid pixel", 0, None, None)
    for w, p in ((word(1000.0), F(1000.0)), (0x7FC00123, None)):
        result = guarded(8, RESULT)
        result[0] = signed(w)
        run_meter(c.dev["no valid pixel"], W, H, flags=ref.ADAPT, prev="result", result=result, hist=False)
        got = written(result, 8, RESULT, ref.resolve(none, prev=p), f"no valid pixel, prev {w:#x}")
        assert got[:1].view(np.float32)[0] == (p if p is not None else 1.0)
    # the clamps of the exposure
    for key, lo, hi in ((0.18, 2.0 ** -4, 2.0 ** -2), (1e6, 0.5, 8.0), (1e-6, 0.5, 8.0)):
        res, _, _, _ = run_meter(c.dev["constant"], W, H, key=key, lo=lo, hi=hi, hist=False)
        want = ref.resolve(c.stats("constant", 0, None, None), key=key, min_exposure=lo, max_exposure=hi)
        got = written(res, 8, RESULT, want, f"clamp {key}")
        assert got[:1].view(np.float32)[0] in (F(lo), F(hi))


# ---- crtx_expose ------------------------------------------------------------------------------------------------------------------------------
def same(got, want, what=""):
    """every bit, except that a NaN equals any NaN: the payload of a NaN an operation generates is the hardware's choice (tests/test_gpu_present.py)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    assert got.shape == want.shape and np.array_equal(gn, wn), f"{what}: the NaN patterns differ"
    differ = (bits(got) != bits(want)) & ~gn
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} values differ, the first at {tuple(int(i[0]) for i in np.nonzero(differ))}"


def run_expose(color, w, h, record, *, ao=None, strength=1.0, flags=0, out=None):
    """crtx_expose on device tensors: (out as (h, w, 4), the whole guarded allocation or None when out was given)"""
    whole = None
    if out is None:
        whole = gu.poison((h * w * 4 + GUARD,), 0x500)
        out = whole[:h * w * 4].reshape(h, w, 4)
    e = _lib.CrtxExpose(w, h, color.data_ptr(), ao.data_ptr() if ao is not None else None, record.data_ptr(), strength, flags)
    lib = _lib.meter()
    rc = lib.crtx_expose(C.byref(e), out.data_ptr(), stream())
    assert rc == 0, lib.crtx_error_string(rc)
    return out, whole


def guard_intact(whole, words, salt=0x500):
    tail = (np.arange(words, words + GUARD, dtype=np.int64) + (0x7FC00000 + salt)).astype(np.uint32)
    assert np.array_equal(whole.cpu().numpy().view(np.uint32)[words:], tail), "the words behind the output were written"


def record_of(exposure):
    """a record on the device whose exposure is the float32 `exposure` and whose other words are poison"""
    r = gu.poison((8,), 0x600, "int32")
    r[0] = signed(word(exposure))
    return r


@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_expose_matches_the_reference_in_every_bit(W, H):
    import torch
    c = case_of(W, H)
    host, color = c.host["sprinkled"].copy(), c.dev["sprinkled"]
    host[..., 3] = np.arange(W * H, dtype=np.float32).reshape(H, W)          # alpha passes through
    color = gu.dev(host)
    for exposure in (1.0, 0.37, 2.0 ** 9):
        record = record_of(exposure)
        for flags in (0, ref.HEAL):
            for strength in (None, 0.0, 0.35, 1.0):
                out, whole = run_expose(color, W, H, record, ao=None if strength is None else c.aod, strength=1.0 if strength is None else strength, flags=flags)
                want = ref.expose(host, exposure, flags, None if strength is None else c.aoh, 1.0 if strength is None else strength)
                same(out.cpu().numpy(), want, f"{W}x{H} exposure {exposure} flags {flags} ao {strength}")
                guard_intact(whole, W * H * 4)
                if flags and strength is None:
                    assert np.isfinite(out.cpu().numpy()[..., :3]).all()
    assert np.array_equal(bits(color.cpu().numpy()), bits(host)) and int(record.cpu().numpy().view(np.uint32)[0]) == word(2.0 ** 9)
    # whatever the record holds is multiplied: 0, a negative, a NaN
    for exposure in (0.0, -1.5, np.nan):
        out, whole = run_expose(c.dev["constant"], W, H, record_of(exposure))
        same(out.cpu().numpy(), ref.expose(c.host["constant"], exposure), f"exposure {exposure}")
    # in place
    whole = torch.cat([color.reshape(-1).view(torch.int32), gu.poison((GUARD,), 0x500 + W * H * 4, "int32")]).view(torch.float32)
    image = whole[:W * H * 4].reshape(H, W, 4)
    out, _ = run_expose(image, W, H, record_of(0.37), ao=c.aod, strength=0.35, flags=ref.HEAL, out=image)
    same(out.cpu().numpy(), ref.expose(host, 0.37, ref.HEAL, c.aoh, 0.35), "in place")
    guard_intact(whole, W * H * 4)
    c.untouched()


def test_expose_on_a_side_stream():
    import torch
    W, H = 200, 120
    c = case_of(W, H)
    with side_stream() as side:
        with torch.cuda.stream(side):
            res, hist, scratch, words = run_meter(c.dev["log-uniform"], W, H, fractions=(0.5, 0.9))
            out, whole = run_expose(c.dev["log-uniform"], W, H, res)
        side.synchronize()
    want = ref.resolve(c.stats("log-uniform", 0, None, None), low=0.5, high=0.9)
    written(res, 8, RESULT, want, "side stream")
    same(out.cpu().numpy(), ref.expose(c.host["log-uniform"], want[:1].view(np.float32)[0]), "side stream")
    guard_intact(whole, W * H * 4)


def test_present_of_the_exposed_image_is_present_with_that_exposure():
    """The consequence include/crt_meter.h states: for inputs whose products are finite and without CRTP_HEAL, all eight flag sets at 33 x 16"""
    import test_gpu_present as gp
    W, H = 33, 16
    rng = np.random.RandomState(9)
    host = rng.uniform(0.0, 1.5, (H, W, 4)).astype(np.float32)
    host[..., 3] = 1.0
    aoh = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    color, aod = gu.dev(host), gu.dev(aoh)
    for ao, strength in ((None, 1.0), (aod, 0.35)):
        res, _, _, _ = run_meter(color, W, H, ao=ao, strength=strength, key=0.3, hist=False)
        e = float(res.cpu().numpy().view(np.float32)[0])
        assert np.isfinite(e) and e > 0 and e != 1.0
        exposed, whole = run_expose(color, W, H, res, ao=ao, strength=strength)
        guard_intact(whole, W * H * 4)
        assert np.isfinite(exposed.cpu().numpy()).all()                     # the products are finite (PostProcess may still make a NaN of one)
        for f in range(8):
            got = gp.raw_present(exposed, f)
            want = gp.raw_present(color, f, ao, strength, e)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), (f, strength)
        assert not np.array_equal(gp.raw_present(color, 7, ao, strength, 1.0)[1], want[1])      # the exposure shows


# ---- the Session ------------------------------------------------------------------------------------------------------------------------------
def test_render_meter_expose_present_on_tiny_and_again_behind_a_held_stream():
    import torch
    W, H = 160, 96
    flags = present_ref.UNORM8 | present_ref.FXAA
    case = "meter, expose and present on a held stream"
    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get("tiny"))
        s.render(postprocess=False)
        frame = np.array(s.output(), copy=True)
        record, hist = s.meter(histogram=True, low=0.5, high=0.95)           # the frame itself
        assert tuple(record.shape) == (8,) and record.dtype == torch.float32 and tuple(hist.shape) == (256,) and hist.dtype == torch.int32
        want_record, want_hist = ref.meter(frame, low=0.5, high=0.95)
        assert np.array_equal(record.cpu().numpy().view(np.uint32), want_record) and np.array_equal(hist.cpu().numpy().view(np.uint32), want_hist)
        assert want_record[4] == W * H and record.view(torch.int32)[4].item() == W * H
        e1 = want_record[:1].view(np.float32)[0]
        assert e1 != 1.0 and 2.0 ** -8 < e1 < 2.0 ** 8
        color = gu.dev(frame)
        image = s.expose(color, record)
        want_image = ref.expose(frame, e1)
        same(image.cpu().numpy(), want_image, "expose")
        got = s.present(image, exposure=1.0, postprocess=False, fxaa=True)
        assert np.array_equal(got.cpu().numpy(), present_ref.present(want_image, flags)[1])
        assert np.array_equal(got.cpu().numpy(), present_ref.present(frame, flags, exposure=e1)[1])     # the consequence, on bytes
        # a second frame, adapting from the first one's record, over a region, with an AO plane
        s.render(postprocess=False)
        frame2 = np.array(s.output(), copy=True)
        aoh = np.random.RandomState(2).uniform(0.2, 1.0, (H, W)).astype(np.float32)
        aod = gu.dev(aoh)
        kw = dict(key=0.36, rate_up=0.5, rate_down=0.25, min_exposure=0.01, max_exposure=100.0)
        record2 = s.meter(ao=aod, ao_strength=0.8, prev=record, region=(16, 8, 150, 90), groups=3, **kw)
        want2 = ref.meter(frame2, (16, 8, 150, 90), ref.ADAPT, aoh, 0.8, prev=e1, **kw)[0]
        assert np.array_equal(record2.cpu().numpy().view(np.uint32), want2)
        assert want2[0] != want2[1] and np.array_equal(record.cpu().numpy().view(np.uint32), want_record)      # it adapts; prev is only read
        assert s.frame_readers_pending() >= 0
        # the same three calls behind a held stream: none of them waits, and the results are the same
        color2 = gu.dev(frame2)
        with side_stream() as side:
            with torch.cuda.stream(side):
                out = torch.empty((H, W, 4), device="cuda:0")

                def chain():
                    r = s.meter(color2, ao=aod, ao_strength=0.8, prev=record, region=(16, 8, 150, 90), groups=3, **kw)
                    img = s.expose(color2, r, ao=aod, ao_strength=0.8, out=out)
                    return r, img, s.present(img, exposure=1.0, postprocess=False, fxaa=True)

                chain()                                                         # once unheld: nothing allocates inside the window
            side.synchronize()
            out.fill_(-1.0)
            torch.cuda.synchronize()
            hold = Hold(side)
            with torch.cuda.stream(side):
                r, img, packed = chain()
            hold.must_be_pending(case)
            hold.release()
            side.synchronize()
        assert np.array_equal(r.cpu().numpy().view(np.uint32), want2), case
        want_image = ref.expose(frame2, want2[:1].view(np.float32)[0], 0, aoh, 0.8)
        same(img.cpu().numpy(), want_image, case)
        assert np.array_equal(packed.cpu().numpy(), present_ref.present(want_image, flags)[1]), case


def test_session_refusals():
    import torch
    sc = scenes.get("tiny")
    W, H = 160, 96
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(sc)
        for call in (lambda: s.meter(), lambda: s.expose(None, None)):
            with pytest.raises(ValueError, match="host-only"):
                call()
    with driver.Session(W, H, device=0) as s:
        s.load_scene(sc)
        with pytest.raises(ValueError, match="no frame has been rendered"):
            s.meter()
        color = torch.zeros((H, W, 4), device="cuda:0")
        record = s.meter(color)
        assert record.cpu().numpy().view(np.uint32).tolist() == ref.meter(np.zeros((H, W, 4), np.float32))[0].tolist()
        for kw in (dict(ao_strength=1.5), dict(key=0.0), dict(low=0.6, high=0.5), dict(high=1.5), dict(min_exposure=0.0), dict(min_exposure=2.0, max_exposure=1.0),
                   dict(rate_up=-0.1), dict(rate_down=float("nan")), dict(region=(0, 0, W + 1, H)), dict(region=(5, 5, 5, 9)), dict(region=(-1, 0, 4, 4))):
            with pytest.raises(driver.CrtError, match="bad argument"):
                s.meter(color, **kw)
        for bad in (dict(color=color.cpu()), dict(color=color[:-1]), dict(color=color, ao=torch.zeros((H, W, 1), device="cuda:0")),
                    dict(color=color, prev=torch.zeros(7, device="cuda:0")), dict(color=color, prev=torch.zeros(8, device="cuda:0", dtype=torch.int32)),
                    dict(color=color, region=(1, 2, 3)), dict(color=color, groups=-1), dict(color=color, groups=_lib.CRTX_MAX_GROUPS + 1)):
            with pytest.raises(ValueError):
                s.meter(**bad)
        with pytest.raises(driver.CrtError, match="bad argument"):
            s.expose(color, record, ao_strength=2.0)
        for bad in (dict(color=None, record=record), dict(color=color, record=record[:4]), dict(color=color, record=record.cpu()),
                    dict(color=color, record=record, out=torch.zeros((H, W, 3), device="cuda:0"))):
            with pytest.raises(ValueError):
                s.expose(**bad)
        same(s.expose(color, record, out=color).cpu().numpy(), np.zeros((H, W, 4), np.float32), "in place")      # out may be color
        s.render_raw(0)
        s.set_row_bands(16, 0, 2)
        with pytest.raises(ValueError, match="row bands"):
            s.meter()
