"""The guard of the traversal's short reciprocal (clraytracer_amd/csrc/crt_device.h: recip, recip3, recip_needs_division), restated in
numpy with the constants READ FROM THE HEADER, over the boundary bit patterns of both signs: the short sequence (v_rcp_f32 + one Newton
step + v_div_fixup_f32) is wrong exactly for denormal operands and for finite |x| >= 2^126, so the set the guard sends to the division
must contain every one of those -- and zeros, infinities and NaNs, which the short sequence gets right, must stay on the fast path.
The device side of the same statement is crt_debug_recip_sweep over all 2^32 patterns (tests/test_gpu_recip.py)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "clraytracer_amd", "csrc", "crt_device.h")).read()

# positive patterns; every one is also checked with the sign bit set
BOUNDARY = {
    "zero": 0x00000000, "smallest denormal": 0x00000001, "largest denormal": 0x007FFFFF, "smallest normal": 0x00800000,
    "below 2^126": 0x7E7FFFFF, "2^126": 0x7E800000, "largest finite": 0x7F7FFFFF, "infinity": 0x7F800000,
    "signalling NaN": 0x7F800001, "signalling NaN, full payload": 0x7FBFFFFF, "quiet NaN": 0x7FC00000, "quiet NaN, full payload": 0x7FFFFFFF,
}


def guard_constants():
    """(bias, width) of `(uint32_t)(e + bias) > width` and (hi, lo) of `hi > .. || lo < ..`, as the header states them"""
    one = re.search(r"recip_needs_division\(int e\) \{ return \(uint32_t\)\(e \+ (\d+)\) > (\d+)u; \}", HEADER)
    three = re.search(r"__ballot\(hi > (-?\d+) \|\| lo < (-?\d+)\)", HEADER)
    assert one and three, "the guard's text changed: restate it here"
    return (int(one.group(1)), int(one.group(2))), (int(three.group(1)), int(three.group(2)))


def frexp_exp(bits):
    """v_frexp_exp_i32_f32 with denormals kept: the exponent of x = m 2^e, 0.5 <= |m| < 1; 0 for zeros, infinities and NaNs"""
    x = np.asarray(bits, np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        _, e = np.frexp(x)
    return np.where(np.isfinite(x), e, 0).astype(np.int64)


def needs_division(bits):
    (bias, width), _ = guard_constants()
    return ((frexp_exp(bits) + bias) & 0xFFFFFFFF) > width


def needs_division3(bits3):
    _, (hi, lo) = guard_constants()
    e = frexp_exp(bits3)
    return (e.max(-1) > hi) | (e.min(-1) < lo)


def both_signs(bits):
    bits = np.atleast_1d(np.asarray(bits, np.uint32))
    return np.concatenate([bits, bits | np.uint32(0x80000000)])


def is_denormal(bits):
    b = np.asarray(bits, np.uint32) & np.uint32(0x7FFFFFFF)
    return (b > 0) & (b < 0x00800000)


def is_huge_finite(bits):
    b = np.asarray(bits, np.uint32) & np.uint32(0x7FFFFFFF)
    return (b >= 0x7E800000) & (b < 0x7F800000)


def test_the_fallback_set_holds_every_denormal_and_every_finite_value_from_2_to_the_126():
    named = both_signs(list(BOUNDARY.values()))
    want = is_denormal(named) | is_huge_finite(named)
    got = needs_division(named)
    for b, w, g in zip(named, want, got):
        assert bool(g) == bool(w), f"{int(b):#010x}: needs the division {bool(w)}, the guard says {bool(g)}"
    # the two classes densely: every denormal exponent step and mantissa edge, every pattern class from 2^126 upwards
    rng = np.random.RandomState(7)
    den = both_signs(np.concatenate([np.uint32(1) << np.arange(23, dtype=np.uint32), (np.uint32(1) << np.arange(1, 24, dtype=np.uint32)) - np.uint32(1),
                                     rng.randint(1, 0x00800000, 4096).astype(np.uint32)]))
    huge = both_signs(np.concatenate([np.array([0x7E800000, 0x7E800001, 0x7EFFFFFF, 0x7F000000, 0x7F000001, 0x7F7FFFFE, 0x7F7FFFFF], np.uint32),
                                      rng.randint(0x7E800000, 0x7F800000, 4096).astype(np.uint32)]))
    assert is_denormal(den).all() and needs_division(den).all()
    assert is_huge_finite(huge).all() and needs_division(huge).all()


def test_zeros_infinities_nans_and_the_ordinary_range_stay_on_the_fast_path():
    for name in ("zero", "infinity", "signalling NaN", "signalling NaN, full payload", "quiet NaN", "quiet NaN, full payload", "smallest normal", "below 2^126"):
        assert not needs_division(both_signs(BOUNDARY[name])).any(), name
    rng = np.random.RandomState(8)
    ordinary = both_signs(rng.randint(0x00800000, 0x7E800000, 1 << 16).astype(np.uint32))
    assert not needs_division(ordinary).any()
    nans = both_signs(rng.randint(0x7F800001, 0x80000000, 4096).astype(np.uint32))
    assert not needs_division(nans).any()


def test_the_three_operand_guard_is_the_or_of_the_three():
    """Traversal::enter's single decision (largest and smallest exponent of the three) = any operand needs the division: every triple of
    boundary patterns, both signs"""
    named = both_signs(list(BOUNDARY.values()))
    triples = np.stack(np.meshgrid(named, named, named, indexing="ij"), -1).reshape(-1, 3)
    assert np.array_equal(needs_division3(triples), needs_division(triples).any(-1))


def test_the_constants_are_the_documented_ones():
    assert guard_constants() == ((125, 251), (126, -125))
    # one switch restores the division everywhere, and both call sites go through the helpers
    assert HEADER.count("#ifdef CRT_IEEE_RECIP") == 1
    assert "inv = recip3<DIVIDE>(md);" in HEADER and "const float f = recip<DIVIDE>(a);" in HEADER
    assert len(re.findall(r"1\.0f / md\.", HEADER)) == 0 and "1.0f / a;" not in HEADER
