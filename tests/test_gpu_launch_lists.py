"""The three launch-list kernels (crt_cost_spread_kernel, crt_order_kernel, crt_identity_order_kernel) on chosen costs, through
crt_debug_launch_lists -- production's launches on a scratch copy of a slot's lists -- against the numpy restatement
tests/launch_lists_ref.py: every list must cover every tile exactly once (one entry, or four quadrant entries), heaviest bin first,
split count and length as the reference says. The inputs are the grid tests/test_launch_lists_cpu.py proves robust (no list whose
threshold bin depends on the order of the device's float additions)."""
import ctypes as C

import numpy as np
import pytest

from clraytracer_amd import _lib, driver
import launch_lists_ref as ll

pytestmark = pytest.mark.gpu


def test_diagnostics_need_a_session():
    # first in the file: the module's session does not exist yet
    hip = _lib.hip()
    buf = np.zeros(8, np.uint32); n = C.c_int(0)
    assert hip.crt_debug_launch_lists(buf.ctypes.data, 1, 1, 0, 0.0, 0.0, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data) == _lib.CRT_E_NOT_INITIALIZED
    assert hip.crt_debug_read_launch_lists(None, 0, buf.ctypes.data, C.byref(n), C.byref(n)) == _lib.CRT_E_NOT_INITIALIZED


@pytest.fixture(scope="module")
def session():
    with driver.Session(64, 48, device=0) as s:
        yield s


def test_sorted_lists_match_the_reference(session):
    s = session
    lists = none = some = capped = cut = 0
    for family, S, tiles_x, spread, sf, ms in ll.grid():
        cost = ll.costs(family, S)
        ref = ll.reference(cost, tiles_x, ms, sf, spread)
        assert not ref["fragile"].any(), (family, S, spread, sf)
        given = cost.copy()
        order, length, after = s.launch_lists(cost, tiles_x, ms, sf, spread)
        assert np.array_equal(cost, given)                                  # the caller's costs are read only
        try:
            ll.check_lists(order, length, ref["bins"], ref["nsplit"], after)
        except AssertionError as e:
            raise AssertionError(f"{family} S={S} tilesX={tiles_x} spread={spread} splitFactor={sf} maxSplit={ms}: {e}") from e
        n = ref["nsplit"]
        lists += 8
        none += int((n == 0).sum()); some += int(((n > 0) & (n < ms)).sum()); capped += int((n == ms).sum()) if ms == ll.MAX_SPLIT else 0
        cut += int(ref["cut"].sum())
    print(f"{lists} lists equal to the reference; nSplit == 0: {none}, 0 < nSplit < maxSplit: {some}, nSplit == maxSplit == 96: {capped}, "
          f"threshold inside a bin of several tiles: {cut}")
    # the cases this test exists for were reached, not assumed
    assert lists == 8 * 14 * 7 * 4 * 3
    assert none > 0 and some > 0 and capped > 0 and cut > 0


@pytest.mark.parametrize("S", [s for s, _ in ll.SIZES])
def test_identity_lists(session, S):
    order, length = session.identity_lists(S)
    assert (length == S).all()
    assert np.array_equal(order[:, :S], np.tile(np.arange(S, dtype=np.uint32), (8, 1)))
    ll.check_structure(order, length, S)


def test_refusals_are_codes(session):
    hip = _lib.hip()
    S = 50
    cost = ll.costs("lognormal", S)
    order = np.zeros((8, S + 3 * ll.MAX_SPLIT), np.uint32); length = np.zeros(8, np.uint32); after = np.zeros((8, S), np.uint32)

    def rc(cost=cost, S=S, tiles_x=25, ms=96, sf=0.05, spread=0.0, order=order, length=length, after=after):
        p = lambda a: None if a is None else a.ctypes.data
        return hip.crt_debug_launch_lists(p(cost), S, tiles_x, ms, C.c_float(sf), C.c_float(spread), p(order), p(length), p(after))

    assert rc() == 0
    for bad in (dict(cost=None), dict(order=None), dict(length=None), dict(after=None), dict(S=0), dict(S=(1 << 20) + 1, tiles_x=1),
                dict(S=-(1 << 20) - 1), dict(tiles_x=0), dict(tiles_x=-5), dict(tiles_x=7), dict(tiles_x=100), dict(ms=97), dict(ms=-1),
                dict(sf=-0.01), dict(sf=1.01), dict(sf=float("nan")), dict(sf=float("inf")), dict(spread=-0.5), dict(spread=1.5),
                dict(spread=float("nan")), dict(spread=float("-inf"))):
        assert rc(**bad) == _lib.CRT_E_BAD_ARGUMENT, bad
    high = cost.copy(); high[3, 7] = ll.SATURATED + 1                       # more than a frame's waves can add to a tile
    assert rc(cost=high) == _lib.CRT_E_BAD_ARGUMENT
    assert rc(S=-S, order=None) == _lib.CRT_E_BAD_ARGUMENT and rc(S=-S, cost=None, after=None) == 0
    assert rc() == 0
    ref = ll.reference(cost, 25, 96, 0.05)
    ll.check_lists(order, length, ref["bins"], ref["nsplit"], after)
    # a session that has rendered nothing keeps no lists
    n, cap = C.c_int(0), C.c_int(0)
    assert hip.crt_debug_read_launch_lists(None, 0, length.ctypes.data, C.byref(n), C.byref(cap)) == _lib.CRT_E_UNSUPPORTED
    assert hip.crt_debug_read_launch_lists(None, 0, None, C.byref(n), C.byref(cap)) == _lib.CRT_E_BAD_ARGUMENT
