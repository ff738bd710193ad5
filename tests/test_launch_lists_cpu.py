"""The numpy side of the launch-list tests (tests/launch_lists_ref.py) without a GPU: the shared input grid holds no fragile list and
reaches the cases the GPU test relies on, the validator rejects every kind of wrong list, the spread key is right by hand, and the two
diagnostics are declared where they belong."""
import os
import re

import numpy as np
import pytest

import launch_lists_ref as ll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_shared_grid_is_robust_and_reaches_every_case():
    lists = fragile = 0
    none = some = capped = cut = 0
    for family, S, tiles_x, spread, sf, ms in ll.grid():
        ref = ll.reference(ll.costs(family, S), tiles_x, ms, sf, spread)
        lists += 8
        fragile += int(ref["fragile"].sum())
        n = ref["nsplit"]
        none += int((n == 0).sum()); some += int(((n > 0) & (n < ms)).sum()); capped += int((n == ms).sum()) if ms == ll.MAX_SPLIT else 0
        cut += int(ref["cut"].sum())
        ll.check_lists(*ll.build_lists(ref), ref["bins"], n)            # the reference's own lists pass its validator
    print(f"{lists} lists: {fragile} fragile; nSplit == 0: {none}, 0 < nSplit < maxSplit: {some}, nSplit == maxSplit == 96: {capped}, threshold inside a bin: {cut}")
    assert lists == 8 * 14 * 7 * 4 * 3
    assert fragile == 0
    assert none > 0 and some > 0 and capped > 0 and cut > 0
    # 1920x1080 (S = 4050), lognormal costs, production's split factor: every XCD reaches the cap
    assert (ll.reference(ll.costs("lognormal", 4050), 225, ll.MAX_SPLIT, ll.SPLIT_FACTORS[1])["nsplit"] == ll.MAX_SPLIT).all()


@pytest.fixture(scope="module")
def valid():
    """A reference-built list with split and unsplit tiles in several bins on XCD `x`"""
    cost = ll.costs("lognormal", 50)
    ref = ll.reference(cost, 25, ll.MAX_SPLIT, 0.05)
    order, length = ll.build_lists(ref)
    x = next(x for x in range(8) if 2 <= ref["nsplit"][x] <= 40)
    ll.check_lists(order, length, ref["bins"], ref["nsplit"], np.zeros_like(cost))
    return ref, order, length, x


def rejected(ref, order, length, cost_after=None):
    with pytest.raises(AssertionError):
        ll.check_lists(order, length, ref["bins"], ref["nsplit"], cost_after)


def test_validator_rejects_a_dropped_tile(valid):
    ref, order, length, x = valid
    n = int(ref["nsplit"][x])
    o = order.copy(); o[x, 4 * n + 3] = o[x, 4 * n + 4]                  # an unsplit tile replaced by its neighbour: one missing, one twice
    rejected(ref, o, length)
    o = order.copy(); lens = length.copy()
    o[x, 4 * n:int(lens[x]) - 1] = order[x, 4 * n + 1:int(lens[x])]; lens[x] -= 1          # an entry taken out
    rejected(ref, o, lens)


def test_validator_rejects_a_tile_both_split_and_unsplit(valid):
    ref, order, length, x = valid
    n = int(ref["nsplit"][x])
    o = order.copy(); o[x, 4 * n] = o[x, 0] & np.uint32(0x0FFFFFFF)
    rejected(ref, o, length)


def test_validator_rejects_a_wrong_quadrant_quad(valid):
    ref, order, length, x = valid
    o = order.copy(); o[x, 7] = o[x, 6]                                  # quadrant 2 twice, 3 missing
    rejected(ref, o, length)
    o = order.copy(); o[x, 3] &= np.uint32(0x0FFFFFFF)                   # the fourth quadrant entry lost its flag: three quadrants
    rejected(ref, o, length)
    o = order.copy(); o[x, 5] = (o[x, 5] & np.uint32(0xF0000000)) | (o[x, 0] & np.uint32(0x0FFFFFFF))     # a quad naming two tiles
    rejected(ref, o, length)


@pytest.mark.parametrize("delta", [3, -3])
def test_validator_rejects_a_list_length_off_by_three(valid, delta):
    ref, order, length, x = valid
    lens = length.copy(); lens[x] = int(lens[x]) + delta
    rejected(ref, order, lens)


def test_validator_rejects_a_split_tile_lighter_than_an_unsplit_one(valid):
    ref, order, length, x = valid
    L = int(length[x])
    heavy, light = int(order[x, 0] & np.uint32(0x0FFFFFFF)), int(order[x, L - 1])
    assert ref["bins"][x][heavy] < ref["bins"][x][light]
    o = order.copy()
    o[x, 0:4] = (o[x, 0:4] & np.uint32(0xF0000000)) | np.uint32(light); o[x, L - 1] = heavy
    ll.check_structure(o, length, 50)                                    # still a cover of every tile: only the order is wrong
    rejected(ref, o, length)


def test_validator_rejects_costs_left_behind(valid):
    ref, order, length, x = valid
    after = np.zeros((8, 50), np.uint32); after[x, 17] = 1
    rejected(ref, order, length, after)


def test_validator_never_reads_beyond_the_list(valid):
    ref, order, length, x = valid
    o = order.copy()
    for k in range(8):
        o[k, int(length[k]):] = 0x80000000
    ll.check_lists(o, length, ref["bins"], ref["nsplit"])


def test_spread_key_by_hand():
    """3 tiles wide, 16 tile rows: slotsPerXcd = 6, slot i of XCD x is tile row (i // 3) * 8 + x, column i % 3. One hot tile of 1000 among
    10s, spread 0.8: its neighbours inside the grid get uint32(1000 * 0.8f) = 800, every other tile keeps 10 (10 * 0.8f = 8 < 10)."""
    def keys(x, i):
        cost = np.full((8, 6), 10, np.uint32); cost[x, i] = 1000
        return ll.spread_keys(cost, 3, 0.8)

    def want(hot, lifted):
        w = np.full((8, 6), 10, np.uint32); w[hot] = 1000
        for xi in lifted:
            w[xi] = 800
        return w

    assert int(np.float32(1000.0) * np.float32(0.8)) == 800
    # corner: tile row 0, column 0 -> (row 0, col 1), (row 1, col 0), (row 1, col 1)
    assert np.array_equal(keys(0, 0), want((0, 0), [(0, 1), (1, 0), (1, 1)]))
    # left edge: tile row 4, column 0 -> rows 3 and 5 columns 0-1, row 4 column 1
    assert np.array_equal(keys(4, 0), want((4, 0), [(3, 0), (3, 1), (4, 1), (5, 0), (5, 1)]))
    # the wrap between the rounds: tile row 7 (XCD 7, round 0), column 1 -> row 6 (XCD 6), row 7, and row 8 = XCD 0 of round 1 (slots 3-5)
    assert np.array_equal(keys(7, 1), want((7, 1), [(6, 0), (6, 1), (6, 2), (7, 0), (7, 2), (0, 3), (0, 4), (0, 5)]))
    # and from the other side: tile row 8, column 2 (XCD 0, slot 5) -> row 7 = XCD 7 round 0, row 9 = XCD 1 round 1
    assert np.array_equal(keys(0, 5), want((0, 5), [(7, 1), (7, 2), (0, 4), (1, 4), (1, 5)]))
    # bottom edge: tile row 15 (XCD 7, round 1), column 1 -> row 14 (XCD 6, round 1), row 15; nothing below
    assert np.array_equal(keys(7, 4), want((7, 4), [(6, 3), (6, 4), (6, 5), (7, 3), (7, 5)]))
    # spread 0 and a lifted key below the own cost change nothing
    cost = ll.costs("lognormal", 6)
    assert np.array_equal(ll.spread_keys(cost, 3, 0.0), cost)


def test_spread_key_equals_the_kernel_loop():
    """the vectorised key against a transcription of crt_cost_spread_kernel's loop, tile by tile"""
    for S, tiles_x in ((7, 7), (50, 25), (6, 1)):
        cost = ll.costs("unowned", S)
        got = ll.spread_keys(cost, tiles_x, ll.SPREAD)
        rows = (S // tiles_x) * 8
        for x in range(8):
            for i in range(S):
                rnd, tx = divmod(i, tiles_x)
                k = rnd * 8 + x
                nb = 0
                for dk in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        kk, xx = k + dk, tx + dx
                        if (dk or dx) and 0 <= kk < rows and 0 <= xx < tiles_x:
                            nb = max(nb, int(cost[kk & 7, (kk >> 3) * tiles_x + xx]))
                lifted = int(np.float32(nb) * np.float32(ll.SPREAD))
                assert int(got[x, i]) == max(int(cost[x, i]), lifted), (S, x, i)


def test_bins_at_the_edges():
    # scale 1: one bin per value, the maximum in bin 0, zero in bin 1023
    assert np.array_equal(ll.bins_of(np.array([0, 1, 1022, 1023], np.uint32)), [1023, 1022, 1, 0])
    # all zero: the maximum stays 1, every tile in the lightest bin, nothing heavier than the threshold bin
    ref = ll.reference(np.zeros((8, 7), np.uint32), 7, ll.MAX_SPLIT, 0.05)
    assert (ref["bins"] == 1023).all() and (ref["b"] == 1023).all() and (ref["nsplit"] == 0).all()


def test_diagnostics_are_declared_outside_the_drop_in_surface():
    names = ("crt_debug_launch_lists", "crt_debug_read_launch_lists")
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    dbg, api, lib = read("include", "crt_debug.h"), read("include", "crt_api.h"), read("clraytracer_amd", "_lib.py")
    for n in names:
        assert re.search(r"\bint\s+%s\s*\(" % n, dbg), n
        assert '"%s"' % n in lib, n
        assert n not in api, n
