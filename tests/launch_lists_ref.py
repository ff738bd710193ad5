"""numpy restatement of the feedback launch lists (csrc/crt_kernels.h: crt_cost_spread_kernel, crt_order_kernel, crt_identity_order_kernel),
the validator of a list against it, and the input grid the CPU and the GPU test share.

A frame is right only if the eight per-XCD lists cover every tile exactly once -- by one entry, or by four quadrant entries. What the
kernels fix is restated here one float32 operation per numpy operation, so bins and split counts are exact:

  key   = max(own cost, uint32(float32(heaviest of the 8 neighbours) * float32(spread)))        (spread > 0; else the cost itself)
  bin   = clip(1023 - int(float32(key) * scale), 0, 1023),  scale = float32(1023) / float32(max(1, max key))
  b     = clip(1023 - int(float32(splitFactor) * sum(own costs) * scale), 0, 1023)
  nSplit = min(number of tiles in bins < b, maxSplit);  listLen = S + 3 * nSplit

Two things are order-dependent on the device by construction, and the reference does not pretend otherwise:
  * the order of the tiles inside one bin (atomics): `check_lists` compares the bins along a list, never positions inside a bin;
  * the float32 sum of the costs (per-thread partial sums, a wave reduction, 16 atomics): the reference sums in float64 and calls a list
    `fragile` unless b is the same for that sum scaled by 1 - 2^-18 and by 1 + 2^-18 (at most 4 + 6 + 16 float32 roundings of 2^-24 for
    the S <= 4050 used here: below 2^-19). Test inputs must have no fragile list -- a condition on the inputs, not a tolerance.
"""
import numpy as np

MAX_SPLIT = 96                      # CRT_MAX_SPLIT
SPLIT_FLAG = np.uint32(0x80000000)
SATURATED = 0x3FFFFFFC              # the most four quadrant waves, each saturating at 0x0FFFFFFF, can add to one tile
F32 = np.float32


def spread_keys(cost, tiles_x, spread):
    """crt_cost_spread_kernel: cost (8, S) uint32 -> key (8, S) uint32. Slot i of XCD x is the tile (row k = (i // tilesX) * 8 + x, column
    i % tilesX) of the rank's tile grid; neighbours outside the grid are left out (a cost is >= 0, so padding with zeros leaves them out)."""
    cost = np.asarray(cost, np.uint32)
    S = cost.shape[1]
    rounds = S // tiles_x
    grid = cost.reshape(8, rounds, tiles_x).transpose(1, 0, 2).reshape(rounds * 8, tiles_x)      # [k, tx]
    pad = np.zeros((rounds * 8 + 2, tiles_x + 2), np.uint32)
    pad[1:-1, 1:-1] = grid
    nb = np.zeros_like(grid)
    for dk in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dk, dx) != (1, 1):
                nb = np.maximum(nb, pad[dk:dk + rounds * 8, dx:dx + tiles_x])
    lifted = (nb.astype(F32) * F32(spread)).astype(np.int64).astype(np.uint32)
    key = np.maximum(grid, lifted)
    return np.ascontiguousarray(key.reshape(rounds, 8, tiles_x).transpose(1, 0, 2).reshape(8, S))


def _scale(keys):
    return F32(1023.0) / F32(max(1, int(keys.max())))


def bins_of(keys):
    """Bins of one XCD's keys (S,) -> (S,) int64, heaviest = 0"""
    t = np.asarray(keys, np.uint32).astype(F32) * _scale(keys)
    return np.clip(1023 - t.astype(np.int64), 0, 1023)


def _threshold_bin(total, keys, split_factor):
    t = (F32(split_factor) * F32(total)) * _scale(keys)
    return int(np.clip(1023 - int(t), 0, 1023))


def reference(cost, tiles_x, max_split, split_factor, spread=0.0):
    """What the sort must produce for cost (8, S): dict of
       keys (8, S), bins (8, S), b (8,), nsplit (8,), fragile (8,) bool, cut (8,) bool.
    cut: the threshold splitFactor * sum lies strictly between two keys of bin b -- it cuts inside a bin that holds several tiles, and
    none of that bin's tiles may be split."""
    cost = np.asarray(cost, np.uint32)
    keys = spread_keys(cost, tiles_x, spread) if spread > 0 else cost
    out = {"keys": keys, "bins": np.empty(cost.shape, np.int64), "b": np.empty(8, np.int64), "nsplit": np.empty(8, np.int64),
           "fragile": np.zeros(8, bool), "cut": np.zeros(8, bool)}
    for x in range(8):
        bins = bins_of(keys[x])
        total = float(cost[x].astype(np.float64).sum())                  # the sum runs over the costs, not the keys
        b = _threshold_bin(total, keys[x], split_factor)
        out["fragile"][x] = any(_threshold_bin(total * (1.0 + s * 2.0 ** -18), keys[x], split_factor) != b for s in (-1.0, 1.0))
        out["bins"][x] = bins; out["b"][x] = b
        out["nsplit"][x] = min(int((bins < b).sum()), int(max_split))
        kb = keys[x][bins == b].astype(np.float64)
        thr = float(F32(split_factor) * F32(total))
        out["cut"][x] = len(kb) >= 2 and kb.min() < thr < kb.max()
    return out


def check_structure(order, list_len, S):
    """The part of the contract that needs no costs: per XCD, listLen = S + 3 n with 0 <= n <= min(S, 96); the first 4 n entries are n
    distinct tiles, each as four consecutive entries with the split flag and quadrants 0, 1, 2, 3 in bits 28-29; the other S - n entries
    are unflagged; together they hold every tile 0 .. S-1 exactly once. Entries at and beyond listLen are not read.
    Returns per XCD (n, tiles in list order -- a split tile counted once)."""
    order = np.asarray(order, np.uint32)
    out = []
    for x in range(8):
        L = int(list_len[x])
        assert L >= S and (L - S) % 3 == 0, (x, L, S)
        n = (L - S) // 3
        assert n <= min(S, MAX_SPLIT) and L <= order.shape[1], (x, L, S)
        e = order[x, :L]
        head, tail = e[:4 * n].reshape(n, 4), e[4 * n:]
        assert np.array_equal(head >> np.uint32(28), np.tile(np.arange(8, 12, dtype=np.uint32), (n, 1))), (x, "split flag / quadrants 0, 1, 2, 3")
        tiles = head & np.uint32(0x0FFFFFFF)
        assert (tiles == tiles[:, :1]).all(), (x, "the four entries of a split tile name one tile")
        assert (tail >> np.uint32(28) == 0).all(), (x, "unsplit entries carry no flag")
        seq = np.concatenate([tiles[:, 0], tail]).astype(np.int64)
        assert len(seq) == S and np.array_equal(np.sort(seq), np.arange(S)), (x, "every tile exactly once")
        out.append((n, seq))
    return out


def check_lists(order, list_len, bins, nsplit, cost_after=None):
    """check_structure, and against the reference: the split count; bins never get heavier along a list (a split tile counts once) -- with
    the permutation that makes the tiles of each bin exactly the reference's and no unsplit tile heavier than a split one; the costs are
    left zeroed."""
    bins = np.asarray(bins)
    S = bins.shape[1]
    for x, (n, seq) in enumerate(check_structure(order, list_len, S)):
        assert n == int(nsplit[x]), (x, n, int(nsplit[x]))
        assert (np.diff(bins[x][seq]) >= 0).all(), (x, "heaviest first")
    if cost_after is not None:
        assert not np.asarray(cost_after).any(), "the sort leaves the costs zeroed"


def build_lists(ref):
    """A valid (order, listLen) for a reference result, as the kernel lays it out (in-bin order: by tile index) -- what the CPU test mutates."""
    S = ref["bins"].shape[1]
    order = np.full((8, S + 3 * MAX_SPLIT), 0xDEADBEEF, np.uint32)
    length = np.empty(8, np.uint32)
    for x in range(8):
        seq = np.argsort(ref["bins"][x], kind="stable").astype(np.uint32)
        n = int(ref["nsplit"][x])
        quads = seq[:n, None] | (np.arange(4, dtype=np.uint32)[None, :] << np.uint32(28)) | SPLIT_FLAG
        order[x, :4 * n] = quads.reshape(-1)
        order[x, 4 * n:S + 3 * n] = seq[n:]
        length[x] = S + 3 * n
    return order, length


# ---- the input grid shared by tests/test_launch_lists_cpu.py and tests/test_gpu_launch_lists.py --------------------------------------------
# (slotsPerXcd, tilesX). 4050 = the 240 x 135 tiles of a 1920x1080 frame over 8 XCDs; the diagnostic wants tilesX to divide slotsPerXcd, so it
# runs with 225 columns (the sort itself never reads tilesX, and S > 1025 runs without the spread). 4080 = 17 x 240 is what a session at
# 1920x1080 really sorts (135 tile rows rounded up to 136).
SIZES = ((1, 1), (7, 7), (50, 25), (1023, 341), (1024, 128), (1025, 205), (4050, 225), (4080, 240))
FAMILIES = ("zeros", "equal", "giant", "saturated", "lognormal", "edges", "unowned")
SPLIT_FACTORS = (0.0, 1.2 / 1024.0, 1e-6, 0.05)         # 1.2 / 1024: production's beta over the 1024 wave slots of an XCD of 32 CUs
MAX_SPLITS = (0, 1, MAX_SPLIT)
SPREAD = 0.8                                            # production's CRT_COST_SPREAD; used for S <= 1025


def costs(family, S, seed=20240607):
    """cost (8, S) uint32 of one family; every XCD gets its own values"""
    rng = np.random.default_rng([seed, FAMILIES.index(family), S])
    if family == "zeros":                               # s_max stays 1
        c = np.zeros((8, S))
    elif family == "equal":
        c = np.full((8, S), 5003.0)
    elif family == "giant":                             # one tile at the most four saturated quadrant waves can add, among 1000s
        c = np.full((8, S), 1000.0)
        c[np.arange(8), (np.arange(8) * 37 + 5) % S] = SATURATED
    elif family == "saturated":
        c = np.full((8, S), float(SATURATED))
    elif family in ("lognormal", "unowned"):
        c = np.floor(np.exp(rng.normal(8.0, 1.5, (8, S))))
        if family == "unowned":                         # the 0.4 of the slots that no rank owns
            c[rng.random((8, S)) < 0.4] = 0.0
    else:                                               # "edges": values 0 .. 1023 (scale 1: one bin per value) with several at the maximum
        c = np.floor(rng.random((8, S)) * 1024.0)
        c[:, :: max(1, S // 5)] = 1023.0
    return c.astype(np.uint32)


def grid():
    """Every (family, S, tilesX, spread, splitFactor, maxSplit) of the shared grid"""
    for S, tiles_x in SIZES:
        for spread in ((0.0, SPREAD) if S <= 1025 else (0.0,)):
            for family in FAMILIES:
                for sf in SPLIT_FACTORS:
                    for ms in MAX_SPLITS:
                        yield family, S, tiles_x, spread, sf, ms
