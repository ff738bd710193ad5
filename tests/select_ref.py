"""A numpy restatement of the definitions in include/crt_select.h, written from the header: compact (a loop-free statement of "the selected
indices in ascending order, then CRTS_NONE"), points (every operation a float32 operation of its own, as tests/temporal_ref.py does its
reprojection line; numpy contracts nothing) and scatter. What crts_compact, crts_points and crts_scatter must give, bit for bit."""
import numpy as np

from temporal_ref import camera, camera_from_struct, dot3, pinhole  # noqa: F401 (the cameras are re-exported)
from upsample_ref import low_size

NONE = 0xFFFFFFFF
RETRACED = 3
CHUNK, SCAN, MAX_ITEMS = 2048, 256, 1 << 28
F = np.float32


def selected(words, values):
    """the header's rule per item: words[k] < 32 && ((values >> words[k]) & 1)"""
    w = np.asarray(words).reshape(-1).astype(np.uint64)
    return (w < 32) & (((np.uint64(values) >> np.minimum(w, np.uint64(31))) & np.uint64(1)) != 0)


def compact(words, values, capacity):
    """(list uint32[capacity], counts uint32[2])"""
    idx = np.flatnonzero(selected(words, values)).astype(np.uint32)
    total = len(idx)
    lst = np.full(capacity, NONE, np.uint32)
    kept = min(total, capacity)
    lst[:kept] = idx[:kept]
    return lst, np.array([total, kept], np.uint32)


def grid_list(width, height, factor, offset=(0, 0)):
    """the pixel index of every item of the grid form: item j is low sample (j % LW, j / LW) on pixel (F*X + ox, F*Y + oy)"""
    lw, lh = low_size(width, height, factor, offset)
    j = np.arange(lw * lh, dtype=np.int64)
    X, Y = j % lw, j // lw
    return ((factor * Y + offset[1]) * width + (factor * X + offset[0])).astype(np.uint32)


def points(lst, geometry, cam):
    """lst: uint32 entries (any values); geometry (H, W, 4) float32 = n, t; cam = temporal_ref.camera(). Returns (positions, normals, dirs),
    (count, 4) float32 each."""
    geometry = np.ascontiguousarray(geometry, np.float32)
    H, W = geometry.shape[:2]
    k = np.asarray(lst, np.uint32).astype(np.int64)
    valid = k < W * H
    kc = np.where(valid, k, 0)
    y, x = kc // W, kc % W
    g = geometry.reshape(-1, 4)[kc]
    n, t = g[:, :3], g[:, 3]
    one, zero = F(1.0), F(0.0)
    R, pos = np.asarray(cam["toRay"], np.float32).reshape(3, 3), np.asarray(cam["pos"], np.float32)
    with np.errstate(all="ignore"):
        px, py = x.astype(np.float32), y.astype(np.float32)
        d = [dot3(R[r, 0], R[r, 1], R[r, 2], px, py, one) for r in range(3)]
        dl = np.sqrt(dot3(d[0], d[1], d[2], d[0], d[1], d[2]))
        d = [d[c] / dl for c in range(3)]
        hit = t <= F(99998.0)
        away = dot3(n[:, 0], n[:, 1], n[:, 2], d[0], d[1], d[2]) > zero
        P = [pos[c] + d[c] * t for c in range(3)]
        positions = np.stack([np.where(hit, P[c], zero) for c in range(3)] + [t], axis=-1).astype(np.float32)
        normals = np.stack([np.where(hit, np.where(away, -n[:, c], n[:, c]), zero) for c in range(3)] + [np.zeros_like(t)], axis=-1).astype(np.float32)
        dirs = np.stack(d + [np.zeros_like(t)], axis=-1).astype(np.float32)
    for a in (positions, normals, dirs):
        a[~valid] = 0.0
    return positions, normals, dirs


def scatter(lst, values, out, state=None, state_word=RETRACED):
    """in place, as the header says: out[k] = values[j] for every entry k = lst[j] below len(out); the list must hold no index twice (which
    value wins is unspecified)"""
    k = np.asarray(lst, np.uint32).astype(np.int64)
    n = out.shape[0]
    ok = k < n
    assert len(np.unique(k[ok])) == ok.sum(), "the reference takes unique lists only"
    out[k[ok]] = np.asarray(values)[ok]
    if state is not None:
        state[k[ok]] = state_word
    return out, state
