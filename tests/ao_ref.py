"""Reference for ambient occlusion (crt_trace_ao / crt_frame_ao, include/crt_api.h): a numpy restatement of the definition -- the hash, the
sample rays of an item, the weighted reduction, the items of a G-buffer frame, the 5 x 5 filter -- in float32 arithmetic with the pinned
dot3 of tests/test_shading_independent.py. The direction table is taken from the library (crt_ao_directions), never recomputed.
What occludes a sample ray is not restated here: the tests take it from Session.trace_rays(mode="occluded") or from the C oracle's records."""
import ctypes as C

import numpy as np

from clraytracer_amd import _lib

F = np.float32
MISS_BEYOND = F(99998.0)                     # a G-buffer pixel with t > 99998 is a miss (a miss carries t = 99999 and a zero normal)


def table():
    """T[256, 3] float32 from the library"""
    out = np.zeros((256, 3), np.float32)
    _lib.check(_lib.hip().crt_ao_directions(out.ctypes.data_as(C.POINTER(C.c_float))), "crt_ao_directions")
    return out


def lowbias32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x


def dot3(a, b):                              # pinned: (a.x*b.x + a.y*b.y) + a.z*b.z, on the last axis
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def rays(P, n, k, params, table):
    """The sample rays of items (P[M, 3], n[M, 3], index k[M]) under params = {"samples", "bias", "seed"}: (o[M, 3], d[M, N, 3], w[M, N])"""
    P, n = np.ascontiguousarray(P, np.float32).reshape(-1, 3), np.ascontiguousarray(n, np.float32).reshape(-1, 3)
    N = int(params["samples"])
    with np.errstate(all="ignore"):
        seed_mul = np.uint32((int(params["seed"]) * 0x9E3779B9) & 0xFFFFFFFF)
        h = lowbias32(np.asarray(k, np.uint32) ^ seed_mul)
        o = P + n * F(params["bias"])
        s = np.arange(N, dtype=np.uint32)
        j = (h[:, None] + s[None, :] * np.uint32(256 // N)) & np.uint32(255)
        d = table[j].astype(np.float32)                                       # (M, N, 3)
        for c, bit in enumerate((8, 9, 10)):
            flip = ((h >> np.uint32(bit)) & np.uint32(1)).astype(bool)
            d[:, :, c] = np.where(flip[:, None], -d[:, :, c], d[:, :, c])
        back = dot3(d, n[:, None, :]) < F(0.0)
        d = np.where(back[:, :, None], -d, d)
        w = dot3(d, n[:, None, :]).astype(np.float32)
    return o, d, w


def compose(w, occ):
    """ao[M] from the weights w[M, N] and the occlusion answers occ[M, N] (bool or 0 / 1): num += w * occ; den += w in sample order"""
    w = np.asarray(w, np.float32)
    occ = np.asarray(occ).astype(np.float32)
    num, den = np.zeros(len(w), np.float32), np.zeros(len(w), np.float32)
    with np.errstate(all="ignore"):
        for s in range(w.shape[1]):
            num = num + w[:, s] * occ[:, s]
            den = den + w[:, s]
        return np.where(den > F(0.0), F(1.0) - num / den, F(1.0)).astype(np.float32)


def frame_items(planes, rays, cam_pos):
    """The items of a G-buffer frame, one per pixel in row-major order: (P[HW, 3], n[HW, 3], k[HW]) from its planes (Session.read_gbuffer),
    the frame's RayGen directions rays[H, W, 3] and the camera position. A miss pixel: the camera position with a zero normal."""
    g = planes["geometry"].reshape(-1)
    d = np.ascontiguousarray(rays, np.float32).reshape(-1, 3)
    cam = np.asarray(cam_pos, np.float32)
    with np.errstate(all="ignore"):
        t = g["t"].astype(np.float32)
        P = cam[None, :] + d * t[:, None]
        n = np.ascontiguousarray(g["normal"], np.float32)
        n = np.where((dot3(n, d) > F(0.0))[:, None], -n, n)
        miss = t > MISS_BEYOND
    P[miss] = cam
    n[miss] = 0.0
    return P.astype(np.float32), n.astype(np.float32), np.arange(len(g), dtype=np.uint32)


def filter5x5(ao, geometry, depthTol, normalCos):
    """CRT_AO_FILTER: ao[H, W] -> the filtered plane, guided by the GEOMETRY plane (t and the normal as stored)"""
    ao = np.asarray(ao, np.float32)
    H, W = ao.shape
    t = geometry["t"].astype(np.float32)
    nrm = np.ascontiguousarray(geometry["normal"], np.float32)
    hit = ~(t > MISS_BEYOND)
    pad = 2
    aoP = np.pad(ao, pad); tP = np.pad(t, pad); hitP = np.pad(hit, pad); nP = np.pad(nrm, ((pad, pad), (pad, pad), (0, 0)))
    inside = np.pad(np.ones((H, W), bool), pad)
    total, cnt = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                sl = (slice(pad + dy, pad + dy + H), slice(pad + dx, pad + dx + W))
                if dx == 0 and dy == 0:
                    m = np.ones((H, W), np.float32)
                else:
                    ok = hitP[sl] & (np.abs(tP[sl] - t) <= F(depthTol) * t) & (dot3(nP[sl], nrm) >= F(normalCos))
                    m = ok.astype(np.float32)
                here = inside[sl]                                             # the window is clipped to the frame
                total = np.where(here, total + aoP[sl] * m, total)
                cnt = np.where(here, cnt + m, cnt)
        return np.where(hit, total / cnt, F(1.0)).astype(np.float32)
