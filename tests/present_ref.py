"""Restatement of include/crt_present.h for the tests. Steps 1-3 of crtp_present (heal, the AO factor, the exposure) and every mode of crtp_view
are numpy float32, one rounding per operation as the header orders them (np.rint is the ties-to-even of rintf). Steps 4-8 -- the RGBA8 store
and load, FXAA, PostProcess, the packed bytes -- are the oracle's own functions (orc_quantize_unorm8, orc_fxaa, orc_postprocess,
orc_pack_unorm8), which already define the frame's stages: the reference of the chain's last step is the reference of the frame."""
import numpy as np

import oracle_lib

UNORM8, POST, FXAA, HEAL = 1, 2, 4, 8
NORMAL, DEPTH, INSTANCE, TRIANGLE, ALBEDO, SCALAR, STATE = range(7)
MODES = {"normal": NORMAL, "depth": DEPTH, "instance": INSTANCE, "triangle": TRIANGLE, "albedo": ALBEDO, "scalar": SCALAR, "state": STATE}
MAGENTA = (255, 0, 255)
PALETTE = {0: (32, 32, 32), 1: (255, 160, 0), 2: (255, 0, 0), 3: (0, 200, 80)}
F = np.float32


def _orc(name, img, *extra):
    img = np.ascontiguousarray(img, np.float32).copy()
    h, w, _ = img.shape
    getattr(oracle_lib.lib(), name)(img.ctypes.data, *extra, w, h, 0, h)
    return img


def quantize(img):
    return _orc("orc_quantize_unorm8", img)


def postprocess(img):
    return _orc("orc_postprocess", img)


def fxaa(img):
    return oracle_lib.fxaa(img)


def pack(img):
    img = np.ascontiguousarray(img, np.float32)
    h, w, _ = img.shape
    out = np.zeros((h, w, 4), np.uint8)
    oracle_lib.lib().orc_pack_unorm8(img.ctypes.data, out.ctypes.data, w, h, 0, h)
    return out


def compose(color, flags=0, ao=None, ao_strength=1.0, exposure=1.0):
    """steps 1-3: the (H, W, 4) float32 image, alpha 1, that step 4 takes"""
    c = np.ascontiguousarray(color, np.float32)[..., :3].copy()
    with np.errstate(all="ignore"):
        if flags & HEAL:
            c[~np.isfinite(c)] = F(0)
        if ao is not None:
            s = F(ao_strength)
            f = (F(1) - s) + s * np.ascontiguousarray(ao, np.float32)
            if flags & HEAL:
                f = np.where(np.isfinite(f), f, F(1)).astype(np.float32)
            c = c * f[..., None]
        if F(exposure) != F(1):
            c = c * F(exposure)
    return np.concatenate([c.astype(np.float32), np.ones(c.shape[:2] + (1,), np.float32)], axis=-1)


def source(color, flags=0, ao=None, ao_strength=1.0, exposure=1.0):
    """steps 1-4: the image S the filter reads"""
    img = compose(color, flags, ao, ao_strength, exposure)
    return quantize(img) if flags & UNORM8 else img


def present(color, flags=0, ao=None, ao_strength=1.0, exposure=1.0):
    """(outColor (H, W, 4) float32, outBytes (H, W, 4) uint8) of crtp_present"""
    img = source(color, flags, ao, ao_strength, exposure)
    if flags & FXAA:
        img = fxaa(img)
    if flags & POST:
        img = postprocess(img)
    if (flags & UNORM8) and (flags & (POST | FXAA)):
        img = quantize(img)
    img[..., 3] = F(1)
    return img, pack(img)


def frame_chain(frame, flags):
    """what tests/test_gpu_flag_matrix.py composes for crt_render's POSTPROCESS / UNORM8 / FXAA on the plain frame: the oracle's own chain"""
    want = np.ascontiguousarray(frame, np.float32).copy()
    if flags & UNORM8:
        want = quantize(want)
    if flags & FXAA:
        want = fxaa(want)
    if flags & POST:
        want = postprocess(want)
    if (flags & UNORM8) and (flags & (POST | FXAA)):
        want = quantize(want)
    return want


# ---- inputs the CPU and the GPU tests share ----------------------------------------------------------------------------------------------------
def fxaa_patterns(W, H):
    """LDR images that drive the filter to its +-8 clamp and to the edge clamps on all four sides: a checkerboard, bright pixels in the four
    corners on black, a vertical and a horizontal step edge (the CPU and the GPU tests run the same)."""
    yy, xx = np.mgrid[0:H, 0:W]
    images = {}
    img = np.zeros((H, W, 4), np.float32)
    img[..., :3] = (((xx + yy) & 1) * 0.8 + 0.1)[..., None]
    images["checkerboard"] = img
    img = np.zeros((H, W, 4), np.float32)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        img[y, x, :3] = (1.0, 0.9, 0.8)
    images["corners"] = img
    img = np.zeros((H, W, 4), np.float32)
    img[:, W // 2:, :3] = (0.9, 0.6, 0.3)
    img[..., :3] += 0.05
    images["vertical edge"] = img
    img = np.zeros((H, W, 4), np.float32)
    img[H // 2:, :, :3] = (0.2, 0.7, 1.0)
    images["horizontal edge"] = img
    return images


# ---- crtp_view ----------------------------------------------------------------------------------------------------------------------------------
def unorm8(v):
    with np.errstate(all="ignore"):
        u = np.asarray(v, np.float32) * F(255)
        r = np.rint(np.where(np.isnan(u), F(0), np.clip(u, F(0), F(255))))
    return r.astype(np.uint32)


def hash32(h):
    h = np.asarray(h, np.uint64) & 0xFFFFFFFF
    h = (h * 0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h.astype(np.uint32)


def _word_rgb(w):
    return np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], axis=-1).astype(np.uint8)


def view(mode, *, normal=None, t=None, instance=None, tri=None, albedo=None, plane=None, scale=10.0, lo=0.0, hi=1.0):
    """(outColor (H, W, 4) float32, outBytes (H, W, 4) uint8) of crtp_view; normal (H, W, 3), t (H, W), instance int32, tri uint32, albedo
    uint32, plane float32 or uint32/int32"""
    mode = MODES.get(mode, mode)
    with np.errstate(all="ignore"):
        if mode == NORMAL:
            hit = np.asarray(t, np.float32) <= F(99998.0)
            rgb = unorm8(np.asarray(normal, np.float32) * F(0.5) + F(0.5)).astype(np.uint8)
            rgb[~hit] = 0
        elif mode == DEPTH:
            t = np.asarray(t, np.float32)
            hit = t <= F(99998.0)
            g = unorm8(F(scale) / (t + F(scale))).astype(np.uint8)
            rgb = np.repeat(g[..., None], 3, axis=-1)
            rgb[~hit] = 0
        elif mode in (INSTANCE, TRIANGLE):
            inst = np.asarray(instance, np.int32)
            key = inst.astype(np.int64).astype(np.uint64) & 0xFFFFFFFF
            if mode == TRIANGLE:
                key = ((key * 0x9E3779B1) & 0xFFFFFFFF) + (np.asarray(tri).astype(np.uint64) & 0xFFFFFFFF)
            rgb = _word_rgb(hash32(key))
            rgb[inst < 0] = 0
        elif mode == ALBEDO:
            rgb = _word_rgb(np.asarray(albedo, np.uint32))
        elif mode == SCALAR:
            v = np.asarray(plane, np.float32)
            g = unorm8((v - F(lo)) / (F(hi) - F(lo))).astype(np.uint8)
            rgb = np.repeat(g[..., None], 3, axis=-1)
            rgb[np.isnan(v)] = MAGENTA
        else:
            s = np.asarray(plane).astype(np.int64) & 0xFFFFFFFF
            rgb = np.empty(s.shape + (3,), np.uint8)
            rgb[...] = MAGENTA
            for word, colour in PALETTE.items():
                rgb[s == word] = colour
    out = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=-1)
    return (out.astype(np.float32) / F(255.0)).astype(np.float32), out
