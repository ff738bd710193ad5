"""Reference for the shaded ray queries (crt_shade_rays, include/crt_api.h).

Surface records are composed from closest-hit records: the first 36 bytes are gbuffer_ref.planes_from_records (the three G-buffer planes'
values), `material`, `texU`, `texV` are a restatement of kernel_main.cl:229 and 238-240 with the same pinned arithmetic. Two things pin the
restatement without a GPU (tests/test_shade_cpu.py): sampling the albedo again from a record's own (material, texU, texV) gives its `albedo`
field, and gbuffer_ref.shade_primary of the records is the oracle's primary-only frame.

Radiance is the C oracle's: Oracle.trace on a (1, m, 3) row of directions, one call per distinct origin. A bounded query is composed as
the API states it: the unbounded answer where the unbounded record's t < tmax, else the miss record and the radiance of the same
direction against no instance at all (pure sky)."""
import numpy as np

from clraytracer_amd import _lib
import gbuffer_ref
import oracle_lib
from test_shading_independent import F, fetch_texel, half, to_int

MISS = np.zeros(1, _lib.SURFACE_HIT_DTYPE)[0]
MISS["t"], MISS["instance"] = gbuffer_ref.MISS_T, -1
PIXEL_FIELDS = ("normal", "t", "instance", "tri", "u", "v", "albedo")
FIELDS = PIXEL_FIELDS + ("material", "texU", "texV")


def surface_from_records(a, rec):
    """one _lib.SURFACE_HIT_DTYPE per closest-hit record of `rec` (_lib.RAYHIT_DTYPE), from the scene arenas `a`"""
    g, ids, alb = gbuffer_ref.planes_from_records(a, rec)
    out = np.zeros(len(rec), _lib.SURFACE_HIT_DTYPE)
    out["normal"], out["t"] = g["normal"], g["t"]
    for k in ("instance", "tri", "u", "v"):
        out[k] = ids[k]
    out["albedo"] = alb
    shaded = np.flatnonzero((rec["instance"] >= 0) & ~(rec["t"] > gbuffer_ref.INF_MINUS_ONE))          # :219
    if len(shaded):
        hr = rec[shaded]
        inst = a["instances"][hr["instance"]]
        tri = a["tris"][hr["tri"]]
        out["material"][shaded] = np.minimum(inst["materialStart"].astype(np.int64) + tri["mat"].astype(np.int64), 255)     # :229
        uu, vv = hr["u"].astype(np.float32), hr["v"].astype(np.float32)
        bx, by, bz = (F(1.0) - uu) - vv, uu, vv                                                                          # :231
        uvh = half(tri["uv"])
        with np.errstate(all="ignore"):
            uv = (uvh[:, 0:2] * bx[:, None] + uvh[:, 2:4] * by[:, None]) + uvh[:, 4:6] * bz[:, None]                     # :238-240
        out["texU"][shaded], out["texV"][shaded] = uv[:, 0], uv[:, 1]
    return out


def resample_albedo(a, surf):
    """record.color (kernel_main.cl:242-245) of every record from its own material, texU, texV: SampleTexture, the texel, MultiplyColorU32"""
    mat = a["materials"][surf["material"]]
    tx = a["textures"][np.minimum(mat["albedo"].astype(np.int64), 31)]
    uv = np.stack([surf["texU"], surf["texV"]], 1).astype(np.float32)
    uvf = uv - np.floor(uv)                                                                                              # MathAndSTL.cl:262
    us = to_int(tx["width"].astype(np.float32) * uvf[:, 0])
    vs = to_int(tx["height"].astype(np.float32) * uvf[:, 1])
    texels = np.ascontiguousarray(a["texels"], np.uint8)
    pr, pg, pb = fetch_texel(texels, vs * tx["width"].astype(np.int64) + tx["offset"].astype(np.int64) + us)
    col = mat["color"].astype(np.uint32)
    cr = (((col & 0xff) * pr) >> 8) & 0xff
    cg = ((((col >> 8) & 0xff) * pg) >> 8) & 0xff
    cb = ((((col >> 16) & 0xff) * pb) >> 8) & 0xff
    return (np.uint32(0xFF000000) | (cb << 16) | (cg << 8) | cr).astype(np.uint32)


def planes_of(surf, h, w):
    """the records as the three planes of an h x w frame (what gbuffer_ref.shade_primary and crt_read_gbuffer speak)"""
    g = np.zeros(len(surf), _lib.GBUFFER_GEOMETRY_DTYPE)
    ids = np.zeros(len(surf), _lib.GBUFFER_IDS_DTYPE)
    g["normal"], g["t"] = surf["normal"], surf["t"]
    for k in ("instance", "tri", "u", "v"):
        ids[k] = surf[k]
    return {"geometry": g.reshape(h, w), "ids": ids.reshape(h, w), "albedo": np.ascontiguousarray(surf["albedo"]).reshape(h, w)}


def surface_of_planes(planes):
    """the first 36 bytes of the records a frame's planes are (material, texU, texV left 0)"""
    g, ids, alb = (np.ascontiguousarray(planes[k]).reshape(-1) for k in ("geometry", "ids", "albedo"))
    out = np.zeros(len(g), _lib.SURFACE_HIT_DTYPE)
    out["normal"], out["t"], out["albedo"] = g["normal"], g["t"], alb
    for k in ("instance", "tri", "u", "v"):
        out[k] = ids[k]
    return out


def same_surface(got, want, fields=FIELDS):
    """bit for bit, field by field"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and all(np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32))
                                           for k in fields)


def broadcast_rays(origins, dirs):
    o, d = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    n = max(len(o), len(d))
    return np.ascontiguousarray(np.broadcast_to(o, (n, 3))), np.ascontiguousarray(np.broadcast_to(d, (n, 3)))


def surface(a, orc, origins, dirs, tmax=None):
    """the records of crt_shade_rays for these rays: the oracle's closest hits, cut at tmax as the API composes it"""
    import trace_rays_ref
    o, d = broadcast_rays(origins, dirs)
    rec, _ = orc.closest_hits(o, d)
    return surface_from_records(a, trace_rays_ref.filtered(rec, tmax))


def radiance(orc, origins, dirs, sun_angle):
    """(n, 4) float32: the oracle's Trace (both bounces) of every ray, one Oracle.trace call per distinct origin"""
    o, d = broadcast_rays(origins, dirs)
    out = np.zeros((len(d), 4), np.float32)
    keys = np.ascontiguousarray(o).view(np.dtype((np.void, 12))).reshape(-1)
    for key in np.unique(keys):
        sel = np.flatnonzero(keys == key)
        img, _ = orc.trace(d[sel].reshape(1, -1, 3), o[sel[0]], sun_angle)
        out[sel] = img[0]
    return out


def sky_oracle(a, nthreads=None):
    """the oracle of the same scene without an instance: every ray ends in the sky (kernel_main.cl:219-223)"""
    b = dict(a)
    b["instances"] = np.ascontiguousarray(a["instances"][:0])
    return oracle_lib.Oracle(b, nthreads=nthreads)


def bounded_radiance(a, orc, origins, dirs, sun_angle, tmax, nthreads=None):
    """radiance under a bound: the unbounded radiance of the rays whose unbounded hit has t < tmax, the sky's for the rest"""
    o, d = broadcast_rays(origins, dirs)
    rec, _ = orc.closest_hits(o, d)
    with np.errstate(invalid="ignore"):
        kept = (rec["instance"] >= 0) & (rec["t"] < np.asarray(tmax, np.float32))
    out = radiance(sky_oracle(a, nthreads), o, d, sun_angle)
    if kept.any():
        out[kept] = radiance(orc, o[kept], d[kept], sun_angle)
    return out, kept
