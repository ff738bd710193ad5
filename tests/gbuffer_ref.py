"""Expected values of the first-hit planes of a CRT_RENDER_GBUFFER frame (include/crt_api.h), composed from closest-hit records:
`ids` and `t` ARE the records (orc_closest_hits, or the session's own crt_query_hits); normal and albedo are a numpy restatement of
kernel_main.cl:226-245 -- attribute fetch, barycentric interpolation, SampleTexture, MultiplyColorU32 -- on those records, with the
pinned arithmetic tests/test_shading_independent.py uses (dot3, normalize, mat3_mul, half, to_int, fetch_texel).

`shade_primary` applies kernel_main.cl:261-267 to the planes (energy 1, the sun as light): tests/test_gbuffer_cpu.py requires the result
to equal the oracle's primary-only frame bit for bit, which pins the restatement without a GPU."""
import numpy as np

from clraytracer_amd import _lib
from test_shading_independent import F, dot3, fetch_texel, half, mat3_mul, mat_mul_xyz, normalize, reflect, to_int

MISS_T = np.float32(99999.0)              # CreateRayHit's distance (kernel_main.cl:189): what a ray without a hit ends with
INF_MINUS_ONE = np.float32(99998.0)       # kernel_main.cl:219: beyond it a pixel is sky


def planes_from_records(a, rec):
    """(geometry, ids, albedo), one element per record of `rec` (_lib.RAYHIT_DTYPE), from the scene arenas `a`"""
    n = len(rec)
    geometry = np.zeros(n, _lib.GBUFFER_GEOMETRY_DTYPE)
    ids = np.zeros(n, _lib.GBUFFER_IDS_DTYPE)
    albedo = np.zeros(n, np.uint32)
    geometry["t"] = rec["t"]
    ids["instance"], ids["tri"], ids["u"], ids["v"] = rec["instance"], rec["tri"], rec["u"], rec["v"]
    shaded = np.flatnonzero((rec["instance"] >= 0) & ~(rec["t"] > INF_MINUS_ONE))          # :219
    if len(shaded) == 0:
        return geometry, ids, albedo
    hr = rec[shaded]
    inst = a["instances"][hr["instance"]]
    m = np.ascontiguousarray(inst["inv"], np.float32)
    tri = a["tris"][hr["tri"]]
    mat = a["materials"][np.minimum(inst["materialStart"].astype(np.int64) + tri["mat"].astype(np.int64), 255)]     # :229
    uu, vv = hr["u"].astype(np.float32), hr["v"].astype(np.float32)
    bx, by, bz = (F(1.0) - uu) - vv, uu, vv                                                                          # :231
    nh = half(tri["n"])
    n0, n1, n2 = mat3_mul(m, nh[:, 0:3]), mat3_mul(m, nh[:, 3:6]), mat3_mul(m, nh[:, 6:9])                           # :233-235
    with np.errstate(all="ignore"):
        geometry["normal"][shaded] = normalize((n0 * bx[:, None] + n1 * by[:, None]) + n2 * bz[:, None])             # :236
    uvh = half(tri["uv"])
    uv = (uvh[:, 0:2] * bx[:, None] + uvh[:, 2:4] * by[:, None]) + uvh[:, 4:6] * bz[:, None]                         # :238-240
    tx = a["textures"][np.minimum(mat["albedo"].astype(np.int64), 31)]
    uvf = uv - np.floor(uv)                                                                                          # MathAndSTL.cl:262
    us = to_int(tx["width"].astype(np.float32) * uvf[:, 0])
    vs = to_int(tx["height"].astype(np.float32) * uvf[:, 1])
    texels = np.ascontiguousarray(a["texels"], np.uint8)
    pr, pg, pb = fetch_texel(texels, vs * tx["width"].astype(np.int64) + tx["offset"].astype(np.int64) + us)         # :242
    col = mat["color"].astype(np.uint32)
    cr = (((col & 0xff) * pr) >> 8) & 0xff                                                                           # MultiplyColorU32, :245
    cg = ((((col >> 8) & 0xff) * pg) >> 8) & 0xff
    cb = ((((col >> 16) & 0xff) * pb) >> 8) & 0xff
    albedo[shaded] = (np.uint32(0xFF000000) | (cb << 16) | (cg << 8) | cr).astype(np.uint32)
    return geometry, ids, albedo


def reference_planes(a, orc, rays, cam_pos):
    """The planes of a frame whose primary rays are `rays` (h, w, 3) from `cam_pos`, as {"geometry", "ids", "albedo"} (h, w) arrays"""
    h, w, _ = rays.shape
    d = np.ascontiguousarray(rays.reshape(-1, 3), np.float32)
    o = np.tile(np.asarray(cam_pos, np.float32), (len(d), 1))
    rec, _ = orc.closest_hits(o, d)
    g, i, c = planes_from_records(a, rec)
    return {"geometry": g.reshape(h, w), "ids": i.reshape(h, w), "albedo": c.reshape(h, w)}


def shade_primary(a, planes, rays, cam_pos, sun_angle):
    """kernel_main.cl:261-267 at bounce 0 from the planes alone: (rgb (h, w, 3), mask of shaded pixels)"""
    h, w, _ = rays.shape
    g, ids, alb = planes["geometry"].reshape(-1), planes["ids"].reshape(-1), planes["albedo"].reshape(-1)
    hit = np.flatnonzero((ids["instance"] >= 0) & ~(g["t"] > INF_MINUS_ONE))
    d = np.ascontiguousarray(rays.reshape(-1, 3), np.float32)[hit]
    m = np.ascontiguousarray(a["instances"][ids["instance"][hit]]["inv"], np.float32)
    md = mat_mul_xyz(m, d, 0.0)                                                                                      # meshRay.direction, :207
    normal = np.ascontiguousarray(g["normal"][hit], np.float32)
    u255 = F(1.0) / F(255.0)
    c = alb[hit]
    color = np.stack([c & 0xff, (c >> 8) & 0xff, (c >> 16) & 0xff], 1).astype(np.float32) * u255                     # UNPACK_RGB8
    sun = np.float32(sun_angle)
    L = np.tile(np.array([0.0, F(np.sin(np.float64(sun))), F(np.cos(np.float64(sun)))], np.float32), (len(hit), 1))  # :181
    atm = np.tile(np.array([0.255, 0.25, 0.27], np.float32) * F(1.0), (len(hit), 1))                                 # :185
    energy = np.ones((len(hit), 3), np.float32)
    ndl = dot3(normal, -L)                                                                                           # :261
    ambient = (np.fmax(F(0.0) - ndl, F(0.1))[:, None] * atm) * color                                                 # :262
    ndl = np.fmax(ndl, F(0.0))                                                                                       # :263
    spec_light = (ndl * np.fmax(dot3(reflect(-L, normal), md), F(0.0))) * F(0.2)                                     # :265
    out = np.zeros((h * w, 3), np.float32)
    out[hit] = out[hit] + ((energy * (color * ndl[:, None]) + ambient) + spec_light[:, None])                        # :267
    mask = np.zeros(h * w, bool)
    mask[hit] = True
    return out.reshape(h, w, 3), mask.reshape(h, w)
