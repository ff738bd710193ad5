"""Index-coded maps and edge-aimed views for the two texel lookups every frame ends in: SampleSkyboxPixel of a miss and SampleTexture
of a hit (MathAndSTL.cl:253-266). A coded map's texel bytes spell (texture tag, x, y), so a rendered miss pixel or an albedo word of
the G-buffer decodes to the exact texel the kernel read: index is compared with index, whether or not neighbouring texels of an
ordinary image would have differed. No tests in here: tests/test_texel_lookup_cpu.py and tests/test_gpu_texel_lookup.py use it.

    coded_map / decode_sky / decode_albedo   the encoding and its two readings
    view / FAMILIES                          invView matrices no camera produces (hazard H10): planar patches of ray directions aimed
                                             at the atan2 branch cut, the poles, the axes, and NaN / infinite / all-zero vectors
    to_int / sky_index                       the numpy restatement of the skybox index (moved here from tests/test_shading_independent.py,
                                             which imports it back)
    neighbour_indices / exact_rays           the only readings in which two correct math libraries may differ, and the rays that get none
    target_scene                             the textured target: two quads, three Kd = 1 materials with coded maps, UVs below 0 and above 1
"""
import os

import numpy as np

F = np.float32
WHITE, BLACK, NO_CODE = -1, -2, -3       # decode()'s tag for the two default texels (ResourceManager.cpp:168-177) and for bytes no coded map holds


# ------------------------------------------------------------------------------------------------
# the encoding: byte 0 = 1 + (x & 127), byte 1 = 1 + (y & 127), byte 2 = 1 + (tag << 3 | (x >> 7) << 1 | y >> 7)
# ------------------------------------------------------------------------------------------------
def coded_map(w, h, tag):
    """uint8 (h, w, 3), unambiguous up to 512 x 256 and tags 0..30. No byte is 0 (a Kd = 1 material maps a byte px to (255 * px) >> 8 =
    px - 1, so 0 and 1 would collide), bytes 0 and 1 stay below 130 (so neither default texel, white or black, is a code)."""
    assert 0 < w <= 512 and 0 < h <= 256 and 0 <= tag <= 30
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([1 + (x & 127), 1 + (y & 127), 1 + ((tag << 3) | ((x >> 7) << 1) | (y >> 7))], -1)
    assert img.min() >= 1 and img.max() <= 254
    return img.astype(np.uint8)


def decode(rgb_bytes):
    """(tag, x, y) int arrays of coded bytes (..., 3); tag WHITE / BLACK for the default texels, NO_CODE for anything else"""
    b = np.asarray(rgb_bytes).astype(np.int64)
    b0, b1, b2 = b[..., 0], b[..., 1], b[..., 2]
    ok = (b0 >= 1) & (b0 <= 128) & (b1 >= 1) & (b1 <= 128) & (b2 >= 1) & (b2 <= 254)
    hi = b2 - 1
    tag = np.where(ok, hi >> 3, NO_CODE)
    x = np.where(ok, (b0 - 1) | (((hi >> 1) & 3) << 7), 0)
    y = np.where(ok, (b1 - 1) | ((hi & 1) << 7), 0)
    tag = np.where((b0 == 255) & (b1 == 255) & (b2 == 255), WHITE, tag)
    tag = np.where((b0 == 0) & (b1 == 0) & (b2 == 0), BLACK, tag)
    return tag, x, y


def decode_sky(rgb):
    """The sky colour of a primary miss, float (..., 3): energy is 1 and the result starts at 0, so c = px * (1 / 255) and round(c * 255) = px"""
    c = np.asarray(rgb, np.float64)[..., :3]
    px = np.rint(c * 255.0)
    px = np.where(np.isfinite(px), px, -1)
    return decode(px)


def decode_albedo(words):
    """An albedo word of the G-buffer (0xFF000000 | b << 16 | g << 8 | r) behind a Kd = 1 material: MultiplyColorU32 made every byte
    (255 * px) >> 8 = px - 1 (MathAndSTL.cl:243-249). A word of 0 (a miss) decodes to NO_CODE."""
    w = np.asarray(words).astype(np.int64)
    rgb = np.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF], -1) + 1
    tag, x, y = decode(rgb)
    return np.where((w >> 24) == 0xFF, tag, NO_CODE), x, y


def decode_bytes(rgba8):
    """An RGBA8 frame (read_output_rgba8): the quantised sky colour is the texel byte itself"""
    return decode(np.asarray(rgba8)[..., :3])


# ------------------------------------------------------------------------------------------------
# views: with invProj = I the ray of pixel (i, j) is normalize(cx * A + cy * B + C + T), cx = 2i/W - 1, cy = 2j/H - 1 (kernel_main.cl:277-287)
# ------------------------------------------------------------------------------------------------
def view(A, B, C, T=(0.0, 0.0, 0.0), fill=0.0):
    """invView (16 floats, rows x, y, z, w of the row-vector convention) of one planar patch of directions; entries may be -0.0, `fill`
    (0.0 or -0.0) is what the unused entries of the first three columns hold"""
    m = np.full(16, fill, F)
    m[0:3], m[4:7], m[8:11], m[12:15] = A, B, C, T
    m[3] = m[7] = m[11] = 0.0
    m[15] = 1.0
    return m


IDENTITY = np.eye(4, dtype=F).reshape(16)
NZ = F(-0.0)
# A and B of length 0.25-0.75 around the aimed-at direction C (0.75 on the axis families: wide enough for 100 distinct texels of the 64 x 32
# sky as well; every cx * 0.75 is still exact). `seam`: every unused entry is -0.0, so in the column cx = 0 the x component is
# ((-0.5 * 0 + -0 * cy) + -0) + -0: -0 * cy is +0 in the rows with cy < 0 and -0 in the others, and (-0) + (+0) = +0 while (-0) + (-0) = -0 --
# half of that column has d.x == +0, half d.x == -0 (counted by the preconditions of tests/test_texel_lookup_cpu.py).
FAMILIES = {
    "seam": view((-0.5, NZ, NZ), (NZ, 0.5, NZ), (NZ, NZ, 1.0), (NZ, NZ, NZ), fill=NZ),
    "north": view((0.25, 0, 0), (0, 0, 0.25), (0, 1, 0)),
    "south": view((0.25, 0, 0), (0, 0, 0.25), (0, -1, 0)),
    "+x": view((0, 0, 0.75), (0, 0.75, 0), (1, 0, 0)),
    "-x": view((0, 0, 0.75), (0, 0.75, 0), (-1, 0, 0)),
    "-z": view((0.75, 0, 0), (0, 0.75, 0), (0, 0, -1)),
    # x = 1e30 * cx + 1e-30: the squared length overflows -> 1 / sqrt(inf) = 0 -> an all-zero vector, except in the column cx = 0, where it
    # underflows to 0 -> 1 / sqrt(0) = inf -> (inf, +-inf, inf), and (inf, 0 * inf = NaN, inf) in the row cy = 0. Only with numMeshes = 0.
    "degenerate": view((1e30, 0, 0), (0, 1e-30, 0), (0, 0, 1e-30), (1e-30, 0, 0)),
}
SKY_FAMILIES = ("seam", "north", "south", "+x", "-x", "-z", "degenerate")
SKY_SIZES = ((64, 32), (90, 37))         # W / 4 is no integer for 90
FRAME = 64                               # frames are 64 x 64


def family_view(name):
    """(invView, invProj, cameraPos) as Session.render_raw(view=...) takes it"""
    return FAMILIES[name], IDENTITY, np.zeros(3, F)


# ------------------------------------------------------------------------------------------------
# the skybox index (MathAndSTL.cl:253-258; textures[2], pool offset 2), restated in numpy
# ------------------------------------------------------------------------------------------------
def to_int(x):                                      # pinned: truncation, NaN -> 0, saturating
    x = np.asarray(x, np.float32)
    y = np.where(np.isnan(x), F(0), x)
    y = np.clip(y.astype(np.float64), -2147483648.0, 2147483647.0)
    return np.trunc(y).astype(np.int64)


def sky_angles(d):
    """(atan2pi(d.x, -d.z), acospi(d.y)) as float32: evaluated in double, divided by pi, narrowed (the pinned reading)"""
    d = np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        atan2pi = (np.arctan2(d[:, 0].astype(np.float64), (-d[:, 2]).astype(np.float64)) / np.pi).astype(np.float32)
        acospi = (np.arccos(d[:, 1].astype(np.float64)) / np.pi).astype(np.float32)
    return atan2pi, acospi


def index_of_angles(atan2pi, acospi, tw, th):
    with np.errstate(all="ignore"):
        theta = to_int((atan2pi * F(0.5)) * F(tw))
        phi = to_int(acospi * F(th))
    return theta, phi, phi * tw + (theta + 2)                                                                     # mad24(phi, width, theta + 2)


def sky_index(d, tw, th):
    """(theta, phi, index) of directions d (n, 3); the index is not clamped to the pool yet"""
    return index_of_angles(*sky_angles(d), tw, th)


def clamp_index(idx, num_texels):
    """texturePixels[idx] outside the pool is clamped (pinned)"""
    return np.clip(idx, 0, num_texels - 1)


def exact_rays(d):
    """Rays whose atan2 / acos arguments are special values at which every correct library returns the same float: a signed zero in d.x or
    d.z (the result is a multiple of pi / 2), d.y in {0, +-1}, and NaN / infinite / all-zero directions. They get no allowance."""
    d = np.asarray(d, np.float32)
    return (d[:, 0] == 0) | (d[:, 2] == 0) | (d[:, 1] == 0) | (np.abs(d[:, 1]) == 1) | ~np.isfinite(d).all(axis=1)


def neighbour_indices(d, tw, th):
    """(n, 9) indices: the float32 atan2pi and acospi values each kept or moved one float32 ulp either way. A double-precision atan2 or
    acos of a correct library is within an ulp of the true value in DOUBLE, so its float32 narrowing can only land on the float32 next to
    the pinned one -- and only when the true value lies within a double ulp of a rounding boundary. Nothing else is a legitimate reading."""
    at, ac = sky_angles(d)
    out = []
    for a in (at, np.nextafter(at, F(-np.inf)), np.nextafter(at, F(np.inf))):
        for c in (ac, np.nextafter(ac, F(-np.inf)), np.nextafter(ac, F(np.inf))):
            out.append(index_of_angles(a, c, tw, th)[2])
    return np.stack(out, 1)


def judge(got, want, d, tw, th, num_texels):
    """The rule of both sky tests for clamped indices `got` against the restatement's / the oracle's `want` on directions d:
    -> (differing rays, of which on exact-argument rays, of which not explained by neighbour_indices)"""
    diff = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if len(diff) == 0:
        return 0, 0, 0
    exact = exact_rays(d)[diff]
    near = clamp_index(neighbour_indices(d[diff], tw, th), num_texels)
    explained = (near == np.asarray(got)[diff][:, None]).any(axis=1)
    return len(diff), int(exact.sum()), int((~explained & ~exact).sum())


# ------------------------------------------------------------------------------------------------
# the textured target
# ------------------------------------------------------------------------------------------------
TARGET_MAPS = ((7, 5, 1), (1, 3, 2), (16, 4, 3))     # (width, height, tag) of material 0, 1, 2: none is a power-of-two square
SKY_TAG = 0
TINY_U = -1e-6                                       # see target_mesh


def target_mesh():
    """Two quads of two triangles, facing +z around z = -2 and tilted (a flat axis-aligned box is never entered: the slab test is strict),
    a little larger than the frame of TARGET_VIEW.
      quad A, x < 0: UV corners (-1.25, -1.25) .. (2.25, 2.25), all exact in half precision; triangles of material 0 (7 x 5) and 2 (16 x 4)
      quad B, x > 0: u = 0 at three corners -- exact integers: one triangle has u == 0 throughout -- and TINY_U at the fourth; v from
                     -1.25 to 2.25; material 1 (the 1 x 3 map)
    TINY_U: crth_write_obj prints `vt %.6f`, so nothing below 1e-6 in magnitude reaches the file (the smallest half subnormal, -2^-24,
    does not); -0.000001 does, and the importer's ConvertFloatToHalf keeps it as the subnormal -17 * 2^-24 (0x8011; 1e-6 * 2^24 = 16.78). u - floorf(u) == 1.0f then holds wherever that corner's weight is at most 1 / 34. (v cannot carry a subnormal at all: the
    importer stores 1 - v, and 1 + 2^-24 is no float.)"""
    from clraytracer_amd import scenes
    lo, hi = -1.0625, 1.0625

    def z(x, y):
        return -2.0 + 0.125 * x + 0.0625 * y
    corners = [(lo, lo), (0.0, lo), (0.0, hi), (lo, hi), (0.0, lo), (hi, lo), (hi, hi), (0.0, hi)]
    pos = np.array([(x, y, z(x, y)) for x, y in corners], np.float32)
    uv = np.array([(-1.25, -1.25), (2.25, -1.25), (2.25, 2.25), (-1.25, 2.25),
                   (0.0, -1.25), (0.0, -1.25), (TINY_U, 2.25), (0.0, 2.25)], np.float32)
    uv_obj = uv.copy()
    uv_obj[:, 1] = 1.0 - uv[:, 1]                    # the importer stores 1 - v (AssetManager.cpp:250)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (8, 1))
    tri = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 7], [5, 6, 7]], np.int32)
    mat = np.array([0, 2, 1, 1], np.int32)
    return scenes.Mesh(pos, uv_obj, nrm, tri, mat), uv


# No ray has d.x == 0: the quads meet in the plane x = 0, and a ray inside the plane of a box face fails the slab test (0 * inf = NaN).
TARGET_VIEW = (view((0.4375, 0, 0), (0, 0.4375, 0), (1.0 / 128.0, 0, -1.0)), IDENTITY, np.zeros(3, F))


def target_scene(dirpath, sky_size, maps=TARGET_MAPS, name="texel-target"):
    """The target with a coded sky of `sky_size` written into `dirpath` -> scenes.Scene. maps[k] = None: material k gets no map (albedo
    texture 0, the white default texel). Import order, hence pool order: white, black, sky (texture 2, texel offset 2), then the maps in
    material order."""
    from clraytracer_amd import scenes
    dirpath = str(dirpath)
    os.makedirs(dirpath, exist_ok=True)
    sky = os.path.join(dirpath, "sky.ppm")
    scenes.write_ppm(sky, coded_map(sky_size[0], sky_size[1], SKY_TAG))
    materials = []
    for k, m in enumerate(maps):
        if m is None:
            materials.append(((1.0, 1.0, 1.0), None))
            continue
        fname = "map%d.ppm" % k
        scenes.write_ppm(os.path.join(dirpath, fname), coded_map(*m))
        materials.append(((1.0, 1.0, 1.0), fname))
    mesh, _ = target_mesh()
    obj = scenes._write_mesh(dirpath, "target", mesh, materials)
    inst = [scenes.Instance(0, 0xFFFF, np.eye(4, dtype=np.float32))]
    return scenes.Scene(name, dirpath, sky, [obj], inst, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0))


POOL_END_MAPS = (TARGET_MAPS[0], TARGET_MAPS[1], None)


def interpolated_uv(a, rec):
    """(n, 2) float32 UVs of hit records `rec` in arenas `a`, with the arithmetic of gbuffer_ref.reference_planes: the halves of the
    triangle's corners widened, weighted (1 - u) - v, u, v and summed left to right. `uv - np.floor(uv)` is what SampleTexture scales."""
    from test_shading_independent import half
    tri = a["tris"][rec["tri"]]
    uu, vv = rec["u"].astype(np.float32), rec["v"].astype(np.float32)
    bx = (F(1.0) - uu) - vv
    uvh = half(tri["uv"])
    return (uvh[:, 0:2] * bx[:, None] + uvh[:, 2:4] * uu[:, None]) + uvh[:, 4:6] * vv[:, None]


def pool_layout(a):
    """[(tag, offset, width, height)] of the coded textures of arenas `a` in pool order (texture 2 = the sky first)"""
    out = []
    texels = np.ascontiguousarray(a["texels"], np.uint8)
    for t in a["textures"][2:int(a["num_textures"])]:
        tag = int(decode(texels[3 * int(t["offset"]):3 * int(t["offset"]) + 3])[0])
        out.append((tag, int(t["offset"]), int(t["width"]), int(t["height"])))
    return out


def texel_of_index(a, idx):
    """(tag, x, y) a clamped pool index decodes to, through the pool's own bytes"""
    texels = np.ascontiguousarray(a["texels"], np.uint8).reshape(-1, 3)
    return decode(texels[np.asarray(idx)])
