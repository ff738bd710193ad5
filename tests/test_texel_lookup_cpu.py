"""The two texel lookups at their edges, without a GPU: what tests/test_gpu_texel_lookup.py compares the kernels with is pinned here.

  * the preconditions: the direction families of tests/texel_ref.py do reach the atan2 branch cut with both signed zeros, the poles, the
    axes, indices below 0 and past the sky's last row, NaN / infinite / all-zero directions -- counted on orc.raygen, not hoped for;
    the textured target does produce negative UVs, `u - floorf(u) == 1.0f` and a lookup that lands in another texture
  * the oracle (orc_sample_skybox + the clamp, glibc) against the numpy restatement (texel_ref.sky_index) on every family: a differing
    ray is accepted only if it is no exact-argument ray and the oracle's index is one of texel_ref.neighbour_indices, at most 2 a family
  * the evidence that the coded maps do their job: five mutated readings of the index, each of which changes decoded indices on the coded
    sky, and what the gradient sky of scenes._skybox shows of them
  * CPU_RayCast (its own polynomial atan2 / acos): the host mirror against the oracle, bit for bit, on the same directions
  * albedo: gbuffer_ref.reference_planes against the oracle's SampleTexture and its primary-only frame, through decode, no allowance

Measured here (numpy 1.x arctan2 / arccos against glibc, 64 x 64 rays a family): 0 differing indices on every family and both skies.

The signed-zero mutation is not invisible on the gradient sky: the 32 rays with d.x == -0 move from column W/2 of one row to column W/2
of the row above, and the gradient's rows differ -- 32 pixels change, by at most 10/255 (64 x 32) and 8/255 (90 x 37). What hides that
reading from the frame tests is that no camera of theirs looks along +z, not the gradient. The test asserts that no ray other than those
32 changes, each by no more than vertically adjacent texels of the gradient differ, while the coded sky decodes a different index for all
32. The phi-clamp mutation touches at most 2 pixels of the gradient sky."""
import ctypes as C

import numpy as np
import pytest

from clraytracer_amd import driver, scenes
import gbuffer_ref
import oracle_lib
import texel_ref as T
from test_shading_independent import half
from util import bits

F = np.float32
N = T.FRAME
ORC_EXT_PRIMARY_ONLY = 4                  # oracle/crt_oracle.h


def load_arenas(sc):
    """The arenas of scene `sc` through a host-only session (copies: the session is closed again)"""
    with driver.Session(N, N, host_only=True) as s:
        s.load_scene(sc)
        return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}


@pytest.fixture(scope="module")
def world(tmp_path_factory, nthreads):
    """{sky size or "pool-end": (arenas, oracle)} of the textured target; one raygen per family (the rays do not depend on the scene)"""
    w = {}
    for sky in T.SKY_SIZES:
        a = load_arenas(T.target_scene(tmp_path_factory.mktemp("sky%d" % sky[0]), sky))
        w[sky] = (a, oracle_lib.Oracle(a, nthreads=nthreads))
    a = load_arenas(T.target_scene(tmp_path_factory.mktemp("poolend"), (90, 37), maps=T.POOL_END_MAPS))
    w["pool-end"] = (a, oracle_lib.Oracle(a, nthreads=nthreads))
    orc = w[(90, 37)][1]
    w["rays"] = {f: orc.raygen(N, N, *T.family_view(f)[:2]).reshape(-1, 3) for f in T.SKY_FAMILIES}
    w["target_rays"] = orc.raygen(N, N, *T.TARGET_VIEW[:2])
    return w


def oracle_sky_index(a, rays):
    tex = np.ascontiguousarray(a["textures"][2:3])
    L = oracle_lib.lib()
    return np.array([L.orc_sample_skybox(oracle_lib.f32(r)[0], tex.ctypes.data) for r in rays], np.int64)


def num_texels(a):
    return (len(a["texels"]) + 2) // 3


# ------------------------------------------------------------------------------------------------
# the fixture itself
# ------------------------------------------------------------------------------------------------
def test_coded_maps_decode_to_their_own_index():
    for w, h, tag in ((512, 256, 30), (90, 37, 0), (7, 5, 1), (1, 3, 2), (16, 4, 3)):
        img = T.coded_map(w, h, tag)
        assert img.dtype == np.uint8 and img.shape == (h, w, 3) and img.min() >= 1
        y, x = np.mgrid[0:h, 0:w]
        for got in (T.decode(img), T.decode_sky(img.astype(np.float32) * (F(1.0) / F(255.0))), T.decode_bytes(np.dstack([img, img[..., :1]]))):
            assert (got[0] == tag).all() and np.array_equal(got[1], x) and np.array_equal(got[2], y)
        # behind a Kd = 1 material every byte is (255 * px) >> 8 = px - 1
        m = (255 * img.astype(np.uint32)) >> 8
        word = np.uint32(0xFF000000) | (m[..., 2] << 16) | (m[..., 1] << 8) | m[..., 0]
        got = T.decode_albedo(word)
        assert (got[0] == tag).all() and np.array_equal(got[1], x) and np.array_equal(got[2], y)
    assert len(np.unique(T.coded_map(512, 256, 7).reshape(-1, 3), axis=0)) == 512 * 256
    assert T.decode(np.array([[255, 255, 255], [0, 0, 0], [200, 3, 3]]))[0].tolist() == [T.WHITE, T.BLACK, T.NO_CODE]
    assert T.decode_albedo(np.array([0, 0xFFFEFEFE], np.uint32))[0].tolist() == [T.NO_CODE, T.WHITE]


def test_the_pool_is_the_one_the_tests_assume(world):
    for sky in T.SKY_SIZES:
        a = world[sky][0]
        assert T.pool_layout(a) == [(T.SKY_TAG, 2, sky[0], sky[1]), (1, 2 + sky[0] * sky[1], 7, 5), (2, 37 + sky[0] * sky[1], 1, 3), (3, 40 + sky[0] * sky[1], 16, 4)]
        assert num_texels(a) == 2 + sky[0] * sky[1] + 35 + 3 + 64
        assert a["texels"][:6].tolist() == [255, 255, 255, 0, 0, 0]
        assert (a["materials"]["color"][1:4] & 0xFFFFFF == 0xFFFFFF).all() and a["materials"]["albedo"][1:4].tolist() == [3, 4, 5]
    a = world["pool-end"][0]
    assert T.pool_layout(a) == [(T.SKY_TAG, 2, 90, 37), (1, 3332, 7, 5), (2, 3367, 1, 3)] and num_texels(a) == 3370
    assert a["materials"]["albedo"][1:4].tolist() == [3, 4, 0]


@pytest.mark.parametrize("sky", T.SKY_SIZES)
def test_families_reach_the_edges(world, sky):
    W, H = sky
    a, _ = world[sky]
    n = num_texels(a)
    R = world["rays"]
    idx = {f: T.sky_index(R[f], W, H) for f in T.SKY_FAMILIES}
    # seam: both signed zeros in d.x, in front of +z, theta at both ends
    d = R["seam"]
    pz, nz = (d[:, 0] == 0) & ~np.signbit(d[:, 0]), (d[:, 0] == 0) & np.signbit(d[:, 0])
    assert pz.sum() >= 16 and nz.sum() >= 16, (int(pz.sum()), int(nz.sum()))
    assert (d[pz | nz, 2] > 0).all()
    th = idx["seam"][0]
    assert (th[pz] == W // 2).all() and (th[nz] == -(W // 2)).all() and th.max() == W // 2 and th.min() == -(W // 2)
    # north: the pole itself, and indices below 0 (clamped to texel 0, the white default texel)
    d = R["north"]
    assert (d[:, 1] == 1).sum() == 1 and d[(N // 2) * N + N // 2].tolist() == [0.0, 1.0, 0.0]
    below = idx["north"][2] < 0
    assert below.sum() >= 100, int(below.sum())
    assert (T.texel_of_index(a, T.clamp_index(idx["north"][2], n))[0][below] == T.WHITE).all()
    # south: the pole, phi == H: past the sky's last row
    d = R["south"]
    pole = np.flatnonzero(d[:, 1] == -1)
    assert len(pole) == 1 and idx["south"][1][pole[0]] == H and idx["south"][2][pole[0]] == H * W + W // 2 + 2 >= 2 + W * H
    assert (idx["south"][2] >= 2 + W * H).sum() == 1
    # the axes: the centre ray is the axis, its theta the truncated quarter turn
    c = (N // 2) * N + N // 2
    for f, axis, theta in (("+x", [1, 0, 0], int(0.25 * W)), ("-x", [-1, 0, 0], -int(0.25 * W)), ("-z", [0, 0, -1], 0)):
        assert R[f][c].tolist() == [float(v) for v in axis], (f, R[f][c])
        assert idx[f][0][c] == theta and idx[f][1][c] == int(0.5 * H), (f, idx[f][0][c], idx[f][1][c])
    # degenerate: NaN, infinite and all-zero vectors
    d = R["degenerate"]
    has_nan, has_inf, zero = np.isnan(d).any(axis=1), np.isinf(d).any(axis=1), (d == 0).all(axis=1)
    assert has_nan.sum() >= 1 and (has_inf & ~has_nan).sum() >= 32 and zero.sum() >= 1000 and (has_nan | has_inf | zero).all()
    assert {bool(s) for s in np.signbit(d[zero, 0])} == {True, False}
    # every family reads many different texels
    for f in T.SKY_FAMILIES[:-1]:
        distinct = len(np.unique(T.clamp_index(idx[f][2], n)))
        print(f"{f} on {W}x{H}: {distinct} distinct indices")
        assert distinct >= 100, (f, distinct)
    assert T.exact_rays(R["degenerate"]).all() and T.exact_rays(R["seam"])[pz | nz].all()
    assert T.exact_rays(R["south"])[pole[0]] and T.exact_rays(R["+x"])[c] and not T.exact_rays(R["+x"])[0]


# ------------------------------------------------------------------------------------------------
# the oracle against the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sky", T.SKY_SIZES)
def test_oracle_sky_index_against_the_restatement(world, sky):
    W, H = sky
    a, orc = world[sky]
    n = num_texels(a)
    for f in T.SKY_FAMILIES:
        d = world["rays"][f]
        want = T.clamp_index(T.sky_index(d, W, H)[2], n)
        got = T.clamp_index(oracle_sky_index(a, d), n)
        differing, on_exact, unexplained = T.judge(got, want, d, W, H, n)
        print(f"{f} on {W}x{H}: oracle vs numpy: {differing} differing indices ({on_exact} on exact-argument rays, {unexplained} unexplained)")
        assert on_exact == 0 and unexplained == 0 and differing <= 2, (f, differing, on_exact, unexplained)
        # ... and the oracle's frame of these rays (empty scene) decodes to the same texels
        orc.s.numInstances = 0
        try:
            frame, st = orc.trace(d.reshape(N, N, 3), (0.0, 0.0, 0.0), -1.96)
        finally:
            orc.s.numInstances = len(a["instances"])
        assert st["misses"] == N * N and st["traversals"] == 0 and (frame[..., 3] == 1.0).all()
        tag, x, y = T.decode_sky(frame.reshape(-1, 4))
        wt, wx, wy = T.texel_of_index(a, got)
        assert np.array_equal(tag, wt) and np.array_equal(x, wx) and np.array_equal(y, wy), f


def test_pool_end_clamps_to_the_last_texel(world):
    """The kernel reads the sky at pool offset 2 whatever textures[2].offset says (hazard H9), and Session.load_scene imports it first, so the
    sky cannot literally be the last import. The pool-end variant has the same effect: only 38 texels follow the 90 x 37 sky (no map on the
    last material), fewer than the W / 2 = 45 the south pole's index lies past the sky -- it exceeds numTexels and is clamped to the last texel."""
    a, orc = world["pool-end"]
    n = num_texels(a)
    d = world["rays"]["south"]
    idx = oracle_sky_index(a, d)
    pole = int(np.flatnonzero(d[:, 1] == -1)[0])
    assert idx[pole] == 37 * 90 + 45 + 2 >= n and (idx >= n).sum() == 1
    assert np.array_equal(idx, T.sky_index(d, 90, 37)[2])
    orc.s.numInstances = 0
    try:
        frame, _ = orc.trace(d.reshape(N, N, 3), (0.0, 0.0, 0.0), -1.96)
    finally:
        orc.s.numInstances = len(a["instances"])
    tag, x, y = T.decode_sky(frame.reshape(-1, 4))
    assert (int(tag[pole]), int(x[pole]), int(y[pole])) == (2, 0, 2)          # the last texel of the 1 x 3 map
    assert (tag[np.arange(len(d)) != pole] == T.SKY_TAG).all()


# ------------------------------------------------------------------------------------------------
# proof that the fixture does its job
# ------------------------------------------------------------------------------------------------
def mutated_index(d, W, H, n, mode):
    """The clamped pool index under one wrong reading"""
    at, ac = T.sky_angles(d)
    with np.errstate(all="ignore"):
        a, b = (at * F(0.5)) * F(W), ac * F(H)
    if mode == "floor":                                   # truncation replaced by floor
        theta, phi = T.to_int(np.floor(a)), T.to_int(np.floor(b))
    elif mode == "no-signed-zero":                        # -0 treated as +0
        x = np.where(d[:, 0] == 0, F(0.0), d[:, 0])
        return mutated_index(np.stack([x, d[:, 1], d[:, 2]], 1), W, H, n, "none")
    else:
        theta, phi = T.to_int(a), T.to_int(b)
    if mode == "wrap":                                    # negative theta wrapped by + W
        theta = np.where(theta < 0, theta + W, theta)
    if mode == "phi-clamp":                               # phi clamped to H - 1
        phi = np.minimum(phi, H - 1)
    idx = phi * W + (theta + 2)
    if mode == "mod":                                     # the clamp of negative indices removed
        return np.mod(idx, n)
    return T.clamp_index(idx, n)


MUTATIONS = {"floor": "-x", "no-signed-zero": "seam", "wrap": "-x", "phi-clamp": "south", "mod": "north"}   # and the family each is aimed at


@pytest.mark.parametrize("sky", T.SKY_SIZES)
def test_coded_sky_sees_what_the_gradient_sky_hides(world, sky):
    W, H = sky
    a, _ = world[sky]
    n = num_texels(a)
    coded = np.ascontiguousarray(a["texels"], np.uint8).reshape(-1, 3)
    gradient = coded.copy()
    gradient[2:2 + W * H] = scenes._skybox(W, H).reshape(-1, 3)

    def changed(pool, d, mode):
        """pixels of the frame shaded from `pool` that differ between the pinned and the mutated reading, and the largest byte difference"""
        ref, mut = pool[mutated_index(d, W, H, n, "none")].astype(int), pool[mutated_index(d, W, H, n, mode)].astype(int)
        return (ref != mut).any(axis=1), int(np.abs(ref - mut).max())

    for mode, family in MUTATIONS.items():
        d = world["rays"][family]
        on_coded, _ = changed(coded, d, mode)
        index_changed = mutated_index(d, W, H, n, "none") != mutated_index(d, W, H, n, mode)
        on_gradient, step = changed(gradient, d, mode)
        print(f"{mode} on {family}, {W}x{H}: {int(index_changed.sum())} indices change; decoded on the coded sky: {int(on_coded.sum())}; "
              f"colour on the gradient sky: {int(on_gradient.sum())} (at most {step}/255)")
        assert index_changed.sum() >= 1 and np.array_equal(on_coded, index_changed), mode     # the coded sky shows every changed index
        if mode == "phi-clamp":
            assert on_gradient.sum() <= 2
        if mode == "no-signed-zero":
            neg_zero = (d[:, 0] == 0) & np.signbit(d[:, 0])
            assert np.array_equal(index_changed, neg_zero) and neg_zero.sum() >= 16
            # see the module docstring: on those rays and no others, by no more than two vertically adjacent texels of the gradient differ
            row_step = int(np.abs(np.diff(scenes._skybox(W, H).astype(int), axis=0)).max())
            assert not on_gradient[~neg_zero].any() and step <= row_step, (step, row_step)


# ------------------------------------------------------------------------------------------------
# CPU_RayCast: the mirror against the oracle
# ------------------------------------------------------------------------------------------------
def test_cpu_raycast_mirror_on_the_families(world, tmp_path, nthreads):
    """CPURayTrace.cpp:217-224 reads the sky through polynomial ATan2 / ACos (Math.hpp:53-90; oracle/crt_oracle.c ref_atan2 / ref_acos): the
    host mirror and the oracle are both C on one libm, so every record is equal bit for bit -- NaN, infinite and all-zero directions included."""
    sc = T.target_scene(tmp_path, (90, 37))
    sc.instances = []
    with driver.Session(N, N, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        assert len(a["instances"]) == 0
        orc = oracle_lib.Oracle(a, nthreads=nthreads)
        for f in T.SKY_FAMILIES:
            d = world["rays"][f]
            o = np.zeros_like(d)
            got, ref = s.cpu_raycast(o, d, nthreads=nthreads), orc.cpu_raycast(o, d)
            assert got.tobytes() == ref.tobytes(), f
            assert (ref["distance"] == F(1e30)).all()
            c = ref["color"]
            tag, x, y = T.decode(np.stack([c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF], 1))
            assert (tag != T.NO_CODE).all(), f                                          # every colour is a texel of the pool (index 1 is the black one)
            if f != "degenerate":
                assert len(np.unique(c)) >= 100, (f, len(np.unique(c)))


# ------------------------------------------------------------------------------------------------
# the textured target
# ------------------------------------------------------------------------------------------------
def target_samples(a, orc, rays):
    """(records, material slot, interpolated uv, uv - floor(uv)) of the target's primary rays, with gbuffer_ref's arithmetic"""
    d = np.ascontiguousarray(rays.reshape(-1, 3), np.float32)
    rec, _ = orc.closest_hits(np.zeros_like(d), d)
    uv = T.interpolated_uv(a, rec)
    return rec, a["tris"][rec["tri"]]["mat"].astype(int), uv, uv - np.floor(uv)


def test_target_reaches_the_edges_of_sample_texture(world):
    a, orc = world[(90, 37)]
    # the arenas after import: every UV is the half the mesh names; the tiny one is the subnormal -17 * 2^-24 (texel_ref.target_mesh)
    stored = set(int(h) for h in a["tris"]["uv"].reshape(-1))
    assert stored == {0xBD00, 0x4080, 0x0000, 0x8011}, [hex(h) for h in stored]
    assert half(np.array([0x8011], np.uint16))[0] == F(-17.0 * 2.0 ** -24) and half(np.array([0xBD00, 0x4080], np.uint16)).tolist() == [-1.25, 2.25]
    rec, mat, uv, uvf = target_samples(a, orc, world["target_rays"])
    assert (rec["instance"] == 0).all()                                   # the target fills the frame
    assert (uv[:, 0] < 0).sum() >= 50 and (uv[:, 1] < 0).sum() >= 50
    assert uv.min() < -0.8 and uv.max() > 1.9 and (uv[:, 0] == 0).sum() >= 50          # exact integers: u == 0 on one whole triangle
    spill = uvf[:, 0] == F(1.0)
    assert spill.sum() >= 1 and (uv[spill, 0] < 0).all() and (mat[spill] == 1).all()   # uS == width, on the 1 x 3 map
    assert len(np.unique(mat)) == 3 and np.bincount(mat).min() >= 500
    planes = gbuffer_ref.reference_planes(a, orc, world["target_rays"], T.TARGET_VIEW[2])
    tag, x, y = T.decode_albedo(planes["albedo"].reshape(-1))
    named = np.array([m[2] for m in T.TARGET_MAPS])[mat]
    elsewhere = tag != named
    print(f"target: {int((uv[:, 0] < 0).sum())} samples with u < 0, {int((uv[:, 1] < 0).sum())} with v < 0, {int(spill.sum())} with uS == width, "
          f"{int(elsewhere.sum())} read from another texture than their material names")
    assert elsewhere.sum() >= 1 and (tag[elsewhere] == 3).all() and (x[elsewhere] == 0).all() and (y[elsewhere] == 0).all()
    assert (spill[elsewhere]).all()                                       # ... the spill out of the last row of the 1 x 3 map
    assert (tag >= 1).all()


@pytest.mark.parametrize("which", [(64, 32), (90, 37), "pool-end"])
def test_albedo_oracle_against_the_restatement(world, which, nthreads):
    a, orc = world[which]
    rays = world["target_rays"]
    pos = T.TARGET_VIEW[2]
    planes = gbuffer_ref.reference_planes(a, orc, rays, pos)
    rec, mat, uv, uvf = target_samples(a, orc, rays)
    # the oracle's SampleTexture (floorf, f2i, the unsigned index sum) + the clamp, through the pool's own bytes
    L = oracle_lib.lib()
    n = num_texels(a)
    mats = a["materials"][a["instances"]["materialStart"][0] + mat]
    tex = np.ascontiguousarray(a["textures"])
    idx = np.array([L.orc_sample_texture(tex[int(t):int(t) + 1].ctypes.data, float(u), float(v)) for t, (u, v) in zip(mats["albedo"], uv)], np.int64)
    want = T.texel_of_index(a, T.clamp_index(idx, n))
    got = T.decode_albedo(planes["albedo"].reshape(-1))
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)
    if which == "pool-end":
        last_row_spill = (mat == 1) & (uvf[:, 0] == F(1.0)) & (T.to_int(F(3.0) * uvf[:, 1]) == 2)
        assert last_row_spill.sum() >= 1 and (idx[last_row_spill] == n).all()          # one past the pool: clamped to the last texel
        assert (got[0][last_row_spill] == 2).all() and (got[2][last_row_spill] == 2).all()
        assert (got[0][mat == 2] == T.WHITE).all()                                      # no map: the white default texel
    # ... and the whole of bounce 0: shading the reference planes gives the oracle's primary-only frame, bit for bit
    shaded, mask = gbuffer_ref.shade_primary(a, planes, rays, pos, -1.96)
    ref = np.zeros((N, N, 4), np.float32)
    args = oracle_lib.CrtTraceArgs()
    args.cameraPos[0], args.cameraPos[1], args.cameraPos[2] = [float(v) for v in pos]
    args.time = 0.0; args.numMeshes = orc.s.numInstances; args.sunAngle = -1.96
    st = oracle_lib.OrcStats()
    r = np.ascontiguousarray(rays, np.float32)
    L.orc_trace_ex(C.byref(orc.s), C.byref(args), r.ctypes.data, N, N, 0, N, ref.ctypes.data, C.byref(st), nthreads, ORC_EXT_PRIMARY_ONLY)
    assert mask.all() and st.as_dict()["hits"] == N * N
    assert np.array_equal(bits(shaded), bits(ref[..., :3]))
