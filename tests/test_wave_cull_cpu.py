"""The wave test of the staged instance cull (crt_device.h: wave_cone, cone_rejects; restated in tests/wave_cull_ref.py), without a GPU.

Soundness: whenever the test rejects a (wave, instance) pair, the lemma it rests on holds for EVERY lane -- in exact arithmetic
|o + t d - fl(c)|^2 > 1.02 w^2 + 2.8e-6 x^2 for all t > 0 -- checked in float64 on every pair and in rationals on a subsample, with the
special functions' results moved by -1, 0 and +1 ulp. Not vacuous: a sphere well outside the cone is always rejected."""
import numpy as np
import pytest

import wave_cull_ref as ref

F = np.float32
ULPS = (-1, 0, 1)
BENCH_FOV, WIDE_FOV, NARROW_FOV = 60.0, 120.0, 5.0


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def basis(rng, T):
    """random orthonormal frames (T, 3, 3): rows right, up, forward"""
    f = unit(rng.normal(size=(T, 3)))
    r = unit(np.cross(f, rng.normal(size=(T, 3))))
    return np.stack([r, np.cross(r, f), f], 1)


def tiles(rng, T, fov_deg, L=64, W=1920, H=1080):
    """T random 8 x 8 tiles (L = 16: 4 x 4 quadrants) of a pinhole camera, lanes in Morton order; float32 unit directions (T, L, 3) and the frames"""
    m = np.arange(L)
    lx, ly = (m & 1) | ((m >> 1) & 2) | ((m >> 2) & 4), ((m >> 1) & 1) | ((m >> 2) & 2) | ((m >> 3) & 4)
    px = rng.integers(0, W // 8, T)[:, None] * 8 + lx[None, :]
    py = rng.integers(0, H // 8, T)[:, None] * 8 + ly[None, :]
    th = np.tan(np.radians(fov_deg) / 2)
    cx, cy = (px / W * 2 - 1) * th * W / H, (py / H * 2 - 1) * th
    B = basis(rng, T)
    d = cx[..., None] * B[:, None, 0] + cy[..., None] * B[:, None, 1] + B[:, None, 2]
    return unit(d).astype(F), B


def cone64(d):
    """the exact cone of the float32 directions: axis (lane 0, unit), half-angle"""
    d = d.astype(np.float64)
    a = unit(d[:, 0])
    cos = np.einsum("tlc,tc->tl", unit(d), a).min(1)
    return a, np.arccos(np.clip(cos, -1, 1))


def psi64(w, x):
    """half-angle of the sphere the test uses, seen from distance x"""
    r2 = (1.0201 * w * w + 4e-6 * x * x) * (1 + 8e-6)
    return np.arcsin(np.minimum(1.0, np.sqrt(r2) / x))


def at_angle(rng, a, ang):
    """unit vectors at angle `ang` (T, K) from the axes a (T, 3), random azimuth"""
    T, K = ang.shape
    p = unit(np.cross(a, rng.normal(size=(T, 3))))
    q = np.cross(a, p)
    az = rng.uniform(0, 2 * np.pi, (T, K))
    side = np.cos(az)[..., None] * p[:, None] + np.sin(az)[..., None] * q[:, None]
    return np.cos(ang)[..., None] * a[:, None] + np.sin(ang)[..., None] * side


def check_sound(o, d, cf, w, exact=40, expect_rejects=True):
    o, d, cf, w = np.asarray(o, F), np.asarray(d, F), np.asarray(cf, F), np.asarray(w, F)
    with np.errstate(all="ignore"):
        margin = ref.lemma_margin64(o, d, cf, w)
        lane_lets = ~ref.lane_culls(o, d, cf, w)
    rng = np.random.default_rng(7)
    total = 0
    for ulp in ULPS:
        rej = ref.wave_rejects(o, d, cf, w, ulp)
        total += int(rej.sum())
        bad = rej[:, None, :] & ~(margin > 0)
        assert not bad.any(), (ulp, int(bad.sum()), np.argwhere(bad)[:5])
        # what the kernel relies on as well: a rejected instance is in no lane's own mask
        assert not (rej[:, None, :] & lane_lets).any(), ulp
        pairs = np.argwhere(rej)
        for t, k in pairs[rng.permutation(len(pairs))[:exact]]:
            for lane in rng.integers(0, d.shape[1], 3):
                assert ref.lemma_holds_exact(o[t], d[t, lane], cf[t, k], w[t, k]), (ulp, t, k, lane)
    assert not expect_rejects or total > 0
    return total


@pytest.mark.parametrize("fov", [BENCH_FOV, WIDE_FOV, NARROW_FOV])
@pytest.mark.parametrize("lanes", [64, 16])
def test_random_tiles_and_spheres(fov, lanes):
    rng = np.random.default_rng(int(fov) + lanes)
    T, K = 1500, 16
    d, _ = tiles(rng, T, fov, lanes)
    o = rng.normal(size=(T, 3)) * 10
    w = 10.0 ** rng.uniform(-3, 3, (T, K))                                      # radii 1e-3 ... 1e3
    x = w * 10.0 ** rng.uniform(-0.5, 3, (T, K))                                # inside the sphere ... 1000 radii away
    cf = o[:, None] + unit(rng.normal(size=(T, K, 3))) * x[..., None]
    check_sound(o, d, cf, w)


def test_origins_out_to_the_cull_range():
    rng = np.random.default_rng(11)
    T, K = 1500, 16
    d, _ = tiles(rng, T, BENCH_FOV)
    w = 10.0 ** rng.uniform(-3, 3, (T, 1)) * np.ones((1, K))
    cf = unit(rng.normal(size=(T, K, 3))) * w[..., None] * rng.uniform(0, 100, (T, K, 1))
    reach = 13800.0 * w[:, 0] - 0.58 * np.linalg.norm(cf, axis=-1).max(1)      # O_i of a rigid instance (sphere_culls' derivation, (3))
    o = unit(rng.normal(size=(T, 3))) * (0.95 * reach * rng.uniform(0.1, 1, T))[:, None]
    check_sound(o, d, cf, w)


@pytest.mark.parametrize("fov", [BENCH_FOV, WIDE_FOV, NARROW_FOV])
def test_spheres_tangent_to_the_cone_from_both_sides(fov):
    rng = np.random.default_rng(int(fov) + 1)
    T, K = 1500, 16
    d, _ = tiles(rng, T, fov)
    a, theta = cone64(d)
    o = rng.normal(size=(T, 3)) * 10
    w = 10.0 ** rng.uniform(-3, 3, (T, K))
    x = w * 10.0 ** rng.uniform(0.1, 3, (T, K))
    ang = (theta[:, None] + psi64(w, x)) * (1 + rng.uniform(-1e-3, 1e-3, (T, K)))      # grazing within +-1e-3 relative
    cf = o[:, None] + at_angle(rng, a, np.minimum(ang, np.pi)) * x[..., None]
    # (the narrow camera's cones are 5e-4 rad wide: the 4e-6 taken off cos theta is an angle of 3e-3 rad there, more than the +-1e-3 relative of
    # this family, so none of its pairs is rejected)
    n = check_sound(o, d, cf, w, expect_rejects=fov != NARROW_FOV)
    assert n < 3 * T * K          # ... from both sides: not everything is rejected either


def test_centres_behind_the_camera_and_camera_inside_a_sphere():
    rng = np.random.default_rng(13)
    T, K = 1000, 16
    d, B = tiles(rng, T, BENCH_FOV)
    o = rng.normal(size=(T, 3)) * 10
    w = 10.0 ** rng.uniform(-2, 2, (T, K))
    x = w * 10.0 ** rng.uniform(0.05, 2, (T, K))
    back = unit(-B[:, None, 2] + 0.5 * rng.normal(size=(T, K, 3)))
    check_sound(o, d, o[:, None] + back * x[..., None], w)
    # inside: x < w -- never rejected
    xin = w * rng.uniform(0, 0.999, (T, K))
    cf = o[:, None] + unit(rng.normal(size=(T, K, 3))) * xin[..., None]
    assert check_sound(o, d, cf, w, expect_rejects=False) == 0


def test_uncullable_spheres_and_nans_survive():
    rng = np.random.default_rng(17)
    T, K = 500, 16
    d, B = tiles(rng, T, BENCH_FOV)
    o = (rng.normal(size=(T, 3)) * 10).astype(F)
    w = (10.0 ** rng.uniform(-2, 1, (T, K))).astype(F)
    cf = (o[:, None] + unit(-B[:, None, 2] + 0.3 * rng.normal(size=(T, K, 3))) * (w * 50)[..., None]).astype(F)     # far behind: all rejected as they are
    assert all(ref.wave_rejects(o, d, cf, w, u).all() for u in ULPS)
    for bad in (F(-1.0), F(np.nan)):                       # w < 0 (never culled), a NaN w
        w2 = w.copy(); w2[:, ::2] = bad
        for u in ULPS:
            rej = ref.wave_rejects(o, d, cf, w2, u)
            assert not rej[:, ::2].any() and rej[:, 1::2].all()
    o2 = o.copy(); o2[::2, 1] = np.nan                     # a NaN camera
    c2 = cf.copy(); c2[:, ::2, 0] = np.nan                 # a NaN centre
    for u in ULPS:
        assert not ref.wave_rejects(o2, d, cf, w, u)[::2].any()
        assert not ref.wave_rejects(o, d, c2, w, u)[:, ::2].any()


@pytest.mark.parametrize("poison", ["zero", "denormal", "inf", "nan", "long", "short", "backwards"])
@pytest.mark.parametrize("lane", [0, 37])
def test_the_guard_turns_the_test_off(poison, lane):
    rng = np.random.default_rng(19)
    T, K = 200, 16
    d, B = tiles(rng, T, BENCH_FOV)
    o = (rng.normal(size=(T, 3)) * 10).astype(F)
    w = (10.0 ** rng.uniform(-2, 1, (T, K))).astype(F)
    cf = (o[:, None] + unit(-B[:, None, 2] + 0.3 * rng.normal(size=(T, K, 3))) * (w * 50)[..., None]).astype(F)
    d = d.copy()
    d[:, lane] = {"zero": d[:, lane] * 0, "denormal": d[:, lane] * F(1e-40), "inf": d[:, lane] * F(np.inf), "nan": d[:, lane] * F(np.nan),
                  "long": d[:, lane] * F(1.001), "short": d[:, lane] * F(0.999), "backwards": -d[:, lane]}[poison]
    for u in ULPS:
        with np.errstate(all="ignore"):
            assert not ref.wave_cone(d, u)["ok"].any()
            assert not ref.wave_rejects(o, d, cf, w, u).any()


@pytest.mark.parametrize("fov", [BENCH_FOV, WIDE_FOV, NARROW_FOV])
def test_a_sphere_well_outside_the_cone_is_always_rejected(fov):
    """centre at an angle >= 2 (theta + psi) + 0.05 rad from the axis, cullable, origin outside: the margins (an angle of at most 3e-3 rad for the
    narrowest cone) are orders of magnitude below that gap"""
    rng = np.random.default_rng(int(fov) + 2)
    T, K = 1500, 16
    d, _ = tiles(rng, T, fov)
    a, theta = cone64(d)
    o = rng.normal(size=(T, 3)) * 10
    w = 10.0 ** rng.uniform(-3, 3, (T, K))
    x = w * 10.0 ** rng.uniform(0.2, 3, (T, K))             # psi <= asin(1.01 / 1.58) = 0.69 rad
    least = 2 * (theta[:, None] + psi64(w, x)) + 0.05
    assert (least < np.pi).all()
    ang = least + rng.uniform(0, 1, (T, K)) * (np.pi - least)
    cf = o[:, None] + at_angle(rng, a, ang) * x[..., None]
    for u in ULPS:
        assert ref.wave_rejects(o.astype(F), d, cf.astype(F), w.astype(F), u).all()
    check_sound(o, d, cf, w)
