"""The guarded float skybox index (clraytracer_amd/csrc/crt_device.h: sky_index_float, sample_skybox_guarded) on the CPU: its numpy restatement
(tests/sky_fast_ref.py, constants read from the header) against the definition's restatement (tests/texel_ref.py: sky_index).

  * a decided lane has the definition's index -- on the edge families, a million random directions and directions aimed at every texel edge;
  * the arguments at which the definition returns special values are never decided;
  * the guard does not say "undecided" to everything;
  * the header's constants cover the errors recorded in profiles/sky_index_bounds.txt, and a strided subset of the exhaustive sweeps
    (tools/sky_index_bounds.c) stays below what is recorded there.
The device side: tests/test_gpu_sky_index.py."""
import numpy as np
import pytest

import sky_fast_ref as S
import texel_ref as T

F = np.float32
SIZES = tuple(T.SKY_SIZES) + ((2048, 1024), (4096, 2048))
IDS = ["%dx%d" % s for s in SIZES]


def family_rays(name, n=T.FRAME):
    """the oracle's RayGen for a family's view: the rays the kernels generate, bit for bit (tests/test_gpu_texel_lookup.py)"""
    import oracle_lib
    iv, ip, _ = T.family_view(name)
    rays = np.empty((n, n, 3), F)
    oracle_lib.lib().orc_raygen(rays.ctypes.data, n, n, oracle_lib.f32(iv)[0], oracle_lib.f32(ip)[0])
    return rays.reshape(-1, 3)


@pytest.fixture(scope="module")
def random_dirs():
    rng = np.random.RandomState(20240611)
    d = rng.standard_normal((1 << 20, 3))
    return (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)


def check_decided(d, tw, th, what):
    decided, theta, phi, idx = S.decide(d, tw, th)
    rt, rp, ridx = T.sky_index(d, tw, th)
    bad = decided & ((theta != rt) | (phi != rp) | (idx != ridx))
    print(f"{what} on {tw}x{th}: {len(d)} directions, {int((~decided).sum())} undecided, {int(bad.sum())} decided lanes differ")
    assert not bad.any(), (what, tw, th, d[bad][:4], theta[bad][:4], rt[bad][:4], phi[bad][:4], rp[bad][:4])
    return decided


@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_decided_lanes_have_the_definitions_index(size, random_dirs):
    tw, th = size
    some = 0
    for f in T.SKY_FAMILIES:
        some += int(check_decided(family_rays(f), tw, th, f).sum())
    assert some > 0
    dec = check_decided(random_dirs, tw, th, "random")
    assert dec.mean() > 0.9
    cols = S.edge_aimed_columns(tw)
    assert len(cols) == (2 * (tw // 2) + 1) * 17
    dc = check_decided(cols, tw, th, "column edges")
    rows = S.edge_aimed_rows(th)
    assert len(rows) == (th + 1) * 17
    dr = check_decided(rows, tw, th, "row edges")
    # the aimed-at directions do come near the edges: a good part of them is left to the double form
    assert (~dc).mean() > 0.2 and (~dr).mean() > 0.2, ((~dc).mean(), (~dr).mean())


def test_special_values_are_never_decided():
    candidates = np.array([(0.3, 0.4, -0.85), (0.31, 0.43, -0.8), (0.5, 0.37, -0.7), (0.2, 0.61, -0.9)], F)
    for tw, th in SIZES + ((37, 90), (1, 1), (3, 5)):
        # a direction that IS decided on this size, its components replaced one at a time
        ok = tuple(candidates[np.flatnonzero(S.decide(candidates, tw, th)[0])[0]])
        decided = S.decide(special_cases(ok), tw, th)[0]
        assert not decided.any(), (tw, th, special_cases(ok)[decided])
    # a sky without texels decides nothing
    assert not S.decide(candidates, 0, 32)[0].any() and not S.decide(candidates, 64, 0)[0].any()


def special_cases(ok):
    nan, inf = F(np.nan), F(np.inf)
    tiny = np.nextafter(F(0), F(1))                   # the smallest denormal
    big_den = np.nextafter(F(1.17549435e-38), F(0))    # the largest denormal
    over = np.nextafter(F(1), F(2))                   # 1 + 1 ulp
    x, y, z = ok
    cases = []
    for k in range(3):
        for v in (nan, inf, -inf):
            d = list(ok); d[k] = v; cases.append(d)
        for v in (tiny, -tiny, big_den, -big_den):
            d = list(ok); d[k] = v; cases.append(d)
    cases += [[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [nan, nan, nan], [inf, inf, inf], [inf, 0.5, -inf]]
    for zero in (0.0, -0.0):
        cases += [[zero, y, z], [zero, y, -z], [x, y, zero], [-x, y, zero], [x, zero, z]]
    cases += [[x, 1.0, z], [x, -1.0, z], [0.0, 1.0, 0.0], [0.0, -1.0, -0.0], [x, over, z], [x, -over, z]]
    return np.array(cases, F)


def test_the_guard_does_not_give_everything_to_the_double_form(random_dirs):
    """A condition, not a measurement: at most 1 % of random lanes undecided on 2048 x 1024, at most 0.1 % on 64 x 32"""
    for (tw, th), most in (((2048, 1024), 0.01), ((64, 32), 0.001)):
        undecided = float((~S.decide(random_dirs, tw, th)[0]).mean())
        print(f"{tw}x{th}: {100.0 * undecided:.4f} % of {len(random_dirs)} random lanes undecided")
        assert undecided <= most, (tw, th, undecided)


def test_the_headers_constants_cover_the_recorded_errors():
    rec, sweeps = S.recorded()
    safety = 1.25
    # the derivation above sample_skybox_guarded: K = E + 2^-25 + 2^-23 + 1e-15, E_a = E_p + 2^-24 / pi + 2 * 2^-25
    rounding = 2.0 ** -25 + 2.0 ** -23 + 1e-15
    ka = rec["E_p"] + 2.0 ** -24 / np.pi + 2.0 * 2.0 ** -25 + rounding
    kc = rec["E_c"] + rounding
    assert abs(ka - rec["K_a"]) <= 1e-12 and abs(kc - rec["K_c"]) <= 1e-12, (ka, kc, rec)
    assert safety * ka <= float(S.K["KA"]) <= 2.0 * ka, (ka, S.K["KA"])
    assert safety * kc <= float(S.K["KC"]) <= 2.0 * kc, (kc, S.K["KC"])
    assert len(sweeps) == 9 and all(n == 0 for (k, _, _), n in sweeps.items() if k == "q0")
    assert all(n > 0 for (k, _, _), n in sweeps.items() if k != "q0")
    # a strided subset of the two exhaustive sweeps stays below the recorded maxima
    with np.errstate(all="ignore"):
        q = np.arange(0, 0x3F800001, 1021, dtype=np.uint32).view(F)
        assert q.min() == 0 and q.max() <= 1
        ep = np.abs(S.poly_atan(q).astype(np.float64) - np.arctan(q.astype(np.float64)) / np.pi).max()
        y = np.arange(0, 1 << 32, 4099, dtype=np.uint64).astype(np.uint32).view(F)
        ay = np.abs(y)
        y = y[(ay >= S.K["MIN_COMPONENT"]) & (ay < 1)]
        ec = np.abs(S.fast_acos(y).astype(np.float64) - np.arccos(y.astype(np.float64)) / np.pi).max()
    print(f"strided: E_p {ep:.4e} (recorded {rec['E_p']:.4e}), E_c {ec:.4e} (recorded {rec['E_c']:.4e})")
    # numpy's and glibc's double functions may differ in the last place: 1e-15 of the rounding terms is there for that
    assert ep <= rec["E_p"] + 1e-15 and ec <= rec["E_c"] + 1e-15
