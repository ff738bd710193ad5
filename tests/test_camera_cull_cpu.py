"""The camera bounce's staged instance cull (staged_candidate_mask, crt_device.h) against candidate_mask's expression, without a GPU.

A float32 numpy restatement of both, one IEEE operation per numpy operation in the kernels' order (the library is built with
-ffp-contract=off, so the kernels round after every operation too):

  per lane (candidate_mask):   oc = c - o; oc2 = oc.oc; b = oc.d; r2 = w w 1.0201 + 4e-6 oc2
                               cull = (w >= 0) & ((oc2 dd - b b > r2 dd) | ((b < 0) & (oc2 > r2)))
  staged, lane k stores:       oc, oc2, r2' = (w >= 0) ? r2 : +inf, thr = (w >= 0 & oc2 > r2) ? 0 : -inf
  staged, every lane computes: b = oc.d; cull = (oc2 dd - b b > r2' dd) | (b < thr)

The two must agree in every bit of the mask: for both clauses, for never-cull instances (w = -1), a NaN radius, a camera inside a
sphere, an oc2 that overflows, a NaN camera, and directions with zeros, denormals, infinities and NaNs."""
import numpy as np

F = np.float32


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz          # dot3 of crt_device.h: left to right


def per_lane(c, w, o, d):
    """candidate_mask's expression: c (n, 3), w (n,), o (3,), d (m, 3) -> cull (m, n)"""
    ocx, ocy, ocz = c[:, 0] - o[0], c[:, 1] - o[1], c[:, 2] - o[2]
    oc2 = dot3(ocx, ocy, ocz, ocx, ocy, ocz)
    r2 = w * w * F(1.0201) + F(4e-6) * oc2
    dx, dy, dz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    dd = dot3(dx, dy, dz, dx, dy, dz)
    b = dot3(ocx[None], ocy[None], ocz[None], dx, dy, dz)
    return (w >= 0)[None] & ((oc2[None] * dd - b * b > r2[None] * dd) | ((b < 0) & (oc2 > r2)[None]))


def staged_terms(c, w, o):
    """what the staging lane stores per instance: (oc.x, oc.y, oc.z, oc2), (r2', thr) -- as float32 words"""
    ocx, ocy, ocz = c[:, 0] - o[0], c[:, 1] - o[1], c[:, 2] - o[2]
    oc2 = dot3(ocx, ocy, ocz, ocx, ocy, ocz)
    r2 = w * w * F(1.0201) + F(4e-6) * oc2
    cullable = w >= 0
    r2s = np.where(cullable, r2, F(np.inf)).astype(F)
    thr = np.where(cullable & (oc2 > r2), F(0.0), F(-np.inf)).astype(F)
    return np.stack([ocx, ocy, ocz, oc2], 1).astype(F), np.stack([r2s, thr], 1).astype(F)


def staged_lane(rowA, rowB, d):
    dx, dy, dz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    dd = dot3(dx, dy, dz, dx, dy, dz)
    b = dot3(rowA[None, :, 0], rowA[None, :, 1], rowA[None, :, 2], dx, dy, dz)
    return (rowA[None, :, 3] * dd - b * b > rowB[None, :, 0] * dd) | (b < rowB[None, :, 1])


def directions(rng, c, o, n):
    """unit directions at and around the spheres (both clauses decide), plus the special values"""
    d = rng.normal(size=(n, 3))
    aim = c[rng.randint(0, len(c), n)].astype(np.float64) - o.astype(np.float64)
    with np.errstate(all="ignore"):
        aim = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    aim = np.where(np.isfinite(aim), aim, d)
    d = np.where(rng.uniform(size=(n, 1)) < 0.7, aim + d * (10.0 ** rng.uniform(-6, 0, (n, 1))), d)
    d[::7] *= -1.0                                               # centre behind the origin: the second clause
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(F)
    tiny_ = np.float32(1e-42)                                    # a denormal
    special = np.array([[0, 0, -1], [0.0, -0.0, 1], [1, 0, 0], [-0.0, 1, 0.0], [tiny_, -tiny_, 1], [tiny_, tiny_, tiny_], [0, 0, 0],
                        [np.inf, 0, 1], [-np.inf, np.inf, 0], [np.nan, 0, 1], [3e19, 3e19, 3e19], [1e-30, 0, 1e-30]], F)
    return np.concatenate([d, special])


def instances(rng, n):
    scale = 10.0 ** rng.uniform(-3, 3, n)
    c = rng.normal(size=(n, 3)) * (10.0 ** rng.uniform(-2, 6, (n, 1)))
    w = scale * rng.uniform(0.5, 3.0, n)
    return c.astype(F), w.astype(F)


def agree(c, w, o, d):
    with np.errstate(all="ignore"):
        want = per_lane(c, w, o, d)
        rowA, rowB = staged_terms(c, w, o)
        got = staged_lane(rowA, rowB, d)
    assert got.dtype == np.bool_ and got.shape == want.shape
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:4])
    return want


def test_staged_mask_equals_the_per_lane_mask_on_random_scenes():
    rng = np.random.RandomState(21)
    culled = kept = second = 0
    for trial in range(40):
        c, w = instances(rng, 64)
        w[rng.randint(0, 64, 6)] = F(-1.0)                       # never culled
        o = (rng.normal(size=3) * 10.0 ** rng.uniform(-1, 5)).astype(F)
        d = directions(rng, c, o, 500)
        m = agree(c, w, o, d)
        assert not m[:, w < 0].any()                             # a never-cull instance stays a candidate for every direction
        culled += int(m.sum()); kept += int((~m).sum())
        with np.errstate(all="ignore"):
            rowA, rowB = staged_terms(c, w, o)
            dd = dot3(d[:, 0:1], d[:, 1:2], d[:, 2:3], d[:, 0:1], d[:, 1:2], d[:, 2:3])
            b = dot3(rowA[None, :, 0], rowA[None, :, 1], rowA[None, :, 2], d[:, 0:1], d[:, 1:2], d[:, 2:3])
            second += int((~(rowA[None, :, 3] * dd - b * b > rowB[None, :, 0] * dd) & (b < rowB[None, :, 1])).sum())
    print(f"{culled} culled, {kept} kept, {second} culled by the second clause alone")
    assert culled > 10000 and kept > 10000 and second > 100      # both outcomes and both clauses were exercised


def test_special_cameras_and_radii():
    rng = np.random.RandomState(22)
    c, w = instances(rng, 64)
    w[:4] = F(-1.0); w[4] = F(np.nan); w[5] = F(0.0); w[6] = F(np.inf); w[7] = F(-0.0); w[8] = F(1e20)       # w w overflows for 1e20
    cases = {
        "inside a sphere": (c[10].astype(np.float64) + 0.3 * float(w[10]) * np.array([0.5, -0.5, 0.5])).astype(F),
        "at a centre": c[11].copy(),
        "oc2 overflows": np.array([2e19, -2e19, 1e19], F),
        "oc infinite": np.array([np.inf, 0.0, 0.0], F),
        "NaN camera": np.array([np.nan, 1.0, 2.0], F),
        "all NaN": np.array([np.nan] * 3, F),
        "origin": np.zeros(3, F),
    }
    for name, o in cases.items():
        d = directions(rng, c, np.nan_to_num(o, nan=0.0, posinf=1e19, neginf=-1e19).astype(F), 300)
        m = agree(c, w, o, d)
        assert not m[:, :5].any(), name                                       # w = -1 and a NaN w: never culled
        if name == "inside a sphere":
            assert not m[:, 10].any()                                         # the origin inside a sphere: a candidate for every direction
        if name in ("NaN camera", "all NaN"):
            assert not m.any(), name                                          # any NaN keeps the instance


def test_staged_words_of_an_uncullable_instance():
    c = np.array([[1.0, 2.0, 3.0]], F); o = np.array([0.5, 0.5, 0.5], F)
    for w in (F(-1.0), F(np.nan)):
        _, rowB = staged_terms(c, np.array([w], F), o)
        assert rowB.view(np.uint32).tolist() == [[0x7F800000, 0xFF800000]]    # the two words the kernel stores: +inf, -inf
