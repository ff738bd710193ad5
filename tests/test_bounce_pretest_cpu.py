"""The root pre-test of the reflection bounce (crt_device.h: bounce_pretest_mask, (7) above root_pretest_misses) without a GPU. tests/root_pretest_ref.py
as it is, given one origin per ray: its `o` as a (3, n) array, so that o[k] is the k-th component of every ray's origin.

  1. A cleared bit implies that both slab tests of the root return 1e30 at EVERY bound in (0, 99999], for rays with origins of their own: inside,
     on a face of, on an edge of and one ulp outside a child box, far away; zero, denormal, infinite and NaN direction components; rays along a
     face and past a corner (grazing); instances with non-uniform scale.
  2. On small frames over a reflecting floor (tests/bounce_pretest_ref.py) the oracle's hit record of a bounce ray is bit for bit the same when
     ALL the instances the pre-test clears for that ray are left out of the scene at once.
  3. tools/count_bounce_pretest.py's restatement of the bounce ray agrees with the oracle: as many rays as the frame's secondary rays, and traced with
     closest_hits exactly the frame's secondary hits (orc.trace's stats)."""
import numpy as np
import pytest

from clraytracer_amd import driver, scenes
import oracle_lib
import root_pretest_ref as ref
import bounce_pretest_ref as scene_ref
from bounce_pretest_ref import tool
from test_gpu_cull_bound import _nonuniform
from test_root_pretest_cpu import BOUNDS, _kids

F = np.float32


def _adversarial(rng):
    """(m, o (n, 3), d (n, 3), kids): every ray with its own origin"""
    tiny_ = F(1e-42)
    special = np.array([[0, 0, -1], [0.0, -0.0, 1], [1, 0, 0], [-0.0, 1, 0.0], [tiny_, -tiny_, 1], [tiny_, tiny_, tiny_], [0, 0, 0], [np.inf, 0, 1],
                        [-np.inf, np.inf, 0], [np.nan, 0, 1], [0, np.nan, np.nan], [1e-30, 0, 1e-30], [1e38, -1e38, 1e38], [2e-38, 1, 3e-39]], np.float64)
    out = []
    for k in range(16):
        axis, angle, t = tuple(rng.normal(size=3)), rng.uniform(0, 6.28), tuple(rng.normal(size=3) * 5)
        m = (_nonuniform(*(10.0 ** rng.uniform(-1, 1, 3)), axis, angle, t) if k % 2 else scenes._trs(10.0 ** rng.uniform(-2, 2), axis, angle, t)).astype(F)
        lo0 = rng.normal(size=3); hi0 = lo0 + rng.uniform(0.1, 2, 3)
        lo1 = lo0 + rng.uniform(-1, 1, 3); hi1 = lo1 + rng.uniform(0.1, 2, 3)
        kids = _kids(lo0, hi0, lo1, hi1)
        fwd = np.linalg.inv(m.astype(np.float64))
        lo, hi = kids[0]["min"].astype(np.float64), kids[0]["max"].astype(np.float64)
        centre = (lo + hi) / 2
        pts = [centre, [hi[0], centre[1], centre[2]], [hi[0], hi[1], centre[2]], hi,
               np.nextafter(hi.astype(F), F(np.inf)).astype(np.float64), np.nextafter(lo.astype(F), F(-np.inf)).astype(np.float64),
               [np.nextafter(F(hi[0]), F(np.inf)), centre[1], centre[2]], centre + rng.normal(size=3) * 30, hi + (hi - lo) * 1e-3]
        os_, ds = [], []
        for p in pts:
            ow = (np.append(np.asarray(p, np.float64), 1.0) @ fwd)[:3]
            # aimed at the box's centre and corners, along its faces, and past a corner by a hair on either side: grazing
            targets = [centre, lo, hi, [lo[0], hi[1], lo[2]], hi + (hi - lo) * 1e-6, hi - (hi - lo) * 1e-6, lo - (hi - lo) * 1e-6]
            dirs = [(np.append(np.asarray(q, np.float64), 1.0) @ fwd)[:3] - ow for q in targets]
            dirs += [fwd[0, :3], -fwd[1, :3], fwd[0, :3] + fwd[2, :3]]                       # the box's own axes: parallel to its faces
            dirs += list(rng.normal(size=(12, 3)))
            with np.errstate(all="ignore"):
                dirs = [v / np.linalg.norm(v) if np.linalg.norm(v) > 0 else v for v in dirs] + list(special)
            os_ += [ow] * len(dirs); ds += dirs
        out.append((m, np.array(os_, np.float64).astype(F), np.array(ds, np.float64).astype(F), kids))
    # object space = world space: exact face, edge, corner and just-outside origins without a transform's rounding
    eye = np.eye(4, dtype=F)
    unit = _kids([0, 0, 0], [1, 1, 1], [2, 0, 0], [3, 1, 1])
    one_up, one_down = np.nextafter(F(1.0), F(2.0)), np.nextafter(F(0.0), F(-1.0))
    origins = np.array([[0.5, 0.5, 0.5], [1.0, 0.5, 0.5], [1.0, 1.0, 0.5], [1.0, 1.0, 1.0], [one_up, 0.5, 0.5], [one_down, 0.5, 0.5], [one_up, one_up, one_up],
                        [1.5, 0.5, 0.5], [1.5, 1.0, 0.5], [-4.0, 1.0, 1.0]], F)
    axis = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [1, 1, 0], [1, 1, 1], [0.5, 0.25, 0.125], [1, 0, -0.0], [2, 1, 0], [1, 0, 1e-7], [1, -1e-7, 0]], np.float64)
    dirs = np.concatenate([axis, special])
    out.append((eye, np.repeat(origins, len(dirs), 0), np.tile(dirs, (len(origins), 1)).astype(F), unit))
    return out


def test_a_cleared_bit_is_a_miss_at_every_bound_for_rays_with_their_own_origins():
    rng = np.random.RandomState(20262)
    total = cleared = kept = 0
    for m, o, d, kids in _adversarial(rng):
        ot = np.ascontiguousarray(o.T)
        clear = ref.pretest_clears(m, ot, d, kids)
        # one origin per ray is what the restatement computes: ray by ray with the shared-origin form it gives the same answer
        step = max(1, len(d) // 40)
        for r in range(0, len(d), step):
            assert ref.pretest_clears(m, o[r], d[r:r + 1], kids)[0] == clear[r], r
        for bound in list(BOUNDS) + [rng.uniform(0, 99999, len(d)).astype(F)]:
            d1, d2 = ref.root_step(m, ot, d, kids, bound)
            for dist in (d1, d2):
                assert ((dist == ref.MISS) | ((dist > 0) & (dist < bound))).all()             # the restatement decides every case
            assert not (clear & ((d1 != ref.MISS) | (d2 != ref.MISS))).any(), (m, bound)
        d1, d2 = ref.root_step(m, ot, d, kids, ref.BOUND0)
        assert np.array_equal(~clear, (d1 != ref.MISS) | (d2 != ref.MISS))
        nan = np.isnan(d).any(1) | ~d.any(1)
        assert clear[nan].all()                                                               # a NaN or zero direction misses at any bound
        total += len(d); cleared += int(clear.sum()); kept += int((~clear).sum())
    assert cleared > total // 10 and kept > total // 10, (cleared, kept, total)


@pytest.fixture(scope="module")
def frames(nthreads, tmp_path_factory):
    """{(n, w, h): (arenas, oracle, primary stats' view)} of the floor scenes, built once"""
    out = {}
    for n, w, h in ((8, 72, 40), (16, 64, 64)):
        sc = scene_ref.floor_scene(n, w, h, nthreads, tmp_path_factory.mktemp(f"floor{n}"))
        with driver.Session(w, h, host_only=True) as s:
            s.load_scene(sc)
            a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
            iv, ip, pos = s.camera()
        orc = oracle_lib.Oracle(a, nthreads=nthreads)
        out[(n, w, h)] = (a, orc, sc, iv, ip, pos) + scene_ref.wave_view(a, orc, w, h, iv, ip, pos)
    return out


@pytest.mark.parametrize("n,w,h", [(8, 72, 40), (16, 64, 64)])
def test_bounce_rays_keep_their_hit_records_when_their_cleared_instances_are_skipped(n, w, h, frames, nthreads):
    a, orc, sc, iv, ip, pos, alive, o1, d1, sph, use = frames[(n, w, h)]
    assert len(a["instances"]) == n and ref.instance_terms(a, 3)[1] is None
    # the tool's masks are root_pretest_ref's answer with one origin per ray
    ot = np.ascontiguousarray(o1.T)
    clears = np.stack([ref.pretest_clears(*((ref.instance_terms(a, k)[0], ot, d1, ref.instance_terms(a, k)[1]))) for k in range(n)], 1)
    assert np.array_equal(sph & ~use, sph & clears)
    assert not clears[:, 3].any()                                                             # the single-leaf instance
    assert scene_ref.mixed_waves(alive, sph, use, w, h) > 0
    full = orc.closest_hits(o1, d1)[0]
    hit = full["instance"] >= 0
    assert hit.any() and not clears[np.nonzero(hit)[0], full["instance"][hit]].any()          # the instance a ray hits is never cleared for it
    codes = (clears * (1 << np.arange(n))).sum(1)
    checked = 0
    for code in np.unique(codes):
        if code == 0:
            continue
        rays = np.nonzero(codes == code)[0]
        gone = np.array([k for k in range(n) if code >> k & 1])
        b = dict(a); b["instances"] = np.ascontiguousarray(np.delete(a["instances"], gone))
        got = oracle_lib.Oracle(b, nthreads=nthreads).closest_hits(o1[rays], d1[rays])[0]
        want = full[rays].copy()
        want["instance"] = want["instance"] - (gone[None, :] < want["instance"][:, None]).sum(1)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), gone
        checked += len(rays) * len(gone)
    assert checked > len(d1) // 4, (checked, len(d1))


@pytest.mark.parametrize("n,w,h", [(8, 72, 40), (16, 64, 64)])
def test_the_restated_bounce_ray_is_the_oracles(n, w, h, frames):
    a, orc, sc, iv, ip, pos, alive, o1, d1, sph, use = frames[(n, w, h)]
    _, stats = orc.trace(orc.raygen(w, h, iv, ip), pos, sc.sun_angle)
    assert stats["primary"] == w * h and stats["secondary"] == int(alive.sum()) == len(o1) > 0
    second = orc.closest_hits(o1, d1)[0]
    hits = int(((second["instance"] >= 0) & ~(second["t"] > tool.SKY)).sum())
    assert 0 < hits == stats["hits"] - stats["secondary"]                                     # every secondary ray follows a primary hit
