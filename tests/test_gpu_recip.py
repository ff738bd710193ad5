"""The traversal's short reciprocal (crt_device.h: recip, recip3 -- v_rcp_f32 + one Newton step + v_div_fixup_f32 behind a wave-level guard
with the division as the wave's fall-back) on the GPU:
  1. crt_debug_recip_sweep over all 2^32 bit patterns: the guarded helpers return the bits of the device's `1.0f / x`, and the unguarded
     short sequence is wrong only where the guard sends the wave to the division;
  2. one-wave batches of 64 explicit rays whose object-space directions mix, WITHIN the wave, ordinary values with denormals, +-0, +-inf,
     NaN and values >= 2^126 (instance matrices diag(s), s from 2^-130 to 2^127), through the counted query path (crt_query_hits) and
     through crt_trace_rays: hit records and counters bit-equal to the C oracle (same_as_oracle: the one encoding that is the architecture's), and
     the two routes' records bit-equal to each other;
  3. the same for the triangle determinant: triangles with edges of 2^-70 and 2^63 (a denormal or >= 2^126 in some lanes only) and
     degenerate triangles (a = 0: the NaN that poisons the running t must be the one upstream's blend gives);
  4. frames on `tiny` -- plain, shadows, refraction, SSAA2, G-buffer; synchronous and three in flight; a counted frame beside each --
     bit-equal to the oracle frame.
(The counted instantiations keep the division, so a counted launch is the same in every build of the library; the uncounted ones
-- crt_trace_rays, the frames without CRT_RENDER_COUNT -- run the short form.)"""
import ctypes as C

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import gbuffer_ref
import oracle_lib
import trace_rays_ref as rr
from test_gpu_gbuffer import assert_planes_equal
from test_gpu_ssaa import resolve
from test_recip_guard_cpu import needs_division, needs_division3
from test_traversal_independent import matmul_xyz
from util import bits

pytestmark = pytest.mark.gpu

F = np.float32
ASYNC, COUNT, SHADOWS, REFRACT, SSAA2, GBUFFER = 4, 8, 32, 256, 2048, 8192
SCALES = [2.0 ** -130, 2.0 ** -100, 1.0, 2.0 ** 100, 2.0 ** 127]
# direction components that decide the guard: ordinary, denormal, zeros, infinities, NaN, >= 2^126
SPECIAL = np.array([1e-40, -3e-42, 0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** 126, -(2.0 ** 127), 1.5 * 2.0 ** 127, 2.0 ** -126, -(2.0 ** 125)], F)


def same_as_oracle(got, want):
    """rr.same_records -- bit for bit, field by field -- with ONE identification: the NaN an invalid operation (0 * inf, inf - inf) makes
    out of non-NaN operands. Its encoding is the architecture's, not the arithmetic's: 0xFFC00000 on the x86 the C oracle runs on,
    0x7FC00000 on the device -- with the division as with the short reciprocal, in the parent as here (crt_query_hits, which divides,
    shows it alone). A ray with an infinite or huge direction component against a root that is a leaf passes the triangle test with
    t = u = v = that NaN (every comparison false) and carries it into its record. Every other NaN -- a payload, a sign that came from
    an operand -- and every other bit must be equal. What this PR changes is pinned with no identification at all: the short form's
    records (crt_trace_rays) against the division's on the same device (crt_query_hits), check_batches below."""
    def canon(r):
        r = np.array(r, copy=True)
        for k in ("t", "u", "v"):
            w = r[k].view(np.uint32)
            w[w == 0xFFC00000] = 0x7FC00000
        return r
    return rr.same_records(canon(got), canon(want))


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")


def test_sweep_of_all_bit_patterns():
    hip = _lib.hip()
    with driver.Session(64, 36, device=0) as s:
        s.load_scene(scenes.get("tiny"))
        out = (C.c_uint64 * 4)()
        # a short range first: both sides of 2^126 and of the largest finite value, and the wrap to the denormals
        assert hip.crt_debug_recip_sweep(0x7E7FFF00, 1 << 12, out) == 0
        print(f"around 2^126: guarded {out[0]}, unguarded outside the guard {out[1]}, sent to the division although right {out[2]}")
        assert out[0] == 0 and out[1] == 0
        assert hip.crt_debug_recip_sweep(0, 1 << 32, out) == 0
        print(f"all 2^32 patterns: guarded mismatches {out[0]}, unguarded mismatches outside the guard {out[1]}, "
              f"patterns sent to the division although the short sequence is right {out[2]}, first offending pattern {out[3]:#x}")
        assert out[0] == 0 and out[1] == 0 and out[3] == 0xFFFFFFFFFFFFFFFF
        # what the guard costs: it may not send more than the denormals and the finite values from 2^126 to the division
        assert out[2] <= 2 * (0x007FFFFF + (0x7F800000 - 0x7E800000))
        assert hip.crt_debug_recip_sweep(0, (1 << 32) + 1, out) == _lib.CRT_E_BAD_ARGUMENT and hip.crt_debug_recip_sweep(0, 1, None) == _lib.CRT_E_BAD_ARGUMENT


def wave_batches(base_o, base_d, rng):
    """Four batches of 64 rays around (base_o, base_d): no special lane, one, every other lane, all -- a special lane has one, two or all
    three direction components replaced by SPECIAL values, or the whole direction scaled by 2^+-k"""
    out = []
    for name, lanes in (("none", []), ("one", [37]), ("half", list(range(0, 64, 2))), ("all", list(range(64)))):
        o = np.tile(np.asarray(base_o, F), (64, 1)) + rng.uniform(-0.05, 0.05, (64, 3)).astype(F)
        d = np.tile(np.asarray(base_d, F), (64, 1)) + rng.uniform(-0.3, 0.3, (64, 3)).astype(F)
        for n, lane in enumerate(lanes):
            kind = n % 5
            with np.errstate(all="ignore"):
                if kind < 3:
                    for c in rng.choice(3, kind + 1, replace=False):
                        d[lane, c] = SPECIAL[rng.randint(len(SPECIAL))]
                else:
                    d[lane] = d[lane] * F(2.0 ** (int(rng.randint(20, 127)) * (1 if kind == 3 else -1)))
        out.append((name, o, d))
    return out


def check_batches(s, a, batches, what):
    """records of crt_query_hits (counted) and of crt_trace_rays == the oracle's, counters too; returns how many lanes needed the division
    in some instance and how many did not, over the batches (the guard's numpy restatement on upstream's md)"""
    orc = oracle_lib.Oracle(a, nthreads=4)
    inv = [np.ascontiguousarray(inst["inv"], F) for inst in a["instances"]]
    slow = fast = hits = 0
    for name, o, d in batches:
        want, st = orc.closest_hits(o, d)
        got = s.query_hits(o, d)
        assert same_as_oracle(got, want), (what, name, "crt_query_hits")
        assert s.counters() == st, (what, name)
        rays = s.trace_rays(dev(o), dev(d)).numpy()
        assert same_as_oracle(rays, want), (what, name, "crt_trace_rays")
        assert rr.same_records(rays, got), (what, name, "short form against the division on the device")
        with np.errstate(all="ignore"):
            md = np.stack([np.ascontiguousarray(matmul_xyz(m, d, 0.0), F) for m in inv], 1)       # (64, instances, 3)
        lane_slow = needs_division3(md.view(np.uint32)).any(-1)
        slow += int(lane_slow.sum()); fast += int((~lane_slow).sum()); hits += int((want["instance"] >= 0).sum())
    return slow, fast, hits


def upload_diag_instances(s, scales):
    """the session's instance table with inverseTransform = diag(s, s, s, 1), s cycling through `scales`; returns the arenas the oracle sees"""
    a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
    inst = a["instances"]
    for k in range(len(inst)):
        m = np.zeros((4, 4), F)
        m[0, 0] = m[1, 1] = m[2, 2] = F(scales[k % len(scales)]); m[3, 3] = 1.0
        inst["inv"][k] = m
    assert s.hip.crt_upload_instances(inst.ctypes.data, 0, len(inst)) == 0
    return a


def quad_scene(tmp_path, same, ninst):
    """a mesh of two triangles (a unit quad at z = 0) -- or, same > 0, of `same` copies of its first triangle, which no split can
    separate: the root is one leaf -- in `ninst` instances"""
    pos = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, -1, 0], [1, 1, 0], [-1, 1, 0]], F)
    if same:
        pos = np.tile(pos[:3], (same, 1))
    n = len(pos)
    mesh = scenes.Mesh(pos, np.zeros((n, 2), F), np.tile([0, 0, 1], (n, 1)).astype(F), np.arange(n, dtype=np.int32).reshape(-1, 3), np.zeros(n // 3, np.int32))
    path = scenes._write_mesh(str(tmp_path), "quad", mesh, [((0.8, 0.6, 0.4), None)])
    sky = str(tmp_path / "sky.ppm")
    scenes.write_ppm(sky, scenes._skybox(64, 32))
    insts = [scenes.Instance(0, 0xFFFF, np.eye(4, dtype=F)) for _ in range(ninst)]
    return scenes.Scene("recip-quad", str(tmp_path), sky, [path], insts, (0.0, 0.0, 4.0), (0.0, 0.0, -1.0))


@pytest.mark.parametrize("name", ["two-triangles", "tiny"])
def test_direction_components_mixed_within_the_wave(tmp_path, name):
    rng = np.random.RandomState(11)
    sc = quad_scene(tmp_path, 0, len(SCALES)) if name == "two-triangles" else scenes.get("tiny")
    with driver.Session(64, 36, device=0) as s:
        s.load_scene(sc)
        # the scene as loaded (ordinary matrices): only the special direction components reach the guard
        a0 = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        batches = wave_batches(sc.camera_pos, sc.camera_front, rng)
        slow0, fast0, hits0 = check_batches(s, a0, batches, name + ", as loaded")
        # diag(s): the scale alone makes md denormal (2^-130), or >= 2^126 (2^127, and 2^100 under a scaled direction)
        a1 = upload_diag_instances(s, SCALES)
        o = np.asarray(sc.camera_pos, F) * F(0.25)
        slow1, fast1, hits1 = check_batches(s, a1, wave_batches(o, sc.camera_front, rng), name + ", diag(s)")
        print(f"{name}: as loaded {slow0} lanes need the division / {fast0} do not / {hits0} hits; diag(s) {slow1} / {fast1} / {hits1}")
        assert slow0 > 0 and fast0 > 64 and hits0 > 0 and slow1 > 0 and hits1 > 0


def test_triangle_determinant_mixed_within_the_wave(tmp_path):
    """One leaf of eight triangles, rewritten in place after the load: edges of 2^-70 and of 2^63, ordinary ones, and two degenerate ones
    last (parallel edges; three equal vertices). The lanes' directions are (0, 0, -1) 2^e with e from -60 to 66, so that
    a = edge1 . (d x edge2) is denormal, ordinary, >= 2^126 or infinite in different lanes of the same step."""
    sc = quad_scene(tmp_path, 8, 2)
    with driver.Session(64, 36, device=0) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        nodes, tris = a["nodes"], a["tris"]
        root = int(a["roots"][0])
        assert len(tris) == 8 and nodes["triCount"][root] == 8, "eight copies of one triangle were meant to stay one leaf"
        t, h = F(2.0 ** -70), F(2.0 ** 63)
        shapes = [
            ((0, 0, 0), (t, 0, 0), (0, t, 0)),                                 # edges 2^-70: a = 2^-140 |d|
            ((-h / 4, -h / 4, -8), (h - h / 4, -h / 4, -8), (-h / 4, h - h / 4, -8)),   # edges 2^63: a = 2^126 |d|
            ((-1, -1, -1), (1, -1, -1), (-1, 1, -1)),                          # ordinary
            ((0, 0, -2), (t, 0, -2), (0, h, -2)),                              # one edge of each: a = 2^-7 |d|
            ((-3, -3, -3), (3, -3, -3), (-3, 3, -3)),                          # ordinary, behind
            ((-h / 4, -h / 4, -9), (-h / 4, h - h / 4, -9), (h - h / 4, -h / 4, -9)),   # 2^63 again, the other winding
            ((-1, 0, -0.5), (0, 0, -0.5), (1, 0, -0.5)),                       # degenerate: parallel edges, a = 0
            ((0.25, 0.25, -0.25), (0.25, 0.25, -0.25), (0.25, 0.25, -0.25)),   # degenerate: one point, a = 0
        ]
        first = int(nodes["leftFirst"][root])
        for k, (v0, v1, v2) in enumerate(shapes):
            tris["v0"][first + k], tris["v1"][first + k], tris["v2"][first + k] = np.array(v0, F), np.array(v1, F), np.array(v2, F)
        assert s.hip.crt_upload_triangles(tris.ctypes.data, 0, tris.nbytes) == 0
        for order in (list(range(8)), [6, 7, 0, 1, 2, 3, 4, 5]):               # the degenerate pair last, then first (every later t poisoned)
            if order != list(range(8)):
                tris[first:first + 8] = tris[first:first + 8][order]
                assert s.hip.crt_upload_triangles(tris.ctypes.data, 0, tris.nbytes) == 0
            a1 = upload_diag_instances(s, [1.0, 2.0 ** -3])
            a1["tris"] = tris
            orc = oracle_lib.Oracle(a1, nthreads=4)
            e = np.concatenate([np.arange(-60, 68, 2)])                        # 64 lanes
            rng = np.random.RandomState(5)
            o = np.tile(np.array([2.0 ** -72, 2.0 ** -72, 1.0], F), (64, 1))
            o[1::4] = np.array([0.3, 0.2, 2.0], F)
            d = (np.array([0.0, 0.0, -1.0], F)[None, :] * (F(2.0) ** e.astype(F))[:, None]).astype(F)
            d[2::4, :2] = rng.uniform(-0.2, 0.2, (16, 2)).astype(F) * (F(2.0) ** e[2::4].astype(F))[:, None]
            want, st = orc.closest_hits(o, d)
            got = s.query_hits(o, d)
            assert same_as_oracle(got, want) and s.counters() == st, order
            rays = s.trace_rays(dev(o), dev(d)).numpy()
            assert same_as_oracle(rays, want), order
            assert rr.same_records(rays, got), (order, "short form against the division on the device")
            # the determinants of the first instance (md = d), upstream's operation order, and what the guard makes of them
            with np.errstate(all="ignore"):
                e1, e2 = tris["v1"][first:first + 8] - tris["v0"][first:first + 8], tris["v2"][first:first + 8] - tris["v0"][first:first + 8]
                hx = d[:, None, 1] * e2[None, :, 2] - d[:, None, 2] * e2[None, :, 1]
                hy = d[:, None, 2] * e2[None, :, 0] - d[:, None, 0] * e2[None, :, 2]
                hz = d[:, None, 0] * e2[None, :, 1] - d[:, None, 1] * e2[None, :, 0]
                det = ((e1[None, :, 0] * hx + e1[None, :, 1] * hy) + e1[None, :, 2] * hz).astype(F)
            slow = needs_division(det.view(np.uint32).reshape(-1)).reshape(det.shape)
            mixed = int((slow.any(0) & ~slow.all(0)).sum())
            print(f"order {order}: triangles whose determinant needs the division in some lanes only: {mixed} of 8; zero determinants {int((det == 0).sum())}; "
                  f"hits {int((want['instance'] >= 0).sum())}, NaN t in records {int(np.isnan(want['t']).sum())}")
            assert mixed >= 3 and (det == 0).any() and (want["instance"] >= 0).any()


@pytest.mark.parametrize("size", [(64, 36), (203, 117)])
def test_frames_are_the_oracle_frames(monkeypatch, size, nthreads):
    monkeypatch.setenv("CRT_FRAMES_IN_FLIGHT", "3")
    monkeypatch.delenv("CRT_KERNEL", raising=False)
    w, h = size
    sc = scenes.get("tiny")
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        a = s.arenas()
        orc = oracle_lib.Oracle(a, nthreads=nthreads)
        iv, ip, pos = s.camera()
        rays = orc.raygen(w, h, iv, ip)
        plain = orc.trace(rays, pos, sc.sun_angle)
        hi, hi_st = orc.trace(orc.raygen(2 * w, 2 * h, iv, ip), pos, sc.sun_angle)
        forms = {"plain": (0, plain), "shadows": (SHADOWS, orc.trace(rays, pos, sc.sun_angle, shadows=True)),
                 "refraction": (REFRACT, orc.trace(rays, pos, sc.sun_angle, refraction=True)), "ssaa2": (SSAA2, (resolve(hi, 2), hi_st)),
                 "gbuffer": (GBUFFER, plain)}
        planes = gbuffer_ref.reference_planes(a, orc, rays, pos)
        for name, (flags, (want, st)) in forms.items():
            s.render_raw(flags)                                               # synchronous
            assert np.array_equal(bits(s.read_output()), bits(want)), (name, "synchronous")
            if flags & GBUFFER:
                assert_planes_equal(s.read_gbuffer_raw(), planes, what="synchronous")
            for _ in range(4):                                                # three in flight: every slot, and one of them twice
                s.render_raw(flags | ASYNC)
            assert np.array_equal(bits(s.read_output()), bits(want)), (name, "in flight")
            if flags & GBUFFER:
                assert_planes_equal(s.read_gbuffer_raw(), planes, what="in flight")
            else:                                                             # (the G-buffer kernels take no counters)
                s.render_raw(flags | COUNT)                                   # the counted frame: the same in every build
                assert np.array_equal(bits(s.read_output()), bits(want)), (name, "counted")
                assert s.counters() == st, name
        # the G-buffer frame's counted neighbour is the plain counted frame
        s.render_raw(COUNT)
        assert np.array_equal(bits(s.read_output()), bits(plain[0])) and s.counters() == plain[1]
