"""The guarded float skybox index on the device (clraytracer_amd/csrc/crt_device.h: sample_skybox_guarded), smallest shapes only. The first
three parts run tools/ubench/sky_index, a program over the library's own header built by `make` with the library's flags (its kernels are no
part of libcrt_hip.so, whose kernel list stays what it was); the frames run the library.

  directions   the shipped index equals the device's double-only index lane for lane, the decided flags are tests/sky_fast_ref.py's lane for
               lane (which ties the CPU proof, tests/test_sky_index_cpu.py, to the device code), and against the oracle's orc_sample_skybox
               the rule of tests/test_gpu_texel_lookup.py holds: exact-argument rays exact, the others within texel_ref.neighbour_indices
  wave shapes  the result of a lane does not depend on which lanes share its call
  sweeps       all 2^32 patterns of d.y and every float q in [0, 1]: no lane differs from the double form, and the decided totals are the
               ones tools/sky_index_bounds.c recorded on the CPU (profiles/sky_index_bounds.txt)
  frames       the default kernel's frame against the counted launch's (which keeps the double form: an independent path) and the oracle's
"""
import os
import subprocess

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import oracle_lib
import sky_fast_ref as S
import texel_ref as T
from test_gpu_ssaa import resolve
from test_gpu_texel_lookup import render
from util import bits

pytestmark = pytest.mark.gpu

F = np.float32
ASYNC, COUNT, SHADOWS, SSAA2 = 4, 8, 32, 2048
NONE = 0xFFFFFFFFFFFFFFFF
TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "ubench", "sky_index")


def run_tool(*args):
    return subprocess.run([TOOL] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)


def sky_index(tmp, d, tw, th):
    """tools/ubench/sky_index dirs: (shipped index, double-only index, decided flag) per direction; 64 consecutive directions share a call"""
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    n = len(d)
    src, dst = os.path.join(str(tmp), "dirs.f32"), os.path.join(str(tmp), "out.bin")
    d.tofile(src)
    p = run_tool("dirs", src, n, tw, th, dst)
    assert p.returncode == 0, (p.returncode, p.stderr)
    raw = np.fromfile(dst, np.uint8)
    assert len(raw) == 9 * n
    idx = raw[:8 * n].view(np.int32)
    decided = raw[8 * n:]
    assert set(np.unique(decided)) <= {0, 1}
    return idx[:n].astype(np.int64), idx[n:].astype(np.int64), decided.astype(bool)


def hexbits(v):
    return "%08x" % int(np.array([v], F).view(np.uint32)[0])


def sweep(axis, fixed, first, n, tw, th):
    """tools/ubench/sky_index sweep: [decided, undecided, differing, first differing pattern]"""
    p = run_tool("sweep", axis, first, n, hexbits(fixed[0]), hexbits(fixed[1]), hexbits(fixed[2]), tw, th)
    assert p.returncode == 0, (p.returncode, p.stderr)
    return [int(v) for v in p.stdout.split()]


def family_rays(name):
    iv, ip, _ = T.family_view(name)
    rays = np.empty((T.FRAME, T.FRAME, 3), F)
    oracle_lib.lib().orc_raygen(rays.ctypes.data, T.FRAME, T.FRAME, oracle_lib.f32(iv)[0], oracle_lib.f32(ip)[0])
    return rays.reshape(-1, 3)


def oracle_index(d, tw, th):
    tex = np.zeros(1, _lib.TEXTURE_DTYPE)
    tex["width"], tex["height"], tex["offset"] = tw, th, 2
    L = oracle_lib.lib()
    return np.array([L.orc_sample_skybox(oracle_lib.f32(v)[0], tex.ctypes.data) for v in d], np.int64)


@pytest.fixture(scope="module")
def directions():
    rng = np.random.RandomState(77)
    r = rng.standard_normal((4096, 3))
    out = {f: family_rays(f) for f in T.SKY_FAMILIES}
    out["random"] = (r / np.linalg.norm(r, axis=1)[:, None]).astype(F)
    return out


@pytest.mark.parametrize("sky", T.SKY_SIZES, ids=["64x32", "90x37"])
def test_directions_mode(tmp_path, directions, sky):
    tw, th = sky
    sets = dict(directions)
    sets["column edges"], sets["row edges"] = S.edge_aimed_columns(tw), S.edge_aimed_rows(th)
    d = np.concatenate(list(sets.values()))
    assert len(d) <= 65536
    shipped, double, decided = sky_index(tmp_path, d, tw, th)
    want_decided = S.decide(d, tw, th)[0]
    n = tw * th + 2
    oracle = T.clamp_index(oracle_index(d, tw, th), n)
    at = 0
    for name, part in sets.items():
        sl = slice(at, at + len(part))
        at += len(part)
        differing, on_exact, unexplained = T.judge(T.clamp_index(shipped[sl], n), oracle[sl], part, tw, th, n)
        print(f"{name} on {tw}x{th}: {len(part)} directions, {int((~decided[sl]).sum())} undecided, shipped != double-only {int((shipped[sl] != double[sl]).sum())}, "
              f"flags != restatement {int((decided[sl] != want_decided[sl]).sum())}, vs oracle {differing} differing ({on_exact} exact-argument, {unexplained} unexplained)")
        assert np.array_equal(shipped[sl], double[sl]), name
        assert np.array_equal(decided[sl], want_decided[sl]), name
        assert on_exact == 0 and unexplained == 0, name
    assert decided.any() and (~decided).any()


def test_wave_shapes(tmp_path, directions):
    """64 consecutive directions share a call: a lane's index and flag are what they are in any other company"""
    tw, th = 90, 37
    pool = np.concatenate([directions["random"], S.edge_aimed_rows(th), directions["seam"]])
    flags = S.decide(pool, tw, th)[0]
    D, U = pool[flags][:64], pool[~flags][:64]
    assert len(D) == 64 and len(U) == 64
    base = np.concatenate([D, U])
    b_shipped, b_double, b_decided = sky_index(tmp_path, base, tw, th)
    assert np.array_equal(b_shipped, b_double) and b_decided[:64].all() and not b_decided[64:].any()
    cases = {"n = 1": [0], "n = 63": list(range(63)), "n = 64": list(range(64)), "n = 65": list(range(64)) + [0],
             "one undecided lane at lane 0": [64] + list(range(63)), "one undecided lane at lane 63": list(range(63)) + [64 + 5],
             "no undecided lane": list(range(63, -1, -1)), "only undecided lanes": list(range(64, 128)),
             "alone in the second call": list(range(64)) + [64 + 9], "mixed": [k // 2 + 64 * (k % 2) for k in range(128)]}
    for name, pick in cases.items():
        pick = np.array(pick)
        shipped, double, decided = sky_index(tmp_path, base[pick], tw, th)
        assert np.array_equal(shipped, b_shipped[pick]) and np.array_equal(double, b_double[pick]) and np.array_equal(decided, b_decided[pick]), name
    # nothing to sweep, and the argument checks: a count above 2^32, an axis that is none, a direction file that is too short
    assert sweep(1, (0.3, 0.0, -0.9), 0, 0, tw, th) == [0, 0, 0, NONE]
    assert run_tool("sweep", 1, 0, (1 << 32) + 1, hexbits(0.3), hexbits(0.0), hexbits(-0.9), tw, th).returncode == 2
    assert run_tool("sweep", 3, 0, 1, hexbits(0.3), hexbits(0.0), hexbits(-0.9), tw, th).returncode == 2
    base[:4].tofile(os.path.join(str(tmp_path), "short.f32"))
    assert run_tool("dirs", os.path.join(str(tmp_path), "short.f32"), 5, tw, th, os.path.join(str(tmp_path), "none.bin")).returncode == 2
    assert run_tool("dirs").returncode == 2


SWEEP_SIZES = ((64, 32), (90, 37), (2048, 1024))


@pytest.mark.parametrize("sky", SWEEP_SIZES, ids=["64x32", "90x37", "2048x1024"])
def test_sweep_of_every_pattern_of_dy(sky):
    tw, th = sky
    rec, sweeps = S.recorded()
    x, z = rec["sweep_xz"]
    # a short range first: both sides of |y| = 1 and the wrap from NaN to +0
    assert sweep(1, (x, 0.0, z), 0x3F7FFF00, 1 << 9, tw, th)[2:] == [0, NONE]
    assert sweep(1, (x, 0.0, z), 0xFFFFFF00, 1 << 9, tw, th)[2:] == [0, NONE]
    decided, undecided, differing, first = sweep(1, (x, 0.0, z), 0, 1 << 32, tw, th)
    print(f"all 2^32 patterns of d.y on {tw}x{th}: decided {decided}, undecided {undecided}, differing {differing}, first {first:#x}; recorded decided {sweeps[('y', tw, th)]}")
    assert differing == 0 and first == NONE
    assert decided + undecided == 1 << 32 and decided == sweeps[("y", tw, th)]


@pytest.mark.parametrize("sky", SWEEP_SIZES, ids=["64x32", "90x37", "2048x1024"])
def test_sweep_of_every_float_q(sky):
    """d = (q, y, -1), not normalised: y = 0 as the sweep is defined (d.y = 0 is never decided: every lane takes the double form), and the recorded
    y beside it, at which the float decision answers"""
    tw, th = sky
    rec, sweeps = S.recorded()
    n = 0x3F800000 + 1
    for key, y in (("q0", F(0.0)), ("q", rec["sweep_y"])):
        decided, undecided, differing, first = sweep(0, (0.0, y, -1.0), 0, n, tw, th)
        print(f"every float q in [0, 1], d = (q, {float(y):.9g}, -1) on {tw}x{th}: decided {decided}, undecided {undecided}, differing {differing}; recorded decided {sweeps[(key, tw, th)]}")
        assert differing == 0 and first == NONE
        assert decided + undecided == n and decided == sweeps[(key, tw, th)]
    assert sweeps[("q0", tw, th)] == 0 and sweeps[("q", tw, th)] > n // 8


# ------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 64), (203, 117)], ids=["64x64", "203x117"])
def test_frames_of_tiny(size, nthreads, monkeypatch):
    """`tiny` (a 64 x 32 sky): the default kernel's frame = the counted launch's = the oracle's, bit for bit -- synchronous and with three frames
    in flight, plain, with shadow rays and supersampled; 203 x 117 has partial tiles on both edges. (The shadow-ray kernel without the instance
    tree keeps the double form, DESIGN.md 4a: the guarded shadow-ray kernel runs in test_family_frames_over_a_coded_sky.)"""
    monkeypatch.setenv("CRT_FRAMES_IN_FLIGHT", "3")
    for v in ("CRT_KERNEL", "CRT_TLAS"):
        monkeypatch.delenv(v, raising=False)
    w, h = size
    sc = scenes.get("tiny")
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        orc = oracle_lib.Oracle(s.arenas(), nthreads=nthreads)
        iv, ip, pos = s.camera()
        rays = orc.raygen(w, h, iv, ip)
        hi, hi_st = orc.trace(orc.raygen(2 * w, 2 * h, iv, ip), pos, sc.sun_angle)
        forms = {"plain": (0, orc.trace(rays, pos, sc.sun_angle)), "shadows": (SHADOWS, orc.trace(rays, pos, sc.sun_angle, shadows=True)),
                 "ssaa2": (SSAA2, (resolve(hi, 2), hi_st))}
        for name, (flags, (want, st)) in forms.items():
            assert st["misses"] > 0 and st["hits"] > 0
            s.render_raw(flags)
            default = s.read_output()
            assert not s.last_kernel().split("<")[1].startswith("1"), s.last_kernel()
            s.render_raw(flags | COUNT)
            counted = s.read_output()
            assert s.last_kernel().split("<")[1].startswith("1"), s.last_kernel()
            assert s.counters() == st, name
            assert np.array_equal(bits(default), bits(counted)), (name, "default against counted")
            assert np.array_equal(bits(default), bits(want)), (name, "default against the oracle")
            for _ in range(4):                                                # three in flight: every slot, and one of them twice
                s.render_raw(flags | ASYNC)
            assert np.array_equal(bits(s.read_output()), bits(want)), (name, "in flight")


class FamilyReference:
    """What the oracle says about the empty scene of a loaded target at w x h, per family: the rays, the clamped pool indices, the frame and the
    supersampled frame resolved (tests/test_gpu_texel_lookup.py: Sky, which is fixed to 64 x 64)"""

    def __init__(self, arenas, sky, w, h, nthreads):
        self.a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in arenas.items()}
        self.W, self.H = sky
        self.n = (len(self.a["texels"]) + 2) // 3
        self.layout = T.pool_layout(self.a)
        orc = oracle_lib.Oracle(self.a, nthreads=nthreads)
        orc.s.numInstances = 0
        tex = np.ascontiguousarray(self.a["textures"][2:3])
        L = oracle_lib.lib()
        self.rays, self.index, self.frame, self.resolved = {}, {}, {}, {}
        for f in T.SKY_FAMILIES:
            iv, ip, pos = T.family_view(f)
            r = orc.raygen(w, h, iv, ip)
            self.rays[f] = r.reshape(-1, 3)
            idx = np.array([L.orc_sample_skybox(oracle_lib.f32(d)[0], tex.ctypes.data) for d in self.rays[f]], np.int64)
            self.index[f] = T.clamp_index(idx, self.n)
            self.frame[f] = orc.trace(r, pos, SUN)[0]
            self.resolved[f] = resolve(orc.trace(orc.raygen(2 * w, 2 * h, iv, ip), pos, SUN)[0], 2)

    def check_frame(self, frame, family, what):
        """the rule of tests/test_gpu_texel_lookup.py: exact-argument rays exact, every other differing index explained by a neighbouring float of
        the double angles, at most two of them; and where the device read the oracle's texel, the pixel is the oracle's bit for bit"""
        tag, x, y = (np.asarray(v).reshape(-1) for v in T.decode_sky(frame))
        idx = np.full(tag.shape, -1, np.int64)
        idx[tag == T.WHITE], idx[tag == T.BLACK] = 0, 1
        for t, off, tw, th in self.layout:
            m = (tag == t) & (x < tw) & (y < th)
            idx[m] = off + y[m] * tw + x[m]
        differing, on_exact, unexplained = T.judge(idx, self.index[family], self.rays[family], self.W, self.H, self.n)
        print(f"{what} {family}: device vs oracle: {differing} differing indices ({on_exact} on exact-argument rays, {unexplained} unexplained)")
        assert on_exact == 0 and unexplained == 0 and differing <= 2, (what, family, differing, on_exact, unexplained)
        same = idx == self.index[family]
        assert np.array_equal(bits(frame).reshape(-1, 4)[same], bits(self.frame[family]).reshape(-1, 4)[same]), (what, family)
        return idx


SUN = -1.96
_REFERENCES = {}
# CRT_TLAS -> {flags: the uncounted kernel, which runs the guarded form (DESIGN.md 4a lists the instantiations that keep the double form: with shadow
# rays only the kernels with the instance tree are guarded)}
FAMILY_KERNELS = {"0": {0: "crt_trace_kernel<0,0,0,0,0>", SSAA2: "crt_trace_ssaa_kernel<0,0,0,0>"},
                  "1": {0: "crt_trace_kernel<0,0,0,1,0>", SHADOWS: "crt_trace_kernel<0,0,1,1,0>", SSAA2: "crt_trace_ssaa_kernel<0,0,1,0>"}}


@pytest.mark.parametrize("tlas", ["0", "1"], ids=["linear", "tree"])
@pytest.mark.parametrize("size", [(64, 64), (203, 117)], ids=["64x64", "203x117"])
def test_family_frames_over_a_coded_sky(tmp_path, size, tlas, nthreads, monkeypatch):
    """Every edge family over the 64 x 32 index-coded sky, no instance, through every guarded Trace kernel a flag reaches -- plain, with shadow rays,
    supersampled; synchronous and with three frames in flight: the frame is the counted launch's bit for bit (the counted launch keeps the double
    form), it is judged against the oracle as tests/test_gpu_texel_lookup.py judges it (the supersampled one: equal to the oracle's resolved frame),
    and `seam` decodes to texel_ref.sky_index's texels"""
    monkeypatch.delenv("CRT_KERNEL", raising=False)
    monkeypatch.setenv("CRT_TLAS", tlas)                      # read by crt_init
    monkeypatch.setenv("CRT_FRAMES_IN_FLIGHT", "3")
    w, h = size
    sky = (64, 32)
    s = driver.Session(w, h, device=0)
    with s:
        s.load_scene(T.target_scene(tmp_path, sky))
        if size not in _REFERENCES:                            # computed once per size: the target's arenas are the same in every session
            _REFERENCES[size] = FamilyReference(s.arenas(), sky, w, h, nthreads)
        ref = _REFERENCES[size]
        for f in T.SKY_FAMILIES:
            view = T.family_view(f)
            for flags, kernel in FAMILY_KERNELS[tlas].items():
                what = f"CRT_TLAS={tlas} flags {flags} at {w}x{h}"
                render(s, flags, view, 0)
                default = s.read_output()
                assert s.last_kernel() == kernel, (what, s.last_kernel())
                render(s, flags | COUNT, view, 0)
                assert s.last_kernel().split("<")[1].startswith("1"), s.last_kernel()
                assert np.array_equal(bits(default), bits(s.read_output())), (what, f, "default against counted")
                for _ in range(4):                                            # three in flight: every slot, and one of them twice
                    render(s, flags | ASYNC, view, 0)
                assert np.array_equal(bits(s.read_output()), bits(default)), (what, f, "in flight")
                if flags & SSAA2:
                    differ = int((bits(default) != bits(ref.resolved[f])).any(axis=2).sum())
                    print(f"{what} {f}: {differ} pixels differ from the resolved oracle frame")
                    assert differ == 0, (what, f)
                    continue
                idx = ref.check_frame(default, f, what)
                if f == "seam" and flags == 0:
                    want = T.clamp_index(T.sky_index(ref.rays[f], *sky)[2], ref.n)
                    differing, on_exact, unexplained = T.judge(idx, want, ref.rays[f], sky[0], sky[1], ref.n)
                    print(f"seam at {w}x{h}: {differing} texels differ from the restatement ({on_exact} exact-argument, {unexplained} unexplained)")
                    assert on_exact == 0 and unexplained == 0 and differing <= 2
