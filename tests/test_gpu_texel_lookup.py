"""The texel a miss and a hit read, on the GPU, at the edges of both lookups (sample_skybox, sample_texture, f2i, clamp_texel, the texel
relayout): the skybox and the textures are index-coded maps (tests/texel_ref.py), so every pixel decodes to the texel the kernel read and
is compared with the oracle's index -- at the atan2 branch cut with both signed zeros, the poles, the axes, indices below 0 and past the
sky's last row, NaN / infinite / all-zero directions; negative UVs, `u - floorf(u) == 1.0f`, non-power-of-two maps and the end of the pool.
tests/test_texel_lookup_cpu.py proves that the views reach those cases and pins the references.

The rule for a sky pixel (texel_ref.judge): a ray whose atan2 / acos arguments are exact must read the oracle's texel; any other difference
must be one of texel_ref.neighbour_indices (the float32 atan2pi / acospi one ulp either way: the only readings in which OCML and glibc may
differ), at most 2 a frame. Albedo words get no allowance at all. The counts are printed.

RayGen buffers are compared bit for bit except that a NaN component only has to be a NaN on both sides: the sign and payload of the NaN an
invalid operation produces are the processor's (x86: negative quiet NaN), not the algorithm's."""
import ctypes as C

import numpy as np
import pytest

from clraytracer_amd import _lib, driver
import gbuffer_ref
import oracle_lib
import texel_ref as T
from test_gpu_ssaa import resolve
from util import bits

pytestmark = pytest.mark.gpu

WRITE_RAYS, ASYNC, COUNT, SHADOWS, UNORM8, REFRACT = 2, 4, 8, 32, 64, 256
SSAA2, GBUFFER = 2048, 8192
N = T.FRAME
SUN = -1.96
KERNEL_OF = {"wavefront": "crt_primary_kernel<", "refill": "crt_trace_refill_kernel<", "block": "crt_trace_block_kernel<", "ldstop": "crt_trace_ldstop_kernel<"}


def render_rc(s, flags, view, num_meshes=None):
    """crt_render's return code for explicit matrices and, if given, an explicit instance count"""
    a, _, _ = s.trace_args(SUN)
    iv, ip = np.ascontiguousarray(view[0], np.float32).reshape(16), np.ascontiguousarray(view[1], np.float32).reshape(16)
    a.cameraPos[0], a.cameraPos[1], a.cameraPos[2] = (float(v) for v in view[2])
    if num_meshes is not None:
        a.numMeshes = num_meshes
    fp = C.POINTER(C.c_float)
    return s.hip.crt_render(C.byref(a), iv.ctypes.data_as(fp), ip.ctypes.data_as(fp), int(flags))


def render(s, flags, view, num_meshes=None):
    _lib.check(render_rc(s, flags, view, num_meshes), "crt_render")


class Sky:
    """What the oracle says about the empty scene of one loaded target: per family the rays, the clamped indices, the frame and the counters"""

    def __init__(self, arenas, sky, nthreads):
        self.a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in arenas.items()}
        self.W, self.H = sky
        self.n = (len(self.a["texels"]) + 2) // 3
        self.orc = oracle_lib.Oracle(self.a, nthreads=nthreads)
        self.layout = T.pool_layout(self.a)
        tex = np.ascontiguousarray(self.a["textures"][2:3])
        L = oracle_lib.lib()
        self.rays, self.index, self.stats, self.frame = {}, {}, {}, {}
        self.orc.s.numInstances = 0
        for f in T.SKY_FAMILIES:
            iv, ip, pos = T.family_view(f)
            r = self.orc.raygen(N, N, iv, ip)
            self.rays[f] = r
            idx = np.array([L.orc_sample_skybox(oracle_lib.f32(d)[0], tex.ctypes.data) for d in r.reshape(-1, 3)], np.int64)
            self.index[f] = T.clamp_index(idx, self.n)
            self.frame[f], self.stats[f] = self.orc.trace(r, pos, SUN)
        self.orc.s.numInstances = len(self.a["instances"])

    def pool_index(self, tag, x, y):
        """The pool index a decoded texel stands for (-1: the bytes are no texel of this pool)"""
        idx = np.full(tag.shape, -1, np.int64)
        idx[tag == T.WHITE], idx[tag == T.BLACK] = 0, 1
        for t, off, w, h in self.layout:
            m = (tag == t) & (x < w) & (y < h)
            idx[m] = off + y[m] * w + x[m]
        return idx

    def check_indices(self, got, family, what):
        """The rule of the module docstring for the decoded (tag, x, y) of every pixel of one frame"""
        d = self.rays[family].reshape(-1, 3)
        idx = self.pool_index(*[np.asarray(g).reshape(-1) for g in got])
        differing, on_exact, unexplained = T.judge(idx, self.index[family], d, self.W, self.H, self.n)
        print(f"{what} {family} on {self.W}x{self.H}: device vs oracle: {differing} differing indices ({on_exact} on exact-argument rays, {unexplained} unexplained)")
        assert on_exact == 0 and unexplained == 0 and differing <= 2, (what, family, differing, on_exact, unexplained)
        return idx == self.index[family]

    def check_frame(self, frame, family, what):
        """... and where the device read the oracle's texel, the pixel is the oracle's, bit for bit"""
        assert frame.shape == (N, N, 4) and (frame[..., 3] == 1.0).all(), (what, family)
        same = self.check_indices(T.decode_sky(frame), family, what)
        assert np.array_equal(bits(frame).reshape(-1, 4)[same], bits(self.frame[family]).reshape(-1, 4)[same]), (what, family)


def open_target(tmp_path, sky, nthreads, maps=T.TARGET_MAPS):
    s = driver.Session(N, N, device=0)
    try:
        s.load_scene(T.target_scene(tmp_path, sky, maps=maps))
        return s, Sky(s.arenas(), sky, nthreads)
    except Exception:
        s.close()
        raise


def rays_equal(got, want):
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(w)
    return np.array_equal(np.isnan(g), nan) and np.array_equal(bits(g)[~nan], bits(w)[~nan])


# ------------------------------------------------------------------------------------------------
# sky, empty scene
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sky", T.SKY_SIZES, ids=["64x32", "90x37"])
def test_sky_texels_of_the_empty_scene(tmp_path, sky, nthreads, monkeypatch):
    for v in ("CRT_KERNEL", "CRT_TLAS"):
        monkeypatch.delenv(v, raising=False)
    s, ref = open_target(tmp_path, sky, nthreads)
    with s:
        for f in T.SKY_FAMILIES:
            view = T.family_view(f)
            render(s, WRITE_RAYS, view, 0)
            assert rays_equal(s.read_rays(), ref.rays[f]), f
            ref.check_frame(s.read_output(), f, "plain+rays")
            render(s, COUNT, view, 0)
            assert s.last_kernel() == "crt_trace_kernel<1,0,0,0,0>"
            ref.check_frame(s.read_output(), f, "count")
            cnt = s.counters()
            assert cnt == ref.stats[f] and cnt["misses"] == N * N and cnt["traversals"] == 0 and cnt["hits"] == 0, (f, cnt)


@pytest.mark.parametrize("sky", T.SKY_SIZES, ids=["64x32", "90x37"])
def test_sky_texels_under_every_flag_of_the_default_kernel(tmp_path, sky, nthreads, monkeypatch):
    for v in ("CRT_KERNEL", "CRT_TLAS"):
        monkeypatch.delenv(v, raising=False)
    s, ref = open_target(tmp_path, sky, nthreads)
    kernels = {0: "crt_trace_kernel<0,0,0,0,0>", SHADOWS: "crt_trace_kernel<0,0,1,0,0>", REFRACT: "crt_trace_kernel<0,0,0,0,1>",
               GBUFFER: "crt_trace_gbuffer_kernel<0,0,0>", ASYNC: "crt_trace_kernel<0,0,0,0,0>"}
    with s:
        for f in T.SKY_FAMILIES:
            view = T.family_view(f)
            for flags, kernel in kernels.items():
                render(s, flags, view, 0)
                assert s.last_kernel() == kernel, (flags, s.last_kernel())
                ref.check_frame(s.read_output(), f, f"flags {flags}")
                if flags == GBUFFER:                      # every pixel a miss: the miss record in all three planes
                    p = s.read_gbuffer_raw()
                    assert (p["ids"]["instance"] == -1).all() and (p["albedo"] == 0).all() and (p["geometry"]["t"] == gbuffer_ref.MISS_T).all()


@pytest.mark.parametrize("tlas", ["0", "1"], ids=["linear", "tree"])
@pytest.mark.parametrize("sky", T.SKY_SIZES, ids=["64x32", "90x37"])
def test_sky_texels_with_either_candidate_search(tmp_path, sky, tlas, nthreads, monkeypatch):
    monkeypatch.delenv("CRT_KERNEL", raising=False)
    monkeypatch.setenv("CRT_TLAS", tlas)                      # read by crt_init
    s, ref = open_target(tmp_path, sky, nthreads)
    with s:
        names = set()
        for f in T.SKY_FAMILIES:
            view = T.family_view(f)
            for flags in (0, COUNT, SHADOWS):
                render(s, flags, view, 0)
                names.add(s.last_kernel())
                assert s.last_kernel().startswith("crt_trace_kernel<"), s.last_kernel()
                ref.check_frame(s.read_output(), f, f"CRT_TLAS={tlas} flags {flags}")
                if flags == COUNT:
                    assert s.counters() == ref.stats[f], f
        print(f"CRT_TLAS={tlas}: {sorted(names)}")
        # the instantiation follows the forced search even with no instance to find (crt_frame.h use_tlas: the tree of the uploaded instance exists)
        assert names == {"crt_trace_kernel<%d,0,%d,%s,0>" % (c, sh, tlas) for c, sh in ((0, 0), (1, 0), (0, 1))}


@pytest.mark.parametrize("form", ["wavefront", "refill", "block", "ldstop"])
@pytest.mark.parametrize("sky", T.SKY_SIZES, ids=["64x32", "90x37"])
def test_sky_texels_of_every_kernel_form(tmp_path, sky, form, nthreads, monkeypatch):
    monkeypatch.delenv("CRT_TLAS", raising=False)
    monkeypatch.setenv("CRT_KERNEL", form)                    # read by crt_init
    s, ref = open_target(tmp_path, sky, nthreads)
    with s:
        for f in T.SKY_FAMILIES:
            view = T.family_view(f)
            for flags in (0, COUNT, ASYNC):
                render(s, flags, view, 0)
                assert s.last_kernel().startswith(KERNEL_OF[form]), (form, s.last_kernel())
                ref.check_frame(s.read_output(), f, f"{form} flags {flags}")
                if flags == COUNT:
                    assert s.counters() == ref.stats[f], (form, f)
            name = s.last_kernel()
            for flags in (SHADOWS, REFRACT, GBUFFER):     # what the form refuses stays refused, and renders nothing
                assert render_rc(s, flags, view, 0) == _lib.CRT_E_UNSUPPORTED, (form, flags)
                assert s.last_kernel() == name


@pytest.mark.parametrize("sky", T.SKY_SIZES, ids=["64x32", "90x37"])
def test_supersampled_sky_is_the_resolved_oracle_frame(tmp_path, sky, nthreads, monkeypatch):
    """An averaged pixel cannot be decoded: the SSAA2 frame is the oracle's 128 x 128 frame of the same matrices, resolved (test_gpu_ssaa.resolve)"""
    for v in ("CRT_KERNEL", "CRT_TLAS"):
        monkeypatch.delenv(v, raising=False)
    s, ref = open_target(tmp_path, sky, nthreads)
    with s:
        ref.orc.s.numInstances = 0
        for f in T.SKY_FAMILIES:
            iv, ip, pos = T.family_view(f)
            hi, st = ref.orc.trace(ref.orc.raygen(2 * N, 2 * N, iv, ip), pos, SUN)
            render(s, SSAA2 | COUNT, (iv, ip, pos), 0)
            assert s.last_kernel() == "crt_trace_ssaa_kernel<1,0,0,0>", s.last_kernel()
            got = s.read_output()
            differ = int((bits(got) != bits(resolve(hi, 2))).any(axis=2).sum())
            print(f"SSAA2 {f} on {sky[0]}x{sky[1]}: {differ} pixels differ from the resolved oracle frame")
            assert differ == 0, f
            assert s.counters() == st and st["misses"] == 4 * N * N


def test_rgba8_target_keeps_every_coded_byte(tmp_path, nthreads, monkeypatch):
    for v in ("CRT_KERNEL", "CRT_TLAS"):
        monkeypatch.delenv(v, raising=False)
    s, ref = open_target(tmp_path, (90, 37), nthreads)
    with s:
        for f in ("seam", "south"):
            render(s, UNORM8, T.family_view(f), 0)
            rgba = s.read_output_rgba8()
            assert rgba.shape == (N, N, 4) and (rgba[..., 3] == 255).all()
            ref.check_indices(T.decode_bytes(rgba), f, "RGBA8")
            # the bytes are the texel's own: what the float frame decodes to
            render(s, 0, T.family_view(f), 0)
            plain = T.decode_sky(s.read_output())
            for a_, b_ in zip(T.decode_bytes(rgba), plain):
                assert np.array_equal(a_, b_), f


# ------------------------------------------------------------------------------------------------
# albedo
# ------------------------------------------------------------------------------------------------
def target_reference(ref):
    rays = ref.orc.raygen(N, N, *T.TARGET_VIEW[:2])
    pos = T.TARGET_VIEW[2]
    d = np.ascontiguousarray(rays.reshape(-1, 3), np.float32)
    rec, _ = ref.orc.closest_hits(np.tile(pos, (len(d), 1)), d)
    return rays, rec, gbuffer_ref.reference_planes(ref.a, ref.orc, rays, pos)


def spill_pixels(ref, rec):
    """(pixels whose interpolated u has u - floorf(u) == 1.0f (uS == width), v - floorf(v) of every pixel)"""
    uv = T.interpolated_uv(ref.a, rec)
    uvf = uv - np.floor(uv)
    return np.flatnonzero(uvf[:, 0] == np.float32(1.0)), uvf[:, 1]


@pytest.mark.parametrize("tlas", ["0", "1"], ids=["linear", "tree"])
def test_albedo_words_decode_to_the_reference_texels(tmp_path, tlas, nthreads, monkeypatch):
    monkeypatch.delenv("CRT_KERNEL", raising=False)
    monkeypatch.setenv("CRT_TLAS", tlas)
    s, ref = open_target(tmp_path, (90, 37), nthreads)
    with s:
        rays, rec, want = target_reference(ref)
        render(s, GBUFFER | WRITE_RAYS, T.TARGET_VIEW)
        assert s.last_kernel() == "crt_trace_gbuffer_kernel<0,%s,0>" % tlas, s.last_kernel()
        assert rays_equal(s.read_rays(), rays)
        got = s.read_gbuffer_raw()
        ids = got["ids"].reshape(-1)
        assert (rec["instance"] == 0).all()
        assert np.array_equal(ids["instance"], rec["instance"]) and np.array_equal(ids["tri"], rec["tri"])
        for plane, field in ((ids["u"], "u"), (ids["v"], "v"), (got["geometry"]["t"].reshape(-1), "t")):
            assert np.array_equal(bits(plane), bits(rec[field])), field
        g, w_ = T.decode_albedo(got["albedo"]), T.decode_albedo(want["albedo"])
        wrong = (g[0] != w_[0]) | (g[1] != w_[1]) | (g[2] != w_[2])
        print(f"CRT_TLAS={tlas}: {int(wrong.sum())} of {N * N} albedo words decode to another texel than the reference's")
        assert not wrong.any(), [(int(y), int(x), [int(c[y, x]) for c in g], [int(c[y, x]) for c in w_]) for y, x in zip(*np.nonzero(wrong))][:8]
        assert (w_[0] >= 1).all() and np.array_equal(got["albedo"], want["albedo"])
        # the uS == width pixels: the plane and Session.pick hold the same word, the texel one past the row's end
        spill, _ = spill_pixels(ref, rec)
        assert len(spill) >= 1
        for k in spill[:: max(1, len(spill) // 8)]:
            y, x = divmod(int(k), N)
            px = s.pick(x, y)
            assert px["albedo"] == want["albedo"][y, x] and px["tri"] == rec["tri"][k] and px["instance"] == 0, (x, y)
        colour, _ = ref.orc.trace(rays, T.TARGET_VIEW[2], SUN)
        assert np.array_equal(bits(s.read_output()), bits(colour))


def test_pool_end_reads_the_last_texel(tmp_path, nthreads, monkeypatch):
    """No map on the last material: 38 texels follow the 90 x 37 sky, the 1 x 3 map last. The south pole's index (phi == H) and the
    uS == width sample in the map's last row both lie past the pool and are clamped to its last texel (tests/test_texel_lookup_cpu.py)."""
    for v in ("CRT_KERNEL", "CRT_TLAS"):
        monkeypatch.delenv(v, raising=False)
    s, ref = open_target(tmp_path, (90, 37), nthreads, maps=T.POOL_END_MAPS)
    with s:
        assert ref.n == 3370 and ref.layout[-1] == (2, 3367, 1, 3)
        d = ref.rays["south"].reshape(-1, 3)
        pole = int(np.flatnonzero(d[:, 1] == -1)[0])
        assert ref.index["south"][pole] == ref.n - 1
        render(s, 0, T.family_view("south"), 0)
        frame = s.read_output()
        ref.check_frame(frame, "south", "pool-end")
        tag, x, y = [c.reshape(-1) for c in T.decode_sky(frame)]
        assert (int(tag[pole]), int(x[pole]), int(y[pole])) == (2, 0, 2)
        rays, rec, want = target_reference(ref)
        render(s, GBUFFER, T.TARGET_VIEW)
        got = s.read_gbuffer_raw()
        assert np.array_equal(got["albedo"], want["albedo"])
        spill, vf = spill_pixels(ref, rec)
        last_row = spill[T.to_int(np.float32(3.0) * vf[spill]) == 2]
        assert len(last_row) >= 1
        g = [c.reshape(-1) for c in T.decode_albedo(got["albedo"])]
        assert (g[0][last_row] == 2).all() and (g[1][last_row] == 0).all() and (g[2][last_row] == 2).all()
        y0, x0 = divmod(int(last_row[0]), N)
        assert s.pick(x0, y0)["albedo"] == want["albedo"][y0, x0]
