"""libcrt_vfilter.so without a GPU: the header, the ctypes table and the exports agree; the struct layouts match; every refusal of
include/crt_vfilter.h is answered before anything is dereferenced or enqueued; the numpy restatement (tests/vfilter_ref.py) agrees bit for bit with
tests/denoise_ref.py where the two definitions coincide and has the properties the filter exists for; the kernels cross-compile for gfx950 without
scratch, spills or AGPRs; the library's source owns no HIP object, waits on nothing and copies nothing."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clraytracer_amd import _lib

if not os.path.exists(getattr(_lib, "VFILTER_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import denoise_ref
import vfilter_ref as ref
from test_abi import HIP_OWNING_CALLS
from util import bits, kernel_resource_rows, resource_line, unit_sources

VFILTER_DIR = os.path.join(ROOT, "clraytracer_amd", "vfilter")
IMAGE_DIR = os.path.join(ROOT, "clraytracer_amd", "image")          # the headers the image libraries share, compiled into each
A = 0x10000                                      # dummy device addresses, 64 KiB apart: a refusal looks at none of them
NAMES = ["crtv_error_string", "crtv_filter", "crtv_scratch_bytes"]


def test_header_table_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "crt_vfilter.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(crtv_\w+)\s*\(", text)))
    assert names == NAMES
    assert sorted(_lib.VFILTER_API) == names
    lib = _lib.vfilter()
    for n in names:
        assert hasattr(lib, n), n
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.VFILTER_SO], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(crtv_\w+)$", out, re.M))) == names
        assert not re.findall(r"\bcrt[dt]?_\w+$", out, re.M)        # no crt_, crtd_ or crtt_ name: those belong to the other libraries
    for name, value in (("CRTV_OK", 0), ("CRTV_E_BAD_ARGUMENT", -2), ("CRTV_E_OUT_OF_RANGE", -3), ("CRTV_GUIDES_PLANES", 0), ("CRTV_GUIDES_SURFACE", 1),
                        ("CRTV_DEMODULATE", 1), ("CRTV_MATCH_INSTANCE", 2)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text) and getattr(_lib, name) == value, name
    assert (_lib.CRTV_E_BAD_ARGUMENT, _lib.CRTV_E_OUT_OF_RANGE) == (_lib.CRT_E_BAD_ARGUMENT, _lib.CRT_E_OUT_OF_RANGE)
    assert (_lib.CRTV_GUIDES_PLANES, _lib.CRTV_GUIDES_SURFACE) == (_lib.CRTD_GUIDES_PLANES, _lib.CRTD_GUIDES_SURFACE)
    assert (ref.DEMODULATE, ref.MATCH_INSTANCE) == (_lib.CRTV_DEMODULATE, _lib.CRTV_MATCH_INSTANCE)


def test_struct_sizes_offsets_and_scratch_bytes():
    """The figures the header states and crt_vfilter.hip static_asserts. LP64: the int32 `guides` sits at 24, behind the two image pointers, with 4
    bytes of padding behind it."""
    header = open(os.path.join(ROOT, "include", "crt_vfilter.h")).read()
    source = open(os.path.join(VFILTER_DIR, "crt_vfilter.hip")).read()
    for struct, size in ((_lib.CrtvFrame, 56), (_lib.CrtvParams, 28)):
        assert C.sizeof(struct) == size, struct
        assert re.search(r"/\* %d bytes[^\n]*\*/\ntypedef struct \{(?:(?!typedef).)*?\} %s;" % (size, struct.__name__), header, re.S), struct
        assert "sizeof(%s) == %d" % (struct.__name__, size) in source, struct
    offsets = {_lib.CrtvFrame: dict(width=0, height=4, color=8, moments=16, guides=24, geometry=32, ids=40, albedo=48),
               _lib.CrtvParams: dict(iterations=0, flags=4, depthTol=8, normalCos=12, lumaSigma=16, lumaFloor=20, minHistory=24)}
    for struct, fields in offsets.items():
        assert [n for n, _ in struct._fields_] == list(fields), struct
        for name, off in fields.items():
            assert getattr(struct, name).offset == off, (struct, name)
            if off and name != "height":
                assert "offsetof(%s, %s) == %d" % (struct.__name__, name, off) in source, (struct, name)
    lib = _lib.vfilter()
    for it in range(1, 6):
        assert lib.crtv_scratch_bytes(70, 37, it) == 70 * 37 * 16
        assert lib.crtv_scratch_bytes(1, 1, it) == 16
    assert lib.crtv_scratch_bytes(16384, 16384, 1) == 2 ** 32 and lib.crtv_scratch_bytes(16384, 16383, 5) == 16384 * 16383 * 16      # 2^32 and around
    for w, h, it in ((0, 37, 2), (70, -1, 2), (70, 37, 0), (70, 37, 6), (70, 37, -3)):
        assert lib.crtv_scratch_bytes(w, h, it) == 0
    assert b"argument" in lib.crtv_error_string(-2) and b"range" in lib.crtv_error_string(-3) and lib.crtv_error_string(0) == b"ok"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
OUT, VARIANCE, SCRATCH = 6 * A, 7 * A, 8 * A


def call(frame=None, params=None, out=OUT, variance=VARIANCE, scratch=SCRATCH, null_frame=False, null_params=False):
    f = dict(width=70, height=37, color=1 * A, moments=2 * A, guides=_lib.CRTV_GUIDES_PLANES, geometry=3 * A, ids=4 * A, albedo=5 * A)
    p = dict(iterations=4, flags=_lib.CRTV_DEMODULATE | _lib.CRTV_MATCH_INSTANCE, depthTol=0.05, normalCos=0.9, lumaSigma=4.0, lumaFloor=1e-4, minHistory=4.0)
    f.update(frame or {}); p.update(params or {})
    fs, ps = _lib.CrtvFrame(**f), _lib.CrtvParams(**p)
    return _lib.vfilter().crtv_filter(None if null_frame else C.byref(fs), None if null_params else C.byref(ps), out, variance, scratch, None)


BAD, RANGE = _lib.CRTV_E_BAD_ARGUMENT, _lib.CRTV_E_OUT_OF_RANGE
SURFACE = dict(guides=_lib.CRTV_GUIDES_SURFACE, ids=None, albedo=None)
INPUTS = (("the colour", 1 * A), ("the moments", 2 * A), ("the geometry", 3 * A), ("the ids", 4 * A), ("the albedo", 5 * A))
NAN, INF = float("nan"), float("inf")
REFUSALS = {
    "null frame": (dict(null_frame=True), BAD),
    "null params": (dict(null_params=True), BAD),
    "null colour": (dict(frame=dict(color=None)), BAD),
    "null moments": (dict(frame=dict(moments=None)), BAD),
    "null geometry": (dict(frame=dict(geometry=None)), BAD),
    "null out": (dict(out=None), BAD),
    "null scratch": (dict(scratch=None), BAD),
    "null scratch for one pass": (dict(scratch=None, params=dict(iterations=1)), BAD),
    "no ids under MATCH_INSTANCE": (dict(frame=dict(ids=None)), BAD),
    "no albedo under DEMODULATE": (dict(frame=dict(albedo=None)), BAD),
    "ids under SURFACE": (dict(frame=dict(SURFACE, ids=4 * A)), BAD),
    "albedo under SURFACE": (dict(frame=dict(SURFACE, albedo=5 * A)), BAD),
    **{f"out is {b}": (dict(out=addr), BAD) for b, addr in INPUTS},
    **{f"scratch is {b}": (dict(scratch=addr), BAD) for b, addr in INPUTS},
    **{f"outVariance is {b}": (dict(variance=addr), BAD) for b, addr in INPUTS},
    "out is scratch": (dict(out=SCRATCH), BAD),
    "outVariance is out": (dict(variance=OUT), BAD),
    "outVariance is scratch": (dict(variance=SCRATCH), BAD),
    "out is the records under SURFACE": (dict(frame=SURFACE, out=3 * A), BAD),
    "iterations 0": (dict(params=dict(iterations=0)), BAD),
    "iterations 6": (dict(params=dict(iterations=6)), BAD),
    "negative iterations": (dict(params=dict(iterations=-1)), BAD),
    "unknown flag": (dict(params=dict(flags=4)), BAD),
    "unknown high flag": (dict(params=dict(flags=0x80000001)), BAD),
    "unknown guides": (dict(frame=dict(guides=2)), BAD),
    "negative guides": (dict(frame=dict(guides=-1)), BAD),
    "negative depthTol": (dict(params=dict(depthTol=-0.01)), BAD),
    "NaN depthTol": (dict(params=dict(depthTol=NAN)), BAD),
    "NaN normalCos": (dict(params=dict(normalCos=NAN)), BAD),
    "infinite normalCos": (dict(params=dict(normalCos=INF)), BAD),
    "-infinite normalCos": (dict(params=dict(normalCos=-INF)), BAD),
    "negative lumaSigma": (dict(params=dict(lumaSigma=-1.0)), BAD),
    "NaN lumaSigma": (dict(params=dict(lumaSigma=NAN)), BAD),
    "infinite lumaSigma": (dict(params=dict(lumaSigma=INF)), BAD),
    "negative lumaFloor": (dict(params=dict(lumaFloor=-1e-6)), BAD),
    "NaN lumaFloor": (dict(params=dict(lumaFloor=NAN)), BAD),
    "infinite lumaFloor": (dict(params=dict(lumaFloor=INF)), BAD),
    "NaN minHistory": (dict(params=dict(minHistory=NAN)), BAD),
    "width 0": (dict(frame=dict(width=0)), BAD),
    "height 0": (dict(frame=dict(height=0)), BAD),
    "negative width": (dict(frame=dict(width=-5)), BAD),
    "width 16385": (dict(frame=dict(width=16385)), RANGE),
    "height 16385": (dict(frame=dict(height=16385)), RANGE),
    "width 2^31 - 1": (dict(frame=dict(width=2 ** 31 - 1)), RANGE),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_come_before_anything_is_enqueued(case):
    """Every pointer is a dummy address: a refusal that dereferenced one would fault, and one that enqueued would need a device."""
    kwargs, want = REFUSALS[case]
    assert call(**kwargs) == want, case


# ---- the reference itself, on hand-made planes ----------------------------------------------------------------------------------------------
H, W = 37, 70


def planes(seed=0):
    p = ref.guides(H, W, seed=seed)
    return p["geometry"], p["ids"]["instance"].astype(np.int32), p["albedo"]


def flat(h, w):
    """one surface: every pixel a hit with the same normal and distance, one instance, an albedo of 0x80 per channel"""
    g = np.zeros((h, w, 4), np.float32)
    g[...] = (0.0, 1.0, 0.0, 10.0)
    return g, np.zeros((h, w), np.int32), np.full((h, w), 0xFF808080, np.uint32)


def moments_of(color, variance, history=32.0):
    L = ref.luma(color[..., :3])
    return np.stack([L, L * L + np.float32(variance), np.full_like(L, history), np.full_like(L, variance)], axis=-1).astype(np.float32)


@pytest.mark.parametrize("flags", range(4))
def test_with_every_luminance_weight_one_the_colour_is_denoise_ref_s(flags):
    """lumaSigma = 0 and lumaFloor = 1e30 make sd = 1e30, so xl = |dL| / 1e30 is below 2^-25 for every finite luminance, 1 - xl rounds to 1 and a
    counted tap's w is k * (1 * 1) = k: the taps that count are those of crt_denoise.h without CRTD_LUMA_STOP (the variances here are all >= 0)
    with its weights. A tap that does not count adds Iq * 0 there and nothing here: +-0 to a sum that is +0 or not zero, the same bits for a
    finite Iq. So rgb and alpha equal tests/denoise_ref.py's, an independent restatement of an independent definition, bit for bit."""
    g, inst, albedo = planes()
    color = ref.noisy_color(H, W, nans=False)
    moments = ref.moments_content(color, g, edge_cases=False)
    for iterations in range(1, 6):
        got, _ = ref.filter(color, moments, g, inst, albedo, iterations=iterations, flags=flags, luma_sigma=0.0, luma_floor=1e30)
        want = denoise_ref.denoise(color, g, inst, albedo, iterations=iterations, flags=flags)
        assert np.array_equal(bits(got), bits(want)), iterations


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_an_edge_is_kept_or_crossed_with_the_variance(iterations):
    """A flat plane whose colour is 0.25 left of x = EW // 2 and 0.75 right of it (a luminance step of 0.5), the same geometry on both sides. Every
    k is 3^a 2^-b with a <= 2, so c * k, the partial sums (multiples of 2^-10 below 1) and their quotient by the sum of the k are exact: a pixel
    whose counted taps all have its own colour keeps it bit for bit."""
    EH, EW = 24, 80
    g, inst, albedo = flat(EH, EW)
    xx = np.mgrid[0:EH, 0:EW][1]
    color = np.empty((EH, EW, 4), np.float32)
    color[..., :3] = np.where(xx < EW // 2, 0.25, 0.75)[..., None]
    color[..., 3] = np.random.RandomState(5).uniform(0, 1, (EH, EW))
    # converged: variance 0, so sd = lumaFloor = 0.1 is below the step and no tap crosses the edge
    kept, var = ref.filter(color, moments_of(color, 0.0), g, inst, albedo, iterations=iterations, flags=0, luma_floor=0.1)
    assert np.array_equal(bits(kept), bits(color)) and (var == 0).all()
    # noisy: variance 1, so sd = 4 * 1 + 0.1 exceeds the step and the taps cross it
    crossed, var = ref.filter(color, moments_of(color, 1.0), g, inst, albedo, iterations=iterations, flags=0, luma_floor=0.1)
    reach = 2 * (2 ** iterations - 1)                                   # 2 * step pixels per pass
    distance = np.where(xx < EW // 2, EW // 2 - xx, xx - (EW // 2 - 1))  # to the nearest pixel of the other colour
    changed = (bits(crossed) != bits(color)).any(axis=-1)
    assert changed[distance <= 2].all()                                 # next to the edge every pixel moves
    assert changed[distance <= reach].mean() > 0.5
    assert not changed[distance > reach].any() and (distance > reach).any()
    assert (var > 0).all() and (var < 1).all()


def test_both_estimates_are_seen():
    g, inst, albedo = flat(H, W)
    color = ref.noisy_color(H, W, nans=False)
    moments = ref.moments_content(color, g, edge_cases=False)
    I0 = lambda m, **kw: ref.filter(color, m, g, inst, albedo, flags=0, working=True, **kw)[0]
    # above every N: the spatial estimate. moments.w is not read; a neighbour's m2 reaches the centre (and the 48 other pixels whose window it is in)
    base = I0(moments, min_history=100.0)
    other = moments.copy(); other[..., 3] += 1.0
    assert np.array_equal(bits(I0(other, min_history=100.0)), bits(base))
    other = moments.copy(); other[20, 30, 1] += 0.5
    differs = bits(I0(other, min_history=100.0))[..., 3] != bits(base)[..., 3]
    yy, xx = np.mgrid[0:H, 0:W]
    window = (np.abs(yy - 20) <= 3) & (np.abs(xx - 30) <= 3)
    assert differs[20, 29] and differs[17, 33] and differs[window].all() and not differs[~window].any()
    # at or below every N: the temporal one, which is moments.w
    temporal = I0(moments, min_history=0.0)
    assert np.array_equal(bits(temporal[..., 3]), bits(moments[..., 3]))
    other = moments.copy(); other[20, 30, 1] += 0.5
    assert np.array_equal(bits(I0(other, min_history=0.0)), bits(temporal))
    # mixed: each pixel by its own N
    mixed = I0(moments, min_history=4.0)[..., 3]
    N = moments[..., 2]
    assert (N >= 4).any() and (N < 4).any()
    assert np.array_equal(bits(mixed[N >= 4]), bits(temporal[..., 3][N >= 4])) and np.array_equal(bits(mixed[N < 4]), bits(base[..., 3][N < 4]))
    # the spatial estimate scales with 4 / max(N, 1): N = 0 and N = 1 give the same, N = 2 half of it
    for a, b, scale in ((0.0, 1.0, 1.0), (1.0, 2.0, 0.5)):
        ma, mb = moments.copy(), moments.copy()
        ma[..., 2], mb[..., 2] = a, b
        assert np.array_equal(bits(I0(ma, min_history=100.0)[..., 3] * np.float32(scale)), bits(I0(mb, min_history=100.0)[..., 3]))


def test_noise_falls():
    """iid noise of luminance variance v0 over a flat plane, the moments saying so: after any number of passes the variance plane is below v0 at
    every interior pixel (a pass writes sum w^2 var_q / (sum w)^2 <= max var_q * sum w^2 / (sum w)^2, which is below max var_q <= v0 once two
    taps count), and the sample variance of the output falls with each added pass."""
    g, inst, albedo = flat(H, W)
    rng = np.random.RandomState(11)
    color = np.empty((H, W, 4), np.float32)
    color[..., :3] = 0.5 + rng.normal(0, 0.1, (H, W, 1))                     # grey noise: the luminance is the channels' value
    color[..., 3] = 1.0
    v0 = np.float32(0.01)
    moments = moments_of(color, v0)
    images = ref.filter(color, moments, g, inst, albedo, iterations=5, flags=0, working=True)
    interior = np.zeros((H, W), bool); interior[2:-2, 2:-2] = True
    assert (images[0][..., 3] == v0).all()
    for after in images[1:]:
        assert (after[..., 3][interior] < v0).all() and (after[..., 3] > 0).all()
    sample = [float(np.var(ref.filter(color, moments, g, inst, albedo, iterations=k, flags=0)[0][..., 0].astype(np.float64))) for k in range(1, 6)]
    print("sample variance of the input %.3e, after 1..5 passes:" % np.var(color[..., 0].astype(np.float64)), ["%.3e" % s for s in sample])
    assert sample[0] < float(np.var(color[..., 0].astype(np.float64))) and all(b < a for a, b in zip(sample, sample[1:]))
    out, variance = ref.filter(color, moments, g, inst, albedo, iterations=5, flags=0)
    assert np.array_equal(bits(variance), bits(images[5][..., 3])) and np.array_equal(bits(out[..., 3]), bits(color[..., 3]))


@pytest.mark.parametrize("what", ["colour", "variance", "m1", "m2", "N"])
@pytest.mark.parametrize("min_history", [0.0, 100.0])
def test_a_nan_heals(what, min_history):
    """A NaN in one pixel's colour, variance or moments: every other pixel's result is finite. Multiplied by zero instead of selected away it
    would have reached every pixel it is a tap of."""
    g, inst, albedo = flat(H, W)
    color = ref.noisy_color(H, W, nans=False)
    moments = ref.moments_content(color, g, edge_cases=False)
    clean, clean_var = ref.filter(color, moments, g, inst, albedo, iterations=3, min_history=min_history)
    assert np.isfinite(clean).all() and np.isfinite(clean_var).all()
    if what == "colour":
        color[20, 30, 1] = np.nan
    else:
        moments[20, 30, {"m1": 0, "m2": 1, "N": 2, "variance": 3}[what]] = np.nan
    out, variance = ref.filter(color, moments, g, inst, albedo, iterations=3, min_history=min_history)
    others = np.ones((H, W), bool); others[20, 30] = False
    assert np.isfinite(out[others]).all() and np.isfinite(variance[others]).all()
    if what == "colour":                                                    # the pixel itself keeps it: the centre always counts
        assert np.isnan(out[20, 30, 1]) and (bits(out) != bits(clean)).any(axis=-1).sum() > 1


def test_pixels_that_are_no_hit_come_out_exactly():
    g, inst, albedo = planes()
    color = ref.noisy_color(H, W)
    moments = ref.moments_content(color, g)
    hit = g[..., 3] <= 99998.0
    assert (~hit).sum() >= 50 and np.isnan(g[..., 3]).any()
    for flags in range(4):
        out, variance = ref.filter(color, moments, g, inst, albedo, iterations=4, flags=flags)
        assert np.array_equal(bits(out)[~hit], bits(color)[~hit]) and (bits(variance)[~hit] == 0).all()
        assert np.array_equal(bits(out[..., 3]), bits(color[..., 3]))                     # alpha is the colour's everywhere
        assert (bits(out)[hit][:, :3] != bits(color)[hit][:, :3]).any(axis=-1).mean() > 0.9


def test_every_flag_and_parameter_changes_some_pixel():
    g, inst, albedo = planes()
    color = ref.noisy_color(H, W, nans=False)
    moments = ref.moments_content(color, g, edge_cases=False)
    key = lambda r: np.concatenate([bits(r[0]).reshape(-1), bits(r[1]).reshape(-1)])
    seen = [key(ref.filter(color, moments, g, inst, albedo))]
    for kw in (dict(flags=0), dict(flags=ref.MATCH_INSTANCE), dict(flags=ref.DEMODULATE | ref.MATCH_INSTANCE), dict(iterations=3), dict(depth_tol=0.01),
               dict(normal_cos=0.999), dict(luma_sigma=1.0), dict(luma_floor=0.05), dict(min_history=8.0), dict(min_history=1.0)):
        out = key(ref.filter(color, moments, g, inst, albedo, **kw))
        assert not any(np.array_equal(out, s) for s in seen), kw
        seen.append(out)


def test_the_reference_makes_no_nan_of_its_own_on_the_gpu_tests_inputs():
    """The GPU tests compare NaNs bit for bit, which holds while every NaN stored is a planted one carried along (payload 0x7FC00000): a NaN an
    operation makes (inf - inf, 0 * inf) has its sign set on the host and clear on the device. The inputs of tests/test_gpu_vfilter.py make none."""
    import test_gpu_vfilter as gpu
    for w, h in gpu.SHAPES:
        for flags in range(4):
            for min_history in (0.0, 4.0, gpu.ABOVE_EVERY_N):
                out, variance = gpu.reference(w, h, 5, flags, min_history)
                for a in (out, variance):
                    assert not (np.isnan(a) & (bits(a) != 0x7FC00000)).any(), (w, h, flags, min_history)


# ---- the unit as the compiler sees it -------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_kernels_need_no_scratch_no_spill_and_no_agprs():
    rows = kernel_resource_rows(source=os.path.join(VFILTER_DIR, "crt_vfilter.hip"))
    for n, r in rows:
        print(resource_line(n, r))
    # per guide layout: the estimate's taps through L1 or from a 38 x 14 tile in LDS; a pass's through L1 or from a tile with a halo of 2, 4 or 8
    tf = ("false", "true")
    want = {f"crtv_estimate_kernel<{s}, {l}>": (38 * 14 * 28 if l == "true" else 0) for s in tf for l in tf}
    want.update({f"crtv_pass_kernel<{s}, {st}>": ((32 + 4 * st) * (8 + 4 * st) * 36 if st else 0) for s in tf for st in (0, 1, 2, 4)})
    assert sorted(n for n, _ in rows) == sorted(want)
    for n, r in rows:
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r.get("SGPRs Spill", 0) == 0 and r["AGPRs"] == 0, resource_line(n, r)
        assert r["LDS Size"] == want[n], resource_line(n, r)                     # nothing but the staged tile
        # by registers every kernel fits six waves per SIMD; the step-4 tile (40.5 KiB) admits three workgroups of four waves per CU
        assert r["Occupancy"] >= (3 if n.endswith(", 4>") else 6), resource_line(n, r)


def test_the_library_owns_no_hip_object_and_follows_the_recipe():
    sources = sorted(f for f in os.listdir(VFILTER_DIR) if f.endswith((".h", ".hip", ".cpp", ".hpp")))
    assert sources == ["crt_vfilter.hip"]
    # the unit and every in-tree header it includes, transitively: the shared steps of clraytracer_amd/image/ are this library's source too
    scanned = unit_sources("clraytracer_amd/vfilter/crt_vfilter.hip")
    assert {os.path.join(VFILTER_DIR, f) for f in sources} | {os.path.join(ROOT, "include", "crt_vfilter.h"), os.path.join(IMAGE_DIR, "crt_image_device.h"),
                                                            os.path.join(IMAGE_DIR, "crt_image_host.h"), os.path.join(IMAGE_DIR, "crt_image_env.h")} <= set(scanned)
    for path in scanned:
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        assert not re.findall(HIP_OWNING_CALLS, text), path
        assert not re.findall(r"\bhip(DeviceSynchronize|StreamSynchronize|EventSynchronize|Memcpy\w*|Memset\w*)\s*\(", text), path     # nor waits or copies
    if shutil.which("make"):
        p = subprocess.run(["make", "-n", "-W", "clraytracer_amd/vfilter/crt_vfilter.hip", _lib.VFILTER_SO.replace(ROOT + os.sep, "")], cwd=ROOT,
                           stdout=subprocess.PIPE, text=True, check=True)
        makefile = open(os.path.join(ROOT, "Makefile")).read()
        flags = re.search(r"^HIPFLAGS = (.*)$", makefile, re.M).group(1).replace("$(ARCH)", "gfx950").split()
        lines = [l.split() for l in p.stdout.splitlines() if "-shared" in l.split()]
        assert len(lines) == 1 and lines[0][1:] == flags + ["-shared", "-o", "clraytracer_amd/vfilter/libcrt_vfilter.so", "clraytracer_amd/vfilter/crt_vfilter.hip"]
        assert re.search(r"^all:.*\$\(VFILTER_SO\)", makefile, re.M) and re.search(r"rm -f .*\$\(VFILTER_SO\)", makefile)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.vfilter()" in entry
