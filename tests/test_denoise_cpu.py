"""libcrt_denoise.so without a GPU: the header, the ctypes table and the exports agree; every refusal of include/crt_denoise.h is answered before
anything is dereferenced or enqueued; the numpy restatement (tests/denoise_ref.py) has the properties the filter exists for; the pass kernels
cross-compile for gfx950 without scratch, spills or AGPRs; the library's sources own no HIP object."""
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

if not os.path.exists(_lib.DENOISE_SO):
    import __graft_entry__
    __graft_entry__.build()

import denoise_ref as ref
from test_abi import HIP_OWNING_CALLS
from util import bits, kernel_resource_rows, resource_line, unit_sources

DENOISE_DIR = os.path.join(ROOT, "clraytracer_amd", "denoise")
IMAGE_DIR = os.path.join(ROOT, "clraytracer_amd", "image")          # the headers the image libraries share, compiled into each
A = 0x10000                                      # dummy device addresses, 64 KiB apart: a refusal looks at none of them


def test_header_table_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "crt_denoise.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(crtd_\w+)\s*\(", text)))
    assert names == ["crtd_denoise", "crtd_error_string", "crtd_scratch_bytes"]
    assert sorted(_lib.DENOISE_API) == names
    lib = _lib.denoise()
    for n in names:
        assert hasattr(lib, n), n
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.DENOISE_SO], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(crtd_\w+)$", out, re.M))) == names
        assert not re.findall(r"\bcrt_\w+$", out, re.M)          # no crt_ name: those belong to libcrt_hip.so (tests/test_abi.py)
    # the constants of the header, as the table's users see them
    for name, value in (("CRTD_OK", 0), ("CRTD_E_BAD_ARGUMENT", -2), ("CRTD_E_OUT_OF_RANGE", -3), ("CRTD_GUIDES_PLANES", 0), ("CRTD_GUIDES_SURFACE", 1),
                        ("CRTD_DEMODULATE", 1), ("CRTD_MATCH_INSTANCE", 2), ("CRTD_LUMA_STOP", 4)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text) and getattr(_lib, name) == value, name
    assert (_lib.CRTD_E_BAD_ARGUMENT, _lib.CRTD_E_OUT_OF_RANGE) == (_lib.CRT_E_BAD_ARGUMENT, _lib.CRT_E_OUT_OF_RANGE)


def test_struct_sizes_and_scratch_bytes():
    # LP64: two int32, a pointer, an int32 and its padding, three pointers; five 4-byte fields (static_asserts in crt_denoise.hip hold the C side)
    assert C.sizeof(_lib.CrtdFrame) == 48 and C.sizeof(_lib.CrtdParams) == 20
    assert _lib.CrtdFrame.geometry.offset == 24 and _lib.CrtdFrame.albedo.offset == 40 and _lib.CrtdParams.lumaTol.offset == 16
    lib = _lib.denoise()
    assert lib.crtd_scratch_bytes(70, 37, 1) == 0
    for it in range(2, 7):
        assert lib.crtd_scratch_bytes(70, 37, it) == 70 * 37 * 16
    assert lib.crtd_scratch_bytes(16384, 16384, 2) == 16384 * 16384 * 16       # beyond 2^32
    assert b"argument" in lib.crtd_error_string(-2) and b"range" in lib.crtd_error_string(-3) and lib.crtd_error_string(0) == b"ok"


def call(frame=None, params=None, out=5 * A, scratch=6 * A, null_frame=False, null_params=False):
    f = dict(width=70, height=37, color=1 * A, guides=_lib.CRTD_GUIDES_PLANES, geometry=2 * A, ids=3 * A, albedo=4 * A)
    p = dict(iterations=3, flags=_lib.CRTD_DEMODULATE | _lib.CRTD_MATCH_INSTANCE | _lib.CRTD_LUMA_STOP, depthTol=0.05, normalCos=0.9, lumaTol=0.5)
    f.update(frame or {}); p.update(params or {})
    fs, ps = _lib.CrtdFrame(**f), _lib.CrtdParams(**p)
    return _lib.denoise().crtd_denoise(None if null_frame else C.byref(fs), None if null_params else C.byref(ps), out, scratch, None)


BAD, RANGE = _lib.CRTD_E_BAD_ARGUMENT, _lib.CRTD_E_OUT_OF_RANGE
SURFACE = dict(guides=_lib.CRTD_GUIDES_SURFACE, ids=None, albedo=None)
REFUSALS = {
    "null frame": (dict(null_frame=True), BAD),
    "null params": (dict(null_params=True), BAD),
    "null colour": (dict(frame=dict(color=None)), BAD),
    "null geometry": (dict(frame=dict(geometry=None)), BAD),
    "null out": (dict(out=None), BAD),
    "no ids under MATCH_INSTANCE": (dict(frame=dict(ids=None)), BAD),
    "no albedo under DEMODULATE": (dict(frame=dict(albedo=None)), BAD),
    "ids under SURFACE": (dict(frame=dict(SURFACE, ids=3 * A)), BAD),
    "albedo under SURFACE": (dict(frame=dict(SURFACE, albedo=4 * A)), BAD),
    "no scratch for two passes": (dict(scratch=None, params=dict(iterations=2)), BAD),
    "out is colour": (dict(out=1 * A), BAD),
    "out is geometry": (dict(out=2 * A), BAD),
    "out is ids": (dict(out=3 * A), BAD),
    "out is albedo": (dict(out=4 * A), BAD),
    "scratch is colour": (dict(scratch=1 * A), BAD),
    "scratch is geometry": (dict(scratch=2 * A), BAD),
    "scratch is ids": (dict(scratch=3 * A), BAD),
    "scratch is albedo": (dict(scratch=4 * A), BAD),
    "scratch is out": (dict(scratch=5 * A), BAD),
    "scratch is colour, one pass": (dict(scratch=1 * A, params=dict(iterations=1)), BAD),
    "out is the records under SURFACE": (dict(frame=SURFACE, out=2 * A), BAD),
    "0 iterations": (dict(params=dict(iterations=0)), BAD),
    "7 iterations": (dict(params=dict(iterations=7)), BAD),
    "-1 iterations": (dict(params=dict(iterations=-1)), BAD),
    "unknown flag": (dict(params=dict(flags=8)), BAD),
    "unknown high flag": (dict(params=dict(flags=0x80000001)), BAD),
    "unknown guides": (dict(frame=dict(guides=2)), BAD),
    "negative guides": (dict(frame=dict(guides=-1)), BAD),
    "negative depthTol": (dict(params=dict(depthTol=-0.01)), BAD),
    "NaN depthTol": (dict(params=dict(depthTol=float("nan"))), BAD),
    "NaN normalCos": (dict(params=dict(normalCos=float("nan"))), BAD),
    "infinite normalCos": (dict(params=dict(normalCos=float("inf"))), BAD),
    "-infinite normalCos": (dict(params=dict(normalCos=float("-inf"))), BAD),
    "negative lumaTol under LUMA_STOP": (dict(params=dict(lumaTol=-1.0)), BAD),
    "NaN lumaTol under LUMA_STOP": (dict(params=dict(lumaTol=float("nan"))), BAD),
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


# ---- the reference itself, on hand-made planes --------------------------------------------------------------------------------------------
H, W = 37, 70
ALL = ref.DEMODULATE | ref.MATCH_INSTANCE | ref.LUMA_STOP


def run(color, planes, **kw):
    return ref.denoise(color, planes["geometry"], planes["ids"]["instance"], planes["albedo"], **kw)


def test_reference_keeps_the_two_sides_of_a_depth_edge_apart():
    planes = ref.guides(H, W)
    color = ref.noisy_color(H, W, nans=False)
    other = color.copy()
    other[:, W // 2:, :3] = ref.noisy_color(H, W, seed=9, nans=False)[:, W // 2:, :3] + 3.0          # the far side's colours change
    for flags in (0, ref.DEMODULATE):
        a, b = run(color, planes, iterations=5, flags=flags), run(other, planes, iterations=5, flags=flags)
        assert np.array_equal(bits(a[:, :W // 2]), bits(b[:, :W // 2]))                             # the near side: the same bits
        hit = planes["geometry"][:, W // 2:, 3] <= 99998.0
        assert (bits(a[:, W // 2:])[hit] != bits(b[:, W // 2:])[hit]).any()
    # and it filters: over a smooth region, noise around a constant shrinks to less than half
    flat = color.copy()
    flat[..., :3] = 0.5 + np.random.RandomState(5).normal(0, 0.2, (H, W, 3))
    region = (slice(2, H // 2 - 2), slice(2, W // 2 - 2))
    ok = planes["geometry"][region][..., 3] <= 99998.0
    assert run(flat, planes, iterations=3, flags=0)[region][ok][:, 0].std() < 0.5 * flat[region][ok][:, 0].std()


@pytest.mark.parametrize("flags", [0, ref.DEMODULATE, ALL])
def test_reference_leaves_pixels_that_are_no_hit_alone(flags):
    planes = ref.guides(H, W)
    color = ref.noisy_color(H, W)
    out = run(color, planes, iterations=6, flags=flags, luma_tol=0.3)
    miss = ~(planes["geometry"][..., 3] <= 99998.0)
    assert miss.sum() >= 3 and np.isnan(planes["geometry"][..., 3]).any()
    assert np.array_equal(bits(out)[miss], bits(color)[miss])
    assert np.array_equal(bits(out[..., 3]), bits(color[..., 3]))                                    # alpha: the centre's, everywhere


def test_every_flag_and_parameter_changes_some_output():
    planes = ref.guides(H, W)
    color = ref.noisy_color(H, W, nans=False)
    base = run(color, planes, iterations=3, flags=0)
    seen = [bits(base)]
    for kw in (dict(flags=ref.DEMODULATE), dict(flags=ref.MATCH_INSTANCE), dict(flags=ref.LUMA_STOP, luma_tol=0.2), dict(flags=0, depth_tol=0.5),
               dict(flags=0, normal_cos=-1.0), dict(flags=0, iterations=4), dict(flags=ALL, luma_tol=0.2)):
        out = bits(run(color, planes, **dict(dict(iterations=3), **kw)))
        assert not any(np.array_equal(out, s) for s in seen), kw
        seen.append(out)


def test_reference_poisons_exactly_the_taps_of_a_nan_colour():
    planes = ref.guides(H, W)
    planes["geometry"][...] = (0.0, 1.0, 0.0, 10.0)                                                 # every pixel a hit on one plane
    color = ref.noisy_color(H, W, nans=False)
    color[20, 30, 1] = np.nan
    out = run(color, planes, iterations=1, flags=0)
    want = np.zeros((H, W), bool); want[18:23, 28:33] = True
    assert np.array_equal(np.isnan(out[..., 1]), want) and not np.isnan(out[..., 0]).any()


# ---- the unit as the compiler sees it -------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_pass_kernels_need_no_scratch_no_spill_and_no_agprs():
    rows = kernel_resource_rows(source=os.path.join(DENOISE_DIR, "crt_denoise.hip"))
    for n, r in rows:
        print(resource_line(n, r))
    # per guide layout: the taps through L1 / L2 at any step (0), the taps from LDS at steps 1, 2 and 4; two planes of float4 over tile + halo
    lds = {0: 0, **{s: (32 + 4 * s) * (8 + 4 * s) * 32 for s in (1, 2, 4)}}
    assert sorted(n for n, _ in rows) == sorted(f"crtd_pass_kernel<{g}, {s}>" for g in ("false", "true") for s in lds)
    for n, r in rows:
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r.get("SGPRs Spill", 0) == 0 and r["AGPRs"] == 0, resource_line(n, r)
        stage = int(n[n.index(", ") + 2:-1])
        assert r["LDS Size"] == lds[stage], resource_line(n, r)                      # nothing but the staged tile: no array of the kernel went to LDS
        assert r["Occupancy"] >= 4 and 4 * r["LDS Size"] <= 160 * 1024, resource_line(n, r)     # four workgroups per CU at least, by registers and by LDS


def test_the_library_owns_no_hip_object_and_follows_the_recipe():
    sources = sorted(f for f in os.listdir(DENOISE_DIR) if f.endswith((".h", ".hip", ".cpp", ".hpp")))
    assert sources == ["crt_denoise.hip"]
    # the unit and every in-tree header it includes, transitively: the shared steps of clraytracer_amd/image/ are this library's source too
    scanned = unit_sources("clraytracer_amd/denoise/crt_denoise.hip")
    assert {os.path.join(DENOISE_DIR, f) for f in sources} | {os.path.join(ROOT, "include", "crt_denoise.h"), os.path.join(IMAGE_DIR, "crt_image_device.h"),
                                                            os.path.join(IMAGE_DIR, "crt_image_host.h"), os.path.join(IMAGE_DIR, "crt_image_env.h")} <= set(scanned)
    for path in scanned:
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        assert not re.findall(HIP_OWNING_CALLS, text), path
        assert not re.findall(r"\bhip(DeviceSynchronize|StreamSynchronize|EventSynchronize|Memcpy\w*|Memset\w*)\s*\(", text), path     # nor waits or copies
    if shutil.which("make"):
        p = subprocess.run(["make", "-n", "-W", "clraytracer_amd/denoise/crt_denoise.hip", _lib.DENOISE_SO.replace(ROOT + os.sep, "")], cwd=ROOT,
                           stdout=subprocess.PIPE, text=True, check=True)
        makefile = open(os.path.join(ROOT, "Makefile")).read()
        flags = re.search(r"^HIPFLAGS = (.*)$", makefile, re.M).group(1).replace("$(ARCH)", "gfx950").split()
        lines = [l.split() for l in p.stdout.splitlines() if "-shared" in l.split()]
        assert len(lines) == 1 and lines[0][1:] == flags + ["-shared", "-o", "clraytracer_amd/denoise/libcrt_denoise.so", "clraytracer_amd/denoise/crt_denoise.hip"]
