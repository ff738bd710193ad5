"""libcrt_present.so without a GPU: the header, the ctypes table and the exports agree; the struct layouts match the header's comments and the
unit's static_asserts; every refusal of include/crt_present.h is answered with dummy addresses before anything is dereferenced or enqueued;
crtp_scratch_bytes is 0 for refused sizes and monotone otherwise; the numpy restatement (tests/present_ref.py) with no AO, exposure 1 and no
heal is the oracle's own chain for all eight flag sets, and its FXAA inputs are no fixed points of the filter; the per-pixel stages are written
once (csrc/crt_post.h) and compiled into both libraries; every kernel cross-compiles for gfx950 without scratch, spills or AGPRs; the unit owns
no HIP object, waits on nothing and copies nothing."""
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

if not os.path.exists(getattr(_lib, "PRESENT_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import present_ref as ref
from test_abi import HIP_OWNING_CALLS
from util import bits, kernel_resource_rows, resource_line, unit_sources

PRESENT_DIR = os.path.join(ROOT, "clraytracer_amd", "present")
IMAGE_DIR = os.path.join(ROOT, "clraytracer_amd", "image")
CSRC_DIR = os.path.join(ROOT, "clraytracer_amd", "csrc")
A = 0x10000                                      # dummy device addresses, 64 KiB apart: a refusal looks at none of them
NAMES = ["crtp_error_string", "crtp_present", "crtp_scratch_bytes", "crtp_view"]
BAD, RANGE = _lib.CRTP_E_BAD_ARGUMENT, _lib.CRTP_E_OUT_OF_RANGE
INF, NAN = float("inf"), float("nan")


def test_header_table_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "crt_present.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(crtp_\w+)\s*\(", text)))
    assert names == NAMES
    assert sorted(_lib.PRESENT_API) == names
    lib = _lib.present()
    for n in names:
        assert hasattr(lib, n), n
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.PRESENT_SO], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(crtp_\w+)$", out, re.M))) == names
        assert not re.findall(r"\bcrt[dtvmus]?_\w+$", out, re.M)     # no name of another library's
    for name, value in (("CRTP_OK", 0), ("CRTP_E_BAD_ARGUMENT", -2), ("CRTP_E_OUT_OF_RANGE", -3), ("CRTP_GUIDES_PLANES", 0), ("CRTP_GUIDES_SURFACE", 1),
                        ("CRTP_UNORM8", 1), ("CRTP_POST", 2), ("CRTP_FXAA", 4), ("CRTP_HEAL", 8), ("CRTP_VIEW_NORMAL", 0), ("CRTP_VIEW_DEPTH", 1),
                        ("CRTP_VIEW_INSTANCE", 2), ("CRTP_VIEW_TRIANGLE", 3), ("CRTP_VIEW_ALBEDO", 4), ("CRTP_VIEW_SCALAR", 5), ("CRTP_VIEW_STATE", 6),
                        ("CRTP_FXAA_HALO", 5)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text) and getattr(_lib, name) == value, name
    assert (_lib.CRTP_E_BAD_ARGUMENT, _lib.CRTP_E_OUT_OF_RANGE) == (_lib.CRT_E_BAD_ARGUMENT, _lib.CRT_E_OUT_OF_RANGE)
    assert (_lib.CRTP_GUIDES_PLANES, _lib.CRTP_GUIDES_SURFACE) == (_lib.CRTD_GUIDES_PLANES, _lib.CRTD_GUIDES_SURFACE)
    assert (ref.UNORM8, ref.POST, ref.FXAA, ref.HEAL) == (_lib.CRTP_UNORM8, _lib.CRTP_POST, _lib.CRTP_FXAA, _lib.CRTP_HEAL)
    assert ref.MODES == _lib.CRTP_VIEW_MODES
    # the state palette names the words of the upsample and of the re-trace
    assert sorted(ref.PALETTE) == sorted([_lib.CRTU_STATE_INTERPOLATED, _lib.CRTU_STATE_NEAREST, _lib.CRTU_STATE_EMPTY, _lib.CRTS_STATE_RETRACED])
    assert len(set(ref.PALETTE.values()) | {ref.MAGENTA}) == 5


def test_struct_sizes_and_offsets_are_the_header_s():
    """The figures the header's comments state, crt_present.hip static_asserts and _lib mirrors (LP64)."""
    header = open(os.path.join(ROOT, "include", "crt_present.h")).read()
    source = open(os.path.join(PRESENT_DIR, "crt_present.hip")).read()
    offsets = {_lib.CrtpPresent: (40, dict(width=0, height=4, color=8, ao=16, aoStrength=24, exposure=28, flags=32)),
               _lib.CrtpView: (64, dict(width=0, height=4, guides=8, mode=12, geometry=16, ids=24, albedo=32, plane=40, scale=48, lo=52, hi=56))}
    for struct, (size, fields) in offsets.items():
        assert C.sizeof(struct) == size, struct
        m = re.search(r"/\* %d bytes([^\n]*)\*/\ntypedef struct \{(?:(?!typedef).)*?\} %s;" % (size, struct.__name__), header, re.S)
        assert m, struct
        stated = {n: int(o) for n, o in re.findall(r"\b(\w+) (\d+)\b", m.group(1).split(":", 1)[1]) if n != "and"}
        stated.pop("bytes", None)
        assert stated == fields, (struct, stated)                           # the comment names every field with its offset
        assert "sizeof(%s) == %d" % (struct.__name__, size) in source, struct
        assert [n for n, _ in struct._fields_] == list(fields), struct
        for name, off in fields.items():
            assert getattr(struct, name).offset == off, (struct, name)
            if off:
                assert "offsetof(%s, %s) == %d" % (struct.__name__, name, off) in source, (struct, name)


def test_scratch_bytes_is_zero_for_refused_sizes_and_monotone():
    lib = _lib.present()
    for flags in range(16):
        sizes = [lib.crtp_scratch_bytes(w, h, flags) for w, h in ((1, 1), (3, 2), (33, 9), (200, 120), (1920, 1080), (3840, 2160), (16384, 16384))]
        assert sizes == sorted(sizes), (flags, sizes)
        assert [lib.crtp_scratch_bytes(w, h, flags) for w, h in ((0, 5), (5, 0), (-1, 5), (16385, 5), (5, 16385), (-2 ** 31, 1))] == [0] * 6
    assert lib.crtp_scratch_bytes(1920, 1080, 16) == 0      # an unknown flag


def test_error_strings():
    lib = _lib.present()
    assert lib.crtp_error_string(0) == b"ok"
    assert lib.crtp_error_string(-2) == b"crtp: bad argument" and b"range" in lib.crtp_error_string(-3) and b"16384" in lib.crtp_error_string(-3)
    assert b"unknown" in lib.crtp_error_string(-77)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
COLOR, AO, OUT, BYTES, SCRATCH, GEOMETRY, IDS, ALBEDO, PLANE = (i * A for i in range(1, 10))


def present(p=None, out=OUT, packed=BYTES, scratch=SCRATCH, null=False):
    f = dict(width=70, height=37, color=COLOR, ao=AO, aoStrength=0.5, exposure=1.5, flags=15)
    f.update(p or {})
    s = _lib.CrtpPresent(**f)
    return _lib.present().crtp_present(None if null else C.byref(s), out, packed, scratch, None)


def view(v=None, out=OUT, packed=BYTES, null=False):
    f = dict(width=70, height=37, guides=_lib.CRTP_GUIDES_PLANES, mode=_lib.CRTP_VIEW_NORMAL, geometry=GEOMETRY, ids=IDS, albedo=ALBEDO, plane=PLANE,
             scale=10.0, lo=0.0, hi=1.0)
    f.update(v or {})
    s = _lib.CrtpView(**f)
    return _lib.present().crtp_view(None if null else C.byref(s), out, packed, None)


SURFACE = dict(guides=_lib.CRTP_GUIDES_SURFACE, ids=None, albedo=None)
M = _lib.CRTP_VIEW_MODES
REFUSALS = {
    # crtp_present
    "present: null struct": (present, dict(null=True), BAD),
    "present: null color": (present, dict(p=dict(color=None)), BAD),
    "present: both outputs null": (present, dict(out=None, packed=None), BAD),
    **{f"present: flags {f}": (present, dict(p=dict(flags=f)), BAD) for f in (16, 32, 31, 0x80000000, 0xFFFFFFFF)},
    **{f"present: outColor is {n}": (present, dict(out=a), BAD) for n, a in (("color", COLOR), ("ao", AO))},
    **{f"present: outBytes is {n}": (present, dict(packed=a), BAD) for n, a in (("color", COLOR), ("ao", AO), ("outColor", OUT))},
    **{f"present: in place under flags {f}": (present, dict(p=dict(flags=f), out=COLOR), BAD) for f in (0, 1, 2, 3, 8)},
    "present: bytes in place without outColor": (present, dict(out=None, packed=COLOR), BAD),
    **{f"present: aoStrength {v}": (present, dict(p=dict(aoStrength=v)), BAD) for v in (NAN, INF, -INF, -0.001, 1.001, 2.0)},
    "present: aoStrength out of range without ao": (present, dict(p=dict(ao=None, aoStrength=1.5)), BAD),
    **{f"present: exposure {v}": (present, dict(p=dict(exposure=v)), BAD) for v in (NAN, INF, -INF, 0.0, -0.0, -1.0)},
    "present: width 0": (present, dict(p=dict(width=0)), BAD),
    "present: height 0": (present, dict(p=dict(height=0)), BAD),
    "present: negative width": (present, dict(p=dict(width=-5)), BAD),
    "present: negative height": (present, dict(p=dict(height=-2 ** 31)), BAD),
    "present: width 16385": (present, dict(p=dict(width=16385)), RANGE),
    "present: height 16385": (present, dict(p=dict(height=16385)), RANGE),
    "present: width 2^31 - 1": (present, dict(p=dict(width=2 ** 31 - 1)), RANGE),
    # crtp_view
    "view: null struct": (view, dict(null=True), BAD),
    "view: both outputs null": (view, dict(out=None, packed=None), BAD),
    **{f"view: mode {m}": (view, dict(v=dict(mode=m)), BAD) for m in (-1, 7, 100)},
    **{f"view: guides {g}": (view, dict(v=dict(guides=g, ids=None, albedo=None)), BAD) for g in (-1, 2)},
    "view: scalar under an unknown layout": (view, dict(v=dict(mode=M["scalar"], guides=2, ids=None, albedo=None)), BAD),
    **{f"view: {m} without geometry": (view, dict(v=dict(mode=M[m], geometry=None)), BAD) for m in ("normal", "depth")},
    **{f"view: {m} without ids": (view, dict(v=dict(mode=M[m], ids=None)), BAD) for m in ("instance", "triangle")},
    "view: albedo without albedo": (view, dict(v=dict(mode=M["albedo"], albedo=None)), BAD),
    **{f"view: {m} under SURFACE without records": (view, dict(v=dict(mode=M[m], geometry=None, **SURFACE)), BAD)
       for m in ("normal", "depth", "instance", "triangle", "albedo")},
    **{f"view: {m} without plane": (view, dict(v=dict(mode=M[m], plane=None)), BAD) for m in ("scalar", "state")},
    **{f"view: {m}, ids under SURFACE": (view, dict(v=dict(mode=M[m], guides=_lib.CRTP_GUIDES_SURFACE, albedo=None)), BAD) for m in M},
    **{f"view: {m}, albedo under SURFACE": (view, dict(v=dict(mode=M[m], guides=_lib.CRTP_GUIDES_SURFACE, ids=None)), BAD) for m in M},
    **{f"view: depth, scale {v}": (view, dict(v=dict(mode=M["depth"], scale=v)), BAD) for v in (NAN, INF, 0.0, -1.0)},
    **{f"view: scalar, lo {lo} hi {hi}": (view, dict(v=dict(mode=M["scalar"], lo=lo, hi=hi)), BAD)
       for lo, hi in ((NAN, 1.0), (0.0, NAN), (-INF, 1.0), (0.0, INF), (1.0, 1.0), (2.0, 1.0))},
    **{f"view: outColor is {n}": (view, dict(out=a), BAD) for n, a in (("geometry", GEOMETRY), ("ids", IDS), ("albedo", ALBEDO), ("plane", PLANE))},
    **{f"view: outBytes is {n}": (view, dict(packed=a), BAD)
       for n, a in (("geometry", GEOMETRY), ("ids", IDS), ("albedo", ALBEDO), ("plane", PLANE), ("outColor", OUT))},
    "view: state, outBytes is the plane": (view, dict(v=dict(mode=M["state"]), out=None, packed=PLANE), BAD),
    "view: width 0": (view, dict(v=dict(width=0)), BAD),
    "view: negative height": (view, dict(v=dict(height=-3)), BAD),
    "view: width 16385": (view, dict(v=dict(width=16385)), RANGE),
    "view: height 16385": (view, dict(v=dict(mode=M["state"], height=16385)), RANGE),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_come_before_anything_is_enqueued(case):
    """Every pointer is a dummy address: a refusal that dereferenced one would fault, and one that enqueued would need a device."""
    fn, kwargs, want = REFUSALS[case]
    assert fn(**kwargs) == want, case


# ---- the reference itself -------------------------------------------------------------------------------------------------------------------
def test_without_ao_exposure_and_heal_the_reference_is_the_oracle_s_chain():
    rng = np.random.RandomState(11)
    for W, H in ((33, 9), (16, 16), (70, 37)):
        frame = rng.uniform(0.0, 1.2, (H, W, 4)).astype(np.float32)
        frame[..., 3] = 1.0
        for flags in range(8):
            got, packed = ref.present(frame, flags)
            want = ref.frame_chain(frame, flags)
            assert np.array_equal(bits(got), bits(want)), (W, H, flags)
            assert np.array_equal(packed, ref.pack(want)) and (packed[..., 3] == 255).all(), (W, H, flags)
            # the bytes of the float result, by numpy: saturating, ties to even
            assert np.array_equal(packed[..., :3], ref.unorm8(got[..., :3]).astype(np.uint8)), (W, H, flags)
    # an exposure of 1 and an AO plane of ones at any strength change nothing; strength 0 ignores the plane
    ones = np.ones((H, W), np.float32)
    for flags in (0, 1, 5):
        base = ref.present(frame, flags)[0]
        assert np.array_equal(bits(ref.present(frame, flags, ao=ones, ao_strength=0.35)[0]), bits(base))
        assert np.array_equal(bits(ref.present(frame, flags, ao=rng.uniform(size=(H, W)).astype(np.float32), ao_strength=0.0)[0]), bits(base))


def test_heal_makes_every_output_finite_and_leaves_finite_pixels_alone():
    rng = np.random.RandomState(12)
    H, W = 9, 33
    frame = rng.uniform(-0.5, 3.0, (H, W, 4)).astype(np.float32)
    frame[1, 2, 0] = np.nan; frame[3, 4, 1] = np.inf; frame[5, 6, 2] = -np.inf
    ao = rng.uniform(size=(H, W)).astype(np.float32)
    ao[7, 8] = np.nan
    plain = ref.compose(frame, 0, ao, 0.35, 1.7)
    healed = ref.compose(frame, ref.HEAL, ao, 0.35, 1.7)
    assert np.isfinite(healed).all() and not np.isfinite(plain).all()
    same = np.isfinite(plain).all(axis=-1)
    assert np.array_equal(bits(plain[same]), bits(healed[same]))
    assert healed[1, 2, 0] == 0 and healed[3, 4, 1] == 0 and healed[5, 6, 2] == 0
    assert np.array_equal(healed[7, 8, :3], frame[7, 8, :3] * np.float32(1.7))      # a healed factor is 1
    for flags in (ref.HEAL, ref.HEAL | ref.FXAA, ref.HEAL | ref.UNORM8 | ref.FXAA):
        assert np.isfinite(ref.present(frame, flags, ao, 0.35, 1.7)[0]).all()


def test_the_fxaa_patterns_are_no_fixed_points_and_reach_the_clamps():
    for W, H in ((33, 9), (64, 16), (3, 2)):
        for name, img in ref.fxaa_patterns(W, H).items():
            img[..., 3] = 1.0
            out = ref.fxaa(img)
            if (W, H) != (3, 2) or name == "checkerboard":
                assert not np.array_equal(bits(out[..., :3]), bits(img[..., :3])), (W, H, name)
    # the direction's clamp: on the checkerboard's diagonal neighbours dir * rcpDirMin is 0 / small or large / small
    W, H = 64, 16
    img = ref.fxaa_patterns(W, H)["vertical edge"]
    luma = img[..., :3] @ np.array([0.299, 0.587, 0.114], np.float32)
    x = W // 2
    diry = (luma[0, x - 1] + luma[2, x - 1]) - (luma[0, x + 1] + luma[2, x + 1])
    reduce = max((luma[0, x - 1] + luma[0, x + 1] + luma[2, x - 1] + luma[2, x + 1]) * 0.03125, 1.0 / 128.0)
    assert abs(diry) / reduce > 8.0             # min(|dirx|, |diry|) is 0 on a straight edge: the ratio is clamped to 8


def test_view_reference_properties():
    t = np.array([[1.0, 99998.0, 99998.5, 99999.0, np.nan, 0.0]], np.float32)
    n = np.tile(np.array([0.0, 1.0, -1.0], np.float32), (1, 6, 1))
    f, b = ref.view("normal", normal=n, t=t)
    assert b[0, :2].tolist() == [[128, 255, 0, 255]] * 2 and b[0, 2:5].tolist() == [[0, 0, 0, 255]] * 3       # 127.5 rounds to even: 128
    assert np.array_equal(bits(f), bits(b.astype(np.float32) / np.float32(255)))
    f, b = ref.view("depth", t=t, scale=10.0)
    assert b[0, 5, 0] == 255 and b[0, 0, 0] == int(np.rint(np.float32(10.0) / np.float32(11.0) * np.float32(255))) and (b[0, 2:5, :3] == 0).all()
    inst = np.array([[-1, 0, 1, 2, 2 ** 31 - 1, -7]], np.int32)
    tri = np.array([[0, 0, 0, 5, 6, 7]], np.uint32)
    _, bi = ref.view("instance", instance=inst)
    _, bt = ref.view("triangle", instance=inst, tri=tri)
    assert (bi[0, 0, :3] == 0).all() and (bi[0, 5, :3] == 0).all() and (bt[0, 0, :3] == 0).all()
    assert len({tuple(p) for p in bi[0, 1:5, :3]}) == 4 and not np.array_equal(bi[0, 3], bt[0, 3])
    assert int(ref.hash32(1)) == int(ref.hash32(np.array([1], np.uint64))[0]) != 0 and int(ref.hash32(0)) == 0
    _, ba = ref.view("albedo", albedo=np.array([[0xFF102030, 0]], np.uint32))
    assert ba[0].tolist() == [[0x30, 0x20, 0x10, 255], [0, 0, 0, 255]]
    _, bs = ref.view("scalar", plane=np.array([[0.0, 0.5, 1.0, 2.0, -1.0, np.nan, np.inf, -np.inf]], np.float32))
    assert bs[0, :, 0].tolist() == [0, 128, 255, 255, 0, 255, 255, 0] and bs[0, 5].tolist() == [255, 0, 255, 255]
    _, bw = ref.view("state", plane=np.array([[0, 1, 2, 3, 7, -1]], np.int32))
    assert bw[0, :, :3].tolist() == [list(ref.PALETTE[k]) for k in range(4)] + [list(ref.MAGENTA)] * 2


# ---- the unit as the compiler sees it -------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_kernels_need_no_scratch_no_spill_and_no_agprs():
    rows = kernel_resource_rows(source=os.path.join(PRESENT_DIR, "crt_present.hip"))
    for n, r in rows:
        print(resource_line(n, r))
    tile = (32 + 2 * _lib.CRTP_FXAA_HALO) * (8 + 2 * _lib.CRTP_FXAA_HALO) * 16         # {S, 0} per texel of the tile and its halo
    # every flag set is an instantiation; an FXAA form has two: taps from LDS (true) and through L1 (false). Only the staged forms use LDS
    want = {**{f"crtp_present_kernel<{f}u, false>": 0 for f in range(16)},
            **{f"crtp_present_kernel<{f}u, true>": tile for f in range(16) if f & _lib.CRTP_FXAA},
            **{f"crtp_view_kernel<{m}, false>": 0 for m in range(7)},
            **{f"crtp_view_kernel<{m}, true>": 0 for m in range(5)}}
    assert sorted(n for n, _ in rows) == sorted(want)
    for n, r in rows:
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r.get("SGPRs Spill", 0) == 0 and r["AGPRs"] == 0, resource_line(n, r)
        assert r["LDS Size"] == want[n], resource_line(n, r)
        # the forms that recompute S at every tap hold a pixel's taps in registers (80-odd): the measured alternative, not the default
        l1_taps = n.startswith("crtp_present_kernel") and n.endswith("false>") and int(n.split("<")[1].split("u")[0]) & _lib.CRTP_FXAA
        assert r["Occupancy"] >= (5 if l1_taps else 8), resource_line(n, r)


def test_the_stages_are_written_once_and_the_library_owns_no_hip_object():
    sources = sorted(f for f in os.listdir(PRESENT_DIR) if f.endswith((".h", ".hip", ".cpp", ".hpp")))
    assert sources == ["crt_present.hip"]
    scanned = unit_sources("clraytracer_amd/present/crt_present.hip")
    assert set(scanned) == {os.path.join(PRESENT_DIR, "crt_present.hip"), os.path.join(ROOT, "include", "crt_present.h"),
                            os.path.join(IMAGE_DIR, "crt_image_device.h"), os.path.join(IMAGE_DIR, "crt_image_host.h"), os.path.join(IMAGE_DIR, "crt_image_env.h"),
                            os.path.join(CSRC_DIR, "crt_post.h"), os.path.join(CSRC_DIR, "crt_vec3.h")}
    # both libraries compile the one text of the stages, and nothing defines one of them a second time
    frame_unit = unit_sources("clraytracer_amd/csrc/crt_shim.hip")
    assert os.path.join(CSRC_DIR, "crt_post.h") in frame_unit and os.path.join(CSRC_DIR, "crt_vec3.h") in frame_unit
    for fn in ("post_pixel", "unorm8", "quantize1", "quantize3", "pack_rgba8", "fxaa_texel", "fxaa_linear", "fxaa_pixel", "mk3", "dot3"):
        defs = {}
        for path in sorted(set(scanned) | set(frame_unit)):
            text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))
            n = len(re.findall(r"__forceinline__\s+[\w:<> ]+?\b%s\s*\(" % fn, text))
            if n:
                defs[os.path.basename(path)] = n
        home = "crt_vec3.h" if fn in ("mk3", "dot3") else "crt_post.h"
        assert defs == {home: 2 if fn == "pack_rgba8" else 1}, (fn, defs)
    launches = 0
    for path in scanned:
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        assert not re.findall(HIP_OWNING_CALLS, text), path
        assert not re.findall(r"\bhip(DeviceSynchronize|StreamSynchronize|EventSynchronize|Memcpy\w*|Memset\w*|Malloc\w*|Free\w*)\s*\(", text), path
        assert not re.findall(r"\batomic\w*|__hip_atomic\w*|__atomic\w*|\bwhile\s*\(|\bvolatile\b|__threadfence\w*|\basm\b", text), path
        launches += len(re.findall(r"<<<", text))
    assert launches == 4                    # present: staged or not, the flags a template argument of the launcher; view: SURFACE or not
    if shutil.which("make"):
        p = subprocess.run(["make", "-n", "-W", "clraytracer_amd/present/crt_present.hip", _lib.PRESENT_SO.replace(ROOT + os.sep, "")], cwd=ROOT,
                           stdout=subprocess.PIPE, text=True, check=True)
        makefile = open(os.path.join(ROOT, "Makefile")).read()
        flags = re.search(r"^HIPFLAGS = (.*)$", makefile, re.M).group(1).replace("$(ARCH)", "gfx950").split()
        lines = [l.split() for l in p.stdout.splitlines() if "-shared" in l.split()]
        assert len(lines) == 1 and lines[0][1:] == flags + ["-shared", "-o", "clraytracer_amd/present/libcrt_present.so", "clraytracer_amd/present/crt_present.hip"]
        assert re.search(r"^all:.*\$\(PRESENT_SO\)", makefile, re.M) and re.search(r"rm -f .*\$\(PRESENT_SO\)", makefile)
        # a change of the shared stages rebuilds both libraries
        for so in (_lib.PRESENT_SO, _lib.HIP_SO):
            p = subprocess.run(["make", "-n", "-W", "clraytracer_amd/csrc/crt_post.h", so.replace(ROOT + os.sep, "")], cwd=ROOT, stdout=subprocess.PIPE, text=True, check=True)
            assert "-shared" in p.stdout, so
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.present()" in entry
