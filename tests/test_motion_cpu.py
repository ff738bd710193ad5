"""libcrt_motion.so without a GPU: the header, the ctypes table and the exports agree; the struct layouts match; every refusal of
include/crt_motion.h -- crtt_accumulate's own among them -- is answered before anything is dereferenced or enqueued; crtm_motion agrees with the
float64 statement in tests/motion_ref.py and takes an instance's points back to where they were; the numpy restatement equals
tests/temporal_ref.py bit for bit wherever nothing moves and follows a translated, a new and a rotated instance where that one cannot; the four
kernels cross-compile for gfx950 without scratch, spills or AGPRs at the sibling's occupancy; the library's source owns no HIP object, waits on
nothing and copies nothing."""
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

if not os.path.exists(getattr(_lib, "MOTION_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import motion_ref as ref
import temporal_ref
import test_temporal_cpu as sibling                     # its table of crtt_accumulate's refusals: every one is a refusal of crtm_accumulate
from test_abi import HIP_OWNING_CALLS
from util import bits, kernel_resource_rows, resource_line, unit_sources

MOTION_DIR = os.path.join(ROOT, "clraytracer_amd", "motion")
IMAGE_DIR = os.path.join(ROOT, "clraytracer_amd", "image")          # the headers the image libraries share, compiled into each
A = 0x10000                                      # dummy device addresses, 64 KiB apart: a refusal looks at none of them
NAMES = ["crtm_accumulate", "crtm_error_string", "crtm_motion", "crtm_motions"]
BAD = _lib.CRTT_E_BAD_ARGUMENT


def test_header_table_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "crt_motion.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert '#include "crt_temporal.h"' in text and not re.search(r"\bcrtt_\w+\s*\(", text)      # the sibling's types, none of its functions again
    names = sorted(set(re.findall(r"\b(crtm_\w+)\s*\(", text)))
    assert names == NAMES
    assert sorted(_lib.MOTION_API) == names
    lib = _lib.motion()
    for n in names:
        assert hasattr(lib, n), n
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.MOTION_SO], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(crtm_\w+)$", out, re.M))) == names
        assert not re.findall(r"\bcrt[dtv]?_\w+$", out, re.M)        # no crt_, crtd_, crtt_ or crtv_ name: those belong to the other libraries
    for name, value in (("CRTM_STATIC", 0), ("CRTM_MOVING", 1), ("CRTM_NEW", 2), ("CRTM_MAX_COUNT", 65536)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text) and getattr(_lib, name) == value, name
    assert (ref.STATIC, ref.MOVING, ref.NEW) == (_lib.CRTM_STATIC, _lib.CRTM_MOVING, _lib.CRTM_NEW)
    assert ref.MOTION_DTYPE == _lib.MOTION_DTYPE
    assert lib.crtm_error_string(0) == b"ok" and b"argument" in lib.crtm_error_string(-2) and b"range" in lib.crtm_error_string(-3)


def test_struct_sizes_and_offsets():
    header = open(os.path.join(ROOT, "include", "crt_motion.h")).read()
    source = open(os.path.join(MOTION_DIR, "crt_motion.hip")).read()
    for struct, size in ((_lib.CrtmMotion, 88), (_lib.CrtmMotionArgs, 24)):
        assert C.sizeof(struct) == size, struct
        assert re.search(r"/\* %d bytes[^\n]*\*/\ntypedef struct \{(?:(?!typedef).)*?\} %s;" % (size, struct.__name__), header, re.S), struct
        assert "sizeof(%s) == %d" % (struct.__name__, size) in source, struct
    assert C.alignment(_lib.CrtmMotion) == 4 and "alignof(CrtmMotion) == 4" in source
    offsets = {_lib.CrtmMotion: dict(kind=0, point=4, normal=52), _lib.CrtmMotionArgs: dict(table=0, count=8, vectors=16)}
    for struct, fields in offsets.items():
        assert [n for n, _ in struct._fields_] == list(fields), struct
        for name, off in fields.items():
            assert getattr(struct, name).offset == off, (struct, name)
            if off:
                assert "offsetof(%s, %s) == %d" % (struct.__name__, name, off) in source, (struct, name)
    assert [(n, _lib.MOTION_DTYPE.fields[n][1]) for n in _lib.MOTION_DTYPE.names] == [("kind", 0), ("point", 4), ("normal", 52)]
    assert _lib.MOTION_DTYPE.itemsize == 88 and _lib.INSTANCE_DTYPE.itemsize == 80 and "CRTM_INSTANCE_STRIDE 80" in source
    # the sibling's types are used as they are
    for struct, size in ((_lib.CrttCamera, 84), (_lib.CrttFrame, 128), (_lib.CrttHistory, 120), (_lib.CrttParams, 24)):
        assert "sizeof(%s) == %d" % (struct.__name__, size) in source, struct


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def call(frame=None, prev=None, nxt=None, params=None, motion=None, null_frame=False, null_prev=False, null_next=False, null_params=False,
         null_motion=False):
    """test_temporal_cpu.call with the motion arguments behind it: a table of 5 records at 12 * A and a vectors plane at 13 * A"""
    f = dict(width=70, height=37, color=1 * A, guides=_lib.CRTT_GUIDES_PLANES, geometry=2 * A, ids=3 * A)
    h0 = dict(color=4 * A, moments=5 * A, geometry=6 * A, instance=7 * A)
    h1 = dict(color=8 * A, moments=9 * A, geometry=10 * A, instance=11 * A)
    p = dict(flags=_lib.CRTT_MATCH_INSTANCE | _lib.CRTT_CLAMP, alpha=0.2, momentsAlpha=0.2, maxHistory=32.0, depthTol=0.05, normalCos=0.9)
    m = dict(table=12 * A, count=5, vectors=13 * A)
    f.update(frame or {}); h0.update(prev or {}); h1.update(nxt or {}); p.update(params or {}); m.update(motion or {})
    fs, h0s, h1s, ps, ms = _lib.CrttFrame(**f), _lib.CrttHistory(**h0), _lib.CrttHistory(**h1), _lib.CrttParams(**p), _lib.CrtmMotionArgs(**m)
    return _lib.motion().crtm_accumulate(None if null_frame else C.byref(fs), None if null_prev else C.byref(h0s), None if null_next else C.byref(h1s),
                                         None if null_params else C.byref(ps), None if null_motion else C.byref(ms), None)


NO_MATCH_NO_INSTANCE = dict(params=dict(flags=_lib.CRTT_CLAMP), nxt=dict(instance=None))
OWN_REFUSALS = {
    "null motion arguments": dict(null_motion=True),
    "null motion arguments on a reset": dict(null_motion=True, null_prev=True),
    "null table with a count": dict(motion=dict(table=None)),
    "a table with count 0": dict(motion=dict(count=0)),
    "count 65537": dict(motion=dict(count=65537)),
    "count 2^32 - 1": dict(motion=dict(count=2 ** 32 - 1)),
    "a table without ids under PLANES": dict(NO_MATCH_NO_INSTANCE, frame=dict(ids=None)),
    **{f"vectors is {what}": dict(motion=dict(vectors=k * A)) for k, what in enumerate(
        ("cur's colour", "cur's geometry", "cur's ids", "prev's colour", "prev's moments", "prev's geometry", "prev's instance", "next's colour",
         "next's moments", "next's geometry", "next's instance"), start=1)},
    "vectors is the records under SURFACE": dict(frame=sibling.SURFACE, motion=dict(vectors=2 * A)),
}


@pytest.mark.parametrize("case", list(sibling.REFUSALS))
def test_every_refusal_of_the_sibling_is_one_of_this_library(case):
    """Every pointer is a dummy address: a refusal that dereferenced one would fault, and one that enqueued would need a device. With a
    table and a vectors plane, and with neither."""
    kwargs, want = sibling.REFUSALS[case]
    assert call(**kwargs) == want, case
    assert call(**kwargs, motion=dict(table=None, count=0, vectors=None)) == want, case


@pytest.mark.parametrize("case", list(OWN_REFUSALS))
def test_refusals_of_the_motion_arguments(case):
    assert call(**OWN_REFUSALS[case]) == BAD, case


def test_what_is_no_refusal_is_not_in_the_tables_by_accident():
    """The count's bound is inclusive, and a table is allowed without ids where the layout carries them (checked through the next refusal in
    line: a width beyond 16384 is OUT_OF_RANGE only once every BAD_ARGUMENT test has passed)."""
    wide = dict(width=16385)
    assert call(frame=wide) == _lib.CRTT_E_OUT_OF_RANGE
    assert call(frame=wide, motion=dict(count=65536)) == _lib.CRTT_E_OUT_OF_RANGE
    assert call(frame=wide, motion=dict(table=None, count=0)) == _lib.CRTT_E_OUT_OF_RANGE
    assert call(frame=wide, motion=dict(vectors=None)) == _lib.CRTT_E_OUT_OF_RANGE
    assert call(frame=dict(sibling.SURFACE, width=16385)) == _lib.CRTT_E_OUT_OF_RANGE
    assert call(frame=dict(wide, ids=None), motion=dict(table=None, count=0), **NO_MATCH_NO_INSTANCE) == _lib.CRTT_E_OUT_OF_RANGE


# ---- crtm_motion ----------------------------------------------------------------------------------------------------------------------------
def lib_motion(prev, cur):
    out = _lib.CrtmMotion()
    ptr = lambda a: None if a is None else _lib.fptr(np.asarray(a).reshape(16))[0]
    keep = [np.ascontiguousarray(a, np.float32) for a in (prev, cur) if a is not None]      # noqa: F841
    rc = _lib.motion().crtm_motion(ptr(prev), ptr(cur), C.byref(out))
    return rc, out.kind, np.array(out.point[:], np.float32), np.array(out.normal[:], np.float32)


def trs_pairs():
    """Seeded (forward transform of the previous frame, of this frame) in float64 at the sizes of the multi-1M instance table (scenes._multi:
    scales 0.5 .. 2, any rotation, translations within 25 of the origin): a pure translation, a pure rotation, a uniform and a non-uniform
    scale change, and all of them at once; each as a small step (an animation's) and as a large one."""
    rng = np.random.RandomState(77)
    pairs = []
    for k in range(200):
        base = ref.trs(translate=rng.uniform(-25, 25, 3), axis=rng.normal(size=3), angle=rng.uniform(0, 2 * np.pi), scale=np.full(3, rng.uniform(0.5, 2.0)))
        size = (1e-3, 1.0)[k % 2]
        step = [dict(translate=size * rng.uniform(-5, 5, 3)), dict(axis=rng.normal(size=3), angle=size * rng.uniform(-3, 3)),
                dict(scale=np.full(3, 1.0 + size * rng.uniform(-0.5, 1.0))), dict(scale=1.0 + size * rng.uniform(-0.5, 1.0, 3)),
                dict(translate=size * rng.uniform(-5, 5, 3), axis=rng.normal(size=3), angle=size * rng.uniform(-3, 3), scale=1.0 + size * rng.uniform(-0.5, 1.0, 3))][k // 2 % 5]
        pairs.append((base, ref.trs(**step) @ base if k % 4 < 2 else base @ ref.trs(**step)))
    return pairs


# The largest element-wise |crtm_motion - float32(motion_ref.motion)| over trs_pairs(), measured on the CPU (printed by the test): 3.553e-15. Both
# are float64 computations rounded to float32 once, by different routes (cofactors of the 3 x 3 blocks here, LAPACK on the 4 x 4 there), which
# agree to about 1e-15: every element of a size that matters rounds to the same float32 (the translations reach 64, an ulp of 3.8e-6, and none
# differs), and what is left is the difference between two float32 roundings of an entry that is zero but for the double rounding.
MOTION_MEASURED = 3.56e-15
MOTION_BOUND = 4 * MOTION_MEASURED
# The largest distance between where `point` (float32, evaluated in float64) puts a point of the instance (within 3 units of the mesh's origin, as
# the meshes of multi-1M are) and where the float64 forward transforms had it in the previous frame, over the same pairs: 3.003e-6, the float32
# rounding of the two inverseTransforms and of the record (2^-24 relative on translations of up to 50 units).
POINT_MEASURED = 3.01e-6
POINT_BOUND = 4 * POINT_MEASURED


def test_motion_agrees_with_the_float64_statement_and_takes_points_back():
    rng = np.random.RandomState(78)
    worst, worst_point, worst_normal = 0.0, 0.0, 0.0
    for prev_fwd, cur_fwd in trs_pairs():
        prev_inv, cur_inv = ref.inverse32(prev_fwd), ref.inverse32(cur_fwd)
        rc, kind, point, normal = lib_motion(prev_inv, cur_inv)
        want_kind, want_point, want_normal = ref.motion(prev_inv, cur_inv)
        assert rc == 0 and kind == want_kind == ref.MOVING
        worst = max(worst, float(np.abs(point - want_point.astype(np.float32)).max()), float(np.abs(normal - want_normal.astype(np.float32)).max()))
        # functional: points of the instance, moved by the forward transforms in float64
        local = np.concatenate([rng.uniform(-3, 3, (16, 3)), np.ones((16, 1))], axis=1)
        now, before = (local @ cur_fwd)[:, :3], (local @ prev_fwd)[:, :3]
        pt = point.astype(np.float64).reshape(3, 4)
        worst_point = max(worst_point, float(np.linalg.norm(now @ pt[:, :3].T + pt[:, 3] - before, axis=1).max()))
        # and normals: a plane's normal n (as a row vector's dual) follows the inverse transpose; the record's map agrees up to its length
        n_now = rng.normal(size=(8, 3))
        T = ref.affine(cur_inv) @ np.linalg.inv(ref.affine(prev_inv))
        m = n_now @ normal.astype(np.float64).reshape(3, 3).T
        tangent = rng.normal(size=(8, 3)); tangent -= n_now * ((tangent * n_now).sum(1) / (n_now * n_now).sum(1))[:, None]      # in the plane now
        worst_normal = max(worst_normal, float(np.abs(((tangent @ T[:3, :3]) * m).sum(1) / (np.linalg.norm(tangent @ T[:3, :3], axis=1) * np.linalg.norm(m, axis=1))).max()))
    print(f"crtm_motion against float32(motion_ref.motion): largest difference {worst:.3e}; points taken back to within {worst_point:.3e}; "
          f"|cos| between a moved tangent and the moved normal at most {worst_normal:.3e}")
    assert worst <= MOTION_BOUND
    assert worst_point <= POINT_BOUND
    assert worst_normal <= 1e-5                                              # perpendicular stays perpendicular (float32 rounding of nine entries)


def test_motion_kinds_and_refusals():
    fwd = ref.trs(translate=(3.0, 4.0, -5.0), axis=(1.0, 2.0, 3.0), angle=0.7, scale=(1.5, 1.5, 1.5))
    inv = ref.inverse32(fwd)
    eye_p, eye_n = np.eye(3, 4, dtype=np.float32).reshape(-1), np.eye(3, dtype=np.float32).reshape(-1)
    rc, kind, point, normal = lib_motion(inv, inv.copy())
    assert (rc, kind) == (0, _lib.CRTM_STATIC) and np.array_equal(point, eye_p) and np.array_equal(normal, eye_n)
    rc, kind, point, normal = lib_motion(None, inv)
    assert (rc, kind) == (0, _lib.CRTM_NEW) and np.array_equal(point, eye_p) and np.array_equal(normal, eye_n)
    # one bit of one element: MOVING -- also of an element of the fourth column, which the map itself never reads (crt_device.h: xform_xyz)
    nudged = inv.copy(); nudged[3, 0] = np.nextafter(nudged[3, 0], np.float32(np.inf))
    assert lib_motion(inv, nudged)[1] == _lib.CRTM_MOVING
    col3 = inv.copy(); col3[:, 3] = (5.0, -6.0, 7.0, 0.5)
    rc, kind, point, normal = lib_motion(inv, col3)
    assert (rc, kind) == (0, _lib.CRTM_MOVING)
    assert np.abs(point - eye_p).max() <= 4e-6 and np.abs(normal - eye_n).max() <= 4e-7      # ... and so moves nothing (rounding of A A^-1 only)

    def edited(m, i, j, v):
        m = m.copy(); m[i, j] = v
        return m

    out = _lib.CrtmMotion(); out.kind = 77
    lib = _lib.motion()
    p_inv, k1 = _lib.fptr(inv.reshape(16))
    assert lib.crtm_motion(p_inv, None, C.byref(out)) == BAD and lib.crtm_motion(p_inv, p_inv, None) == BAD and lib.crtm_motion(None, None, C.byref(out)) == BAD
    flat = inv.copy(); flat[:3, 2] = 0.0                                      # a 3 x 3 block that spans no volume
    huge = np.eye(4, dtype=np.float32) * np.float32(1e30); tiny = np.eye(4, dtype=np.float32) * np.float32(1e-30)
    for what, (a, b) in {"NaN in cur": (inv, edited(inv, 1, 1, np.nan)), "inf in prev": (edited(inv, 3, 0, np.inf), inv),
                         "NaN in the fourth column": (inv, edited(inv, 0, 3, np.nan)), "a singular prev": (flat, inv), "a singular L": (inv, flat),
                         "a result beyond float32": (tiny, huge), "NaN in cur of a new instance": (None, edited(inv, 2, 0, np.nan))}.items():
        pa = None if a is None else _lib.fptr(a.reshape(16))
        pb = _lib.fptr(b.reshape(16))
        assert lib.crtm_motion(None if pa is None else pa[0], pb[0], C.byref(out)) == BAD, what
    assert out.kind == 77                                                     # a refusal writes nothing


def test_motions_is_a_loop_of_motion():
    pairs = trs_pairs()[:12]
    prev = np.zeros(9, _lib.INSTANCE_DTYPE); cur = np.zeros(12, _lib.INSTANCE_DTYPE)
    prev["pad"], cur["pad"], cur["meshIndex"] = 0xAB, 0xCD, 7                # what lies between the matrices is skipped, not read
    for i, (a, b) in enumerate(pairs):
        cur["inv"][i] = ref.inverse32(b)
        if i < len(prev):
            prev["inv"][i] = ref.inverse32(a) if i % 3 else cur["inv"][i]
    table = _lib.crtm_motions(prev, cur)
    assert table.dtype == _lib.MOTION_DTYPE and table.shape == (12,)
    for i in range(12):
        rc, kind, point, normal = lib_motion(prev["inv"][i] if i < 9 else None, cur["inv"][i])
        assert rc == 0 and table["kind"][i] == kind == (_lib.CRTM_NEW if i >= 9 else _lib.CRTM_MOVING if i % 3 else _lib.CRTM_STATIC), i
        assert np.array_equal(bits(table["point"][i]), bits(point)) and np.array_equal(bits(table["normal"][i]), bits(normal)), i
    assert (_lib.crtm_motions(None, cur)["kind"] == _lib.CRTM_NEW).all()
    assert _lib.crtm_motions(prev, cur[:4]).shape == (4,) and _lib.crtm_motions(prev, cur[:0]).shape == (0,)
    lib = _lib.motion()
    out = np.zeros(12, _lib.MOTION_DTYPE)
    assert lib.crtm_motions(None, 3, cur.ctypes.data, 12, out.ctypes.data) == BAD and lib.crtm_motions(prev.ctypes.data, 9, None, 12, out.ctypes.data) == BAD
    assert lib.crtm_motions(prev.ctypes.data, 9, cur.ctypes.data, 12, None) == BAD and lib.crtm_motions(None, 0, None, 0, None) == 0
    bad = cur.copy(); bad["inv"][5, 0, 0] = np.nan
    with pytest.raises(_lib.CrtError, match="bad argument"):
        _lib.crtm_motions(prev, bad)
    # instance_records: the two forms Session.accumulate takes
    assert np.array_equal(_lib.instance_records(cur["inv"])["inv"], cur["inv"]) and _lib.instance_records(cur) is not None
    for wrong in (cur["inv"].astype(np.float64), cur["inv"][0], np.zeros((3, 16), np.float32), [1, 2, 3]):
        with pytest.raises(ValueError, match="instances"):
            _lib.instance_records(wrong)


# ---- the reference itself, on hand-made planes ----------------------------------------------------------------------------------------------
H, W = 37, 70
PLANES = ("color", "moments", "geometry", "instance")


def same_history(a, b):
    for k in PLANES[:3]:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(a["instance"], b["instance"])


@pytest.mark.parametrize("flags", range(4))
def test_where_nothing_moves_the_reference_is_the_siblings(flags):
    planes = ref.guides(H, W, seed=0)
    g, inst, color = planes["geometry"], planes["ids"]["instance"].astype(np.int32), ref.noisy_color(H, W, seed=0)
    assert set(np.unique(inst)) == {-1, 3, 7}
    cur, prev_cam = ref.camera_pairs(W, H)["translation"]
    prev = temporal_ref.history_content(H, W, prev_cam, seed=0)
    want = temporal_ref.accumulate(color, g, inst, cur, prev=prev, flags=flags)
    assert (want["moments"][..., 2] > 1).any() and (want["moments"][..., 2] == 1).any()
    moving = ref.hand_made_table()[2]
    static = ref.table([ref.motion(np.eye(4), np.eye(4))] * 8)
    for name, motions in {"no table": None, "an empty table": static[:0], "every entry static": static,
                          "ids out of range": ref.table([(ref.MOVING, moving["point"], moving["normal"])] * 3)}.items():   # 3 and 7 lie beyond it, -1 below
        got, vectors = ref.accumulate(color, g, inst, cur, prev=prev, motions=motions, flags=flags)
        same_history(got, want)
        assert set(np.unique(vectors[..., 3])) == {0.0, 1.0, 2.0}, name
        assert np.array_equal(vectors[..., 3] == 2.0, want["moments"][..., 2] > 1), name
    # while a moving entry that is reached changes the result: the table is looked at
    got, _ = ref.accumulate(color, g, inst, cur, prev=prev, motions=ref.table([(ref.MOVING, moving["point"], moving["normal"])] * 8), flags=flags)
    assert not np.array_equal(bits(got["color"]), bits(want["color"]))
    # a reset: the frame itself and no vectors, whatever the table says
    got, vectors = ref.accumulate(color, g, inst, cur, prev=None, motions=ref.hand_made_table(), flags=flags)
    same_history(got, temporal_ref.accumulate(color, g, inst, cur, flags=flags))
    assert not vectors.any()


Z0 = 20.0                                        # the fronto-parallel plane of the scenarios below
REGION = (18, 52, 8, 30)                         # x from, x to, y from, y to of the moving instance in the previous frame


def plane_frame(cam, normal=(0.0, 0.0, -1.0), through=(0.0, 0.0, Z0)):
    """the {n, t} plane of a camera at the origin looking at the plane through `through` with `normal` (float64 t, rounded)"""
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.stack([xx, yy, np.ones_like(xx)], axis=-1).astype(np.float64) @ cam["toRay"].astype(np.float64).T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    n = np.asarray(normal, np.float64)
    g = np.empty((H, W, 4), np.float32)
    g[..., :3] = n
    g[..., 3] = (np.asarray(through, np.float64) @ n) / (d @ n)
    return g


def own_colour(x0):
    """a smooth colour over the region's own coordinates (x - x0, y): what a texture on the moving instance looks like"""
    yy, xx = np.mgrid[0:H, 0:W]
    c = np.ones((H, W, 4), np.float32)
    for ch in range(3):
        c[..., ch] = 0.5 + 0.4 * np.sin(0.23 * (xx - x0) + 0.11 * yy + ch)
    return c


# |vectors.xy - (-k, 0)| on the region, measured on the reference (printed by the test): 3.815e-6 for k = 1, 7.629e-6 for k = 3 -- the float32
# rounding of the direction, of P and of fx, one or two ulps of a pixel coordinate of up to 70
VECTOR_MEASURED = 7.63e-6
VECTOR_BOUND = 4 * VECTOR_MEASURED


@pytest.mark.parametrize("k", [1, 3])
def test_a_translated_instance_keeps_the_history_of_its_own_surface(k):
    cam = ref.pinhole(W, H)
    g = plane_frame(cam)
    xa, xb, ya, yb = REGION
    yy, xx = np.mgrid[0:H, 0:W]
    inst_prev = np.where((xx >= xa) & (xx < xb) & (yy >= ya) & (yy < yb), 1, 0).astype(np.int32)
    inst_cur = np.where((xx >= xa + k) & (xx < xb + k) & (yy >= ya) & (yy < yb), 1, 0).astype(np.int32)
    pixel = Z0 * 2.0 * np.tan(0.5) / W                                      # the width of a pixel on the plane
    before = ref.trs(translate=(1.0, 2.0, Z0))
    now = before @ ref.trs(translate=(k * pixel, 0.0, 0.0))
    motions = ref.table([ref.motion(np.eye(4), np.eye(4)), ref.motion(ref.inverse32(before), ref.inverse32(now))])
    color_prev, color_cur = own_colour(xa), own_colour(xa + k)
    prev = temporal_ref.accumulate(color_prev, g, inst_prev, cam)
    kw = dict(flags=ref.MATCH_INSTANCE, alpha=0.2)
    got, vectors = ref.accumulate(color_cur, g, inst_cur, cam, prev=prev, motions=motions, **kw)
    static = temporal_ref.accumulate(color_cur, g, inst_cur, cam, prev=prev, **kw)
    inner = (xx >= xa + k + 1) & (xx < xb - 1) & (yy >= ya + 1) & (yy < yb - 1)      # the instance in both frames, a tap's width from its border
    assert inner.sum() > 400
    assert (got["moments"][..., 2][inner] == 2).all() and (vectors[..., 3][inner] == 2).all()
    off = float(np.maximum(np.abs(vectors[..., 0] + k), np.abs(vectors[..., 1]))[inst_cur == 1].max())
    print(f"k = {k}: |vectors.xy - (-k, 0)| at most {off:.3e}")
    assert off <= VECTOR_BOUND
    # vectors.z is the distance from the previous camera to where the point was: k pixels to the side of where it is
    d = np.stack([xx, yy, np.ones_like(xx)], axis=-1).astype(np.float64) @ cam["toRay"].astype(np.float64).T
    was = d / np.linalg.norm(d, axis=-1, keepdims=True) * g[..., 3:4].astype(np.float64) - (k * pixel, 0.0, 0.0)
    assert np.abs(vectors[..., 2] - np.linalg.norm(was, axis=-1))[inst_cur == 1].max() <= 1e-4
    # the history came from the same place on the surface: what is left is the frame itself (the colour is the same function of the region's
    # coordinates in both frames; a fetch a few 1e-5 pixel off a smooth function changes it by less than 1e-5)
    assert np.abs(got["color"][..., :3] - color_cur[..., :3])[inner].max() < 1e-5
    # the camera-only reprojection also keeps history there -- the same instance at the same depth and normal -- but from k pixels to the side
    assert (static["moments"][..., 2][inner] == 2).all()
    smear = np.abs(static["color"][..., :3] - color_cur[..., :3])[inner].max(axis=-1)
    assert np.median(smear) > 0.01 * k and (bits(static["color"]) != bits(got["color"]))[inner].any(axis=-1).mean() > 0.99
    # the static part of the frame is the sibling's, bit for bit
    rest = (inst_cur == 0) & (inst_prev == 0)
    for name in PLANES[:3]:
        assert np.array_equal(bits(got[name])[rest], bits(static[name])[rest]), name
    # a new instance has no history anywhere, and no vector
    fresh = ref.table([motions[0], ref.motion(None, ref.inverse32(now))])
    got_new, vectors_new = ref.accumulate(color_cur, g, inst_cur, cam, prev=prev, motions=fresh, **kw)
    assert (got_new["moments"][..., 2][inst_cur == 1] == 1).all() and not vectors_new[inst_cur == 1].any()
    assert np.array_equal(bits(got_new["color"])[inst_cur == 1], bits(color_cur)[inst_cur == 1])
    for name in PLANES[:3]:
        assert np.array_equal(bits(got_new[name])[rest], bits(static[name])[rest]), name


def test_a_rotated_instance_is_tested_against_its_rotated_normal():
    """The whole frame is one instance: a plane that faces the camera now and stood turned by 40 degrees about the vertical through its centre
    a frame ago -- more than acos(normalCos) = 25.8 degrees. The history's normals are the turned plane's."""
    theta, normal_cos = np.radians(40.0), 0.9
    assert theta > np.arccos(normal_cos)
    cam = ref.pinhole(W, H)
    centre = np.array([0.0, 0.0, Z0])
    about = ref.trs(translate=centre)
    turn = np.linalg.inv(about) @ ref.trs(axis=(0.0, 1.0, 0.0), angle=theta) @ about      # p -> (p - centre) R + centre
    before = ref.trs(translate=(0.5, -1.0, Z0), scale=(1.5, 1.5, 1.5))
    now = before @ turn
    kind, point, normal = ref.motion(ref.inverse32(before), ref.inverse32(now))
    T = np.linalg.inv(now) @ before                                          # a point now -> the point a frame ago
    n_now = np.array([0.0, 0.0, -1.0])
    n_before = n_now @ np.linalg.inv(T[:3, :3]).T
    assert abs(np.linalg.norm(n_before) - 1.0) < 1e-12 and abs(n_before @ n_now - np.cos(theta)) < 1e-12
    g_now, g_before = plane_frame(cam), plane_frame(cam, normal=n_before, through=centre)
    inst = np.zeros((H, W), np.int32)
    color = ref.noisy_color(H, W, seed=4, nans=False)
    prev = temporal_ref.accumulate(color, g_before, inst, cam)
    motions = ref.table([(kind, point, normal)])
    kw = dict(flags=ref.MATCH_INSTANCE, normal_cos=normal_cos, depth_tol=0.05)
    got, vectors = ref.accumulate(color, g_now, inst, cam, prev=prev, motions=motions, **kw)
    unrotated, vectors_unrotated = ref.accumulate(color, g_now, inst, cam, prev=prev, motions=motions, static_normal=True, **kw)
    assert np.array_equal(bits(vectors[..., :3]), bits(vectors_unrotated[..., :3]))     # the same v, the same taps
    inner = (vectors[..., 3] > 0) & (vectors[..., 0] + np.mgrid[0:H, 0:W][1] >= 1) & (vectors[..., 0] + np.mgrid[0:H, 0:W][1] < W - 2) \
        & (vectors[..., 1] + np.mgrid[0:H, 0:W][0] >= 1) & (vectors[..., 1] + np.mgrid[0:H, 0:W][0] < H - 2)
    assert inner.mean() > 0.5                                                 # the turn keeps most of the plane on the screen
    assert np.abs(vectors[..., 0][inner]).max() > 5.0                         # ... and moves it: away from the axis by many pixels
    assert (got["moments"][..., 2][inner] == 2).all() and (vectors[..., 3][inner] == 2).all()
    assert (unrotated["moments"][..., 2][inner] == 1).all() and (vectors_unrotated[..., 3][inner] == 1).all()
    # the camera-only reprojection looks straight behind the pixel, where the turned plane lies at another depth except near the axis
    static = temporal_ref.accumulate(color, g_now, inst, cam, prev=prev, **kw)
    assert (static["moments"][..., 2][inner] == 1).all()


def test_the_hand_made_table_reaches_every_kind():
    """What tests/test_gpu_motion.py relies on, at its largest shapes: all five ids occur, each moving entry keeps some history and loses
    some, and the moving pixels' taps are not the static reprojection's."""
    table = ref.hand_made_table()
    assert list(table["kind"]) == [ref.STATIC, ref.MOVING, ref.MOVING, ref.NEW] and np.isfinite(table["point"]).all() and np.isfinite(table["normal"]).all()
    for w, h in ((70, 37), (257, 19)):
        planes, color, hist = ref.hand_made_inputs(h, w)
        inst = planes["ids"]["instance"].astype(np.int32)
        assert set(np.unique(inst)) == {-1, 0, 1, 2, 3, 4} and set(np.unique(hist["instance"])) == {-1, 0, 1, 2, 3, 4}
        for pair in ("identical", "sub-pixel pan"):
            cur, prev_cam = ref.camera_pairs(w, h)[pair]
            prev = dict(hist, camera=prev_cam)
            got, vectors = ref.accumulate(color, planes["geometry"], inst, cur, prev=prev, motions=table, flags=3)
            static = temporal_ref.accumulate(color, planes["geometry"], inst, cur, prev=prev, flags=3)
            hit = planes["geometry"][..., 3] <= 99998.0
            for i in (1, 2):
                N = got["moments"][..., 2][hit & (inst == i)]
                assert (N > 1).any() and (N == 1).any(), (w, h, pair, i)
                assert (bits(got["color"]) != bits(static["color"]))[hit & (inst == i)].any(), (w, h, pair, i)
            assert (got["moments"][..., 2][hit & (inst == 3)] == 1).all() and not vectors[inst == 3].any()
            for i in (0, 4):
                assert np.array_equal(bits(got["color"])[inst == i], bits(static["color"])[inst == i]), (w, h, pair, i)
            assert set(np.unique(vectors[..., 3])) == {0.0, 1.0, 2.0}


# ---- the unit as the compiler sees it -------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_kernels_need_no_scratch_no_spill_no_agprs_and_keep_the_siblings_occupancy():
    source = open(os.path.join(MOTION_DIR, "crt_motion.hip")).read()
    # the unit's own constants, the tile's from the shared device steps and the halo from the shared kernel's header
    defines = lambda text, names: {k: int(v) for k, v in re.findall(r"^#define (%s) (\d+)\b" % names, text, re.M)}
    const = {**defines(source, "CRTM_TABLE_LDS|CRTM_UNSTAGED_PAD"), **defines(open(os.path.join(IMAGE_DIR, "crt_image_device.h")).read(), "CRTI_TILE_W|CRTI_TILE_H"),
             **defines(open(os.path.join(IMAGE_DIR, "crt_accumulate.h")).read(), "CRT_ACCUMULATE_HALO")}
    assert len(const) == 5
    tile = (const["CRTI_TILE_W"] + 2 * const["CRT_ACCUMULATE_HALO"]) * (const["CRTI_TILE_H"] + 2 * const["CRT_ACCUMULATE_HALO"]) * 16 + const["CRTM_TABLE_LDS"]
    rows = kernel_resource_rows(source=os.path.join(MOTION_DIR, "crt_motion.hip"))
    for n, r in rows:
        print(resource_line(n, r))
    tf = ("false", "true")
    # instantiations over this library's pass of the template it shares with libcrt_temporal.so: <PASS, SURFACE, GATED, STAGE>, always gated, and nothing else
    assert sorted(n for n, _ in rows) == sorted(f"crt_accumulate_kernel<CrtmPass, {s}, true, {l}>" for s in tf for l in tf)
    for n, r in rows:
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r.get("SGPRs Spill", 0) == 0 and r["AGPRs"] == 0, resource_line(n, r)
        assert r["LDS Size"] == (tile if n.endswith("true>") else 0), resource_line(n, r)       # nothing but the staged tile
        assert r["Occupancy"] >= 5, resource_line(n, r)                         # crt_accumulate_kernel<CrttPass, *, true, *>'s
    # The unstaged kernels' registers would allow 8 waves per SIMD, which measures slower than 5: they are launched with a pad of
    # dynamic LDS they never touch (no remark counts it) that holds a CU's 160 KiB to 5 workgroups of 4 waves; the staged ones with none
    assert (160 * 1024) // const["CRTM_UNSTAGED_PAD"] == 5 and const["CRTM_UNSTAGED_PAD"] % 1024 == 0
    assert "crt_accumulate_kernel<CrtmPass, SURFACE, true, false><<<grid, CRTI_BLOCK, CRTM_UNSTAGED_PAD, stream>>>" in source
    assert "crt_accumulate_kernel<CrtmPass, SURFACE, true, true><<<grid, CRTI_BLOCK, 0, stream>>>" in source
    assert not any("extern __shared__" in open(path).read() for path in unit_sources("clraytracer_amd/motion/crt_motion.hip"))


def test_the_library_owns_no_hip_object_and_follows_the_recipe():
    sources = sorted(f for f in os.listdir(MOTION_DIR) if f.endswith((".h", ".hip", ".cpp", ".hpp")))
    assert sources == ["crt_motion.hip"]
    # what the image libraries share, exactly: headers that are compiled into each library; this one leaves out the environment's
    assert sorted(os.listdir(IMAGE_DIR)) == ["crt_accumulate.h", "crt_image_device.h", "crt_image_env.h", "crt_image_host.h"]
    # the unit and every in-tree header it includes, transitively: the shared steps of clraytracer_amd/image/ are this library's source too
    scanned = unit_sources("clraytracer_amd/motion/crt_motion.hip")
    assert {os.path.join(MOTION_DIR, f) for f in sources} | {os.path.join(ROOT, "include", "crt_motion.h"), os.path.join(IMAGE_DIR, "crt_image_device.h"),
                                                            os.path.join(IMAGE_DIR, "crt_image_host.h"), os.path.join(IMAGE_DIR, "crt_accumulate.h")} <= set(scanned)
    for path in scanned:
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        assert not re.findall(HIP_OWNING_CALLS, text), path
        assert not re.findall(r"\bhip(DeviceSynchronize|StreamSynchronize|EventSynchronize|Memcpy\w*|Memset\w*)\s*\(", text), path     # nor waits or copies
        assert not re.findall(r"\basm\b|getenv", text), path                  # plain C++ stores, and no switch in the environment
    assert os.path.join(IMAGE_DIR, "crt_image_env.h") not in scanned
    assert len(re.findall(r"<<<", open(os.path.join(MOTION_DIR, "crt_motion.hip")).read())) == 2     # one launch per call: STAGE or not
    assert sum(len(re.findall(r"<<<", open(path).read())) for path in scanned) == 2                  # ... and none in a header
    if shutil.which("make"):
        p = subprocess.run(["make", "-n", "-W", "clraytracer_amd/motion/crt_motion.hip", _lib.MOTION_SO.replace(ROOT + os.sep, "")], cwd=ROOT,
                           stdout=subprocess.PIPE, text=True, check=True)
        makefile = open(os.path.join(ROOT, "Makefile")).read()
        flags = re.search(r"^HIPFLAGS = (.*)$", makefile, re.M).group(1).replace("$(ARCH)", "gfx950").split()
        lines = [l.split() for l in p.stdout.splitlines() if "-shared" in l.split()]
        assert len(lines) == 1 and lines[0][1:] == flags + ["-shared", "-o", "clraytracer_amd/motion/libcrt_motion.so", "clraytracer_amd/motion/crt_motion.hip"]
        assert re.search(r"^all:.*\$\(MOTION_SO\)", makefile, re.M) and re.search(r"rm -f .*\$\(MOTION_SO\)", makefile)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.motion()" in entry
