"""libcrt_select.so without a GPU: the header, the ctypes table and the exports agree; the struct layouts match the header's comments;
crts_scratch_bytes is positive and monotone; every refusal of include/crt_select.h is answered before anything is dereferenced or enqueued; the
numpy restatement (tests/select_ref.py) has the properties the library exists for -- an ascending list padded with NONE, a state plane that
compacts back to the list it was scattered from, zero rows for entries that name no pixel, a zero normal for a pixel that is no hit, points that
lie on the wall they were shot at; the selection the GPU session test re-traces is neither empty nor too large for its capacity; the kernels
cross-compile for gfx950 without scratch, spills or AGPRs; the library's source owns no HIP object, waits on nothing, copies nothing and uses no
atomic."""
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
from clraytracer_amd import _lib, driver, scenes

if not os.path.exists(getattr(_lib, "SELECT_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import gbuffer_ref
import oracle_lib
import select_ref as ref
import upsample_ref
from test_abi import HIP_OWNING_CALLS
from util import bits, kernel_resource_rows, resource_line, unit_sources

SELECT_DIR = os.path.join(ROOT, "clraytracer_amd", "select")
IMAGE_DIR = os.path.join(ROOT, "clraytracer_amd", "image")
A = 0x10000                                      # dummy device addresses, 64 KiB apart: a refusal looks at none of them
NAMES = ["crts_compact", "crts_error_string", "crts_points", "crts_scatter", "crts_scratch_bytes"]
BAD, RANGE = _lib.CRTS_E_BAD_ARGUMENT, _lib.CRTS_E_OUT_OF_RANGE


def test_header_table_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "crt_select.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(crts_\w+)\s*\(", text)))
    assert names == NAMES
    assert sorted(_lib.SELECT_API) == names
    lib = _lib.select()
    for n in names:
        assert hasattr(lib, n), n
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.SELECT_SO], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(crts_\w+)$", out, re.M))) == names
        assert not re.findall(r"\bcrt[dtvmu]?_\w+$", out, re.M)     # no name of another library's
    for name, value in (("CRTS_OK", 0), ("CRTS_E_BAD_ARGUMENT", -2), ("CRTS_E_OUT_OF_RANGE", -3), ("CRTS_GUIDES_PLANES", 0), ("CRTS_GUIDES_SURFACE", 1),
                        ("CRTS_STATE_RETRACED", 3), ("CRTS_CHUNK", 2048), ("CRTS_SCAN", 256)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text) and getattr(_lib, name) == value, name
    assert re.search(r"\bCRTS_MAX_ITEMS\s*=\s*1 << 28\b", text) and _lib.CRTS_MAX_ITEMS == 1 << 28 == 16384 * 16384
    assert re.search(r"#define CRTS_NONE 0xFFFFFFFFu\b", text) and _lib.CRTS_NONE == 0xFFFFFFFF and np.uint32(_lib.CRTS_NONE).view(np.int32) == -1
    assert (_lib.CRTS_E_BAD_ARGUMENT, _lib.CRTS_E_OUT_OF_RANGE) == (_lib.CRT_E_BAD_ARGUMENT, _lib.CRT_E_OUT_OF_RANGE)
    assert (_lib.CRTS_GUIDES_PLANES, _lib.CRTS_GUIDES_SURFACE) == (_lib.CRTD_GUIDES_PLANES, _lib.CRTD_GUIDES_SURFACE)
    assert _lib.CRTS_STATE_RETRACED not in (_lib.CRTU_STATE_INTERPOLATED, _lib.CRTU_STATE_NEAREST, _lib.CRTU_STATE_EMPTY)
    assert (ref.NONE, ref.RETRACED, ref.CHUNK, ref.SCAN, ref.MAX_ITEMS) == (_lib.CRTS_NONE, _lib.CRTS_STATE_RETRACED, _lib.CRTS_CHUNK, _lib.CRTS_SCAN,
                                                                            _lib.CRTS_MAX_ITEMS)


def test_struct_sizes_and_offsets_are_the_header_s():
    """The figures the header's comments state, crt_select.hip static_asserts and _lib mirrors (LP64)."""
    header = open(os.path.join(ROOT, "include", "crt_select.h")).read()
    source = open(os.path.join(SELECT_DIR, "crt_select.hip")).read()
    offsets = {_lib.CrtsCompact: (24, dict(words=0, wordBytes=8, values=12, n=16, capacity=20)),
               _lib.CrtsFrame: (112, dict(width=0, height=4, guides=8, geometry=16, camera=24)),
               _lib.CrtsItems: (24, dict(list=0, count=8, factor=12, offsetX=16, offsetY=20)),
               _lib.CrtsScatter: (48, dict(list=0, values=8, out=16, outState=24, count=32, channels=36, n=40, stateWord=44))}
    for struct, (size, fields) in offsets.items():
        assert C.sizeof(struct) == size, struct
        m = re.search(r"/\* %d bytes([^\n]*)\*/\ntypedef struct \{(?:(?!typedef).)*?\} %s;" % (size, struct.__name__), header, re.S)
        assert m, struct
        stated = {n: int(o) for n, o in re.findall(r"\b(\w+) (\d+)\b", m.group(1).split(":", 1)[1])}
        assert stated == fields, (struct, stated)                           # the comment names every field with its offset
        assert "sizeof(%s) == %d" % (struct.__name__, size) in source, struct
        assert [n for n, _ in struct._fields_] == list(fields), struct
        for name, off in fields.items():
            assert getattr(struct, name).offset == off, (struct, name)
            if off:
                assert "offsetof(%s, %s) == %d" % (struct.__name__, name, off) in source, (struct, name)
    assert _lib.CrtsFrame.camera.size == C.sizeof(_lib.CrttCamera) == 84


def test_scratch_bytes_is_positive_and_monotone():
    lib = _lib.select()
    ns = sorted({1, 2, 255, 256, 257, ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1, 3 * ref.CHUNK + 17, ref.CHUNK * ref.SCAN, ref.CHUNK * ref.SCAN + 1,
                 1920 * 1080, ref.MAX_ITEMS - 1, ref.MAX_ITEMS})
    sizes = [lib.crts_scratch_bytes(n) for n in ns]
    assert all(s > 0 and s % 4 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    # a word per chunk sum and one for the total
    assert all(s >= 4 * (-(-n // ref.CHUNK) + 1) for n, s in zip(ns, sizes))
    assert [lib.crts_scratch_bytes(n) for n in (0, -1, ref.MAX_ITEMS + 1, -2 ** 31)] == [0, 0, 0, 0]


def test_error_strings():
    lib = _lib.select()
    assert lib.crts_error_string(0) == b"ok"
    assert lib.crts_error_string(-2) == b"crts: bad argument" and b"range" in lib.crts_error_string(-3) and b"2^28" in lib.crts_error_string(-3)
    assert b"unknown" in lib.crts_error_string(-77)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
WORDS, LIST, COUNTS, SCRATCH, GEOMETRY, POSITIONS, NORMALS, DIRS, VALUES, OUT, STATE = (i * A for i in range(1, 12))


def compact(c=None, list=LIST, counts=COUNTS, scratch=SCRATCH, null=False):
    f = dict(words=WORDS, wordBytes=4, values=6, n=70 * 37, capacity=300)
    f.update(c or {})
    s = _lib.CrtsCompact(**f)
    return _lib.select().crts_compact(None if null else C.byref(s), list, counts, scratch, None)


def points(frame=None, items=None, positions=POSITIONS, normals=NORMALS, dirs=DIRS, null_frame=False, null_items=False):
    f = dict(width=70, height=37, guides=_lib.CRTS_GUIDES_PLANES, geometry=GEOMETRY)
    i = dict(list=LIST, count=300, factor=1, offsetX=0, offsetY=0)
    f.update(frame or {}); i.update(items or {})
    fs, its = _lib.CrtsFrame(**f), _lib.CrtsItems(**i)
    return _lib.select().crts_points(None if null_frame else C.byref(fs), None if null_items else C.byref(its), positions, normals, dirs, None)


def scatter(s=None, null=False):
    f = dict(list=LIST, values=VALUES, out=OUT, outState=STATE, count=300, channels=1, n=70 * 37, stateWord=3)
    f.update(s or {})
    st = _lib.CrtsScatter(**f)
    return _lib.select().crts_scatter(None if null else C.byref(st), None)


def grid(factor, ox=0, oy=0, count=None, w=70, h=37):
    lw, lh = upsample_ref.low_size(w, h, factor, (ox, oy)) if factor in (1, 2, 4) else (1, 1)
    return dict(list=None, factor=factor, offsetX=ox, offsetY=oy, count=lw * lh if count is None else count)


COMPACT_BUFFERS = (("words", WORDS), ("list", LIST), ("counts", COUNTS), ("scratch", SCRATCH))
REFUSALS = {
    # crts_compact
    "compact: null struct": (compact, dict(null=True), BAD),
    "compact: null words": (compact, dict(c=dict(words=None)), BAD),
    "compact: null list": (compact, dict(list=None), BAD),
    "compact: null counts": (compact, dict(counts=None), BAD),
    "compact: null scratch": (compact, dict(scratch=None), BAD),
    **{f"compact: wordBytes {b}": (compact, dict(c=dict(wordBytes=b)), BAD) for b in (0, 2, 3, 8, -1)},
    "compact: n 0": (compact, dict(c=dict(n=0)), BAD),
    "compact: negative n": (compact, dict(c=dict(n=-5)), BAD),
    "compact: capacity 0": (compact, dict(c=dict(capacity=0)), BAD),
    "compact: negative capacity": (compact, dict(c=dict(capacity=-1)), BAD),
    **{f"compact: {a} is {b}": (compact, dict(c=dict(words=addr)) if a == "words" else {a: addr}, BAD)
       for i, (a, _) in enumerate(COMPACT_BUFFERS) for b, addr in COMPACT_BUFFERS[:i] + COMPACT_BUFFERS[i + 1:]},
    "compact: n 2^28 + 1": (compact, dict(c=dict(n=2 ** 28 + 1)), RANGE),
    "compact: capacity 2^28 + 1": (compact, dict(c=dict(capacity=2 ** 28 + 1)), RANGE),
    "compact: n 2^31 - 1": (compact, dict(c=dict(n=2 ** 31 - 1)), RANGE),
    # crts_points
    "points: null frame": (points, dict(null_frame=True), BAD),
    "points: null items": (points, dict(null_items=True), BAD),
    "points: null geometry": (points, dict(frame=dict(geometry=None)), BAD),
    "points: null positions": (points, dict(positions=None), BAD),
    "points: null normals": (points, dict(normals=None), BAD),
    "points: unknown guides": (points, dict(frame=dict(guides=2)), BAD),
    "points: negative guides": (points, dict(frame=dict(guides=-1)), BAD),
    "points: width 0": (points, dict(frame=dict(width=0)), BAD),
    "points: height 0": (points, dict(frame=dict(height=0)), BAD),
    "points: negative width": (points, dict(frame=dict(width=-5)), BAD),
    "points: width 16385": (points, dict(frame=dict(width=16385)), RANGE),
    "points: height 16385": (points, dict(frame=dict(height=16385)), RANGE),
    "points: count 0": (points, dict(items=dict(count=0)), BAD),
    "points: negative count": (points, dict(items=dict(count=-1)), BAD),
    "points: count 2^28 + 1": (points, dict(items=dict(count=2 ** 28 + 1)), RANGE),
    "points: grid, count 0": (points, dict(items=grid(2, count=0)), BAD),
    **{f"points: grid, factor {f}": (points, dict(items=grid(f)), BAD) for f in (0, 3, 8, -2)},
    "points: grid, offsetX = factor": (points, dict(items=grid(2, ox=2, count=35 * 19)), BAD),
    "points: grid, offsetY = factor": (points, dict(items=grid(4, oy=4, count=18 * 10)), BAD),
    "points: grid, offset 1 at factor 1": (points, dict(items=grid(1, ox=1, count=70 * 37)), BAD),
    "points: grid, negative offsetX": (points, dict(items=grid(2, ox=-1, count=35 * 19)), BAD),
    "points: grid, negative offsetY": (points, dict(items=grid(2, oy=-1, count=35 * 19)), BAD),
    "points: grid, offsetX not below the width": (points, dict(frame=dict(width=1), items=dict(list=None, factor=2, offsetX=1, count=19)), BAD),
    "points: grid, offsetY not below the height": (points, dict(frame=dict(height=3), items=dict(list=None, factor=4, offsetY=3, count=18)), BAD),
    "points: grid, a count that is not the grid's": (points, dict(items=grid(2, count=35 * 19 - 1)), BAD),
    "points: grid, the full frame's count at factor 2": (points, dict(items=grid(2, count=70 * 37)), BAD),
    **{f"points: {o} is {b}": (points, {o: addr}, BAD) for o in ("positions", "normals", "dirs") for b, addr in (("the list", LIST), ("the geometry", GEOMETRY))},
    "points: normals is positions": (points, dict(normals=POSITIONS), BAD),
    "points: dirs is positions": (points, dict(dirs=POSITIONS), BAD),
    "points: dirs is normals": (points, dict(dirs=NORMALS), BAD),
    "points: grid, positions is the geometry": (points, dict(items=grid(2), positions=GEOMETRY), BAD),
    # crts_scatter
    "scatter: null struct": (scatter, dict(null=True), BAD),
    "scatter: null list": (scatter, dict(s=dict(list=None)), BAD),
    "scatter: null values": (scatter, dict(s=dict(values=None)), BAD),
    "scatter: null out": (scatter, dict(s=dict(out=None)), BAD),
    **{f"scatter: channels {c}": (scatter, dict(s=dict(channels=c)), BAD) for c in (0, 2, 3, 8)},
    "scatter: count 0": (scatter, dict(s=dict(count=0)), BAD),
    "scatter: negative count": (scatter, dict(s=dict(count=-3)), BAD),
    "scatter: n 0": (scatter, dict(s=dict(n=0)), BAD),
    "scatter: count 2^28 + 1": (scatter, dict(s=dict(count=2 ** 28 + 1)), RANGE),
    "scatter: n 2^28 + 1": (scatter, dict(s=dict(n=2 ** 28 + 1)), RANGE),
    "scatter: out is the list": (scatter, dict(s=dict(out=LIST)), BAD),
    "scatter: out is the values": (scatter, dict(s=dict(out=VALUES)), BAD),
    "scatter: outState is the list": (scatter, dict(s=dict(outState=LIST)), BAD),
    "scatter: outState is the values": (scatter, dict(s=dict(outState=VALUES)), BAD),
    "scatter: outState is out": (scatter, dict(s=dict(outState=OUT)), BAD),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_come_before_anything_is_enqueued(case):
    """Every pointer is a dummy address: a refusal that dereferenced one would fault, and one that enqueued would need a device."""
    fn, kwargs, want = REFUSALS[case]
    assert fn(**kwargs) == want, case


# ---- the reference itself -------------------------------------------------------------------------------------------------------------------
def test_the_list_is_strictly_ascending_up_to_the_count_and_none_behind_it():
    rng = np.random.RandomState(5)
    for n in (1, 2, 65, 257, ref.CHUNK + 1, 3 * ref.CHUNK + 17):
        for words, values in ((rng.randint(0, 4, n).astype(np.uint32), 6), ((rng.uniform(size=n) < 0.5).astype(np.uint8), 2),
                              (np.zeros(n, np.uint8), 2), (np.ones(n, bool), 2), (rng.randint(0, 40, n).astype(np.uint32), 0xFFFFFFFF)):
            sel = ref.selected(words, values)
            total = int(sel.sum())
            for capacity in sorted({1, max(1, total - 1), max(1, total), total + 5, n}):
                lst, counts = ref.compact(words, values, capacity)
                kept = int(counts[1])
                assert lst.dtype == np.uint32 and lst.shape == (capacity,) and tuple(counts) == (total, min(total, capacity))
                assert (np.diff(lst[:kept].astype(np.int64)) > 0).all() and (lst[kept:] == ref.NONE).all()
                assert sel[lst[:kept]].all() and (kept == total or lst[kept - 1] < np.flatnonzero(sel)[kept])      # the FIRST `capacity` of them
    # a word of 32 or more is never selected, whatever values holds
    assert not ref.selected(np.array([32, 33, 255, 2 ** 31], np.uint32), 0xFFFFFFFF).any() and ref.selected(np.array([0, 31], np.uint32), 0x80000001).all()


def test_compact_of_what_scatter_marked_returns_the_list():
    rng = np.random.RandomState(6)
    n = 5000
    state = rng.randint(0, 3, n).astype(np.uint32)
    lst, counts = ref.compact(state, 6, 4000)
    out, values = np.zeros(n, np.float32), rng.uniform(size=4000).astype(np.float32)
    before = state.copy()
    ref.scatter(lst, values, out, state)
    again, counts2 = ref.compact(state, 1 << ref.RETRACED, 4000)
    assert np.array_equal(again, lst) and np.array_equal(counts, counts2) and 0 < counts[0] < 4000
    kept = lst[:counts[1]]
    assert np.array_equal(out[kept], values[:counts[1]]) and (np.delete(out, kept) == 0).all()
    assert np.array_equal(np.delete(state, kept), np.delete(before, kept))
    assert not ref.selected(state, 6).any()                                 # nothing is left to re-trace


def wall(W, H, z=5.0, fov=1.0):
    """a wall at z facing a pinhole camera at the origin: every pixel a hit at t = z / d.z along its unit ray, normal (0, 0, -1)"""
    cam = ref.pinhole(W, H, fov=fov)
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.stack([xx, yy, np.ones_like(xx)], axis=-1).astype(np.float64) @ cam["toRay"].astype(np.float64).T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    g = np.zeros((H, W, 4), np.float32)
    g[..., 2] = -1.0
    g[..., 3] = (z / d[..., 2]).astype(np.float32)
    return cam, g, d


def test_points_of_an_entry_that_names_no_pixel_are_zeros_and_a_pixel_that_is_no_hit_has_a_zero_normal():
    W, H = 33, 9
    cam, g, d64 = wall(W, H)
    g[2, 3, 3] = 99999.0
    g[4, 5, 3] = np.nan
    g[6, 7, 3] = 99998.5
    lst = np.array([0, 2 * W + 3, ref.NONE, W * H, 4 * W + 5, 2 ** 31, W * H - 1, 6 * W + 7, 2 ** 31 + 5], np.uint32)
    p, n, d = ref.points(lst, g, cam)
    for j in (2, 3, 5, 8):
        assert (bits(p[j]) == 0).all() and (bits(n[j]) == 0).all() and (bits(d[j]) == 0).all()
    for j, t in ((1, 99999.0), (4, np.nan), (7, 99998.5)):
        assert (bits(n[j]) == 0).all() and (bits(p[j, :3]) == 0).all() and bits(p[j, 3]) == bits(np.float32(t))
        assert abs(float(np.linalg.norm(d[j, :3].astype(np.float64))) - 1.0) < 1e-6 and d[j, 3] == 0     # it keeps its direction
    for j in (0, 6):
        assert p[j, 3] == g.reshape(-1, 4)[lst[j], 3] and (n[j] == (0, 0, -1, 0)).all()
    # a normal that looks away from the viewer is turned, sign bit by sign bit
    g[..., :3] = (0.0, 0.25, 1.0)
    _, n, _ = ref.points(lst[[0, 6]], g, cam)
    assert np.array_equal(bits(n), bits(np.array([[-0.0, -0.25, -1.0, 0.0]] * 2, np.float32)))


def test_on_a_wall_facing_the_camera_the_points_lie_on_the_wall():
    """P.z = d.z * t with t = z / d.z rounded once: the unit direction carries the roundings of three dot3s, a square root and a division (each
    half an ulp of operands of similar size: below 4 ulp in all), t and the product one each: 8 ulp of z bounds it with room. x and y likewise
    against the double-precision point."""
    W, H, z = 70, 37, 5.0
    cam, g, d64 = wall(W, H, z)
    p, n, d = ref.points(ref.grid_list(W, H, 1), g, cam)
    ulp = z * 2.0 ** -23
    assert np.abs(p[:, 2].astype(np.float64) - z).max() <= 8 * ulp
    exact = d64.reshape(-1, 3) * (z / d64.reshape(-1, 3)[:, 2:3])
    assert np.abs(p[:, :3].astype(np.float64) - exact).max() <= 8 * ulp
    assert np.array_equal(p[:, 3], g.reshape(-1, 4)[:, 3]) and (n == (0, 0, -1, 0)).all()
    # the grid form's items are the pixels the low samples sit on, row-major
    for factor, offset in ((2, (0, 0)), (2, (1, 1)), (4, (3, 0)), (4, (2, 3)), (1, (0, 0))):
        ys, xs = upsample_ref.sample_pixels(W, H, factor, offset)
        want = (ys[:, None] * W + xs[None, :]).reshape(-1)
        assert np.array_equal(ref.grid_list(W, H, factor, offset), want)


# ---- what the GPU session test re-traces, counted here on the oracle's planes --------------------------------------------------------------
def test_on_tiny_the_selection_is_not_empty_and_fits_a_capacity_of_256_but_not_32(nthreads):
    """tests/test_gpu_select.py re-traces the NEAREST and EMPTY pixels of an upsample on `tiny` at 160 x 96, factor 2, default stops, with
    capacities 256 and 32: under the oracle's G-buffer there are such pixels, 256 entries hold them and 32 do not."""
    w, h = 160, 96
    sc = scenes.get("tiny")
    with driver.Session(w, h, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        iv, ip, pos = s.camera()
    orc = oracle_lib.Oracle(a, nthreads=nthreads)
    p = gbuffer_ref.reference_planes(a, orc, orc.raygen(w, h, iv, ip), pos)
    geometry = np.concatenate([p["geometry"]["normal"], p["geometry"]["t"][..., None]], axis=-1).astype(np.float32)
    inst = p["ids"]["instance"].astype(np.int32)
    for offset in ((0, 0), (1, 1)):
        lw, lh = upsample_ref.low_size(w, h, 2, offset)
        _, state = upsample_ref.upsample(np.ones((lh, lw), np.float32), geometry, inst, p["albedo"], 2, offset, 0, **upsample_ref.DEFAULTS)
        values = 1 << upsample_ref.NEAREST | 1 << upsample_ref.EMPTY
        lst, counts = ref.compact(state, values, 256)
        total = int(counts[0])
        print(f"tiny {w}x{h}, factor 2, offset {offset}: {total} of {w * h} pixels are selected")
        assert 1 <= total <= 256 and counts[1] == total and (lst[total:] == ref.NONE).all()
        short, counts = ref.compact(state, values, 32)
        assert counts[0] == total > 32 == counts[1] and np.array_equal(short, lst[:32])


# ---- the unit as the compiler sees it -------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_kernels_need_no_scratch_no_spill_and_no_agprs():
    rows = kernel_resource_rows(source=os.path.join(SELECT_DIR, "crt_select.hip"))
    for n, r in rows:
        print(resource_line(n, r))
    waves, rounds = 256 // 64, ref.CHUNK // 256
    # LDS: a workgroup's wave sums (count, scan), a chunk's (round, wave) sums (write); the gather and the scatter stage nothing
    want = {"crts_scan_kernel": 4 * waves,
            **{f"crts_count_kernel<{w}>": 4 * waves for w in (1, 4)},
            **{f"crts_write_kernel<{w}>": 4 * waves * rounds for w in (1, 4)},
            **{f"crts_points_kernel<{s}, {g}>": 0 for s in ("false", "true") for g in ("false", "true")},
            **{f"crts_scatter_kernel<{c}>": 0 for c in (1, 4)}}
    assert sorted(n for n, _ in rows) == sorted(want)
    for n, r in rows:
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r.get("SGPRs Spill", 0) == 0 and r["AGPRs"] == 0, resource_line(n, r)
        assert r["LDS Size"] == want[n], resource_line(n, r)
        assert r["Occupancy"] >= 8, resource_line(n, r)


def test_the_library_owns_no_hip_object_and_follows_the_recipe():
    sources = sorted(f for f in os.listdir(SELECT_DIR) if f.endswith((".h", ".hip", ".cpp", ".hpp")))
    assert sources == ["crt_select.hip"]
    scanned = unit_sources("clraytracer_amd/select/crt_select.hip")
    assert set(scanned) == {os.path.join(SELECT_DIR, "crt_select.hip"), os.path.join(ROOT, "include", "crt_select.h"), os.path.join(ROOT, "include", "crt_temporal.h"),
                            os.path.join(IMAGE_DIR, "crt_image_device.h"), os.path.join(IMAGE_DIR, "crt_image_host.h")}
    launches = 0
    for path in scanned:
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        assert not re.findall(HIP_OWNING_CALLS, text), path
        assert not re.findall(r"\bhip(DeviceSynchronize|StreamSynchronize|EventSynchronize|Memcpy\w*|Memset\w*|Malloc\w*|Free\w*)\s*\(", text), path
        # no atomic, and no loop that waits for memory: the scan's only loop runs over the chunk sums
        assert not re.findall(r"\batomic\w*|__hip_atomic\w*|__atomic\w*|\bwhile\s*\(|\bvolatile\b|__threadfence\w*", text), path
        launches += len(re.findall(r"<<<", text))
    assert launches == 11                   # count and write per word size and the one scan; the gather per layout and form; the scatter per channel count
    if shutil.which("make"):
        p = subprocess.run(["make", "-n", "-W", "clraytracer_amd/select/crt_select.hip", _lib.SELECT_SO.replace(ROOT + os.sep, "")], cwd=ROOT,
                           stdout=subprocess.PIPE, text=True, check=True)
        makefile = open(os.path.join(ROOT, "Makefile")).read()
        flags = re.search(r"^HIPFLAGS = (.*)$", makefile, re.M).group(1).replace("$(ARCH)", "gfx950").split()
        lines = [l.split() for l in p.stdout.splitlines() if "-shared" in l.split()]
        assert len(lines) == 1 and lines[0][1:] == flags + ["-shared", "-o", "clraytracer_amd/select/libcrt_select.so", "clraytracer_amd/select/crt_select.hip"]
        assert re.search(r"^all:.*\$\(SELECT_SO\)", makefile, re.M) and re.search(r"rm -f .*\$\(SELECT_SO\)", makefile)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.select()" in entry
