"""libcrt_temporal.so without a GPU: the header, the ctypes table and the exports agree; the struct layouts match; every refusal of
include/crt_temporal.h is answered before anything is dereferenced or enqueued; crtt_camera takes RayGen's directions back to their pixels; the
numpy restatement (tests/temporal_ref.py) has the properties the stage exists for; the kernels cross-compile for gfx950 without scratch, spills
or AGPRs; the library's source owns no HIP object, waits on nothing and copies nothing."""
import ctypes as C
import functools
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

if not os.path.exists(getattr(_lib, "TEMPORAL_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import gbuffer_ref
import oracle_lib
import temporal_ref as ref
from test_abi import HIP_OWNING_CALLS
from util import bits, kernel_resource_rows, resource_line, unit_sources

TEMPORAL_DIR = os.path.join(ROOT, "clraytracer_amd", "temporal")
IMAGE_DIR = os.path.join(ROOT, "clraytracer_amd", "image")          # the headers the image libraries share, compiled into each
A = 0x10000                                      # dummy device addresses, 64 KiB apart: a refusal looks at none of them
NAMES = ["crtt_accumulate", "crtt_camera", "crtt_error_string", "crtt_history_bytes"]


def test_header_table_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "crt_temporal.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(crtt_\w+)\s*\(", text)))
    assert names == NAMES
    assert sorted(_lib.TEMPORAL_API) == names
    lib = _lib.temporal()
    for n in names:
        assert hasattr(lib, n), n
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.TEMPORAL_SO], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(crtt_\w+)$", out, re.M))) == names
        assert not re.findall(r"\bcrtd?_\w+$", out, re.M)         # no crt_ or crtd_ name: those belong to the other libraries
    for name, value in (("CRTT_OK", 0), ("CRTT_E_BAD_ARGUMENT", -2), ("CRTT_E_OUT_OF_RANGE", -3), ("CRTT_GUIDES_PLANES", 0), ("CRTT_GUIDES_SURFACE", 1),
                        ("CRTT_MATCH_INSTANCE", 1), ("CRTT_CLAMP", 2), ("CRTT_PLANE_COLOR", 0), ("CRTT_PLANE_MOMENTS", 1), ("CRTT_PLANE_GEOMETRY", 2),
                        ("CRTT_PLANE_INSTANCE", 3)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text) and getattr(_lib, name) == value, name
    assert (_lib.CRTT_E_BAD_ARGUMENT, _lib.CRTT_E_OUT_OF_RANGE) == (_lib.CRT_E_BAD_ARGUMENT, _lib.CRT_E_OUT_OF_RANGE)
    assert (_lib.CRTT_GUIDES_PLANES, _lib.CRTT_GUIDES_SURFACE) == (_lib.CRTD_GUIDES_PLANES, _lib.CRTD_GUIDES_SURFACE)
    assert (ref.MATCH_INSTANCE, ref.CLAMP) == (_lib.CRTT_MATCH_INSTANCE, _lib.CRTT_CLAMP)


def test_struct_sizes_offsets_and_history_bytes():
    """The figures the header states and crt_temporal.hip static_asserts. LP64: the int32 `guides` sits at 16 with 4 bytes of padding behind it,
    in front of the pointers; the 84-byte cameras leave 4 bytes of tail padding in the structs that hold pointers."""
    header = open(os.path.join(ROOT, "include", "crt_temporal.h")).read()
    source = open(os.path.join(TEMPORAL_DIR, "crt_temporal.hip")).read()
    for struct, size in ((_lib.CrttCamera, 84), (_lib.CrttFrame, 128), (_lib.CrttHistory, 120), (_lib.CrttParams, 24)):
        assert C.sizeof(struct) == size, struct
        assert re.search(r"/\* %d bytes[^\n]*\*/\ntypedef struct \{(?:(?!typedef).)*?\} %s;" % (size, struct.__name__), header, re.S), struct
        assert "sizeof(%s) == %d" % (struct.__name__, size) in source, struct
    offsets = {_lib.CrttCamera: dict(pos=0, toRay=12, toScreen=48),
               _lib.CrttFrame: dict(width=0, height=4, color=8, guides=16, geometry=24, ids=32, camera=40),
               _lib.CrttHistory: dict(color=0, moments=8, geometry=16, instance=24, camera=32),
               _lib.CrttParams: dict(flags=0, alpha=4, momentsAlpha=8, maxHistory=12, depthTol=16, normalCos=20)}
    for struct, fields in offsets.items():
        assert [n for n, _ in struct._fields_] == list(fields), struct
        for name, off in fields.items():
            assert getattr(struct, name).offset == off, (struct, name)
            if off and name not in ("height", "alpha", "momentsAlpha", "maxHistory", "depthTol"):
                assert "offsetof(%s, %s) == %d" % (struct.__name__, name, off) in source, (struct, name)
    lib = _lib.temporal()
    for plane, per_pixel in ((_lib.CRTT_PLANE_COLOR, 16), (_lib.CRTT_PLANE_MOMENTS, 16), (_lib.CRTT_PLANE_GEOMETRY, 16), (_lib.CRTT_PLANE_INSTANCE, 4)):
        assert lib.crtt_history_bytes(70, 37, plane) == 70 * 37 * per_pixel
        assert lib.crtt_history_bytes(1, 1, plane) == per_pixel
        assert lib.crtt_history_bytes(16384, 16384, plane) == 16384 * 16384 * per_pixel        # 2^32 and beyond
        assert lib.crtt_history_bytes(0, 37, plane) == 0 and lib.crtt_history_bytes(70, -1, plane) == 0
    assert lib.crtt_history_bytes(70, 37, 4) == 0 and lib.crtt_history_bytes(70, 37, -1) == 0
    assert lib.crtt_history_bytes(16384, 16384, _lib.CRTT_PLANE_COLOR) == 2 ** 32
    assert b"argument" in lib.crtt_error_string(-2) and b"range" in lib.crtt_error_string(-3) and lib.crtt_error_string(0) == b"ok"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def call(frame=None, prev=None, nxt=None, params=None, null_frame=False, null_prev=False, null_next=False, null_params=False):
    f = dict(width=70, height=37, color=1 * A, guides=_lib.CRTT_GUIDES_PLANES, geometry=2 * A, ids=3 * A)
    h0 = dict(color=4 * A, moments=5 * A, geometry=6 * A, instance=7 * A)
    h1 = dict(color=8 * A, moments=9 * A, geometry=10 * A, instance=11 * A)
    p = dict(flags=_lib.CRTT_MATCH_INSTANCE | _lib.CRTT_CLAMP, alpha=0.2, momentsAlpha=0.2, maxHistory=32.0, depthTol=0.05, normalCos=0.9)
    f.update(frame or {}); h0.update(prev or {}); h1.update(nxt or {}); p.update(params or {})
    fs, h0s, h1s, ps = _lib.CrttFrame(**f), _lib.CrttHistory(**h0), _lib.CrttHistory(**h1), _lib.CrttParams(**p)
    return _lib.temporal().crtt_accumulate(None if null_frame else C.byref(fs), None if null_prev else C.byref(h0s), None if null_next else C.byref(h1s),
                                           None if null_params else C.byref(ps), None)


BAD, RANGE = _lib.CRTT_E_BAD_ARGUMENT, _lib.CRTT_E_OUT_OF_RANGE
SURFACE = dict(guides=_lib.CRTT_GUIDES_SURFACE, ids=None)
NO_MATCH = dict(flags=_lib.CRTT_CLAMP)
REFUSALS = {
    "null frame": (dict(null_frame=True), BAD),
    "null next": (dict(null_next=True), BAD),
    "null params": (dict(null_params=True), BAD),
    "null params on a reset": (dict(null_params=True, null_prev=True), BAD),
    "null colour": (dict(frame=dict(color=None)), BAD),
    "null geometry": (dict(frame=dict(geometry=None)), BAD),
    "null next colour": (dict(nxt=dict(color=None)), BAD),
    "null next moments": (dict(nxt=dict(moments=None)), BAD),
    "null next geometry": (dict(nxt=dict(geometry=None)), BAD),
    "null prev colour": (dict(prev=dict(color=None)), BAD),
    "null prev moments": (dict(prev=dict(moments=None)), BAD),
    "null prev geometry": (dict(prev=dict(geometry=None)), BAD),
    "no ids under MATCH_INSTANCE": (dict(frame=dict(ids=None), nxt=dict(instance=None)), BAD),
    "no ids for next's instance plane": (dict(frame=dict(ids=None), params=NO_MATCH), BAD),
    "no next instance under MATCH_INSTANCE": (dict(nxt=dict(instance=None)), BAD),
    "no prev instance under MATCH_INSTANCE": (dict(prev=dict(instance=None)), BAD),
    "no next instance under MATCH_INSTANCE on a reset": (dict(nxt=dict(instance=None), null_prev=True), BAD),
    "ids under SURFACE": (dict(frame=dict(SURFACE, ids=3 * A)), BAD),
    **{f"next {a} is {b}": (dict(nxt={a: addr}), BAD) for a in ("color", "moments", "geometry", "instance")
       for b, addr in (("cur's colour", 1 * A), ("cur's geometry", 2 * A), ("cur's ids", 3 * A), ("prev's colour", 4 * A), ("prev's moments", 5 * A),
                       ("prev's geometry", 6 * A), ("prev's instance", 7 * A))},
    "next colour is next moments": (dict(nxt=dict(moments=8 * A)), BAD),
    "next geometry is next colour": (dict(nxt=dict(geometry=8 * A)), BAD),
    "next instance is next geometry": (dict(nxt=dict(instance=10 * A)), BAD),
    "next colour is cur's colour on a reset": (dict(nxt=dict(color=1 * A), null_prev=True), BAD),
    "next geometry is the records under SURFACE": (dict(frame=SURFACE, nxt=dict(geometry=2 * A)), BAD),
    "unknown flag": (dict(params=dict(flags=4)), BAD),
    "unknown high flag": (dict(params=dict(flags=0x80000001)), BAD),
    "unknown guides": (dict(frame=dict(guides=2)), BAD),
    "negative guides": (dict(frame=dict(guides=-1)), BAD),
    "alpha 0": (dict(params=dict(alpha=0.0)), BAD),
    "alpha above 1": (dict(params=dict(alpha=1.5)), BAD),
    "negative alpha": (dict(params=dict(alpha=-0.2)), BAD),
    "NaN alpha": (dict(params=dict(alpha=float("nan"))), BAD),
    "momentsAlpha 0": (dict(params=dict(momentsAlpha=0.0)), BAD),
    "momentsAlpha above 1": (dict(params=dict(momentsAlpha=1.0000001)), BAD),
    "NaN momentsAlpha": (dict(params=dict(momentsAlpha=float("nan"))), BAD),
    "maxHistory below 1": (dict(params=dict(maxHistory=0.5)), BAD),
    "NaN maxHistory": (dict(params=dict(maxHistory=float("nan"))), BAD),
    "infinite maxHistory": (dict(params=dict(maxHistory=float("inf"))), BAD),
    "negative depthTol": (dict(params=dict(depthTol=-0.01)), BAD),
    "NaN depthTol": (dict(params=dict(depthTol=float("nan"))), BAD),
    "NaN normalCos": (dict(params=dict(normalCos=float("nan"))), BAD),
    "infinite normalCos": (dict(params=dict(normalCos=float("inf"))), BAD),
    "-infinite normalCos": (dict(params=dict(normalCos=float("-inf"))), BAD),
    "width 0": (dict(frame=dict(width=0)), BAD),
    "height 0": (dict(frame=dict(height=0)), BAD),
    "negative width": (dict(frame=dict(width=-5)), BAD),
    "width 16385": (dict(frame=dict(width=16385)), RANGE),
    "height 16385": (dict(frame=dict(height=16385)), RANGE),
    "width 2^31 - 1 on a reset": (dict(frame=dict(width=2 ** 31 - 1), null_prev=True), RANGE),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_come_before_anything_is_enqueued(case):
    """Every pointer is a dummy address: a refusal that dereferenced one would fault, and one that enqueued would need a device."""
    kwargs, want = REFUSALS[case]
    assert call(**kwargs) == want, case


# ---- crtt_camera ----------------------------------------------------------------------------------------------------------------------------
CAM_W, CAM_H = 1920, 1080
# The largest distance in pixels, at 1920 x 1080, between a pixel's own (i, j) and where the float32 toScreen (evaluated in float64) puts the
# oracle's float32 RayGen direction of that pixel. Measured on the CPU: tiny 2.84e-4, cornell-1k 2.28e-4, tiny with a translated invView 2.49e-4
# (each is printed by its test; all three are of the size of RayGen's own float32 rounding of a direction, 1080 pixels * a few 1e-7).
# The bound is 4 x the largest, for other cameras of the same conditioning.
CAMERA_MEASURED_PX = 2.85e-4
CAMERA_BOUND_PX = 4 * CAMERA_MEASURED_PX


@functools.lru_cache(maxsize=None)
def session_matrices(name):
    with driver.Session(CAM_W, CAM_H, host_only=True) as s:
        s.load_scene(scenes.get(name))
        return tuple(np.array(m) for m in s.camera())


def camera_cases():
    iv, ip, pos = session_matrices("tiny")
    moved = iv.copy()
    moved[12:15] += np.array([3.5, -2.25, 7.0], np.float32)                   # a translated invView: RayGen's directions carry it
    return {"tiny": session_matrices("tiny"), "cornell-1k": session_matrices("cornell-1k"), "translated invView": (moved, ip, pos)}


@pytest.mark.parametrize("case", ["tiny", "cornell-1k", "translated invView"])
def test_camera_takes_raygen_directions_back_to_their_pixels(case, nthreads):
    iv, ip, pos = camera_cases()[case]
    cam = ref.camera_from_struct(_lib.crtt_camera(iv, ip, pos, CAM_W, CAM_H))
    assert np.array_equal(cam["pos"], pos)
    rays = raygen(CAM_W, CAM_H, iv, ip, nthreads)
    u = rays @ cam["toScreen"].astype(np.float64).T
    jj, ii = np.mgrid[0:CAM_H, 0:CAM_W]
    deviation = float(np.maximum(np.abs(u[..., 0] / u[..., 2] - ii), np.abs(u[..., 1] / u[..., 2] - jj)).max())
    identity = float(np.abs(cam["toRay"].astype(np.float64) @ cam["toScreen"].astype(np.float64) - np.eye(3)).max())
    print(f"{case}: largest deviation {deviation:.3e} pixel, |toRay toScreen - 1| {identity:.3e}")
    assert (u[..., 2] > 0).all()                                              # every pixel's own direction is in front of the camera
    assert deviation < 0.01                                                   # the condition: far below what a bilinear fetch can see
    assert deviation <= CAMERA_BOUND_PX
    # toRay . toScreen = 1 to the same order: both are float32 roundings (2^-24 relative per entry) of exact inverses whose entries
    # reach |toRay| |toScreen| ~ 1e3 in pixel units, the deviation's bound expressed per entry
    assert identity <= CAMERA_BOUND_PX
    # and toRay is RayGen's direction up to its length
    d = np.stack([ii, jj, np.ones_like(ii)], axis=-1).astype(np.float64) @ cam["toRay"].astype(np.float64).T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    assert np.abs(d - rays).max() < 1e-5


def raygen(w, h, iv, ip, nthreads):
    """the oracle's RayGen directions (float32) as float64; it needs a scene only for its handle"""
    with driver.Session(64, 48, host_only=True) as s:
        s.load_scene(scenes.get("tiny"))
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
    return oracle_lib.Oracle(a, nthreads=nthreads).raygen(w, h, iv, ip).astype(np.float64)


def test_camera_refusals():
    iv, ip, pos = session_matrices("tiny")
    lib = _lib.temporal()
    out = _lib.CrttCamera()
    out.pos[0] = 123.0

    def rc(iv=iv, ip=ip, pos=pos, w=CAM_W, h=CAM_H, out=out):
        ptr = lambda a: None if a is None else _lib.fptr(a)[0]
        keep = [np.ascontiguousarray(a, np.float32) for a in (iv, ip, pos) if a is not None]      # noqa: F841
        return lib.crtt_camera(ptr(iv), ptr(ip), ptr(pos), w, h, None if out is None else C.byref(out))

    assert rc() == 0 and out.pos[0] == pos[0]
    out.pos[0] = 123.0

    def edited(m, i, v):
        m = m.copy(); m[i] = v
        return m

    zero_w = edited(edited(ip, 11, 0.0), 15, 0.0)                            # w = ip[3] cx + ip[7] cy + ip[11] + ip[15]
    flipping_w = edited(ip, 3, 2.0 * abs(ip[11] + ip[15]))                   # w changes sign between the left and the right border
    singular = edited(edited(edited(ip, 0, 0.0), 1, 0.0), 2, 0.0)            # a column of zeros in invProj: the direction ignores i
    singular[3] = 0.0
    for what, r in {"null invView": rc(iv=None), "null invProj": rc(ip=None), "null pos": rc(pos=None), "null out": rc(out=None),
                    "width 0": rc(w=0), "negative height": rc(h=-1), "NaN in invView": rc(iv=edited(iv, 5, np.nan)),
                    "inf in invProj": rc(ip=edited(ip, 0, np.inf)), "NaN in pos": rc(pos=edited(pos, 2, np.nan)), "w of zero at the centre": rc(ip=zero_w),
                    "w of differing sign at the corners": rc(ip=flipping_w), "a singular toRay": rc(ip=singular)}.items():
        assert r == BAD, what
    assert out.pos[0] == 123.0                                                # a refusal writes nothing


# ---- the reference itself, on hand-made planes ----------------------------------------------------------------------------------------------
H, W = 37, 70


def frames(seed=0, nans=False):
    planes = ref.guides(H, W, seed=seed)
    return planes["geometry"], planes["ids"]["instance"].astype(np.int32), ref.noisy_color(H, W, seed=seed, nans=nans)


def test_constant_colour_under_a_static_camera_stays_and_the_history_grows():
    """The colour is a power of two per channel and alpha is 0.25. Then every product c*b is exact, so the fetch gives c * (sum of b) / (sum
    of b) = c whatever the fractional weights are; and with a = max(0.25, 1/N) >= 0.25, fl(1 - a) + a rounds to 1 (the error of fl(1 - a) is at
    most half an ulp of a, 2^-25, a tie that goes to the even 1.0), so h*(1 - a) + c*a = c. N_h is a weighted mean of equal counts k: each
    of its at most four products, three sums and one quotient rounds once (2^-24 relative), so N is k + 1 to within 8 * 2^-24 relative."""
    g, inst, color = frames()
    color[..., :3] = (0.5, 2.0, 0.125)
    hit = g[..., 3] <= 99998.0
    cam = ref.camera_pairs(W, H)["identical"][0]
    hist = None
    for k in range(1, 8):
        hist = ref.accumulate(color, g, inst, cam, prev=hist, alpha=0.25, max_history=5.0)
        assert np.array_equal(bits(hist["color"]), bits(color)), k
        N = hist["moments"][..., 2]
        want = min(k, 5)
        assert np.abs(N[hit] - want).max() <= want * 8 * 2.0 ** -24 and (np.rint(N[hit]) == want).all(), k
        assert (N[~hit] == 0).all()
        assert np.array_equal(bits(hist["geometry"]), bits(g)) and np.array_equal(hist["instance"], inst)


def test_noise_under_a_static_camera_falls_over_eight_frames():
    g, inst, _ = frames()
    hit = g[..., 3] <= 99998.0
    yy, xx = np.mgrid[0:H, 0:W]
    clean = np.stack([0.5 + 0.3 * np.sin(0.2 * xx + ch) * np.cos(0.15 * yy) for ch in range(3)], axis=-1)
    cam = ref.camera_pairs(W, H)["identical"][0]
    hist, errors = None, []
    for k in range(8):
        noisy = ref.noisy_color(H, W, seed=k, nans=False)                     # the same signal, a fresh seed's noise
        hist = ref.accumulate(noisy, g, inst, cam, prev=hist)
        errors.append(float(np.abs(hist["color"][..., :3] - clean)[hit].mean()))
    print("mean absolute error per frame:", ["%.4f" % e for e in errors])
    assert all(b < a for a, b in zip(errors[:5], errors[1:5]))                # a running mean while 1/N > alpha: every frame helps
    # from then on alpha = 0.2 weighs the frames 0.2 * 0.8^k: a standard deviation of at most sqrt(0.2 / 1.8) = 1/3 of one frame's
    assert errors[7] < 0.5 * errors[0]


def test_a_sideways_camera_drops_the_history_behind_the_depth_edge():
    """guides() has a near surface (t about 10) left of x = W // 2 and a far one (t about 40) right of it. The camera steps to the left: the
    picture moves right, the near surface by more, and the strip of the far surface next to the edge was hidden behind the near one."""
    g, inst, color = frames()
    prev_cam, cam = ref.pinhole(W, H), ref.pinhole(W, H, pos=(-2.0, 0.0, 0.0))
    first = ref.accumulate(color, g, inst, prev_cam)
    second = ref.accumulate(color, g, inst, cam, prev=first, depth_tol=0.2)
    fx, fy, uz, _ = ref.reproject64(cam, prev_cam, g)
    hit = g[..., 3] <= 99998.0
    xx = np.mgrid[0:H, 0:W][1]
    uncovered = hit & (xx >= W // 2) & (fx >= 0) & (fx + 1 < W // 2 - 0.01)     # a far pixel both of whose tap columns show the near surface
    assert uncovered.sum() >= H
    N = second["moments"][..., 2]
    assert (N[uncovered] == 1).all()
    assert np.array_equal(bits(second["color"])[uncovered], bits(color)[uncovered])
    kept = hit & (xx >= W // 2 + 6) & (fx + 1 < W)
    assert (N[kept] > 1).mean() > 0.8                                       # while the far surface away from the edge keeps its history


def test_a_previous_camera_facing_away_leaves_no_history():
    g, inst, color = frames()
    cam = ref.pinhole(W, H)
    away = ref.pinhole(W, H, yaw=np.pi)
    second = ref.accumulate(color, g, inst, cam, prev=ref.accumulate(color, g, inst, away))
    hit = g[..., 3] <= 99998.0
    assert (ref.reproject64(cam, away, g)[2][hit] < 0).all()
    assert (second["moments"][..., 2][hit] == 1).all() and (second["moments"][..., 2][~hit] == 0).all()
    assert np.array_equal(bits(second["color"]), bits(color))


def test_a_nan_in_the_history_heals():
    g, inst, color = frames()
    g = g.copy(); g[...] = (0.0, 1.0, 0.0, 10.0)                            # every pixel a hit on one surface: the NaN is a tap of its neighbours
    cur, prev_cam = ref.camera_pairs(W, H)["sub-pixel pan"]
    first = ref.accumulate(color, g, inst, prev_cam)
    first["color"][20, 30, 1] = np.nan
    first["moments"][9, 50, 0] = np.inf
    second = ref.accumulate(color, g, inst, cur, prev=first)
    fx, fy, _, _ = ref.reproject64(cur, prev_cam, g)
    taps = lambda x, y: (np.floor(fx) <= x) & (np.floor(fx) + 1 >= x) & (np.floor(fy) <= y) & (np.floor(fy) + 1 >= y)
    taps_it = taps(30, 20) | taps(50, 9)
    assert 2 <= taps(30, 20).sum() <= 4 and 2 <= taps(50, 9).sum() <= 4
    assert np.isfinite(second["color"]).all() and np.isfinite(second["moments"]).all()
    assert (second["moments"][..., 2][taps_it] == 2).all()                   # the other taps carry the history on
    # multiplied by zero instead of selected away, the NaN would have reached every pixel it is a tap of
    clean = ref.accumulate(color, g, inst, cur, prev=ref.accumulate(color, g, inst, prev_cam))
    differs = (bits(second["color"]) != bits(clean["color"])).any(axis=-1)
    assert differs.any() and not (differs & ~taps_it).any()


def test_every_flag_and_parameter_changes_some_output():
    g, inst, color = frames()
    cur, prev_cam = ref.camera_pairs(W, H)["translation"]
    first = ref.accumulate(color, g, inst, prev_cam)
    prev = ref.accumulate(ref.noisy_color(H, W, seed=5, nans=False), g, inst, prev_cam, prev=first)
    newer = ref.noisy_color(H, W, seed=6, nans=False)
    key = lambda h: np.concatenate([bits(h["color"]).reshape(-1), bits(h["moments"]).reshape(-1)])
    seen = [key(ref.accumulate(newer, g, inst, cur, prev=prev))]
    for kw in (dict(flags=ref.MATCH_INSTANCE), dict(flags=ref.CLAMP), dict(flags=ref.MATCH_INSTANCE | ref.CLAMP), dict(alpha=0.5), dict(moments_alpha=0.5),
               dict(max_history=2.0), dict(depth_tol=0.01), dict(normal_cos=0.99)):
        out = key(ref.accumulate(newer, g, inst, cur, prev=prev, **kw))
        assert not any(np.array_equal(out, s) for s in seen), kw
        seen.append(out)
    # and a reset ignores all of it
    assert np.array_equal(bits(ref.accumulate(newer, g, inst, cur, flags=3)["color"]), bits(newer))


def test_the_hand_made_camera_pairs_reach_every_border_case():
    """What tests/test_gpu_temporal.py relies on, at its largest shapes: under the four pans fx and fy fall into [-1, 0) and taps leave the
    frame on each side; the previous camera behind the surface has u.z <= 0; the translation rejects by depth."""
    for w, h in ((70, 37), (257, 19)):
        g = ref.guides(h, w, seed=w)["geometry"]
        hit = g[..., 3] <= 99998.0
        pairs = ref.camera_pairs(w, h)
        seen = {k: False for k in ("fx in [-1, 0)", "fy in [-1, 0)", "x0 + 1 = W", "y0 + 1 = H", "fx < -1", "fx >= W", "fy < -1", "fy >= H")}
        for name in ("pan left", "pan right", "pan up", "pan down"):
            fx, fy, uz, _ = ref.reproject64(*pairs[name], g)
            fx, fy = fx[hit], fy[hit]
            for k, m in (("fx in [-1, 0)", (fx >= -1) & (fx < 0)), ("fy in [-1, 0)", (fy >= -1) & (fy < 0)), ("x0 + 1 = W", (fx >= w - 1) & (fx < w)),
                         ("y0 + 1 = H", (fy >= h - 1) & (fy < h)), ("fx < -1", fx < -1), ("fx >= W", fx >= w), ("fy < -1", fy < -1), ("fy >= H", fy >= h)):
                seen[k] |= bool(m.any())
        assert all(seen.values()), seen
        assert (ref.reproject64(*pairs["previous camera behind the surface"], g)[2][hit] <= 0).all()
        fx, fy, uz, _ = ref.reproject64(*pairs["sub-pixel pan"], g)
        assert ((fx - np.floor(fx))[hit] > 0.05).all() and ((fx - np.floor(fx))[hit] < 0.95).all()      # fractional weights on every tap
        hist = ref.history_content(h, w, pairs["translation"][1], seed=w)
        inst = ref.guides(h, w, seed=w)["ids"]["instance"].astype(np.int32)
        N = ref.accumulate(ref.noisy_color(h, w, seed=w), g, inst, pairs["translation"][0], prev=hist)["moments"][..., 2]
        assert (N[hit] == 1).mean() > 0.05 and (N[hit] > 1).mean() > 0.05


# ---- the camera pair of the Session test -------------------------------------------------------------------------------------------------------
def test_the_session_camera_pair_keeps_and_loses_history(nthreads):
    w, h = ref.SESSION_SIZE
    sc = scenes.get("tiny")
    views = []
    with driver.Session(w, h, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        orc = oracle_lib.Oracle(a, nthreads=nthreads)
        for move in (False, True):
            if move:
                s.set_camera(*ref.session_second_camera(sc))
            iv, ip, pos = s.camera()
            planes = gbuffer_ref.reference_planes(a, orc, orc.raygen(w, h, iv, ip), pos)
            g = np.concatenate([planes["geometry"]["normal"], planes["geometry"]["t"][..., None]], axis=-1).astype(np.float32)
            views.append((g, planes["ids"]["instance"].astype(np.int32), ref.camera_from_struct(_lib.crtt_camera(iv, ip, pos, w, h))))
    color = ref.noisy_color(h, w, nans=False)
    first = ref.accumulate(color, *views[0])
    still = ref.accumulate(color, *views[0], prev=first)
    hit0 = views[0][0][..., 3] <= 99998.0
    assert hit0.sum() >= 1000 and (still["moments"][..., 2][hit0] == 2).all()           # an unmoved camera: every hit pixel has N == 2
    hit1 = views[1][0][..., 3] <= 99998.0
    for prev, kw in ((first, {}), (still, ref.SESSION_MOVED_PARAMS)):             # with the defaults, and as the GPU test calls it
        N = ref.accumulate(color, *views[1], prev=prev, **kw)["moments"][..., 2][hit1]
        keep, lose = float((N == 2).mean()), float((N == 1).mean())
        print(f"session pair: {int(hit1.sum())} hit pixels, {keep:.1%} keep their history, {lose:.1%} lose it")
        assert hit1.sum() >= 1000 and keep >= 0.05 and lose >= 0.05 and keep + lose == 1.0


# ---- the unit as the compiler sees it -------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_kernels_need_no_scratch_no_spill_and_no_agprs():
    rows = kernel_resource_rows(source=os.path.join(TEMPORAL_DIR, "crt_temporal.hip"))
    for n, r in rows:
        print(resource_line(n, r))
    # per guide layout: the taps' colour loaded with the geometry or behind its test, the clamp's pixels through L1 or from a 34 x 10 tile in LDS
    tf = ("false", "true")
    # (instantiations over this library's pass of the template it shares with libcrt_motion.so: <PASS, SURFACE, GATED, STAGE>, and nothing else)
    assert sorted(n for n, _ in rows) == sorted(f"crt_accumulate_kernel<CrttPass, {s}, {g}, {l}>" for s in tf for g in tf for l in tf)
    for n, r in rows:
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r.get("SGPRs Spill", 0) == 0 and r["AGPRs"] == 0, resource_line(n, r)
        assert r["LDS Size"] == (34 * 10 * 16 if n.endswith("true>") else 0), resource_line(n, r)     # nothing but the staged tile
        assert r["Occupancy"] >= 4, resource_line(n, r)                          # four workgroups of four waves per CU at least


def test_the_library_owns_no_hip_object_and_follows_the_recipe():
    sources = sorted(f for f in os.listdir(TEMPORAL_DIR) if f.endswith((".h", ".hip", ".cpp", ".hpp")))
    assert sources == ["crt_temporal.hip"]
    # the unit and every in-tree header it includes, transitively: the shared steps of clraytracer_amd/image/ are this library's source too
    scanned = unit_sources("clraytracer_amd/temporal/crt_temporal.hip")
    assert {os.path.join(TEMPORAL_DIR, f) for f in sources} | {os.path.join(ROOT, "include", "crt_temporal.h"), os.path.join(IMAGE_DIR, "crt_image_device.h"),
                                                            os.path.join(IMAGE_DIR, "crt_image_host.h"), os.path.join(IMAGE_DIR, "crt_image_env.h"), os.path.join(IMAGE_DIR, "crt_accumulate.h")} <= set(scanned)
    for path in scanned:
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        assert not re.findall(HIP_OWNING_CALLS, text), path
        assert not re.findall(r"\bhip(DeviceSynchronize|StreamSynchronize|EventSynchronize|Memcpy\w*|Memset\w*)\s*\(", text), path     # nor waits or copies
    assert sum(len(re.findall(r"<<<", open(path).read())) for path in scanned) == 4          # <GATED, STAGE>, all in the unit itself
    assert len(re.findall(r"<<<", open(os.path.join(TEMPORAL_DIR, "crt_temporal.hip")).read())) == 4
    if shutil.which("make"):
        p = subprocess.run(["make", "-n", "-W", "clraytracer_amd/temporal/crt_temporal.hip", _lib.TEMPORAL_SO.replace(ROOT + os.sep, "")], cwd=ROOT,
                           stdout=subprocess.PIPE, text=True, check=True)
        makefile = open(os.path.join(ROOT, "Makefile")).read()
        flags = re.search(r"^HIPFLAGS = (.*)$", makefile, re.M).group(1).replace("$(ARCH)", "gfx950").split()
        lines = [l.split() for l in p.stdout.splitlines() if "-shared" in l.split()]
        assert len(lines) == 1 and lines[0][1:] == flags + ["-shared", "-o", "clraytracer_amd/temporal/libcrt_temporal.so", "clraytracer_amd/temporal/crt_temporal.hip"]
        assert re.search(r"^all:.*\$\(TEMPORAL_SO\)", makefile, re.M) and re.search(r"rm -f .*\$\(TEMPORAL_SO\)", makefile)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.temporal()" in entry
