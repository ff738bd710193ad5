"""The committing form of the camera bounce's root pre-test on the device (crt_device.h: root_pretest_enters, (7g) -- a lane whose first surviving
instance passes the root step stays inside it, and the trip loop starts with that lane at the root's nearer child): the uncounted Trace kernels,
which take it, against the counted kernels, which do not, and against the oracle -- bit for bit, with the kernel that ran checked by name.

The grazing scenes of tests/test_gpu_root_pretest.py with their single-leaf instance moved to the highest index (at index 3 it stands below almost
every instance and keeps the lanes that hold it from committing to anything above: that order is what test_gpu_root_pretest.py itself runs), as
8, 16, 64 and 65 instances (65 with CRT_TLAS=0: two 64-chunks, no pre-test), at 64x64 and 72x40, every flag set of Frames.flag_sets and the
shadowed forms; frames in flight, split tiles and row bands. Not vacuous: the restatement (tests/pretest_entry_ref.py) finds, in every scene of
at most 64 instances, a full tile whose committing lanes stay inside two different instances and a full tile whose lowest committed instance
pushes its far child to stack row 0.

The tie scene (the order hazard): a one-triangle mesh -- a root that is a leaf, which the pre-test never enters -- at instance 1 and, under the
same transform at instance 5, a mesh with an inner root that holds the identical triangle under another material. Both hit at the same t to the
bit; upstream keeps the first, `t < out.t` being strict. A lane that committed to instance 5 over the bit of instance 1 would shade the other
material."""
import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import oracle_lib
import pretest_entry_ref as entry
from test_gpu_camera_cull import ASYNC, Frames, _instances, _one_triangle_mesh, _scene
from test_gpu_root_pretest import grazing_scene, shadowed_forms
from util import bits

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(64, 64), (72, 40)]


def leaf_last(sc):
    """grazing_scene's instances with the single-leaf one (index 3) moved behind the others"""
    insts = list(sc.instances)
    sc.instances = insts[:3] + insts[4:] + [insts[3]]
    return sc


def committing_lanes(s, orc):
    """(inside, pushed, masks) per pixel of the session's frame: the instance the pre-test leaves the lane in (-1: none) and whether it pushed"""
    a = s.arenas()
    iv, ip, pos = s.camera()
    d = np.asarray(orc.raygen(s.width, s.height, iv, ip), F).reshape(-1, 3)
    o = np.asarray(pos, F)
    terms = [entry.instance_terms(a, k) for k in range(len(a["instances"]))]
    masks = entry.lane_masks(a, o, d)
    _, inside, pushed, _ = entry.wave_commits(masks, terms, o, d)
    return inside, pushed, masks


def assert_entry_waves(s, orc):
    """some full tile whose committing lanes have two different first instances, and one whose first survivor pushes"""
    w, h = s.width, s.height
    inside, pushed, _ = committing_lanes(s, orc)
    th, tw = h // 8, w // 8
    tiles = lambda x: x.reshape(h, w)[:th * 8, :tw * 8].reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(th * tw, 64)
    ins, psh = tiles(inside), tiles(pushed)
    two = [t for t in range(th * tw) if len(set(ins[t][ins[t] >= 0])) >= 2]
    first_pushes = [t for t in range(th * tw) if (ins[t] >= 0).any() and psh[t][ins[t] == ins[t][ins[t] >= 0].min()].any()]
    assert two, "no full tile whose committing lanes stay inside two different instances"
    assert first_pushes, "no full tile whose first surviving instance pushes its far child"
    return len(two), len(first_pushes)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n", [8, 16, 64, 65])
def test_committing_lanes_every_flag_set(n, w, h, monkeypatch, nthreads, tmp_path):
    if n > 64:
        monkeypatch.setenv("CRT_TLAS", "0")                                   # read by crt_init: the chunked loop, 64 + 1
    sc = leaf_last(grazing_scene(n, w, h, nthreads, tmp_path))
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        assert len(s.arenas()["instances"]) == n
        f = Frames(s, sc, nthreads)
        if n <= 64:
            assert_entry_waves(s, f.orc)
        f.flag_sets(f"{n} instances, {w}x{h}")
        shadowed_forms(f, f"{n} instances, {w}x{h}")


def test_row_bands_split_tiles_and_frames_in_flight(monkeypatch, nthreads, tmp_path):
    monkeypatch.setenv("CRT_FRAMES_IN_FLIGHT", "3")
    w, h = 72, 40
    sc = leaf_last(grazing_scene(16, w, h, nthreads, tmp_path))
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        f = Frames(s, sc, nthreads)
        ref_frame = f.plain()
        for _ in range(3):                      # later frames run on lists built from the first one's costs: quadrant waves of split tiles
            assert np.array_equal(bits(f.render(0, "crt_trace_kernel<0,0,0,0,0>")), bits(ref_frame))
        s.set_row_bands(16, 1, 2)
        part = f.render(0, "crt_trace_kernel<0,0,0,0,0>")
        own = np.array([_lib.hip().crt_row_owner(y, 16, 2) == 1 for y in range(s.height)])
        assert own.any() and np.array_equal(bits(part[own]), bits(ref_frame[own]))
        s.set_row_bands(16, 0, 1)
        cams = [((0.5 + 0.7 * k, 7.0 - 0.4 * k, 16.0 - k), scenes._normalize((0.05 * k, -0.3, -1.0))) for k in range(4)]
        got = []
        for pos, front in cams:
            s.set_camera(pos, front)
            s.render_raw(ASYNC)
            assert s.last_kernel() == "crt_trace_kernel<0,0,0,0,0>"
            s.sync()
            got.append(s.read_output())
        for k, (pos, front) in enumerate(cams):
            s.set_camera(pos, front)
            assert np.array_equal(bits(got[k]), bits(f.plain(what=f"camera {k}"))), k


def tie_scene(tmp_path):
    """8 instances (the fewest that take the pre-test); 1: the one-triangle mesh, 5: the same triangle in a mesh with an inner root, the same matrix"""
    one = _one_triangle_mesh(tmp_path)
    pos = np.array([[-2, -2, 0], [2, -2, 0.1], [0, 2, 0.2], [60, 60, 60], [60.5, 60, 60], [60, 60.5, 60.1]], np.float32)
    two = scenes.Mesh(pos, np.zeros((6, 2), np.float32), np.tile([0, 0, 1], (6, 1)).astype(np.float32), np.array([[0, 1, 2], [3, 4, 5]], np.int32),
                      np.zeros(2, np.int32))
    two = scenes._write_mesh(str(tmp_path), "two", two, [((0.1, 0.9, 0.2), None)])
    insts = _instances(8)
    m = scenes._trs(1.2, (0.2, 1.0, 0.1), 0.3, (0.5, 4.5, 8.0)).astype(np.float32)
    insts[1] = scenes.Instance(2, 0xFFFF, m)
    insts[5] = scenes.Instance(3, 0xFFFF, m.copy())
    return _scene("pretest-entry-tie", insts, [one, two])


@pytest.mark.parametrize("w,h", SIZES)
def test_a_tie_between_a_single_leaf_instance_and_a_higher_inner_root_keeps_the_lower(w, h, nthreads, tmp_path):
    sc = tie_scene(tmp_path)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        f = Frames(s, sc, nthreads)
        iv, ip, pos = s.camera()
        d = np.asarray(f.orc.raygen(w, h, iv, ip), F).reshape(-1, 3)
        o = np.asarray(pos, F)
        # the scene is what it says: a leaf root and an inner root over the same triangle, the same matrix
        assert entry.instance_terms(a, 1)[1] is None and entry.instance_terms(a, 5)[1] is not None
        assert np.array_equal(a["instances"][1]["inv"], a["instances"][5]["inv"])
        full = f.orc.closest_hits(np.tile(o, (len(d), 1)), d)[0]
        tie = np.nonzero(full["instance"] == 1)[0]
        assert len(tie) >= 16 and not (full["instance"] == 5).any()
        # ... to the bit: with instance 1 taken out, the same rays hit instance 5 (then index 4) with the same t, u and v
        b = dict(a); b["instances"] = np.ascontiguousarray(np.delete(a["instances"], 1))
        other = oracle_lib.Oracle(b, nthreads=nthreads).closest_hits(np.tile(o, (len(tie), 1)), d[tie])[0]
        assert (other["instance"] == 4).all()
        for field in ("t", "u", "v"):
            assert np.array_equal(other[field].view(np.uint32), full[field][tie].view(np.uint32)), field
        # the hazard is live: the pre-test's loop over all eight instances WITHOUT the order condition leaves some of these lanes inside instance 5
        # (the others are inside a lower inner root by then: instance 0, which the trip loop enters first in any case) ...
        inside, _, masks = committing_lanes(s, f.orc)
        terms = [entry.instance_terms(a, k) for k in range(len(a["instances"]))]
        unordered = entry.wave_commits(masks[tie], terms, o, d[tie], ordered=False)[1]
        assert (unordered == 5).sum() >= 16, np.unique(unordered, return_counts=True)
        # ... with it they hold the lower bit and commit to nothing above it
        assert (masks[tie] & np.uint64(2)).all() and not (inside[tie] > 1).any()
        # and the two materials differ, so the frame tells who won: the oracle's frame with the two instances exchanged is another frame there
        c = dict(a); c["instances"] = a["instances"].copy(); c["instances"][[1, 5]] = a["instances"][[5, 1]]
        rays = f.orc.raygen(w, h, iv, ip)
        swapped = oracle_lib.Oracle(c, nthreads=nthreads).trace(rays, pos, sc.sun_angle)[0]
        want = f.oracle()
        assert (bits(swapped).reshape(h * w, -1)[tie] != bits(want).reshape(h * w, -1)[tie]).any(1).all()
        f.flag_sets(f"tie, {w}x{h}")
        shadowed_forms(f, f"tie, {w}x{h}")
