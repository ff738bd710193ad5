"""The root pre-test of the reflection bounce on the device (crt_device.h: bounce_pretest_mask -- root_pretest_misses once per instance and wave behind
candidate_mask, every lane on its own origin): the uncounted Trace kernels, synchronous and with CRT_RENDER_ASYNC, against the counted kernels, which
never take it, and against the oracle, which has no cull at all -- bit for bit, with the kernel that ran checked by name for every frame.

The scenes (tests/bounce_pretest_ref.py): small instances over a reflecting floor, each with the extreme corner of its first root child box a hair
inside or outside a ray the floor reflects, and one instance whose root is a single leaf; 7, 8, 64 and 65 instances -- the edges of the rule of
8 ... 64 (65 with CRT_TLAS=0: two 64-chunks, no pre-test; the same frames all the same) -- at 64x40, 72x72 and 203x117 (partial tiles at the edges).
Every flag set whose kernel the policy lets in -- plain, refraction, SSAA 2 and 4 (also with shadow rays and with refraction), the G-buffer with
shadow rays -- and the ones it leaves out (shadow rays alone, the G-buffer alone: Frames.flag_sets renders both); row bands, split tiles and three frames in
flight. Not vacuous: in every scene the restatement finds a full tile and an instance that the cull keeps for lanes the pre-test clears and for lanes it keeps."""
import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import bounce_pretest_ref as scene_ref
from test_gpu_camera_cull import ASYNC, COUNT, REFRACT, SSAA2, SSAA4, Frames
from test_gpu_root_pretest import shadowed_forms
from test_gpu_ssaa import resolve
from util import bits

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(64, 40), (72, 72), (203, 117)]
PLAIN = "crt_trace_kernel<0,0,0,0,0>"


def asynchronous(f, flags, kernel):
    f.s.render_raw(flags | ASYNC)
    assert f.s.last_kernel() == kernel, (f.s.last_kernel(), kernel)
    f.s.sync()
    return f.s.read_output()


def refracted_ssaa(f, what):
    """the one kernel of the policy that neither Frames.flag_sets nor shadowed_forms renders: supersampled with refraction"""
    for k, flag in ((2, SSAA2), (4, SSAA4)):
        got = f.render(flag | REFRACT, "crt_trace_ssaa_kernel<0,0,0,1>")
        assert np.array_equal(bits(got), bits(resolve(f.oracle(k, refraction=True), k))), (what, "ssaa + refraction", k)
        assert np.array_equal(bits(got), bits(f.render(flag | REFRACT | COUNT, "crt_trace_ssaa_kernel<1,0,0,1>"))), (what, "ssaa + refraction, counted", k)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("n", [7, 8, 64, 65])
def test_reflected_rays_graze_root_boxes_every_flag_set(n, w, h, monkeypatch, nthreads, tmp_path):
    if n > 64:
        monkeypatch.setenv("CRT_TLAS", "0")                                   # read by crt_init: the chunked loop, 64 + 1
    sc = scene_ref.floor_scene(n, w, h, nthreads, tmp_path)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        a = s.arenas()
        assert len(a["instances"]) == n
        f = Frames(s, sc, nthreads)
        iv, ip, pos = s.camera()
        alive, _, _, sph, use = scene_ref.wave_view(a, f.orc, w, h, iv, ip, pos)
        assert not (sph & ~use)[:, 3].any()                                   # the single-leaf instance
        assert scene_ref.mixed_waves(alive, sph, use, w, h) > 0
        what = f"{n} instances over the floor, {w}x{h}"
        f.flag_sets(what)
        shadowed_forms(f, what)
        refracted_ssaa(f, what)
        want = f.oracle()
        assert np.array_equal(bits(asynchronous(f, 0, PLAIN)), bits(want)), (what, "async")
        assert np.array_equal(bits(asynchronous(f, REFRACT, "crt_trace_kernel<0,0,0,0,1>")), bits(f.oracle(refraction=True))), (what, "async + refraction")


def test_row_bands_split_tiles_and_three_frames_in_flight(monkeypatch, nthreads, tmp_path):
    monkeypatch.setenv("CRT_FRAMES_IN_FLIGHT", "3")
    w, h = 72, 72
    sc = scene_ref.floor_scene(16, w, h, nthreads, tmp_path)
    with driver.Session(w, h, device=0) as s:
        s.load_scene(sc)
        f = Frames(s, sc, nthreads)
        ref_frame = f.plain()
        for _ in range(3):                      # later frames run on lists built from the first one's costs: quadrant waves of split tiles
            assert np.array_equal(bits(f.render(0, PLAIN)), bits(ref_frame))
        s.set_row_bands(16, 1, 2)
        part = f.render(0, PLAIN)
        own = np.array([_lib.hip().crt_row_owner(y, 16, 2) == 1 for y in range(s.height)])
        assert own.any() and np.array_equal(bits(part[own]), bits(ref_frame[own]))
        s.set_row_bands(16, 0, 1)
        # frames in flight: a camera that moves every frame, each ASYNC frame against the synchronous frame of the same camera
        cams = [((0.5 + 0.7 * k, 7.0 - 0.4 * k, 16.0 - k), scenes._normalize((0.05 * k, -0.3, -1.0))) for k in range(5)]
        got = []
        for pos, front in cams:
            s.set_camera(pos, front)
            got.append(asynchronous(f, 0, PLAIN))
        for k, (pos, front) in enumerate(cams):
            s.set_camera(pos, front)
            assert np.array_equal(bits(got[k]), bits(f.plain(what=f"camera {k}"))), k
