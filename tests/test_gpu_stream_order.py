"""Who waits for whom: the ordering promises of include/crt_api.h (the comment above crt_trace_rays) and of Session's filters, made visible
by holding a stream back (tests/stream_hold.py). Every case queues a bounded spin on one stream, submits the work that races with it, checks
that the spin was still running when the last of it was submitted, and only then lets everything finish and compares results -- bit for
bit (util.bits, rr.same_records) with what the suite already trusts: oracle_lib.Oracle on Session.arenas() at the moment of submission, and
temporal_ref / vfilter_ref / denoise_ref / ao_ref on the host copies of the frame a filter was handed.

Without the hold every one of these orders holds by luck: on `tiny` each piece of work is over before the host submits the next.
Each case begins with a control (stream_hold.independent): the operation that must not be ordered behind the hold completes while it is
pending, or the case is inconclusive and fails. Nothing here asserts that a call "must not wait" beyond those controls.
The scene is `tiny`, frames are 96 x 64, batches hold 300 rays."""
import ctypes as C
import functools

import numpy as np
import pytest

from clraytracer_amd import _lib, driver, scenes
import ao_ref
import denoise_ref
import gbuffer_ref
import oracle_lib
import scene_edit_ref as E
import shade_ref
import temporal_ref
import trace_rays_ref as rr
import vfilter_ref
from stream_hold import Hold, independent
from util import bits, seeded_rays

pytestmark = pytest.mark.gpu
W, H, N = 96, 64, 300
WRITE_RAYS = 2
AO = dict(samples=8, radius=16.0, bias=1e-3)          # tests/test_gpu_ao.py: the radius at which `tiny` occludes a share of the samples
MOVE = np.array([3.0, 1.5, -2.0], np.float32)         # of mesh 0: the first move of test_queries_frames_and_instance_uploads_stay_ordered


def arenas_of(s):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}


@functools.lru_cache(maxsize=None)
def rays():
    """`tiny`'s arenas, N seeded rays, and N points with normals (the oracle's hit points of those rays; a miss: the camera position with a
    zero normal, as tests/test_gpu_ao.py makes them): computed once, never modified"""
    sc = scenes.get("tiny")
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(sc)
        a = arenas_of(s)
    o, d = seeded_rays(a, sc.camera_pos, N, seed=11)
    rec, _ = oracle_lib.Oracle(a, nthreads=16).closest_hits(o, d)
    geometry, _, _ = gbuffer_ref.planes_from_records(a, rec)
    hit = (rec["instance"] >= 0) & ~(rec["t"] > gbuffer_ref.INF_MINUS_ONE)
    P = (o + d * rec["t"][:, None]).astype(np.float32)
    n = np.ascontiguousarray(geometry["normal"], np.float32).copy()
    P[~hit] = np.asarray(sc.camera_pos, np.float32)
    n[~hit] = 0.0
    assert N // 2 < int(hit.sum()) < N
    for x in (o, d, P, n):
        x.setflags(write=False)
    return a, o, d, P, n


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).to("cuda:0")


def open_session(monkeypatch, camera=None):
    for k in ("CRT_RAYS_GRID", "CRT_TLAS", "CRT_KERNEL"):
        monkeypatch.delenv(k, raising=False)
    rays()                                                        # (its host-only session must not open inside this one)
    s = driver.Session(W, H, device=0)
    try:
        s.load_scene(scenes.get("tiny"))
        if camera is not None:
            s.set_camera(*camera)
    except Exception:
        s.close()
        raise
    return s


def ao_by_the_oracle(orc, P, n, k=None):
    """ao_ref.compose over the oracle's unbounded records filtered by t < radius (include/crt_api.h: exact while u and v are finite)"""
    P, n = np.ascontiguousarray(P, np.float32).reshape(-1, 3), np.ascontiguousarray(n, np.float32).reshape(-1, 3)
    k = np.arange(len(P), dtype=np.uint32) if k is None else k
    S = AO["samples"]
    o, d, w = ao_ref.rays(P, n, k, dict(AO, seed=0), ao_ref.table())
    rec, _ = orc.closest_hits(np.repeat(o, S, axis=0), np.ascontiguousarray(d.reshape(-1, 3)))
    assert np.isfinite(rec["u"]).all() and np.isfinite(rec["v"]).all()
    occ = ((rec["instance"] >= 0) & (rec["t"] < np.float32(AO["radius"]))).reshape(len(P), S)
    return ao_ref.compose(w, occ)


class Queries:
    """The three families of queries on device buffers over the shared inputs: submit() on torch's current stream, host() the result on the
    host (after the caller synchronised), expected() the same from the oracle on given arenas, same() the comparison, bit for bit."""

    def __init__(self, s):
        self.s = s
        _, o, d, P, n = rays()
        self.o, self.d, self.P, self.n = o, d, P, n
        self.to, self.td, self.tP, self.tn = dev(o), dev(d), dev(P), dev(n)
        self.sun = scenes.get("tiny").sun_angle

    def submit(self, family):
        s = self.s
        if family == "trace_rays":
            return s.trace_rays(self.to, self.td).records
        if family == "shade_rays":
            return s.shade_rays(self.to, self.td)
        return s.trace_ao(self.tP, self.tn, AO["samples"], radius=AO["radius"], bias=AO["bias"])

    @staticmethod
    def host(family, t):
        a = t.cpu().numpy()
        return a.view(_lib.RAYHIT_DTYPE).reshape(-1) if family == "trace_rays" else a

    def expected(self, family, arenas, nthreads):
        orc = oracle_lib.Oracle(arenas, nthreads=nthreads)
        if family == "trace_rays":
            return orc.closest_hits(self.o, self.d)[0]
        if family == "shade_rays":
            return shade_ref.radiance(orc, self.o, self.d, self.sun)
        return ao_by_the_oracle(orc, self.P, self.n)

    @staticmethod
    def same(family, got, want):
        return rr.same_records(got, want) if family == "trace_rays" else np.array_equal(bits(got), bits(want))

    def warm(self):
        """every family once, unheld: the context's allocations and the kernels' first launches stay out of the windows"""
        import torch
        out = {f: self.submit(f) for f in ("trace_rays", "shade_rays", "trace_ao")}
        torch.cuda.synchronize()
        return {f: self.host(f, t) for f, t in out.items()}


def held_pair(case, q):
    """The control of the query cases: (hold, s1, s2, the control's result) -- s1 held, and with only the hold queued a trace_rays on s2 was
    done, and a synchronous frame behind it returned, while the hold was pending: neither s2 nor the session's own stream (frames, uploads
    and crt_query_hits run there) is serialised behind s1, so whatever is later found to have waited for s1 was made to."""
    import torch

    def attempt(s2):
        s1 = torch.cuda.Stream(device="cuda:0")
        hold = Hold(s1)
        with torch.cuda.stream(s2):
            got = q.submit("trace_rays")
            done = torch.cuda.Event()
            done.record()
        done.synchronize()
        q.s.render()
        return hold.pending(), (hold, s1, s2, got)

    return independent(case, attempt)


def timed_event():
    import torch
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    return ev


# ---- queries ---------------------------------------------------------------------------------------------------------------------------------
def test_a_query_waits_on_the_device_for_the_query_before_it(monkeypatch, nthreads):
    """Two queries of one family on two streams, no edit between them: the second runs behind the first although only the first is held."""
    import torch
    case = "query behind query"
    with open_session(monkeypatch) as s:
        q = Queries(s)
        want = q.expected("trace_rays", arenas_of(s), nthreads)
        assert q.same("trace_rays", q.warm()["trace_rays"], want)
        hold, s1, s2, control = held_pair(case, q)
        with torch.cuda.stream(s1):
            first = q.submit("trace_rays"); ev_first = timed_event()
        with torch.cuda.stream(s2):
            second = q.submit("trace_rays"); ev_second = timed_event()
        hold.must_be_pending(case)
        ev_second.synchronize()
        assert hold.event.query(), "the second query was over while the first was still held: its stream did not wait for the query before it"
        torch.cuda.synchronize()
        assert ev_first.elapsed_time(ev_second) >= 0
        for got in (control, first, second):
            assert q.same("trace_rays", q.host("trace_rays", got), want)


@pytest.mark.parametrize("family", ["trace_rays", "shade_rays", "trace_ao"])
def test_a_held_query_keeps_the_instance_table_it_was_submitted_under(monkeypatch, nthreads, family):
    """A query held on s1, then an instance upload (and a frame in flight), then a trace_rays on s2: the first answers from the old table,
    the second from the new one, and the second ends no earlier than the first -- the families share one context."""
    import torch
    case = f"instance table snapshot, {family} held"
    with open_session(monkeypatch) as s:
        q = Queries(s)
        old = arenas_of(s)
        warm = q.warm()
        want_first, want_control = q.expected(family, old, nthreads), q.expected("trace_rays", old, nthreads)
        assert q.same(family, warm[family], want_first)
        s.render(pipelined=True)                                  # once unheld: what the first frame in flight of a session allocates
        s.sync()
        hold, s1, s2, control = held_pair(case, q)
        with torch.cuda.stream(s1):
            first = q.submit(family); ev_first = timed_event()
        hold.lap("the held query")
        s.h.crth_set_mesh_position(0, MOVE.ctypes.data_as(C.POINTER(C.c_float)))
        s.render(pipelined=True)                                  # uploads the table, then a frame in flight
        hold.lap("the instance upload and the frame in flight")
        new = arenas_of(s)
        with torch.cuda.stream(s2):
            second = q.submit("trace_rays"); ev_second = timed_event()
        hold.must_be_pending(case)
        torch.cuda.synchronize()
        s.sync()
        assert ev_first.elapsed_time(ev_second) >= 0, "the query submitted second ended before the held one"
        want_second = q.expected("trace_rays", new, nthreads)
        assert not q.same(family, q.expected(family, new, nthreads), want_first) and not q.same("trace_rays", want_second, want_control)   # the move matters
        assert q.same("trace_rays", q.host("trace_rays", control), want_control)
        assert q.same(family, q.host(family, first), want_first), "the held query did not answer from the table it was submitted under"
        assert q.same("trace_rays", q.host("trace_rays", second), want_second), "the query behind the upload did not see the new table"


def test_a_scene_edit_waits_for_the_query_in_flight(monkeypatch, nthreads):
    """A material record uploaded while a shade_rays is held: the upload returns only once the query is over, whose radiance is the old
    table's. (Materials only: every index a kernel follows stays valid whatever the order.)"""
    import torch
    case = "material upload behind a held shade_rays"
    k = 3                                                         # tests/test_gpu_scene_edits.py: materials 1-2 are mesh 0's, 3-4 mesh 1's
    with open_session(monkeypatch) as s:
        q = Queries(s)
        old = arenas_of(s)
        edited, record = E.replace_material(old, k, 0x0040C0FF, int(old["materials"][k]["albedo"]))
        want_old, want_new = q.expected("shade_rays", old, nthreads), q.expected("shade_rays", edited, nthreads)
        assert not np.array_equal(bits(want_old), bits(want_new))
        assert q.same("shade_rays", q.warm()["shade_rays"], want_old)
        hold, s1, s2, _ = held_pair(case, q)
        with torch.cuda.stream(s1):
            held = q.submit("shade_rays")
        hold.must_be_pending(case)
        assert s.hip.crt_upload_materials(record.ctypes.data, k, 1) == 0
        assert hold.event.query(), "crt_upload_materials returned while the stream of the query in flight was still held"
        with torch.cuda.stream(s2):
            after = q.submit("shade_rays")
        torch.cuda.synchronize()
        assert q.same("shade_rays", q.host("shade_rays", held), want_old), "the held query shaded with materials uploaded after it"
        assert q.same("shade_rays", q.host("shade_rays", after), want_new)


WAITERS = {
    "sync": lambda s, q: s.sync(),
    "read_output": lambda s, q: s.read_output(),
    "read_gbuffer_raw": lambda s, q: s.read_gbuffer_raw(),
    "pick": lambda s, q: s.pick(W // 2, H // 2),
    "render": lambda s, q: s.render(),
    "query_hits": lambda s, q: s.query_hits(q.o[:8], q.d[:8]),
}


@pytest.mark.parametrize("waiter", sorted(WAITERS))
def test_what_waits_for_the_frames_waits_for_the_query_in_flight(monkeypatch, nthreads, waiter):
    import torch
    case = f"{waiter} behind a held query"
    with open_session(monkeypatch) as s:
        q = Queries(s)
        want = q.expected("trace_rays", arenas_of(s), nthreads)
        q.warm()
        s.render(gbuffer=True)
        WAITERS[waiter](s, q)                                     # once unheld: its first-use allocations
        hold, s1, s2, _ = held_pair(case, q)
        with torch.cuda.stream(s1):
            held = q.submit("trace_rays")
        hold.must_be_pending(case)
        WAITERS[waiter](s, q)
        # (the hold's event, which lies in front of the query: one recorded behind the query lies behind the library's own event too, and may
        # read as pending for a moment after the library's wait has returned)
        assert hold.event.query(), f"{waiter} returned while the stream of the query in flight was still held"
        torch.cuda.synchronize()
        assert q.same("trace_rays", q.host("trace_rays", held), want)


@pytest.mark.parametrize("kind", ["RayHits", "SurfaceHits"])
def test_numpy_of_records_behind_a_hold_returns_the_finished_records(monkeypatch, nthreads, kind):
    """RayHits.numpy() / SurfaceHits.numpy() called on torch's default stream for a query enqueued on a held side stream: they synchronise
    with the stream that produced the records (the copy itself runs on the current stream, which a side stream does not order)."""
    import torch
    case = f"{kind}.numpy() behind a hold"
    with open_session(monkeypatch) as s:
        q = Queries(s)
        a = arenas_of(s)
        orc = oracle_lib.Oracle(a, nthreads=nthreads)
        q.warm()
        s.shade_rays(q.to, q.td, radiance=False, surface=True)
        torch.cuda.synchronize()

        def attempt(side):
            hold = Hold(side)
            q.to[:1].cpu()                                        # the control: a copy on the current stream is not held
            return hold.pending(), hold

        hold = independent(case, attempt)
        assert torch.cuda.current_stream() == torch.cuda.default_stream()
        with torch.cuda.stream(hold.stream):
            hits = s.trace_rays(q.to, q.td) if kind == "RayHits" else s.shade_rays(q.to, q.td, radiance=False, surface=True)
        hold.must_be_pending(case)
        got = hits.numpy()
        assert hold.event.query(), "numpy() returned while the stream that produces the records was still held"
        if kind == "RayHits":
            assert rr.same_records(got, orc.closest_hits(q.o, q.d)[0])
        else:
            assert shade_ref.same_surface(got, shade_ref.surface(a, orc, q.o, q.d))


# ---- the frame's own buffers -----------------------------------------------------------------------------------------------------------------
def camera_b():
    return temporal_ref.session_second_camera(scenes.get("tiny"))


def frame_copies(s):
    """host copies of the frame a filter is handed: colour, the geometry plane as (H, W, 4) float32, instance ids, albedo, the CrttCamera"""
    g = s.read_gbuffer_raw()
    geometry = np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1).astype(np.float32)
    return {"color": s.read_output(), "geometry": geometry, "instance": g["ids"]["instance"].astype(np.int32), "albedo": g["albedo"],
            "camera": temporal_ref.camera_from_struct(_lib.crtt_camera(*s.camera(), W, H)), "planes": g}


class Denoise:
    name = "denoise"

    def prepare(self, s, A):
        pass

    def run(self, s):
        return s.denoise()

    def host(self, out):
        return [out.cpu().numpy()]

    def reference(self, f):
        return [denoise_ref.denoise(f["color"], f["geometry"], f["instance"], f["albedo"], iterations=4, flags=denoise_ref.DEMODULATE,
                                    depth_tol=0.05, normal_cos=0.9)]


class Accumulate:
    name = "accumulate"

    def prepare(self, s, A):
        self.hist = driver.TemporalHistory(s)

    def run(self, s):
        s.accumulate(self.hist)
        return self.hist

    def host(self, hist):
        return [getattr(hist, k).cpu().numpy() for k in ("color", "moments", "geometry")]

    def reference(self, f):
        want = temporal_ref.accumulate(f["color"], f["geometry"], f["instance"], f["camera"])
        return [want[k] for k in ("color", "moments", "geometry")]


class FilterVariance:
    """filter_variance(color, moments) over what accumulate returned for frame A, guided by the frame's planes: only the guides race"""
    name = "filter_variance"

    def prepare(self, s, A):
        import torch
        self.color, self.moments = s.accumulate(driver.TemporalHistory(s))
        torch.cuda.synchronize()
        self.h_color, self.h_moments = self.color.cpu().numpy(), self.moments.cpu().numpy()

    def run(self, s):
        return s.filter_variance(self.color, self.moments, return_variance=True)

    def host(self, out):
        return [out[0].cpu().numpy(), out[1].cpu().numpy()]

    def reference(self, f):
        return list(vfilter_ref.filter(self.h_color, self.h_moments, f["geometry"], f["instance"], f["albedo"], iterations=4,
                                       flags=vfilter_ref.DEMODULATE, **vfilter_ref.DEFAULTS))


FILTERS = {"denoise": Denoise, "accumulate": Accumulate, "filter_variance": FilterVariance}


def same_planes(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


class HeldFilter:
    """Frame A rendered with gbuffer=True and copied to the host, then a filter of the frame's own buffers queued behind a hold on torch's
    default stream or on a side stream. The control: with only the hold queued, a synchronous render (of A again: the same bits) returns
    while the hold is pending -- a frame's stream is not serialised behind the held one. Each attempt opens a session of its own."""

    def __init__(self, monkeypatch, case, which, on_side):
        import torch
        self.case, self.filter = case, FILTERS[which]()
        self.session = None

        def attempt(side):
            s = open_session(monkeypatch)
            try:
                s.render(gbuffer=True)
                A = frame_copies(s)
                warm = FILTERS[which]()
                warm.prepare(s, A)
                warm.run(s)                                       # once unheld: the kernels' first launches
                self.filter.prepare(s, A)
                torch.cuda.synchronize()
                stream = side if on_side else torch.cuda.default_stream()
                hold = Hold(stream)
                s.render(gbuffer=True)
                if not hold.pending():
                    hold.release()
                    s.close()
                    return False, None
            except Exception:
                s.close()
                raise
            return True, (s, A, stream, hold)

        self.session, self.A, self.stream, self.hold = independent(case, attempt)
        try:
            with torch.cuda.stream(self.stream):
                self.out = self.filter.run(self.session)
            self.hold.must_be_pending(case)
        except Exception:
            self.session.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        import torch
        torch.cuda.synchronize()
        self.session.close()

    def check_output_is_frame_a(self, B=None):
        """the filter's output is the reference on A's copies -- and, given B's, not the reference on those"""
        import torch
        torch.cuda.synchronize()
        want = self.filter.reference(self.A)
        if B is not None:
            assert not same_planes(self.filter.reference(B), want), "frames A and B filter alike: the case shows nothing"
        assert same_planes(self.filter.host(self.out), want), f"{self.case}: the filter read buffers that the call behind it had already overwritten"


@pytest.mark.parametrize("on_side", [False, True], ids=["default-stream", "side-stream"])
@pytest.mark.parametrize("which", sorted(FILTERS))
def test_a_filter_of_frame_a_is_not_overwritten_by_frame_b(monkeypatch, which, on_side):
    """render A; a held filter of A's own buffers; another camera; render B into the same slot: the filter's output is A's."""
    with HeldFilter(monkeypatch, f"{which} then render", which, on_side) as f:
        s = f.session
        s.set_camera(*camera_b())
        s.render(gbuffer=True)
        assert f.hold.event.query(), "render returned while the stream of a filter of the frame's own buffers was still held"
        s.sync()
        f.check_output_is_frame_a(frame_copies(s))


def test_a_filter_of_frame_a_is_not_overwritten_by_render_raw(monkeypatch):
    with HeldFilter(monkeypatch, "denoise then render_raw", "denoise", True) as f:
        s = f.session
        s.set_camera(*camera_b())
        s.render_raw(_lib.CRT_RENDER_GBUFFER)
        assert f.hold.event.query(), "render_raw returned while the stream of a filter of the frame's own buffers was still held"
        s.sync()
        f.check_output_is_frame_a(frame_copies(s))


@pytest.mark.parametrize("call", ["resize", "close"])
def test_resize_and_close_wait_for_a_held_filter(monkeypatch, call):
    """Both free the buffers the filter reads: when they return the filter is over, and its output is A's."""
    with HeldFilter(monkeypatch, f"denoise then {call}", "denoise", True) as f:
        s = f.session
        reader = s._frame_readers[-1]                             # the event the session keeps behind the filter
        s.resize(80, 48) if call == "resize" else s.close()
        assert reader.query() and f.hold.event.query(), f"{call} returned while a filter of the frame's own buffers had yet to run"
        assert s.frame_readers_pending() == 0
        f.check_output_is_frame_a()


def test_the_tensor_forms_leave_nothing_for_a_render_to_wait_for(monkeypatch):
    """color= with surface= touches no buffer of the session's: no event is kept for them (the driver's bookkeeping, not a timing), while
    the same call guided by the frame's planes keeps one until the next render has waited for it."""
    import torch
    case = "tensor forms"
    with open_session(monkeypatch) as s:
        s.render_raw(WRITE_RAYS)
        dirs = s.read_rays().reshape(-1, 3)
        _, _, pos = s.camera()
        hits = s.shade_rays(dev(np.asarray(pos, np.float32)), dev(dirs), radiance=False, surface=True)
        s.render(gbuffer=True)
        color = dev(s.read_output())
        hist = driver.TemporalHistory(s)
        torch.cuda.synchronize()
        assert s.frame_readers_pending() == 0
        hold = Hold(torch.cuda.default_stream())
        s.denoise(color, surface=hits)
        acc, moments = s.accumulate(hist, color, surface=hits)
        s.filter_variance(acc, moments, surface=hits)
        assert s.frame_readers_pending() == 0 and s._frame_readers == []
        s.denoise(color)                                          # guided by the frame's planes
        assert s.frame_readers_pending() == 1
        hold.must_be_pending(case)
        s.render()
        assert hold.event.query() and s.frame_readers_pending() == 0


# ---- frame ambient occlusion -----------------------------------------------------------------------------------------------------------------
def test_frame_ao_behind_a_hold_is_the_ao_of_the_frame_it_was_asked_for(monkeypatch, nthreads):
    """crt_frame_ao held on the null stream, then another camera and a synchronous G-buffer frame into the same slot: the AO plane is that of
    the first frame's planes (ao_ref on their host copies), and the frame waited for the query."""
    import torch
    case = "frame AO then render"
    tol, cos = 0.05, 0.9
    params = _lib.CrtAoParams(AO["samples"], AO["radius"], AO["bias"], 0, _lib.CRT_AO_FILTER, tol, cos)

    def attempt(side):
        s = open_session(monkeypatch)
        try:
            s.render_raw(WRITE_RAYS)
            dirs = s.read_rays()
            s.render(gbuffer=True)
            planes = s.read_gbuffer_raw()
            warm = np.array(s.ambient_occlusion(AO["samples"], radius=AO["radius"], bias=AO["bias"], filter=True, depth_tol=tol, normal_cos=cos))
            torch.cuda.synchronize()
            hold = Hold(torch.cuda.default_stream())
            s.render(gbuffer=True)                                # the control: a frame is not serialised behind the held null stream
            if not hold.pending():
                hold.release()
                s.close()
                return False, None
        except Exception:
            s.close()
            raise
        return True, (s, dirs, planes, warm, hold)

    s, dirs, planes, warm, hold = independent(case, attempt)
    with s:
        _, _, pos = s.camera()
        assert s.h.crth_compute_ao(C.byref(params), None)        # Session.ambient_occlusion without its read-back: enqueue and return
        hold.must_be_pending(case)
        s.set_camera(*camera_b())
        s.render(gbuffer=True)
        assert hold.event.query(), "a synchronous frame returned while the AO query in flight had yet to run"
        got = np.empty((H, W), np.float32)
        _lib.check(s.hip.crt_read_ao(got.ctypes.data, got.size), "crt_read_ao")
        P, n, k = ao_ref.frame_items(planes, dirs, pos)
        raw = ao_by_the_oracle(oracle_lib.Oracle(arenas_of(s), nthreads=nthreads), P, n, k).reshape(H, W)
        want = ao_ref.filter5x5(raw, planes["geometry"], tol, cos)
        assert np.array_equal(bits(warm), bits(want))
        assert np.array_equal(bits(got), bits(want)), "the AO plane is not the AO of the frame it was asked for"
        of_b = s.ambient_occlusion(AO["samples"], radius=AO["radius"], bias=AO["bias"], filter=True, depth_tol=tol, normal_cos=cos)
        assert not np.array_equal(bits(of_b), bits(want))          # frame B's differs: the case shows something
