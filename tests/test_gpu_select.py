"""crts_compact, crts_points, crts_scatter and the Session methods over them on the GPU against the numpy restatement of the definition
(tests/select_ref.py): every word of every output, bit for bit. Outputs start as poison whose payload differs from word to word and have guard
words behind them, so an entry that was not written and a write past the end both show; scratch starts as poison too; the inputs are checked to be
untouched. compact: sizes around a wave, a workgroup, a chunk, several chunks and one more chunk sum than a round of the scanning launch takes;
masks of bytes (also 1 and 3 bytes into an allocation) and state words (some of 32 and more); capacities below, at and above the total. points:
the frames and guides of tests/test_gpu_upsample.py under both layouts with a camera from crtt_camera, lists with NONE and entries that name no
pixel, the grid form at every factor and offset. scatter: 1 and 4 channels, with and without a state plane. A side stream; and a Session on
`tiny` that re-traces what an upsample could not interpolate."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clraytracer_amd import _lib, driver, scenes

if not os.path.exists(getattr(_lib, "SELECT_SO", "")):
    import __graft_entry__
    __graft_entry__.build()

import select_ref as ref
import test_gpu_upsample as gu
import upsample_ref
from util import bits

pytestmark = pytest.mark.gpu
GUARD = 64                              # words behind every output
CHUNK, SCAN, NONE = ref.CHUNK, ref.SCAN, ref.NONE
# around a wave, a workgroup and a chunk; several chunks with a partial one; one more chunk sum than one round of the scanning launch takes
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17, CHUNK * SCAN + 1]
AO = dict(radius=16.0, bias=1e-3)       # tests/test_gpu_ao.py: the radius at which `tiny` occludes a share of the sample rays
WRITE_RAYS = 2


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def guarded(words, salt, dtype="int32"):
    """`words` words of poison and GUARD more behind them"""
    return gu.poison((words + GUARD,), salt, dtype)


def written(t, words, salt, want, what=""):
    """the first `words` words of t are `want`, bit for bit, and the guard behind them is the poison it was"""
    got = t.cpu().numpy().view(np.uint32)
    want = np.ascontiguousarray(want).view(np.uint32).reshape(-1)
    assert want.size == words
    differ = got[:words] != want
    assert not differ.any(), f"{what}: {int(differ.sum())} of {words} words differ, the first at {int(np.flatnonzero(differ)[0])}"
    tail = np.arange(words, words + GUARD, dtype=np.int64) + (0x7FC00000 + salt)
    assert np.array_equal(got[words:], tail.astype(np.uint32)), f"{what}: the guard words were written"


def run_compact(words, word_bytes, values, capacity, scratch=None):
    """(list, counts, scratch) as guarded tensors; `words`: a flat device tensor (or a view into one)"""
    lib = _lib.select()
    n = words.numel()
    lst, counts = guarded(capacity, 0x100), guarded(2, 0x200)
    sw = lib.crts_scratch_bytes(n) // 4
    scratch = guarded(sw, 0x300) if scratch is None else scratch
    c = _lib.CrtsCompact(words.data_ptr(), word_bytes, values, n, capacity)
    rc = lib.crts_compact(C.byref(c), lst.data_ptr(), counts.data_ptr(), scratch.data_ptr(), stream())
    assert rc == 0, lib.crts_error_string(rc)
    return lst, counts, scratch


def check_compact(host, values, capacity, device=None, what=""):
    word_bytes = host.dtype.itemsize
    device = gu.dev(host) if device is None else device
    want = ref.compact(host, values, capacity)
    lst, counts, scratch = run_compact(device, word_bytes, values, capacity)
    written(lst, capacity, 0x100, want[0], f"{what} list")
    written(counts, 2, 0x200, want[1], f"{what} counts")
    sw = _lib.select().crts_scratch_bytes(host.size) // 4
    assert np.array_equal(scratch.cpu().numpy()[sw:], (np.arange(sw, sw + GUARD, dtype=np.int64) + (0x7FC00000 + 0x300)).astype(np.uint32).view(np.int32))
    return lst, counts


def selections(n):
    rng = np.random.RandomState(n)
    m = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "every 2nd": np.arange(n) % 2 == 1, "1 %": rng.uniform(size=n) < 0.01,
         "50 %": rng.uniform(size=n) < 0.5, "the last": np.arange(n) == n - 1, "the first": np.arange(n) == 0}
    return m


@pytest.mark.parametrize("n", SIZES)
def test_compact_every_size_selection_word_size_and_capacity_matches_the_reference(n):
    import torch
    ran = 0
    for name, mask in selections(n).items():
        total = int(mask.sum())
        host = mask.astype(np.uint8)
        device = gu.dev(host)
        for capacity in sorted({1, max(1, total - 1), max(1, total), total + 5, n}):
            check_compact(host, 2, capacity, device, f"n {n}, {name}, capacity {capacity}")
            ran += 1
        assert np.array_equal(device.cpu().numpy(), host)
    # a mask that starts 1 and 3 bytes into an allocation, as a bool tensor
    rng = np.random.RandomState(7 * n)
    for shift in (1, 3):
        host = np.zeros(n + 8, np.uint8)
        host[:shift] = 1; host[shift + n:] = 1                                 # selected bytes around the mask: none of them is an item
        host[shift:shift + n] = rng.uniform(size=n) < 0.3
        whole = gu.dev(host).view(torch.bool)
        check_compact(host[shift:shift + n], 2, n, whole[shift:shift + n], f"n {n}, {shift} bytes in")
        check_compact(host[shift:shift + n], 2, max(1, n // 3), whole[shift:shift + n], f"n {n}, {shift} bytes in")
    # state words: 0 .. 3, and some of 32 and more that no set selects
    words = rng.randint(0, 4, n).astype(np.uint32)
    odd = rng.uniform(size=n) < 0.1
    words[odd] = rng.choice(np.array([32, 33, 34, 63, 64, 255, 256, 2 ** 31, 2 ** 32 - 1], np.uint64), int(odd.sum())).astype(np.uint32)
    device = gu.dev(words.view(np.int32))
    for values in (0, 6, 0xFFFFFFFF, 1 << upsample_ref.NEAREST):
        total = int(ref.selected(words, values).sum())
        for capacity in sorted({1, max(1, total - 1), max(1, total), max(1, total // 2), total + 5, n}):
            check_compact(words, values, capacity, device, f"n {n}, words, values {values:#x}, capacity {capacity}")
    assert np.array_equal(device.cpu().numpy().view(np.uint32), words)
    assert ran >= 7 * 2


def test_compact_twice_in_a_row_gives_the_same_bits_from_one_scratch_buffer():
    n = 3 * CHUNK + 17
    rng = np.random.RandomState(3)
    words = rng.randint(0, 3, n).astype(np.uint32)
    device = gu.dev(words.view(np.int32))
    want = ref.compact(words, 6, 5000)
    first = run_compact(device, 4, 6, 5000)
    second = run_compact(device, 4, 6, 5000, scratch=first[2])                 # calls on one stream may share their scratch
    third = run_compact(gu.dev((words == 2).astype(np.uint8)), 1, 2, 100, scratch=first[2])       # ... and another input in between
    fourth = run_compact(device, 4, 6, 5000, scratch=first[2])
    for got in (first, second, fourth):
        written(got[0], 5000, 0x100, want[0]); written(got[1], 2, 0x200, want[1])
    want = ref.compact((words == 2).astype(np.uint8), 2, 100)
    written(third[0], 100, 0x100, want[0]); written(third[1], 2, 0x200, want[1])
    assert want[1][0] > 100                                                    # an overflow: visible, and no fault


# ---- points -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrices():
    with driver.Session(160, 96, host_only=True) as s:
        s.load_scene(scenes.get("tiny"))
        return tuple(np.array(m) for m in s.camera())


def camera_of(w, h):
    return _lib.crtt_camera(*matrices(), w, h)


def cameras(w, h):
    """the session's camera, its mirror image and one whose y row is turned round: the kernel knows no matrix convention, so each is a camera to
    it, and between them every hit pixel's normal is met from the front and from behind"""
    base, out = camera_of(w, h), []
    for rows in ((1.0, 1.0, 1.0), (-1.0, -1.0, -1.0), (1.0, -1.0, 1.0)):
        c = _lib.CrttCamera()
        C.memmove(C.byref(c), C.byref(base), C.sizeof(c))
        for i in range(9):
            c.toRay[i] = base.toRay[i] * rows[i // 3]
        out.append(c)
    return out


def run_points(b, layout, cam, lst=None, grid=None, dirs=True):
    """(positions, normals, dirs or None) as guarded tensors; b: a gu.Buffers"""
    lib = _lib.select()
    f = _lib.CrtsFrame(b.w, b.h, layout, (b.t_records if layout == _lib.CRTS_GUIDES_SURFACE else b.t_planes["geometry"]).data_ptr(), cam)
    if lst is not None:
        count, items = lst.numel(), _lib.CrtsItems(lst.data_ptr(), lst.numel(), 0, 0, 0)
    else:
        factor, (ox, oy) = grid
        lw, lh = (b.w, b.h) if factor == 1 else upsample_ref.low_size(b.w, b.h, factor, (ox, oy))
        count, items = lw * lh, _lib.CrtsItems(None, lw * lh, factor, ox, oy)
    out = [guarded(4 * count, 0x400 + 0x100 * i, "float32") for i in range(3 if dirs else 2)]
    rc = lib.crts_points(C.byref(f), C.byref(items), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr() if dirs else None, stream())
    assert rc == 0, lib.crts_error_string(rc)
    return out + [None] * (3 - len(out)), count


def check_points(got, count, want, what=""):
    for i, (g, w) in enumerate(zip(got, want)):
        if g is not None:
            written(g, 4 * count, 0x400 + 0x100 * i, bits(w), f"{what} {('positions', 'normals', 'dirs')[i]}")


LAYOUTS = (_lib.CRTS_GUIDES_PLANES, _lib.CRTS_GUIDES_SURFACE)


@pytest.mark.parametrize("shape", gu.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_points_of_lists_and_grids_match_the_reference_under_both_layouts(shape):
    w, h = shape
    b = gu.Buffers(w, h)
    geometry = b.planes["geometry"]                                           # (h, w, 4) float32: n, t
    structs = cameras(w, h)
    rng = np.random.RandomState(w)
    # every pixel in a shuffled order, and among them NONE, the first index behind the frame, 2^31 and more
    lst = np.concatenate([rng.permutation(w * h), [NONE, w * h, 2 ** 31, 2 ** 31 + w, w * h + 1, NONE]]).astype(np.uint32)
    rng.shuffle(lst)
    t_list = gu.dev(lst.view(np.int32))
    for struct in structs:
        want = ref.points(lst, geometry, ref.camera_from_struct(struct))
        for layout in LAYOUTS:
            for dirs in (True, False):
                got, count = run_points(b, layout, struct, lst=t_list, dirs=dirs)
                check_points(got, count, want, f"list, layout {layout}")
    ran = 0
    for factor in (1, 2, 4):
        for ox in range(min(factor, w)):
            for oy in range(min(factor, h)):
                struct = structs[(2 * ran) % 3]
                want = ref.points(ref.grid_list(w, h, factor, (ox, oy)), geometry, ref.camera_from_struct(struct))
                for layout in LAYOUTS:
                    got, count = run_points(b, layout, struct, grid=(factor, (ox, oy)), dirs=(ox + oy) % 2 == 0)
                    check_points(got, count, want, f"grid {factor} {(ox, oy)}, layout {layout}")
                    ran += 1
    assert ran >= 2 * 3
    assert np.array_equal(t_list.cpu().numpy().view(np.uint32), lst)
    b.inputs_untouched()


def test_the_points_inputs_are_not_degenerate():
    """what the cases above gather: hits and pixels that are no hit (a miss, a far t, a NaN t); normals that are turned and normals that are
    not; the reference makes no NaN of its own that the comparison of bits would trip over"""
    planes = gu.guides(70, 37)
    geometry = planes["geometry"]
    t = geometry[..., 3]
    assert (t == 99999.0).any() and np.isnan(t).any() and (t <= 99998.0).mean() > 0.5
    hit = (t <= 99998.0).reshape(-1)
    stored = geometry.reshape(-1, 4)[:, :3]
    shares = []
    for struct in cameras(70, 37):
        p, n, d = ref.points(ref.grid_list(70, 37, 1), geometry, ref.camera_from_struct(struct))
        turned = (bits(n[:, :3]) != bits(stored)).any(axis=-1) & hit
        shares.append(turned.sum() / hit.sum())
        assert np.isfinite(p[hit]).all() and np.isfinite(d).all() and (bits(n[~hit]) == 0).all() and (bits(p[~hit][:, :3]) == 0).all()
        assert np.abs(np.linalg.norm(d[:, :3].astype(np.float64), axis=-1) - 1.0).max() < 1e-6
    print("normals turned under the three cameras:", shares)
    assert shares[0] == 0.0 and shares[1] == 1.0 and 0.05 < shares[2] < 0.95


# ---- scatter ----------------------------------------------------------------------------------------------------------------------------------
def run_scatter(lst, values, n, channels, with_state, state_word=3):
    lib = _lib.select()
    out = guarded(n * channels, 0x700, "float32")
    state = guarded(n, 0x800) if with_state else None
    s = _lib.CrtsScatter(lst.data_ptr(), values.data_ptr(), out.data_ptr(), state.data_ptr() if with_state else None, lst.numel(), channels, n, state_word)
    rc = lib.crts_scatter(C.byref(s), stream())
    assert rc == 0, lib.crts_error_string(rc)
    return out, state


def scatter_reference(lst, values, n, channels, state_word=3):
    out = gu.poison((n * channels,), 0x700).cpu().numpy().reshape((n, 4) if channels == 4 else (n,)).copy()
    state = gu.poison((n,), 0x800, "int32").cpu().numpy().view(np.uint32).copy()
    ref.scatter(lst, values, out, state, state_word)
    return out, state


@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("n", [1, 65, 257, 3 * CHUNK + 17])
def test_scatter_writes_the_listed_items_and_nothing_else(n, channels):
    rng = np.random.RandomState(n + channels)
    for count in sorted({1, max(1, n // 7), n, n + 300}):
        k = rng.permutation(n)[:min(count, n)].astype(np.uint32)
        lst = np.full(count, NONE, np.uint32)
        lst[:len(k)] = k
        if count >= 4:
            lst[rng.randint(0, count, max(1, count // 5))] = np.array([NONE, n, 2 ** 31, n + 1, 2 ** 28], np.uint32)[rng.randint(0, 5, max(1, count // 5))]
        rng.shuffle(lst)
        values = rng.uniform(-1, 1, (count, 4) if channels == 4 else (count,)).astype(np.float32)
        t_list, t_values = gu.dev(lst.view(np.int32)), gu.dev(values)
        want = scatter_reference(lst, values, n, channels, 3 if count % 2 else 0xABCD)
        for with_state in (True, False):
            out, state = run_scatter(t_list, t_values, n, channels, with_state, 3 if count % 2 else 0xABCD)
            written(out, n * channels, 0x700, bits(want[0]), f"n {n}, count {count} out")
            if with_state:
                written(state, n, 0x800, want[1], f"n {n}, count {count} outState")
        if count == n:
            assert (lst < n).sum() < n or n < 4                                 # some pixels keep their poison: `written` compared them
        assert np.array_equal(t_list.cpu().numpy().view(np.uint32), lst) and np.array_equal(bits(t_values.cpu().numpy()), bits(values))


def test_on_another_stream_and_back_to_back():
    """compact -> points -> scatter of the positions, twice, on a side stream, with one scratch buffer"""
    import torch
    w, h = 70, 37
    b = gu.Buffers(w, h)
    geometry = b.planes["geometry"]
    struct = camera_of(w, h)
    cam = ref.camera_from_struct(struct)
    rng = np.random.RandomState(9)
    states = [rng.randint(0, 3, w * h).astype(np.uint32) for _ in range(2)]
    t_states = [gu.dev(s.view(np.int32)) for s in states]
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    got, scratch = [], None
    with torch.cuda.stream(side):
        for t_state, capacity in zip(t_states, (w * h, 500)):
            lst, counts, scratch = run_compact(t_state, 4, 6, capacity, scratch=scratch)
            (p, n, d), count = run_points(b, _lib.CRTS_GUIDES_PLANES, struct, lst=lst[:capacity])
            out, state = run_scatter(lst[:capacity], p[:4 * capacity], w * h, 4, True)
            got.append((lst, counts, p, n, d, out, state))
    side.synchronize()
    for (lst, counts, p, n, d, out, state), host, capacity in zip(got, states, (w * h, 500)):
        want = ref.compact(host, 6, capacity)
        written(lst, capacity, 0x100, want[0]); written(counts, 2, 0x200, want[1])
        pts = ref.points(want[0], geometry, cam)
        check_points((p, n, d), capacity, pts)
        wo, ws = scatter_reference(want[0], pts[0], w * h, 4)
        written(out, 4 * w * h, 0x700, bits(wo)); written(state, w * h, 0x800, ws)
    b.inputs_untouched()


# ---- through Session, on a rendered frame -----------------------------------------------------------------------------------------------------
SW, SH = 160, 96


def test_session_retraces_what_the_upsample_could_not_interpolate():
    import torch
    sc = scenes.get("tiny")
    with driver.Session(SW, SH, device=0) as s:
        s.load_scene(sc)
        s.render_raw(WRITE_RAYS)
        rays = s.read_rays().reshape(-1, 3)
        _, _, pos = s.camera()
        hits = s.shade_rays(gu.dev(np.asarray(pos, np.float32)), gu.dev(rays), radiance=False, surface=True)
        s.render(gbuffer=True)
        g = s.read_gbuffer_raw()
        geometry = np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1).astype(np.float32)
        cam = ref.camera_from_struct(_lib.crtt_camera(*s.camera(), SW, SH))
        hit = geometry[..., 3] <= 99998.0
        assert 0.05 < hit.mean() < 0.95
        # the upsample route's input, made on the device
        want = ref.points(ref.grid_list(SW, SH, 2), geometry, cam)
        for kw in (dict(), dict(surface=hits)):
            got = s.frame_points(factor=2, dirs=True, **kw)
            assert all(x.shape == (SW * SH // 4, 4) and x.dtype == torch.float32 for x in got)
            for x, y in zip(got, want):
                assert np.array_equal(bits(x.cpu().numpy()), bits(y))
        positions, normals = s.frame_points(factor=2)
        low = s.trace_ao(positions[:, :3], normals[:, :3], 8, **AO).reshape(SH // 2, SW // 2)
        ao0, state0 = s.upsample(low, return_state=True)
        ao0, state0 = ao0.cpu().numpy(), state0.cpu().numpy()
        values = 1 << upsample_ref.NEAREST | 1 << upsample_ref.EMPTY
        for capacity in (256, 32):
            lst, counts = ref.compact(state0.view(np.uint32), values, capacity)
            total, kept = int(counts[0]), int(counts[1])
            print(f"tiny {SW}x{SH}, factor 2: {total} pixels to re-trace, capacity {capacity}")
            assert 1 <= total <= 256 and (total > 32 if capacity == 32 else kept == total)
            p, n, _ = ref.points(lst, geometry, cam)
            answers = s.trace_ao(gu.dev(p)[:, :3], gu.dev(n)[:, :3], 8, **AO).cpu().numpy()      # the reference's padded list, position by position
            for kw in (dict(), dict(surface=hits)):
                ao, state = gu.dev(ao0), gu.dev(state0)
                got = s.retrace_ao(ao, state, capacity=capacity, **AO, **kw)
                assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy().view(np.uint32), counts)
                ao, state = ao.cpu().numpy().reshape(-1), state.cpu().numpy().reshape(-1)
                sel = lst[:kept]
                assert np.array_equal(bits(ao[sel]), bits(answers[:kept])) and (state[sel] == ref.RETRACED).all()
                rest = np.ones(SW * SH, bool); rest[sel] = False
                assert np.array_equal(bits(ao[rest]), bits(ao0.reshape(-1)[rest])) and np.array_equal(state[rest], state0.reshape(-1)[rest])
                if capacity == 32:                                          # the pixels behind the first 32 keep their fallback
                    behind = np.flatnonzero(ref.selected(state0.view(np.uint32), values))[32:]
                    assert len(behind) == total - 32 and rest[behind].all() and np.isin(state[behind], (upsample_ref.NEAREST, upsample_ref.EMPTY)).all()
        # the pieces by themselves: a bool mask, the default capacity, a scatter of four channels
        mask = torch.from_numpy(hit).to("cuda:0")
        lst, counts = s.select(mask)
        wl, wc = ref.compact(hit, 2, (SW * SH + 7) // 8)
        assert lst.dtype == torch.int32 and np.array_equal(lst.cpu().numpy().view(np.uint32), wl) and np.array_equal(counts.cpu().numpy().view(np.uint32), wc)
        image = torch.zeros((SH, SW, 4), device="cuda:0")
        pts = s.frame_points(lst)
        s.scatter(lst, pts[0], image)
        wi = np.zeros((SW * SH, 4), np.float32)
        ref.scatter(wl, ref.points(wl, geometry, cam)[0], wi)
        assert np.array_equal(bits(image.cpu().numpy().reshape(-1, 4)), bits(wi))


def test_session_refusals():
    import torch
    sc = scenes.get("tiny")
    with driver.Session(SW, SH, host_only=True) as s:
        s.load_scene(sc)
        for call in (lambda: s.select(torch.zeros(8, dtype=torch.uint8)), lambda: s.frame_points(), lambda: s.scatter(None, None, None),
                     lambda: s.retrace_ao(None, None, **AO)):
            with pytest.raises(ValueError, match="host-only"):
                call()
    with driver.Session(SW, SH, device=0) as s:
        s.load_scene(sc)
        state = torch.zeros((SH, SW), dtype=torch.int32, device="cuda:0")
        ao = torch.zeros((SH, SW), device="cuda:0")
        with pytest.raises(ValueError, match="none has been rendered"):
            s.frame_points()
        with pytest.raises(ValueError, match="none has been rendered"):
            s.retrace_ao(ao, state, **AO)
        s.render(gbuffer=True)
        lst, counts = s.select(state, capacity=16)
        assert counts.cpu().tolist() == [0, 0] and (lst.cpu().numpy() == -1).all()
        for bad in (state.cpu(), state.float(), state.long(), state[:, ::2], state[:0], None, state.cpu().numpy()):
            with pytest.raises(ValueError):
                s.select(bad)
        for kw in (dict(values=(32,)), dict(values=(-1,)), dict(capacity=0), dict(capacity=2 ** 28 + 1)):
            with pytest.raises(ValueError):
                s.select(state, **kw)
        for bad in (lst.cpu(), lst.float(), lst.reshape(4, 4), lst[::2], None if False else lst.long()):
            with pytest.raises(ValueError):
                s.frame_points(bad)
        for kw in (dict(factor=3), dict(factor=8), dict(factor=2, offset=(2, 0)), dict(offset=(1, 0)), dict(factor=4, offset=(0, -1))):
            with pytest.raises(ValueError):
                s.frame_points(**kw)
        hits = s.shade_rays(torch.zeros(3, device="cuda:0"), torch.ones((5, 3), device="cuda:0"), radiance=False, surface=True)
        with pytest.raises(ValueError, match="records"):
            s.frame_points(surface=hits)
        values = torch.zeros(16, device="cuda:0")
        for args in ((lst.cpu(), values, ao), (lst, values.cpu(), ao), (lst, values, ao.cpu()), (lst, values[:15], ao), (lst, values.double(), ao),
                     (lst, values, ao.double()), (lst.float(), values, ao), (lst, torch.zeros((16, 3), device="cuda:0"), ao),
                     (lst, torch.zeros((16, 4), device="cuda:0"), ao), (lst, values, ao[:, ::2])):
            with pytest.raises(ValueError):
                s.scatter(*args)
        for st in (state.cpu(), state.float(), state[:-1]):
            with pytest.raises(ValueError):
                s.scatter(lst, values, ao, st)
        for a, st in ((ao.cpu(), state), (ao, state.cpu()), (ao.double(), state), (ao, state.float()), (ao[:-1], state), (ao, state[:, :-1]),
                      (ao.reshape(-1), state), (torch.zeros((SH, SW, 4), device="cuda:0"), state)):
            with pytest.raises(ValueError):
                s.retrace_ao(a, st, **AO)
        assert s.retrace_ao(ao, state, capacity=8, **AO).cpu().tolist() == [0, 0]
        s.render()
        with pytest.raises(ValueError, match="without gbuffer"):
            s.frame_points()
