#!/usr/bin/env python3
"""Rate of selective re-tracing (libcrt_select.so) on the 1920x1080 G-buffer frames of multi-1M that tools/upsample_rate.py uses: the
headline camera and the dense camera. The state plane is the one crtu_upsample writes for ambient occlusion traced at every 2nd pixel.

    compact      ms of crts_compact of the state plane (4-byte words, NEAREST | EMPTY) and of the same selection as a bool mask, capacity
                 ceil(n / 8), against a device copy of half the bytes it must move (every word read once, every list entry written: the floor; the
                 call itself reads the words twice), against the same list composed from torch ops that do not wait on the host (cumsum, where,
                 an index write with a spare slot for what is not selected), and against torch.nonzero, which waits
    points       ms of crts_points for the list and for the grid of factor 2, against the copy of half its bytes (per item the entry, 16 B of guide
                 read, two rows of 16 B written) and the same values composed from torch ops
    scatter      ms of crts_scatter of one channel with the state plane, against the copy and against torch's index write with a spare slot
    routes       end to end through Session, against crt_frame_ao on the full frame in the same run: frame_points(grid) + trace_ao + upsample,
                 with and without retrace_ao behind it, at factors 2 and 4; the selected pixels and the mean absolute difference to the full frame's AO
    padding      trace_ao on the `capacity` items of the padded list, of which `total` trace, against trace_ao on the first `total` alone

Every leg is timed with events on the stream around `--repeats` back-to-back calls (a fifth as many for the torch compositions and the routes);
the legs alternate for `--rounds` rounds after a warm-up of each; the median round is reported with min .. max. Needs a GPU: there is no fallback.

    python tools/select_rate.py [--rounds R] [--repeats K] [--out profiles/select_rate.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from clraytracer_amd import _lib, driver, scenes
import ao_ref

W, H = 1920, 1080
N = W * H
AO_SAMPLES, BIAS_OF_RADIUS, RADIUS_OF_EXTENT = 8, 1e-3, 0.1     # tools/ao_rate.py's
VALUES = 1 << _lib.CRTU_STATE_NEAREST | 1 << _lib.CRTU_STATE_EMPTY
WRITE_RAYS = 2


def torch_compact(torch, sel, capacity):
    """the list and counts of include/crt_select.h from torch ops, without a host wait: an item that is not selected, or does not fit, is written
    to a spare slot behind the list"""
    n = sel.numel()
    rank = torch.cumsum(sel.view(-1), 0, dtype=torch.int32) - 1
    slot = torch.where(sel.view(-1) & (rank < capacity), rank, capacity).long()
    lst = torch.full((capacity + 1,), -1, dtype=torch.int32, device=sel.device)
    lst[slot] = torch.arange(n, dtype=torch.int32, device=sel.device)
    total = rank[-1] + 1
    return lst[:capacity], torch.stack([total, total.clamp(max=capacity)])


def torch_points(torch, lst, geometry, to_ray, pos):
    """positions and normals of the listed pixels from torch ops (list entries that name no pixel give zero rows)"""
    valid = (lst >= 0) & (lst < N)
    k = torch.where(valid, lst, 0).long()
    g = geometry.view(-1, 4)[k]
    p = torch.stack([(k % W).float(), (k // W).float(), torch.ones_like(k, dtype=torch.float32)], dim=-1)
    d = p @ to_ray.T
    d = d / d.norm(dim=-1, keepdim=True)
    t = g[:, 3:4]
    hit = (t <= 99998.0) & valid[:, None]
    n = torch.where((g[:, :3] * d).sum(dim=-1, keepdim=True) > 0, -g[:, :3], g[:, :3])
    zero = torch.zeros_like(d)
    positions = torch.cat([torch.where(hit, pos + d * t, zero), torch.where(valid[:, None], t, zero[:, :1])], dim=-1)
    normals = torch.cat([torch.where(hit, n, zero), zero[:, :1]], dim=-1)
    return positions, normals


def torch_scatter(torch, lst, values, out, state):
    """out[k] = values[j], state[k] = 3 for the entries that name an item; the others go to a spare slot"""
    k = torch.where((lst >= 0) & (lst < N), lst, N).long()
    out[k] = values
    state[k] = 3


def measure(torch, opt, view_name, emit):
    dev = torch.device("cuda", 0)
    lib = _lib.select()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rec = {}

    def leg(call, repeats, prepare=None):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if prepare is not None:
            prepare(repeats)            # outside the timed window
        ev0.record()
        for _ in range(repeats):
            call()
        ev1.record()
        torch.cuda.current_stream().synchronize()
        return ev0.elapsed_time(ev1) / repeats

    def run(legs):
        for f, _, *prepare in legs.values():
            leg(f, 1, *prepare)
        times = {name: [] for name in legs}
        for _ in range(opt.rounds):
            for name, (f, k, *prepare) in legs.items():
                times[name].append(leg(f, k, *prepare))
        return {name: {"median": round(statistics.median(ts), 5), "min": round(min(ts), 5), "max": round(max(ts), 5)} for name, ts in times.items()}

    def copy_leg(nbytes):
        src, dst = torch.empty(max(1, nbytes // 2), dtype=torch.uint8, device=dev), torch.empty(max(1, nbytes // 2), dtype=torch.uint8, device=dev)
        return (lambda: dst.copy_(src), opt.repeats)

    slow = max(1, opt.repeats // 5)
    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get(view_name))
        rec["device"] = s.hip.crt_device_name().decode()
        s.render_raw(WRITE_RAYS)
        rays = s.read_rays()
        _, _, pos = s.camera()
        s.render(gbuffer=True)
        g = s.read_gbuffer_raw()
        geometry = torch.from_numpy(np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1)).to(dev)
        hit = g["geometry"]["t"] <= 99998.0
        rec["hit_share"] = round(float(hit.mean()), 4)
        P, n, _ = ao_ref.frame_items(s.read_gbuffer(), rays, pos)
        box = P[(n != 0).any(axis=1)].astype(np.float64)
        radius = RADIUS_OF_EXTENT * float(np.linalg.norm(box.max(axis=0) - box.min(axis=0)))
        bias = BIAS_OF_RADIUS * radius
        ao_kw = dict(radius=radius, bias=bias)
        cp = _lib.CrtAoParams(AO_SAMPLES, radius, bias, 0, 0, 0.0, 0.0)
        full = np.array(s.ambient_occlusion(AO_SAMPLES, **ao_kw), copy=True)
        cam = _lib.crtt_camera(*s.camera(), W, H)
        to_ray = torch.tensor(list(cam.toRay), device=dev).view(3, 3)
        cam_pos = torch.tensor(list(cam.pos), device=dev)

        def low_route(factor, retrace, capacity=None):
            lh, lw = (H + factor - 1) // factor, (W + factor - 1) // factor
            p, nn = s.frame_points(factor=factor)
            low = s.trace_ao(p[:, :3], nn[:, :3], AO_SAMPLES, **ao_kw).view(lh, lw)
            ao, state = s.upsample(low, factor=factor, return_state=True)
            counts = s.retrace_ao(ao, state, capacity=capacity, samples=AO_SAMPLES, **ao_kw) if retrace else None
            return ao, state, counts

        # ---- the state plane of the factor-2 route, and what the three calls make of it
        _, state, _ = low_route(2, False)
        capacity = (N + 7) // 8
        sel = (state == _lib.CRTU_STATE_NEAREST) | (state == _lib.CRTU_STATE_EMPTY)
        lst, counts = s.select(state, capacity=capacity)
        total = int(counts[0])
        rec["selected"] = {"total": total, "capacity": capacity, "share_of_pixels": round(total / N, 5)}
        if total > capacity:
            raise SystemExit(f"select_rate: {total} selected pixels do not fit the default capacity {capacity}")
        t_lst, t_counts = torch_compact(torch, sel, capacity)
        m_lst, m_counts = s.select(sel, values=(1,), capacity=capacity)
        if not (torch.equal(t_lst, lst) and torch.equal(m_lst, lst) and torch.equal(t_counts.int(), counts) and torch.equal(m_counts, counts)
                and torch.equal(torch.nonzero(sel.view(-1)).view(-1).int(), lst[:total])):
            raise SystemExit("select_rate: crts_compact, the torch composition and torch.nonzero disagree")
        positions, normals = s.frame_points(lst)
        tp, tn = torch_points(torch, lst, geometry, to_ray, cam_pos)
        rec["points_max_abs_diff_to_torch"] = float(max((positions - tp).abs().max(), (normals - tn).abs().max()))
        if not rec["points_max_abs_diff_to_torch"] < 1e-3 * max(1.0, float(positions[:total, :3].abs().max())):
            raise SystemExit(f"select_rate: crts_points differs from the torch composition by {rec['points_max_abs_diff_to_torch']}")
        values = s.trace_ao(positions[:, :3], normals[:, :3], AO_SAMPLES, **ao_kw)
        out_a, out_b = torch.zeros(N + 1, device=dev), torch.zeros(N + 1, device=dev)
        st_a, st_b = torch.zeros(N + 1, dtype=torch.int32, device=dev), torch.zeros(N + 1, dtype=torch.int32, device=dev)
        s.scatter(lst, values, out_a[:N], st_a[:N])
        torch_scatter(torch, lst, values, out_b, st_b)
        if not (torch.equal(out_a[:N], out_b[:N]) and torch.equal(st_a[:N], st_b[:N])):
            raise SystemExit("select_rate: crts_scatter and the torch composition disagree")

        scratch = torch.empty(lib.crts_scratch_bytes(N) // 4, dtype=torch.int32, device=dev)
        l_out, c_out = torch.empty(capacity, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
        p_out, n_out = torch.empty((N // 4, 4), device=dev), torch.empty((N // 4, 4), device=dev)

        def compact(words):
            c = _lib.CrtsCompact(words.data_ptr(), words.element_size(), VALUES if words.element_size() == 4 else 2, N, capacity)
            rc = lib.crts_compact(C.byref(c), l_out.data_ptr(), c_out.data_ptr(), scratch.data_ptr(), stream)
            if rc:
                raise SystemExit(f"select_rate: crts_compact failed with {rc}")

        def points(grid):
            f = _lib.CrtsFrame(W, H, _lib.CRTS_GUIDES_PLANES, geometry.data_ptr(), cam)
            it = _lib.CrtsItems(None, N // 4, 2, 0, 0) if grid else _lib.CrtsItems(lst.data_ptr(), capacity, 1, 0, 0)
            rc = lib.crts_points(C.byref(f), C.byref(it), p_out.data_ptr(), n_out.data_ptr(), None, stream)
            if rc:
                raise SystemExit(f"select_rate: crts_points failed with {rc}")

        def scatter():
            sc = _lib.CrtsScatter(lst.data_ptr(), values.data_ptr(), out_a.data_ptr(), st_a.data_ptr(), capacity, 1, N, 3)
            rc = lib.crts_scatter(C.byref(sc), stream)
            if rc:
                raise SystemExit(f"select_rate: crts_scatter failed with {rc}")

        grid_list = lst.new_tensor(np.arange(N // 4, dtype=np.int64) % (W // 2) * 2 + np.arange(N // 4, dtype=np.int64) // (W // 2) * 2 * W)
        floors = {"compact-words": N * 4 + capacity * 4, "compact-mask": N + capacity * 4, "points-list": capacity * (4 + 16 + 32),
                  "points-grid": (N // 4) * (16 + 32), "scatter": capacity * 16}
        legs = {
            "compact-words": (lambda: compact(state), opt.repeats), "copy-compact-words": copy_leg(floors["compact-words"]),
            "torch-compact-words": (lambda: torch_compact(torch, (state == 1) | (state == 2), capacity), slow),
            "nonzero-words": (lambda: torch.nonzero(((state == 1) | (state == 2)).view(-1)), slow),
            "compact-mask": (lambda: compact(sel), opt.repeats), "copy-compact-mask": copy_leg(floors["compact-mask"]),
            "torch-compact-mask": (lambda: torch_compact(torch, sel, capacity), slow),
            "nonzero-mask": (lambda: torch.nonzero(sel.view(-1)), slow),
            "points-list": (lambda: points(False), opt.repeats), "copy-points-list": copy_leg(floors["points-list"]),
            "torch-points-list": (lambda: torch_points(torch, lst, geometry, to_ray, cam_pos), slow),
            "points-grid": (lambda: points(True), opt.repeats), "copy-points-grid": copy_leg(floors["points-grid"]),
            "torch-points-grid": (lambda: torch_points(torch, grid_list, geometry, to_ray, cam_pos), slow),
            "scatter": (scatter, opt.repeats), "copy-scatter": copy_leg(floors["scatter"]),
            "torch-scatter": (lambda: torch_scatter(torch, lst, values, out_b, st_b), slow),
        }
        rec["floor_bytes"] = floors
        rec["legs_ms"] = run(legs)

        # ---- the routes, end to end, and the cost of the padding
        routes = {}
        for factor in (2, 4):
            for retrace in (False, True):
                ao, st, cnt = low_route(factor, retrace)
                torch.cuda.current_stream().synchronize()
                got, stn = ao.cpu().numpy(), st.cpu().numpy()
                routes[f"f{factor}{'-retrace' if retrace else ''}"] = {
                    "mean_abs_diff": round(float(np.abs(got - full).mean()), 5), "mean_abs_diff_on_hit_pixels": round(float(np.abs(got - full)[hit].mean()), 5),
                    "left_nearest_or_empty": int(((stn == 1) | (stn == 2)).sum()), "retraced": int((stn == 3).sum()),
                    "counts": None if cnt is None else [int(x) for x in cnt.cpu()]}
        route_legs = {"frame_ao": (lambda: _lib.check(s.hip.crt_frame_ao(C.byref(cp), stream), "crt_frame_ao"), slow)}
        for factor in (2, 4):
            route_legs[f"route-f{factor}"] = (lambda f=factor: low_route(f, False), slow)
            route_legs[f"route-f{factor}-retrace"] = (lambda f=factor: low_route(f, True), slow)
        # retrace_ao marks what it patched, so every call needs a state plane of its own: the copies are made before the clock starts
        fresh = []
        route_legs["retrace-alone"] = (lambda: s.retrace_ao(out_a[:N].view(H, W), fresh.pop(), samples=AO_SAMPLES, **ao_kw), slow,
                                       lambda k: fresh.extend(state.clone() for _ in range(k)))
        route_legs["trace_ao-capacity"] = (lambda: s.trace_ao(positions[:, :3], normals[:, :3], AO_SAMPLES, **ao_kw), slow)
        exact_p, exact_n = positions[:max(2, total)].clone(), normals[:max(2, total)].clone()
        route_legs["trace_ao-total"] = (lambda: s.trace_ao(exact_p[:, :3], exact_n[:, :3], AO_SAMPLES, **ao_kw), slow)
        rec["routes"] = routes
        rec["route_legs_ms"] = run(route_legs)
        rec["ao"] = {"radius": round(radius, 4), "samples": AO_SAMPLES}

    fmt = lambda r: f"{r['median']:8.4f} ms ({r['min']:.4f} .. {r['max']:.4f})"
    L, R = rec["legs_ms"], rec["route_legs_ms"]
    emit(f"== {view_name}: {rec['hit_share']:.1%} of the pixels are hits; {rec['device']}; the state plane of AO at every 2nd pixel selects {total} of {N} pixels "
         f"({total / N:.3%}); capacity {capacity}")
    for key, what in (("compact-words", "crts_compact, state words"), ("compact-mask", "crts_compact, bool mask")):
        emit(f"  {what} ({floors[key] / 1e6:.1f} MB floor): {fmt(L[key])}; copy {fmt(L['copy-' + key])} ({L[key]['median'] / L['copy-' + key]['median']:.2f} x copy); "
             f"torch cumsum + where + index write {fmt(L['torch-' + key])} (torch / fused {L['torch-' + key]['median'] / L[key]['median']:.1f}); "
             f"torch.nonzero (waits on the host) {fmt(L['nonzero-' + key.split('-')[1]])}")
    for key, what in (("points-list", f"crts_points, the list of {capacity}"), ("points-grid", f"crts_points, the grid of factor 2 ({N // 4} items)"),
                      ("scatter", f"crts_scatter, 1 channel + state, {capacity} entries")):
        emit(f"  {what} ({floors[key] / 1e6:.1f} MB floor): {fmt(L[key])}; copy {fmt(L['copy-' + key])} ({L[key]['median'] / L['copy-' + key]['median']:.2f} x copy); "
             f"torch ops {fmt(L['torch-' + key])} (torch / fused {L['torch-' + key]['median'] / L[key]['median']:.1f})")
    emit(f"  ambient occlusion, {AO_SAMPLES} samples, radius {radius:.4f}: crt_frame_ao on the full frame {fmt(R['frame_ao'])}")
    for factor in (2, 4):
        a, b = routes[f"f{factor}"], routes[f"f{factor}-retrace"]
        emit(f"  every {'2nd' if factor == 2 else '4th'} pixel: frame_points + trace_ao + upsample {fmt(R[f'route-f{factor}'])} = "
             f"{R['frame_ao']['median'] / R[f'route-f{factor}']['median']:.2f} x faster than the full frame, {a['left_nearest_or_empty']} pixels NEAREST or EMPTY, mean absolute "
             f"difference {a['mean_abs_diff']} ({a['mean_abs_diff_on_hit_pixels']} over the hit pixels); + retrace_ao {fmt(R[f'route-f{factor}-retrace'])} = "
             f"{R['frame_ao']['median'] / R[f'route-f{factor}-retrace']['median']:.2f} x faster, counts {b['counts']}, {b['left_nearest_or_empty']} left, mean absolute difference "
             f"{b['mean_abs_diff']} ({b['mean_abs_diff_on_hit_pixels']})")
    emit(f"  retrace_ao alone (select + frame_points + trace_ao + scatter, capacity {capacity}): {fmt(R['retrace-alone'])}")
    emit(f"  the padding: trace_ao on {capacity} items of which {total} trace {fmt(R['trace_ao-capacity'])}; on {max(2, total)} items alone {fmt(R['trace_ao-total'])}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=100, help="calls per timed leg (a fifth as many of the torch compositions and the routes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_rate.txt"))
    ap.add_argument("--views", default="multi-1M,multi-1M-dense")
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("select_rate: no GPU (this tool measures; it does not fall back)")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"selective re-tracing (crts_compact, crts_points, crts_scatter) on {W}x{H} G-buffer frames of multi-1M; events on the stream, "
         f"median of {opt.rounds} alternating rounds of {opt.repeats} calls (min .. max); x copy = times the device copy of as many bytes (the floor)")
    result = {"metric": "select_rate", "frame": f"{W}x{H}", "rounds": opt.rounds, "repeats": opt.repeats,
              "views": {v: measure(torch, opt, v, emit) for v in opt.views.split(",")}}
    emit(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
