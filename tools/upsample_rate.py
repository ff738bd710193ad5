#!/usr/bin/env python3
"""Rate of the guided upsample (libcrt_upsample.so) on 1920x1080 G-buffer frames of multi-1M: the headline camera (a third of the
pixels are hits) and the dense camera (nearly all are). The low image is the frame's colour (4 channels) or luminance (1 channel) at every F-th
pixel under seeded noise.

    fused        ms of crtu_upsample for factors 2 and 4, 1 and 4 channels, without flags, with the taps through L1 (CRTU_TAPS=l1) and from LDS
                 (=lds), guided by the planes (the copy's and the torch composition's counterpart) and by CrtSurfaceHit records; with 4 channels also as a caller would run it (CRTU_MATCH_INSTANCE | CRTU_MODULATE), guided by the planes and by
                 CrtSurfaceHit records, in both tap forms
    copy         torch's device-to-device copy of half the bytes the call must move -- per pixel the guide (16 B) read, the result (4 B per
                 channel) and the state word (4 B) written, per low sample its value read -- so that the copy moves as many: the call's floor
    torch        the same definition composed from torch ops (no instance match), what a caller of the API had before; checked against the fused
                 result before anything is timed
    AO route     what the library exists for: crt_trace_ao on the point and normal of every F-th pixel followed by crtu_upsample of its answer,
                 against crt_frame_ao on the full frame at the same sample count, with the mean absolute difference of the two AO planes. The
                 points and normals of the sampled pixels are gathered once, outside the timed window.

Every leg is timed with events on the stream around `--repeats` back-to-back calls (a tenth as many for the torch composition); the legs alternate
for `--rounds` rounds after a warm-up of each; the median round is reported with min .. max. Needs a GPU: there is no fallback.

    python tools/upsample_rate.py [--rounds R] [--repeats K] [--out profiles/upsample_rate.txt]
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
DEPTH_TOL, NORMAL_COS = 0.05, 0.9
AO_SAMPLES, BIAS_OF_RADIUS, RADIUS_OF_EXTENT = 8, 1e-3, 0.1     # tools/ao_rate.py's
WRITE_RAYS = 2
ENV = "CRTU_TAPS"


def low_size(factor, offset=(0, 0)):
    return (W - offset[0] + factor - 1) // factor, (H - offset[1] + factor - 1) // factor


def torch_upsample(torch, low, geometry, factor, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS):
    """the definition of include/crt_upsample.h in torch ops (offset 0, no flags): what the fused call replaces. Returns (out, state)."""
    n, t = geometry[..., :3], geometry[..., 3]
    h, w = t.shape
    lh, lw = low.shape[:2]
    v = low.reshape(lh, lw, -1)
    dev = t.device
    hit = t <= 99998.0
    yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    X0, Y0 = xx // factor, yy // factor
    fx, fy = (xx - X0 * factor).float() / factor, (yy - Y0 * factor).float() / factor
    weights = ((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy)
    dtol = depth_tol * t
    total, wsum = torch.zeros((h, w, v.shape[2]), device=dev), torch.zeros((h, w), device=dev)
    counted = torch.zeros((h, w), dtype=torch.bool, device=dev)
    any_near, any_first = counted.clone(), counted.clone()
    best = torch.zeros((h, w), device=dev)
    nearest, first = torch.zeros_like(total), torch.zeros_like(total)
    for k in range(4):
        X, Y = X0 + (k & 1), Y0 + (k >> 1)
        exists = (X < lw) & (Y < lh)
        Xc, Yc = X.clamp(max=lw - 1), Y.clamp(max=lh - 1)
        vq = v[Yc, Xc]
        tg, ng = t[factor * Yc, factor * Xc], n[factor * Yc, factor * Xc]
        b = weights[k]
        cand = exists & torch.isfinite(vq).all(dim=-1)
        hg = tg <= 99998.0
        d = (tg - t).abs()
        stops = hg & (d <= dtol) & (((ng[..., 0] * n[..., 0] + ng[..., 1] * n[..., 1]) + ng[..., 2] * n[..., 2]) >= normal_cos)
        ok = cand & (b > 0) & torch.where(hit, stops, ~hg)
        total = torch.where(ok[..., None], total + vq * b[..., None], total)
        wsum = torch.where(ok, wsum + b, wsum)
        counted |= ok
        near = cand & hit & hg & ~torch.isnan(d)
        take = near & (~any_near | (d < best))
        nearest, best = torch.where(take[..., None], vq, nearest), torch.where(take, d, best)
        any_near |= near
        first = torch.where((cand & ~any_first)[..., None], vq, first)
        any_first |= cand
    out = torch.where(counted[..., None], total / wsum[..., None], torch.where(any_near[..., None], nearest, first))
    state = torch.where(counted, 0, torch.where(any_first, 1, 2)).to(torch.int32)
    return out.reshape((h, w) + tuple(low.shape[2:])), state


def measure(torch, opt, view_name, emit):
    """every leg on one view; prints through emit() and returns the view's record"""
    dev = torch.device("cuda", 0)
    lib = _lib.upsample()
    os.environ.pop(ENV, None)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rec = {}

    def leg(call, repeats):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(repeats):
            call()
        ev1.record()
        torch.cuda.current_stream().synchronize()
        return ev0.elapsed_time(ev1) / repeats

    def run(legs):
        """legs: name -> (call, repeats); warm-up of each, then alternating rounds"""
        for f, _ in legs.values():
            f()
        torch.cuda.current_stream().synchronize()
        times = {name: [] for name in legs}
        for _ in range(opt.rounds):
            for name, (f, k) in legs.items():
                times[name].append(leg(f, k))
        return {name: {"median": round(statistics.median(ts), 5), "min": round(min(ts), 5), "max": round(max(ts), 5)} for name, ts in times.items()}

    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get(view_name))
        rec["device"] = s.hip.crt_device_name().decode()
        s.render_raw(WRITE_RAYS)
        rays = s.read_rays()
        _, _, pos = s.camera()
        hits = s.shade_rays(torch.from_numpy(np.asarray(pos, np.float32)).to(dev), torch.from_numpy(rays.reshape(-1, 3)).to(dev), radiance=False, surface=True)
        s.render(gbuffer=True)
        frame = s.read_output()
        g = s.read_gbuffer_raw()
        geometry = torch.from_numpy(np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1)).to(dev)
        ids = torch.from_numpy(g["ids"].view(np.int32).reshape(H, W, 4).copy()).to(dev)
        albedo = torch.from_numpy(g["albedo"].view(np.int32).copy()).to(dev)
        hit = g["geometry"]["t"] <= 99998.0
        rec["hit_share"] = round(float(hit.mean()), 4)
        rng = np.random.RandomState(7)
        noisy = (frame + rng.normal(0, 0.2, frame.shape) * np.array([1, 1, 1, 0])).astype(np.float32)
        luma = ((0.299 * noisy[..., 0] + 0.587 * noisy[..., 1]) + 0.114 * noisy[..., 2]).astype(np.float32)
        lows = {(f, c): torch.from_numpy(np.ascontiguousarray((noisy if c == 4 else luma)[::f, ::f])).to(dev) for f in (2, 4) for c in (1, 4)}
        outs = {1: torch.empty((H, W), device=dev), 4: torch.empty((H, W, 4), device=dev)}
        state = torch.empty((H, W), dtype=torch.int32, device=dev)

        def fused(factor, channels, flags=0, surface=False, low=None, out=None, want_state=True):
            f = _lib.CrtuFrame(W, H, _lib.CRTU_GUIDES_SURFACE if surface else _lib.CRTU_GUIDES_PLANES,
                               hits.records.data_ptr() if surface else geometry.data_ptr(), None if surface else ids.data_ptr(), None if surface else albedo.data_ptr())
            l = _lib.CrtuLow((lows[(factor, channels)] if low is None else low).data_ptr(), channels, factor, 0, 0)
            p = _lib.CrtuParams(flags, DEPTH_TOL, NORMAL_COS)
            rc = lib.crtu_upsample(C.byref(f), C.byref(l), C.byref(p), (outs[channels] if out is None else out).data_ptr(),
                                   state.data_ptr() if want_state else None, stream)
            if rc:
                raise SystemExit(f"upsample_rate: crtu_upsample failed with {rc}: {lib.crtu_error_string(rc).decode()}")

        def with_env(value, call):
            def run_():
                if value is None:
                    os.environ.pop(ENV, None)
                else:
                    os.environ[ENV] = value
                call()
                os.environ.pop(ENV, None)
            return run_

        # the tap forms, the guide layouts and the torch composition agree before any is timed (torch rounds a division differently: the
        # largest difference is reported)
        agreement = {}
        for factor in (2, 4):
            for channels in (1, 4):
                res = []
                for taps, surface in (("l1", False), ("lds", False), ("lds", True)):
                    with_env(taps, lambda: fused(factor, channels, surface=surface))()
                    res.append((outs[channels].clone(), state.clone()))
                if not all(torch.equal(a.view(torch.int32), res[0][0].view(torch.int32)) and torch.equal(b, res[0][1]) for a, b in res[1:]):
                    raise SystemExit("upsample_rate: the tap forms or the guide layouts give different bits")
                b, bs = torch_upsample(torch, lows[(factor, channels)], geometry, factor)
                a, as_ = res[0]
                diff = float((a - b).abs().max())
                other = (a.view(torch.int32) != b.view(torch.int32))
                agreement[f"factor {factor}, {channels} ch"] = {
                    "max_abs_diff": diff, "pixels_with_other_bits": int((other.any(dim=-1) if other.dim() == 3 else other).sum()),
                    "pixels_with_other_state": int((as_ != bs).sum()),
                    "not_interpolated_share_of_hit_pixels": round(float((as_ != 0).sum()) / max(1, int(hit.sum())), 4)}
                if not (diff < 1e-5 and int((as_ != bs).sum()) == 0):
                    raise SystemExit(f"upsample_rate: the fused result differs from the torch composition by {diff} at factor {factor}, {channels} channels")
        rec["agreement_with_torch"] = agreement

        legs, floors = {}, {}
        slow = max(1, opt.repeats // 10)
        for factor in (2, 4):
            lw, lh = low_size(factor)
            for channels in (1, 4):
                key = f"f{factor}-c{channels}"
                floors[key] = W * H * (16 + 4 * channels + 4) + lw * lh * 4 * channels
                src, dst = torch.empty(floors[key] // 2, dtype=torch.uint8, device=dev), torch.empty(floors[key] // 2, dtype=torch.uint8, device=dev)
                legs[f"copy-{key}"] = (lambda src=src, dst=dst: dst.copy_(src), opt.repeats)
                for taps in ("l1", "lds"):
                    legs[f"{taps}-{key}"] = (with_env(taps, lambda f=factor, c=channels: fused(f, c)), opt.repeats)
                    legs[f"surface-{taps}-{key}"] = (with_env(taps, lambda f=factor, c=channels: fused(f, c, surface=True)), opt.repeats)
                legs[f"torch-{key}"] = (lambda f=factor, c=channels: torch_upsample(torch, lows[(f, c)], geometry, f), slow)
            both = _lib.CRTU_MATCH_INSTANCE | _lib.CRTU_MODULATE
            for taps in ("l1", "lds"):
                legs[f"planes-flags-{taps}-f{factor}-c4"] = (with_env(taps, lambda f=factor: fused(f, 4, both)), opt.repeats)
                legs[f"surface-flags-{taps}-f{factor}-c4"] = (with_env(taps, lambda f=factor: fused(f, 4, both, surface=True)), opt.repeats)
        rec["floor_bytes"] = floors
        rec["legs_ms"] = run(legs)

        # ---- the route the library exists for: AO at every F-th pixel and the upsample, against AO of the full frame
        P, n, _ = ao_ref.frame_items(s.read_gbuffer(), rays, pos)
        traces = (n != 0).any(axis=1)
        box = P[traces].astype(np.float64)
        extent = float(np.linalg.norm(box.max(axis=0) - box.min(axis=0)))
        radius = RADIUS_OF_EXTENT * extent
        bias = BIAS_OF_RADIUS * radius
        cp = _lib.CrtAoParams(AO_SAMPLES, radius, bias, 0, 0, 0.0, 0.0)
        full = np.array(s.ambient_occlusion(AO_SAMPLES, radius=radius, bias=bias), copy=True)
        ao = {"radius": round(radius, 4), "samples": AO_SAMPLES, "mean_ao_full": round(float(full.mean()), 4)}
        P, n = P.reshape(H, W, 3), n.reshape(H, W, 3)
        pts = {f: (torch.from_numpy(np.ascontiguousarray(P[::f, ::f].reshape(-1, 3))).to(dev), torch.from_numpy(np.ascontiguousarray(n[::f, ::f].reshape(-1, 3))).to(dev))
               for f in (2, 4)}
        up = torch.empty((H, W), device=dev)

        def route(factor):
            lw, lh = low_size(factor)
            low = s.trace_ao(pts[factor][0], pts[factor][1], AO_SAMPLES, radius=radius, bias=bias)
            fused(factor, 1, low=low.reshape(lh, lw), out=up, want_state=True)

        ao_legs = {"frame_ao": (lambda: _lib.check(s.hip.crt_frame_ao(C.byref(cp), stream), "crt_frame_ao"), max(1, opt.repeats // 5))}
        for factor in (2, 4):
            ao_legs[f"route-f{factor}"] = (lambda f=factor: route(f), max(1, opt.repeats // 5))
            ao_legs[f"trace_ao-f{factor}"] = (lambda f=factor: s.trace_ao(pts[f][0], pts[f][1], AO_SAMPLES, radius=radius, bias=bias), max(1, opt.repeats // 5))
        for factor in (2, 4):
            route(factor)
            torch.cuda.current_stream().synchronize()
            got = up.cpu().numpy()
            st = state.cpu().numpy()
            ao[f"factor {factor}"] = {"mean_abs_diff": round(float(np.abs(got - full).mean()), 5), "mean_abs_diff_on_hit_pixels": round(float(np.abs(got - full)[hit].mean()), 5),
                                      "mean_ao": round(float(got.mean()), 4), "not_interpolated_share_of_hit_pixels": round(float((st != 0).sum()) / max(1, int(hit.sum())), 4)}
        ao["legs_ms"] = run(ao_legs)
        rec["ao_route"] = ao

    fmt = lambda r: f"{r['median']:8.4f} ms ({r['min']:.4f} .. {r['max']:.4f})"
    L = rec["legs_ms"]
    emit(f"== {view_name}: {rec['hit_share']:.1%} of the pixels are hits; {rec['device']}")
    emit("fused against the torch composition, no flags: " + "; ".join(
        f"{k}: largest difference {a['max_abs_diff']:.3g}, {a['pixels_with_other_bits']} pixels with other bits, {a['not_interpolated_share_of_hit_pixels']:.2%} of the hit "
        f"pixels' worth not interpolated" for k, a in agreement.items()))
    emit("no flags, outState written; x copy = times the copy of as many bytes (the floor); torch / fused of the medians, against the faster tap form:")
    for factor in (2, 4):
        for channels in (1, 4):
            key = f"f{factor}-c{channels}"
            c, l1, lds, t = (L[f"{k}-{key}"] for k in ("copy", "l1", "lds", "torch"))
            fast = min(l1["median"], lds["median"])
            emit(f"  factor {factor}, {channels} ch ({floors[key] / 1e6:.1f} MB moved): copy {fmt(c)} = {floors[key] / c['median'] * 1e-9:.2f} TB/s; taps through L1 {fmt(l1)} "
                 f"({l1['median'] / c['median']:.2f} x copy); from LDS {fmt(lds)} ({lds['median'] / c['median']:.2f} x copy); torch ops {fmt(t)}; torch / fused {t['median'] / fast:.0f}; "
                 f"guided by surface records: through L1 {fmt(L[f'surface-l1-{key}'])}; from LDS {fmt(L[f'surface-lds-{key}'])}")
    emit("4 channels with CRTU_MATCH_INSTANCE | CRTU_MODULATE, outState written, by guide layout and tap form:")
    for factor in (2, 4):
        emit(f"  factor {factor}: planes, through L1 {fmt(L[f'planes-flags-l1-f{factor}-c4'])}; planes, from LDS {fmt(L[f'planes-flags-lds-f{factor}-c4'])}; "
             f"surface records, through L1 {fmt(L[f'surface-flags-l1-f{factor}-c4'])}; surface records, from LDS {fmt(L[f'surface-flags-lds-f{factor}-c4'])}")
    A = ao["legs_ms"]
    emit(f"ambient occlusion, {AO_SAMPLES} samples, radius {ao['radius']}: crt_frame_ao on the full frame {fmt(A['frame_ao'])}, mean AO {ao['mean_ao_full']}")
    for factor in (2, 4):
        r = ao[f"factor {factor}"]
        emit(f"  every {'2nd' if factor == 2 else '4th'} pixel: crt_trace_ao {fmt(A[f'trace_ao-f{factor}'])}; crt_trace_ao + crtu_upsample {fmt(A[f'route-f{factor}'])} = "
             f"{A['frame_ao']['median'] / A[f'route-f{factor}']['median']:.2f} x faster than the full frame; mean absolute difference of the AO planes "
             f"{r['mean_abs_diff']} ({r['mean_abs_diff_on_hit_pixels']} over the hit pixels), mean AO {r['mean_ao']}, "
             f"{r['not_interpolated_share_of_hit_pixels']:.2%} of the hit pixels' worth not interpolated")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=200, help="calls per timed leg (a tenth as many of the torch composition, a fifth of the AO legs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_rate.txt"))
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("upsample_rate: no GPU (this tool measures; it does not fall back)")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"guided upsample (crtu_upsample) on {W}x{H} G-buffer frames of multi-1M, low image = the noisy frame at every F-th pixel; events on the stream, "
         f"median of {opt.rounds} alternating rounds of {opt.repeats} calls (min .. max)")
    result = {"metric": "upsample_rate", "frame": f"{W}x{H}", "rounds": opt.rounds, "repeats": opt.repeats,
              "views": {view_name: measure(torch, opt, view_name, emit) for view_name in ("multi-1M", "multi-1M-dense")}}
    emit(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
