#!/usr/bin/env python3
"""Rate of the variance-guided a-trous filter (libcrt_vfilter.so) on 1920x1080 G-buffer frames of multi-1M: the headline camera (a
third of the pixels are hits; a pixel of sky is copied) and the dense camera (nearly all are). The colour and the moments plane are what five
crtt_accumulate calls leave of the frame under seeded noise (N = 5 on every hit pixel: the temporal estimate under the default minHistory).

    per step     ms of one pass at steps 2..16, without flags: the call of n passes minus the call of n - 1, with the taps through L1 / L2
                 (CRTV_STAGE_MAX_STEP=0) and, for steps 2 and 4, from LDS (=4); the call of one pass (the estimate and step 1) in both forms
    estimate     the call of one pass with the estimate's taps through L1 / L2 and from LDS (CRTV_ESTIMATE_TAPS), under the temporal estimate (no
                 pixel needs the taps) and with minHistory above every N (every hit pixel does)
    whole call   ms of crtv_filter for 1..5 passes with CRTV_DEMODULATE, guided by the planes and by CrtSurfaceHit records, as shipped
    torch        the same definition composed from torch ops, what a caller of the API had before (checked against the fused result before
                 anything is timed)
    crtd         crtd_denoise with CRTD_DEMODULATE at the same pass count on the same colour and guides, in the same run
    copy         torch's device-to-device copy of a buffer of 24 B per pixel (48 B moved per pixel: one pass's compulsory traffic -- the working
                 image and the geometry read, the working image written)

Every leg is timed with events on the stream around `--repeats` back-to-back calls; the legs alternate for `--rounds` rounds after a warm-up of
each; the median round is reported with min .. max. Needs a GPU: there is no fallback.

    python tools/vfilter_rate.py [--rounds R] [--repeats K] [--out profiles/vfilter_rate.txt]
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
from clraytracer_amd import _lib, driver, scenes

W, H = 1920, 1080
DEPTH_TOL, NORMAL_COS, LUMA_SIGMA, LUMA_FLOOR, MIN_HISTORY = 0.05, 0.9, 4.0, 1e-4, 4.0
K = (0.375, 0.25, 0.0625)
G = (0.25, 0.125, 0.0625)
WRITE_RAYS = 2
FRAMES = 5            # N = 5 on every hit pixel (to within rounding): above the default minHistory of 4
ENV = ("CRTV_STAGE_MAX_STEP", "CRTV_ESTIMATE_TAPS")


def padded(torch, a, pad, fill):
    h, w = a.shape[:2]
    p = torch.full((h + 2 * pad, w + 2 * pad) + tuple(a.shape[2:]), fill, dtype=a.dtype, device=a.device)
    p[pad:pad + h, pad:pad + w] = a
    return p


def torch_filter(torch, color, moments, geometry, albedo, iterations, demodulate, min_history=MIN_HISTORY, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS,
                 luma_sigma=LUMA_SIGMA, luma_floor=LUMA_FLOOR):
    """the definition of include/crt_vfilter.h in torch ops (no instance match): what the fused call replaces. Returns (out, variance)."""
    n, t = geometry[..., :3], geometry[..., 3]
    h, w = t.shape
    hit = t <= 99998.0
    zero, one = torch.zeros_like(t), torch.ones_like(t)
    luma = lambda c: (0.299 * c[..., 0] + 0.587 * c[..., 1]) + 0.114 * c[..., 2]

    def stops(tp, np_, pad, oy, ox, s):
        ys, xs = slice(pad + oy, pad + oy + h), slice(pad + ox, pad + ox + w)
        tq, nq = tp[ys, xs], np_[ys, xs]
        return (tq <= 99998.0) & ((tq - t).abs() <= (depth_tol * t) * float(s)) & (((nq[..., 0] * n[..., 0] + nq[..., 1] * n[..., 1]) + nq[..., 2] * n[..., 2]) >= normal_cos)

    # ---- the estimate
    m1, m2, N, mv = moments.unbind(-1)
    var_t = torch.where(mv >= 0, mv, zero)
    tp, np_, mp = padded(torch, t, 3, 99999.0), padded(torch, n, 3, 0.0), padded(torch, moments[..., :2], 3, 0.0)
    S1, S2, cnt = zero, zero, zero
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            mq = mp[3 + dy:3 + dy + h, 3 + dx:3 + dx + w]
            ok = torch.ones_like(hit) if dx == 0 and dy == 0 else stops(tp, np_, 3, dy, dx, 1) & torch.isfinite(mq[..., 0]) & torch.isfinite(mq[..., 1])
            S1, S2, cnt = torch.where(ok, S1 + mq[..., 0], S1), torch.where(ok, S2 + mq[..., 1], S2), torch.where(ok, cnt + 1.0, cnt)
    a = S1 / cnt
    v = S2 / cnt - a * a
    var_s = torch.where(v > 0, v, zero) * (4.0 / torch.fmax(N, one))
    var = torch.where(hit, torch.where(N >= min_history, var_t, var_s), zero)
    rgb = color[..., :3]
    den = torch.ones_like(rgb)
    if demodulate:
        b = torch.stack([(albedo >> sh) & 255 for sh in (0, 8, 16)], dim=-1).to(torch.float32)
        den = torch.where(b == 0, torch.ones_like(b), b / 255.0)
    ld = luma(den)
    if demodulate:
        rgb = torch.where(hit[..., None], rgb / den, rgb)
        var = torch.where(hit, var / (ld * ld), var)
    # ---- the passes
    for p in range(iterations):
        s = 1 << p
        pad = 2 * s
        tp, np_ = padded(torch, t, pad, 99999.0), padded(torch, n, pad, 0.0)
        Ip, vp = padded(torch, rgb, pad, 0.0), padded(torch, var, pad, 0.0)
        gsum, gw = zero, zero
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ys, xs = slice(pad + dy, pad + dy + h), slice(pad + dx, pad + dx + w)
                ok = (tp[ys, xs] <= 99998.0) & (vp[ys, xs] >= 0)
                g = G[abs(dy)] * G[abs(dx)]
                gsum, gw = torch.where(ok, gsum + vp[ys, xs] * g, gsum), torch.where(ok, gw + g, gw)
        sd = luma_sigma * torch.sqrt(torch.where(gw > 0, gsum / gw, zero)) + luma_floor
        L = luma(rgb)
        Lp = padded(torch, L, pad, 0.0)
        total, vsum, wsum = torch.zeros_like(rgb), zero, zero
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ys, xs = slice(pad + dy * s, pad + dy * s + h), slice(pad + dx * s, pad + dx * s + w)
                k = K[abs(dy)] * K[abs(dx)]
                if dx == 0 and dy == 0:
                    ok, wt = torch.ones_like(hit), torch.full_like(t, k)
                else:
                    xl = (Lp[ys, xs] - L).abs() / sd
                    ok = stops(tp, np_, pad, dy * s, dx * s, s) & (vp[ys, xs] >= 0) & (xl < 1)
                    wt = k * ((1 - xl) * (1 - xl))
                total = torch.where(ok[..., None], total + Ip[ys, xs] * wt[..., None], total)
                vsum, wsum = torch.where(ok, vsum + vp[ys, xs] * (wt * wt), vsum), torch.where(ok, wsum + wt, wsum)
        rgb = torch.where(hit[..., None], total / wsum[..., None], rgb)
        var = torch.where(hit, vsum / (wsum * wsum), var)
    out = torch.cat([torch.where(hit[..., None], rgb * den, color[..., :3]), color[..., 3:]], dim=-1)
    return out, torch.where(hit, var * (ld * ld), zero)


def measure(torch, opt, view_name, emit):
    """every leg on one view; prints through emit() and returns the view's record"""
    dev = torch.device("cuda", 0)
    lib, dlib = _lib.vfilter(), _lib.denoise()
    for e in ENV:
        os.environ.pop(e, None)
    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get(view_name))
        device_name = s.hip.crt_device_name().decode()
        s.render_raw(WRITE_RAYS)
        dirs = torch.from_numpy(s.read_rays().reshape(-1, 3)).to(dev)
        _, _, pos = s.camera()
        hits = s.shade_rays(torch.from_numpy(np.asarray(pos, np.float32)).to(dev), dirs, radiance=False, surface=True)
        s.render(gbuffer=True)
        frame = s.read_output()
        g = s.read_gbuffer_raw()
        hist = driver.TemporalHistory(s)
        for k in range(FRAMES):
            noisy = (frame + np.random.RandomState(1 + k).normal(0, 0.2, frame.shape) * np.array([1, 1, 1, 0])).astype(np.float32)
            c, m = s.accumulate(hist, torch.from_numpy(noisy).to(dev))
        color, moments = c.clone(), m.clone()
        geometry = torch.from_numpy(np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1)).to(dev)
        ids = torch.from_numpy(g["ids"].view(np.int32).reshape(H, W, 4).copy()).to(dev)
        albedo = torch.from_numpy(g["albedo"].astype(np.int64)).to(dev)                      # int64 for torch's shifts; the fused call reads the uint32 plane
        albedo32 = torch.from_numpy(g["albedo"].view(np.int32).copy()).to(dev)
        hit = g["geometry"]["t"] <= 99998.0
        hit_share = float(hit.mean())
        N = moments[..., 2].cpu().numpy()[hit]
        history, below = float(N.min()), float((N < MIN_HISTORY).mean())
    out, scratch, variance = torch.empty((H, W, 4), device=dev), torch.empty((H, W, 4), device=dev), torch.empty((H, W), device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fused(iterations, flags, surface=False, min_history=MIN_HISTORY):
        f = _lib.CrtvFrame(W, H, color.data_ptr(), moments.data_ptr(), _lib.CRTV_GUIDES_SURFACE if surface else _lib.CRTV_GUIDES_PLANES,
                           hits.records.data_ptr() if surface else geometry.data_ptr(), None if surface else ids.data_ptr(), None if surface else albedo32.data_ptr())
        p = _lib.CrtvParams(iterations, flags, DEPTH_TOL, NORMAL_COS, LUMA_SIGMA, LUMA_FLOOR, min_history)
        rc = lib.crtv_filter(C.byref(f), C.byref(p), out.data_ptr(), variance.data_ptr(), scratch.data_ptr(), stream)
        if rc:
            raise SystemExit(f"vfilter_rate: crtv_filter failed with {rc}: {lib.crtv_error_string(rc).decode()}")

    def crtd(iterations):
        f = _lib.CrtdFrame(W, H, color.data_ptr(), _lib.CRTD_GUIDES_PLANES, geometry.data_ptr(), ids.data_ptr(), albedo32.data_ptr())
        p = _lib.CrtdParams(iterations, _lib.CRTD_DEMODULATE, DEPTH_TOL, NORMAL_COS, 0.0)
        rc = dlib.crtd_denoise(C.byref(f), C.byref(p), out.data_ptr(), scratch.data_ptr(), stream)
        if rc:
            raise SystemExit(f"vfilter_rate: crtd_denoise failed with {rc}: {dlib.crtd_error_string(rc).decode()}")

    # the fused call and the torch composition agree before either is timed (torch rounds a division differently: the largest difference is reported)
    agreement = {}
    for n, mh in ((1, MIN_HISTORY), (4, MIN_HISTORY), (2, float("inf"))):
        fused(n, _lib.CRTV_DEMODULATE, min_history=mh)
        a, av = out.clone(), variance.clone()
        fused(n, _lib.CRTV_DEMODULATE, surface=True, min_history=mh)
        b, bv = torch_filter(torch, color, moments, geometry, albedo, n, True, min_history=mh)
        if not (torch.equal(a.view(torch.int32), out.view(torch.int32)) and torch.equal(av.view(torch.int32), variance.view(torch.int32))):
            raise SystemExit("vfilter_rate: the two guide layouts give different bits")
        # relative to the largest value of each image: differences of an ulp per operation, carried through the passes
        diff = float((a - b).abs().nan_to_num(0.0).max() / max(1.0, float(b.abs().nan_to_num(0.0, posinf=0.0).max())))
        vdiff = float((av - bv).abs().nan_to_num(0.0).max() / max(1.0, float(bv.abs().nan_to_num(0.0, posinf=0.0).max())))
        agreement[f"{n} pass(es), {'spatial' if mh > MIN_HISTORY else 'temporal'} estimate"] = {
            "max_abs_diff": diff, "max_abs_diff_variance": vdiff, "pixels_with_other_bits": int((a.view(torch.int32) != b.view(torch.int32)).any(dim=-1).sum())}
        if not (diff < 1e-4 and vdiff < 1e-4):
            raise SystemExit(f"vfilter_rate: the fused result differs from the torch composition by {diff} (variance {vdiff}) at {n} passes")

    def leg(call):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(opt.repeats):
            call()
        ev1.record()
        torch.cuda.current_stream().synchronize()
        return ev0.elapsed_time(ev1) / opt.repeats

    def with_env(values, call):
        def run():
            for e in ENV:
                os.environ.pop(e, None)
            os.environ.update(values)
            call()
            for e in ENV:
                os.environ.pop(e, None)
        return run

    src24, dst24 = torch.empty((H, W, 6), device=dev), torch.empty((H, W, 6), device=dev)
    legs = {"copy24": lambda: dst24.copy_(src24)}
    for taps in ("l1", "lds"):
        legs[f"estimate-{taps}-temporal"] = with_env({"CRTV_ESTIMATE_TAPS": taps}, lambda: fused(1, 0))
        legs[f"estimate-{taps}-spatial"] = with_env({"CRTV_ESTIMATE_TAPS": taps}, lambda: fused(1, 0, min_history=float("inf")))
    for n in range(1, 6):
        legs[f"direct-{n}"] = with_env({"CRTV_STAGE_MAX_STEP": "0"}, lambda n=n: fused(n, 0))
        legs[f"staged-{n}"] = with_env({"CRTV_STAGE_MAX_STEP": "4"}, lambda n=n: fused(n, 0))
        legs[f"planes-{n}"] = with_env({}, lambda n=n: fused(n, _lib.CRTV_DEMODULATE))
        legs[f"surface-{n}"] = with_env({}, lambda n=n: fused(n, _lib.CRTV_DEMODULATE, surface=True))
        legs[f"crtd-{n}"] = lambda n=n: crtd(n)
        legs[f"torch-{n}"] = lambda n=n: torch_filter(torch, color, moments, geometry, albedo, n, True)
    for f in legs.values():
        leg(f)
    times = {name: [] for name in legs}
    for _ in range(opt.rounds):
        for name, f in legs.items():
            times[name].append(leg(f))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    rec = {"device": device_name, "hit_share": round(hit_share, 4), "least_N_on_a_hit_pixel": history, "share_of_hit_pixels_below_min_history": below, "agreement_with_torch": agreement,
           "legs_ms": {name: {"median": round(med[name], 4), "min": round(min(ts), 4), "max": round(max(ts), 4)} for name, ts in times.items()}}
    fmt = lambda r: f"{r['median']:8.4f} ms ({r['min']:.4f} .. {r['max']:.4f})"
    emit(f"== {view_name}: {hit_share:.1%} of the pixels are hits, N >= {history:g} on each after {FRAMES} accumulated frames ({below:.1%} below minHistory = "
         f"{MIN_HISTORY:g}); {device_name}")
    emit("fused against the torch composition, CRTV_DEMODULATE: " + "; ".join(
        f"{n}: largest difference {a['max_abs_diff']:.3g} (variance {a['max_abs_diff_variance']:.3g}) of the largest value, {a['pixels_with_other_bits']} pixels with other bits"
        for n, a in agreement.items()))
    r = rec["legs_ms"]["copy24"]
    emit(f"  copy of 24 B per pixel (48 B moved: one pass's compulsory traffic) {fmt(r)} = {W * H * 48 / r['median'] * 1e-9:.2f} TB/s")
    emit("the call of one pass without flags (estimate + step 1), by where the estimate's 49 taps come from:")
    for kind in ("temporal", "spatial"):
        emit(f"  {kind:8s} estimate: through L1 / L2 {fmt(rec['legs_ms'][f'estimate-l1-{kind}'])}; from LDS {fmt(rec['legs_ms'][f'estimate-lds-{kind}'])}")
    emit("no flags, taps through L1 / L2 and from LDS; one pass = the call of n passes minus the call of n - 1; x copy24 = times the traffic floor:")
    emit(f"  estimate + step 1: L1 / L2 {fmt(rec['legs_ms']['direct-1'])}; LDS {fmt(rec['legs_ms']['staged-1'])}")
    for n in range(2, 6):
        step = 1 << (n - 1)
        d = med[f"direct-{n}"] - med[f"direct-{n - 1}"]
        text = f"  step {step:2d}: taps through L1 / L2 {d:8.4f} ms ({d / med['copy24']:.2f} x copy24)"
        if step <= 4:
            st = med[f"staged-{n}"] - med[f"staged-{n - 1}"]
            text += f"; taps from LDS {st:8.4f} ms ({st / med['copy24']:.2f} x copy24)"
        emit(text)
    emit("the whole call with CRTV_DEMODULATE, as shipped (torch / fused and fused / crtd_denoise: of the planes' medians):")
    for n in range(1, 6):
        p, sf, t, d = (rec["legs_ms"][f"{k}-{n}"] for k in ("planes", "surface", "torch", "crtd"))
        emit(f"  {n} pass(es): planes {fmt(p)}; surface records {fmt(sf)}; torch ops {fmt(t)}; crtd_denoise {fmt(d)}; "
             f"torch / fused {t['median'] / p['median']:.1f}; fused / crtd {p['median'] / d['median']:.2f}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5, help="calls per timed leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vfilter_rate.txt"))
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vfilter_rate: no GPU (this tool measures; it does not fall back)")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"variance-guided a-trous filter (crtv_filter) on {W}x{H} G-buffer frames of multi-1M, colour and moments from {FRAMES} accumulated noisy frames; "
         f"events on the stream, median of {opt.rounds} alternating rounds of {opt.repeats} calls (min .. max)")
    result = {"metric": "vfilter_rate", "frame": f"{W}x{H}", "rounds": opt.rounds, "repeats": opt.repeats,
              "views": {view_name: measure(torch, opt, view_name, emit) for view_name in ("multi-1M", "multi-1M-dense")}}
    emit(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
