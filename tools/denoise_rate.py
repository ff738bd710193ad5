#!/usr/bin/env python3
"""Rate of the a-trous denoiser (libcrt_denoise.so) on 1920x1080 G-buffer frames of multi-1M with seeded noise on their colour: the
headline camera (a third of the pixels are hits; a pixel of sky is copied) and the dense camera (nearly all are).

    per step     ms of one pass at steps 1..32, without flags (so that a call of n passes is exactly its n passes): the call of n passes minus
                 the call of n - 1, with the taps through L1 / L2 (CRTD_STAGE_MAX_STEP=0) and, for steps 1, 2 and 4, from LDS (=4)
    whole call   ms of crtd_denoise for 1..6 passes with CRTD_DEMODULATE, guided by the planes and by CrtSurfaceHit records, as shipped
    torch        the same filter composed from torch ops, what a caller of the API had before: 25 shifted views per pass with materialised masks
                 (checked against the fused result before anything is timed)
    copy         torch's device-to-device copy of a buffer of 48 B per pixel (48 B read and 48 B written per pixel), and of 24 B per pixel
                 (48 B moved per pixel: one pass's compulsory traffic -- colour and geometry read, colour written)

Every leg is timed with events on the stream around `--repeats` back-to-back calls; the legs alternate for `--rounds` rounds after a warm-up of
each; the median round is reported with min .. max. Needs a GPU: there is no fallback.

    python tools/denoise_rate.py [--rounds R] [--repeats K] [--out profiles/denoise_rate.txt]
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
DEPTH_TOL, NORMAL_COS = 0.05, 0.9
K = (0.375, 0.25, 0.0625)
WRITE_RAYS = 2


def torch_denoise(torch, color, geometry, albedo, iterations, demodulate):
    """the definition of include/crt_denoise.h in torch ops (no instance match, no luminance stop): what the fused call replaces"""
    n, t = geometry[..., :3], geometry[..., 3]
    hit = t <= 99998.0
    I = color[..., :3]
    if demodulate:
        b = torch.stack([(albedo >> sh) & 255 for sh in (0, 8, 16)], dim=-1).to(torch.float32)
        den = torch.where(b == 0, torch.ones_like(b), b / 255.0)
        I = torch.where(hit[..., None], I / den, I)
    h, w = t.shape
    for p in range(iterations):
        s = 1 << p
        pad = 2 * s
        Ip = torch.zeros((h + 2 * pad, w + 2 * pad, 3), dtype=torch.float32, device=I.device); Ip[pad:pad + h, pad:pad + w] = I
        tp = torch.full((h + 2 * pad, w + 2 * pad), 99999.0, dtype=torch.float32, device=I.device); tp[pad:pad + h, pad:pad + w] = t
        np_ = torch.zeros((h + 2 * pad, w + 2 * pad, 3), dtype=torch.float32, device=I.device); np_[pad:pad + h, pad:pad + w] = n
        dtol = (DEPTH_TOL * t) * float(s)
        total = torch.zeros_like(I); wsum = torch.zeros_like(t)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ys, xs = slice(pad + dy * s, pad + dy * s + h), slice(pad + dx * s, pad + dx * s + w)
                k = K[abs(dy)] * K[abs(dx)]
                if dx == 0 and dy == 0:
                    wt = torch.full_like(t, k)
                else:
                    tq, nq = tp[ys, xs], np_[ys, xs]
                    m = (tq <= 99998.0) & ((tq - t).abs() <= dtol) & (((nq[..., 0] * n[..., 0] + nq[..., 1] * n[..., 1]) + nq[..., 2] * n[..., 2]) >= NORMAL_COS)
                    wt = torch.where(m, k, 0.0).to(torch.float32)
                total = total + Ip[ys, xs] * wt[..., None]
                wsum = wsum + wt
        I = torch.where(hit[..., None], total / wsum[..., None], I)
    if demodulate:
        I = torch.where(hit[..., None], I * den, I)
    return torch.cat([I, color[..., 3:]], dim=-1)


def measure(torch, opt, view_name, emit):
    """every leg on one view; prints through emit() and returns the view's record"""
    dev = torch.device("cuda", 0)
    lib = _lib.denoise()
    os.environ.pop("CRTD_STAGE_MAX_STEP", None)
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
        noisy = (frame + np.random.RandomState(1).normal(0, 0.2, frame.shape) * np.array([1, 1, 1, 0])).astype(np.float32)
        color = torch.from_numpy(noisy).to(dev)
        geometry = torch.from_numpy(np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1)).to(dev)
        ids = torch.from_numpy(g["ids"].view(np.int32).reshape(H, W, 4).copy()).to(dev)
        albedo = torch.from_numpy(g["albedo"].astype(np.int64)).to(dev)                      # int64 for torch's shifts; the fused call reads the uint32 plane
        albedo32 = torch.from_numpy(g["albedo"].view(np.int32).copy()).to(dev)
        hit_share = float((g["geometry"]["t"] <= 99998.0).mean())
    out, scratch = torch.empty((H, W, 4), device=dev), torch.empty((H, W, 4), device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fused(iterations, flags, surface=False):
        f = _lib.CrtdFrame(W, H, color.data_ptr(), _lib.CRTD_GUIDES_SURFACE if surface else _lib.CRTD_GUIDES_PLANES,
                           hits.records.data_ptr() if surface else geometry.data_ptr(), None if surface else ids.data_ptr(), None if surface else albedo32.data_ptr())
        p = _lib.CrtdParams(iterations, flags, DEPTH_TOL, NORMAL_COS, 0.0)
        rc = lib.crtd_denoise(C.byref(f), C.byref(p), out.data_ptr(), scratch.data_ptr(), stream)
        if rc:
            raise SystemExit(f"denoise_rate: crtd_denoise failed with {rc}: {lib.crtd_error_string(rc).decode()}")

    # the fused call and the torch composition agree before either is timed (torch rounds a division differently: the largest difference is reported)
    agreement = {}
    for n in (1, 4):
        fused(n, _lib.CRTD_DEMODULATE)
        a = out.clone()
        fused(n, _lib.CRTD_DEMODULATE, surface=True)
        b = torch_denoise(torch, color, geometry, albedo, n, True)
        if not torch.equal(a.view(torch.int32), out.view(torch.int32)):
            raise SystemExit("denoise_rate: the two guide layouts give different bits")
        diff = float((a - b).abs().nan_to_num(0.0).max())
        agreement[n] = {"max_abs_diff": diff, "pixels_with_other_bits": int((a.view(torch.int32) != b.view(torch.int32)).any(dim=-1).sum())}
        if not diff < 1e-4:
            raise SystemExit(f"denoise_rate: the fused result differs from the torch composition by {diff} at {n} passes")

    def leg(call):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(opt.repeats):
            call()
        ev1.record()
        torch.cuda.current_stream().synchronize()
        return ev0.elapsed_time(ev1) / opt.repeats

    def with_env(value, call):
        def run():
            if value is None:
                os.environ.pop("CRTD_STAGE_MAX_STEP", None)
            else:
                os.environ["CRTD_STAGE_MAX_STEP"] = value
            call()
            os.environ.pop("CRTD_STAGE_MAX_STEP", None)
        return run

    src48, dst48 = torch.empty((H, W, 12), device=dev), torch.empty((H, W, 12), device=dev)
    src24, dst24 = torch.empty((H, W, 6), device=dev), torch.empty((H, W, 6), device=dev)
    legs = {"copy48": lambda: dst48.copy_(src48), "copy24": lambda: dst24.copy_(src24)}
    for n in range(1, 7):
        legs[f"direct-{n}"] = with_env("0", lambda n=n: fused(n, 0))
        legs[f"staged-{n}"] = with_env("4", lambda n=n: fused(n, 0))
        legs[f"planes-{n}"] = with_env(None, lambda n=n: fused(n, _lib.CRTD_DEMODULATE))
        legs[f"surface-{n}"] = with_env(None, lambda n=n: fused(n, _lib.CRTD_DEMODULATE, surface=True))
        legs[f"torch-{n}"] = lambda n=n: torch_denoise(torch, color, geometry, albedo, n, True)
    for f in legs.values():
        leg(f)
    times = {name: [] for name in legs}
    for _ in range(opt.rounds):
        for name, f in legs.items():
            times[name].append(leg(f))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    rec = {"device": device_name, "hit_share": round(hit_share, 4), "agreement_with_torch": agreement,
           "legs_ms": {name: {"median": round(med[name], 4), "min": round(min(ts), 4), "max": round(max(ts), 4)} for name, ts in times.items()}}
    emit(f"== {view_name}: {hit_share:.1%} of the pixels are hits; {device_name}")
    emit("fused against the torch composition, CRTD_DEMODULATE: " + "; ".join(
        f"{n} pass(es): largest difference {a['max_abs_diff']:.3g}, {a['pixels_with_other_bits']} pixels with other bits" for n, a in agreement.items()))
    for name, what in (("copy48", "copy of 48 B per pixel (48 read + 48 written)"), ("copy24", "copy of 24 B per pixel (48 B moved: one pass's compulsory traffic)")):
        r = rec["legs_ms"][name]
        emit(f"  {what:70s} {r['median']:8.4f} ms ({r['min']:.4f} .. {r['max']:.4f}) = {W * H * 48 * (2 if name == 'copy48' else 1) / r['median'] * 1e-9:.2f} TB/s")
    emit("one pass, no flags (the call of n passes minus the call of n - 1); x copy24 = times the traffic floor:")
    for n in range(1, 7):
        step = 1 << (n - 1)
        d = med[f"direct-{n}"] - (med[f"direct-{n - 1}"] if n > 1 else 0.0)
        text = f"  step {step:2d}: taps through L1 / L2 {d:8.4f} ms ({d / med['copy24']:.2f} x copy24)"
        if step <= 4:
            st = med[f"staged-{n}"] - (med[f"staged-{n - 1}"] if n > 1 else 0.0)
            text += f"; taps from LDS {st:8.4f} ms ({st / med['copy24']:.2f} x copy24)"
        emit(text)
    emit("the whole call with CRTD_DEMODULATE, as shipped (ratio = torch composition / fused, planes):")
    for n in range(1, 7):
        p, sf, t = (rec["legs_ms"][f"{k}-{n}"] for k in ("planes", "surface", "torch"))
        emit(f"  {n} pass(es): planes {p['median']:8.4f} ms ({p['min']:.4f} .. {p['max']:.4f}); surface records {sf['median']:8.4f} ms ({sf['min']:.4f} .. {sf['max']:.4f}); "
             f"torch ops {t['median']:9.4f} ms ({t['min']:.4f} .. {t['max']:.4f}); ratio {t['median'] / p['median']:.1f}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5, help="calls per timed leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_rate.txt"))
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("denoise_rate: no GPU (this tool measures; it does not fall back)")
    lines = []

    def emit(text):
        print(text)
        lines.append(text)

    emit(f"a-trous denoiser (crtd_denoise) on {W}x{H} G-buffer frames of multi-1M, seeded noise on the colour; events on the stream, median of {opt.rounds} "
         f"alternating rounds of {opt.repeats} calls (min .. max)")
    result = {"metric": "denoise_rate", "frame": f"{W}x{H}", "rounds": opt.rounds, "repeats": opt.repeats,
              "views": {view_name: measure(torch, opt, view_name, emit) for view_name in ("multi-1M", "multi-1M-dense")}}
    emit(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
