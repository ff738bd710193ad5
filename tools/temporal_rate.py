#!/usr/bin/env python3
"""Rate of temporal accumulation (libcrt_temporal.so) on 1920x1080 G-buffer frames of multi-1M with seeded noise on their colour:
the headline camera (a third of the pixels are hits; a pixel of sky has no history to fetch) and the dense camera (nearly all are), each under a
static camera (the previous frame is the same view) and under a small pan (the previous frame was shot 0.01 rad to the side).

    fused      ms of crtt_accumulate without flags, with CRTT_CLAMP and with both flags, as shipped
    choices    the two measured choices of the kernel, each form against the other: CRTT_TAPS=all|gated (the taps' colour and moments loaded
               unconditionally, or behind the geometry test) and, under CRTT_CLAMP, CRTT_CLAMP_TAPS=l1|lds (the 3 x 3 neighbourhood as row reads
               through L1, or from a tile staged in LDS)
    torch      the same definition composed from torch ops, what a caller of the API had before: four gathers per plane with materialised masks
               (checked against the fused result before anything is timed)
    copy       torch's device-to-device copy of a buffer of 64 B per pixel (64 B read and 64 B written per pixel: the bytes a call without
               flags must move for a pixel with history -- colour and geometry of the frame, colour, moments and geometry of the history read,
               colour, moments and geometry written), and of 40 B per pixel (what a pixel without history moves)

Every leg is timed with events on the stream around `--repeats` back-to-back calls; the legs alternate for `--rounds` rounds after a warm-up of
each; the median round is reported with min .. max. Needs a GPU: there is no fallback.

    python tools/temporal_rate.py [--rounds R] [--repeats K] [--out profiles/temporal_rate.txt]
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
PARAMS = dict(alpha=0.2, moments_alpha=0.2, max_history=32.0, depth_tol=0.05, normal_cos=0.9)
PAN = 0.01                                  # radians about the y axis: about 15 pixels at this size


def torch_accumulate(torch, color, geometry, prev, cam, prev_cam, clamp):
    """the definition of include/crt_temporal.h in torch ops (no instance match): what the fused call replaces. Returns (color, moments)."""
    dev = color.device
    f = lambda v: torch.tensor(np.asarray(v, np.float32), device=dev)
    R, S, dpos = f(cam.toRay[:]).reshape(3, 3), f(prev_cam.toScreen[:]).reshape(3, 3), f(cam.pos[:]) - f(prev_cam.pos[:])
    n, t = geometry[..., :3], geometry[..., 3]
    hit = t <= 99998.0
    rgb = color[..., :3]
    L = (0.299 * rgb[..., 0] + 0.587 * rgb[..., 1]) + 0.114 * rgb[..., 2]
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    d = torch.stack([(R[r, 0] * xx + R[r, 1] * yy) + R[r, 2] for r in range(3)], dim=-1)
    d = d / torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]
    v = dpos + d * t[..., None]
    dist = torch.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    u = [(S[r, 0] * v[..., 0] + S[r, 1] * v[..., 1]) + S[r, 2] * v[..., 2] for r in range(3)]
    fx, fy = u[0] / u[2], u[1] / u[2]
    want = hit & (u[2] > 0) & (fx >= -1.0) & (fx < float(W)) & (fy >= -1.0) & (fy < float(H))
    flx, fly = torch.floor(fx), torch.floor(fy)
    ax, ay = fx - flx, fy - fly
    x0, y0 = torch.where(want, flx, 0.0).to(torch.int64), torch.where(want, fly, 0.0).to(torch.int64)
    pc, pm, pg = prev["color"].reshape(-1, 4), prev["moments"].reshape(-1, 4), prev["geometry"].reshape(-1, 4)
    sums = torch.zeros((H, W, 6), device=dev)
    wsum = torch.zeros((H, W), device=dev)
    for dy in (0, 1):
        for dx in (0, 1):
            qx, qy = x0 + dx, y0 + dy
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            q = qy.clamp(0, H - 1) * W + qx.clamp(0, W - 1)
            gq, cq, mq = pg[q], pc[q], pm[q]
            ok = inside & (gq[..., 3] <= 99998.0) & ((gq[..., 3] - dist).abs() <= PARAMS["depth_tol"] * dist)
            ok &= ((gq[..., 0] * n[..., 0] + gq[..., 1] * n[..., 1]) + gq[..., 2] * n[..., 2]) >= PARAMS["normal_cos"]
            vals = torch.cat([cq[..., :3], mq[..., :3]], dim=-1)
            ok &= (mq[..., 2] >= 1.0) & torch.isfinite(vals[..., :5]).all(dim=-1)
            b = (ax if dx else 1.0 - ax) * (ay if dy else 1.0 - ay)
            sums = torch.where(ok[..., None], sums + vals * b[..., None], sums)
            wsum = torch.where(ok, wsum + b, wsum)
    have = want & (wsum > 0.01)
    mean = sums / wsum[..., None]
    h = mean[..., :3]
    if clamp:
        pad = torch.nn.functional.pad
        lo = pad(rgb.permute(2, 0, 1), (1, 1, 1, 1), value=float("inf"))
        hi = pad(rgb.permute(2, 0, 1), (1, 1, 1, 1), value=float("-inf"))
        mn = torch.stack([lo[:, 1 + oy:1 + oy + H, 1 + ox:1 + ox + W] for oy in (-1, 0, 1) for ox in (-1, 0, 1)]).amin(dim=0).permute(1, 2, 0)
        mx = torch.stack([hi[:, 1 + oy:1 + oy + H, 1 + ox:1 + ox + W] for oy in (-1, 0, 1) for ox in (-1, 0, 1)]).amax(dim=0).permute(1, 2, 0)
        h = torch.minimum(torch.maximum(h, mn), mx)
    N = torch.clamp(mean[..., 5] + 1.0, max=PARAMS["max_history"])
    a, am = torch.clamp(1.0 / N, min=PARAMS["alpha"]), torch.clamp(1.0 / N, min=PARAMS["moments_alpha"])
    out = torch.where(have[..., None], h * (1.0 - a)[..., None] + rgb * a[..., None], rgb)
    m1 = mean[..., 3] * (1.0 - am) + L * am
    m2 = mean[..., 4] * (1.0 - am) + (L * L) * am
    var = m2 - m1 * m1
    blended = torch.stack([m1, m2, N, torch.where(var > 0, var, 0.0)], dim=-1)
    reset = torch.stack([L, L * L, hit.to(torch.float32), torch.zeros_like(L)], dim=-1)
    return torch.cat([out, color[..., 3:]], dim=-1), torch.where(have[..., None], blended, reset)


def measure(torch, opt, view_name, emit):
    """every leg on one view; prints through emit() and returns the view's record"""
    dev = torch.device("cuda", 0)
    lib = _lib.temporal()
    for name in ("CRTT_TAPS", "CRTT_CLAMP_TAPS"):
        os.environ.pop(name, None)
    sc = scenes.get(view_name)
    frames = []
    with driver.Session(W, H, device=0) as s:
        s.load_scene(sc)
        device_name = s.hip.crt_device_name().decode()
        front = np.asarray(sc.camera_front, np.float64)
        turned = np.array([front[0] * np.cos(PAN) + front[2] * np.sin(PAN), front[1], -front[0] * np.sin(PAN) + front[2] * np.cos(PAN)])
        for i, fr in enumerate((front, turned)):
            s.set_camera(np.asarray(sc.camera_pos, np.float32), fr.astype(np.float32))
            s.render(gbuffer=True)
            g = s.read_gbuffer_raw()
            frame = s.read_output()
            noisy = (frame + np.random.RandomState(1 + i).normal(0, 0.2, frame.shape) * np.array([1, 1, 1, 0])).astype(np.float32)
            frames.append({"color": torch.from_numpy(noisy).to(dev),
                           "geometry": torch.from_numpy(np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1)).to(dev),
                           "ids": torch.from_numpy(g["ids"].view(np.int32).reshape(H, W, 4).copy()).to(dev),
                           "camera": _lib.crtt_camera(*s.camera(), W, H), "hit_share": float((g["geometry"]["t"] <= 99998.0).mean())})
    other = torch.from_numpy((frames[0]["color"].cpu().numpy() + np.random.RandomState(9).normal(0, 0.2, (H, W, 4)) * np.array([1, 1, 1, 0])).astype(np.float32)).to(dev)
    sets = [{"color": torch.empty((H, W, 4), device=dev), "moments": torch.empty((H, W, 4), device=dev), "geometry": torch.empty((H, W, 4), device=dev),
             "instance": torch.empty((H, W), dtype=torch.int32, device=dev)} for _ in range(2)]
    stream = torch.cuda.current_stream(dev).cuda_stream

    def history(i, cam):
        return _lib.CrttHistory(*[sets[i][k].data_ptr() for k in ("color", "moments", "geometry", "instance")], cam)

    def fused(cur, color, flags, reset=False):
        f = _lib.CrttFrame(W, H, color.data_ptr(), _lib.CRTT_GUIDES_PLANES, cur["geometry"].data_ptr(), cur["ids"].data_ptr(), cur["camera"])
        p = _lib.CrttParams(flags, PARAMS["alpha"], PARAMS["moments_alpha"], PARAMS["max_history"], PARAMS["depth_tol"], PARAMS["normal_cos"])
        prev, nxt = history(0, frames[0]["camera"]), history(0 if reset else 1, cur["camera"])
        rc = lib.crtt_accumulate(C.byref(f), None if reset else C.byref(prev), C.byref(nxt), C.byref(p), stream)
        if rc:
            raise SystemExit(f"temporal_rate: crtt_accumulate failed with {rc}: {lib.crtt_error_string(rc).decode()}")

    # set 0: the history of the first view after one frame; every timed call reads it and writes set 1
    fused(frames[0], frames[0]["color"], 0, reset=True)
    moves = {"static": (frames[0], other), "pan": (frames[1], frames[1]["color"])}
    agreement, kept = {}, {}
    for move, (cur, color) in moves.items():
        for clamp in (False, True):
            fused(cur, color, _lib.CRTT_CLAMP if clamp else 0)
            a, am = sets[1]["color"].clone(), sets[1]["moments"].clone()
            b, bm = torch_accumulate(torch, color, cur["geometry"], sets[0], cur["camera"], frames[0]["camera"], clamp)
            diff = max(float((a - b).abs().nan_to_num(0.0).max()), float((am - bm).abs().nan_to_num(0.0).max()))
            other_bits = int(((a.view(torch.int32) != b.view(torch.int32)).any(dim=-1) | (am.view(torch.int32) != bm.view(torch.int32)).any(dim=-1)).sum())
            agreement[f"{move}{'+clamp' if clamp else ''}"] = {"max_abs_diff": diff, "pixels_with_other_bits": other_bits}
            if not diff < 1e-4:
                raise SystemExit(f"temporal_rate: the fused result differs from the torch composition by {diff} ({move}, clamp={clamp})")
        hit = cur["geometry"][..., 3] <= 99998.0
        kept[move] = float((sets[1]["moments"][..., 2][hit] > 1.0).float().mean())

    def leg(call):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(opt.repeats):
            call()
        ev1.record()
        torch.cuda.current_stream().synchronize()
        return ev0.elapsed_time(ev1) / opt.repeats

    def with_env(taps, clamp_taps, call):
        def run():
            for name, value in (("CRTT_TAPS", taps), ("CRTT_CLAMP_TAPS", clamp_taps)):
                if value is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = value
            call()
            os.environ.pop("CRTT_TAPS", None); os.environ.pop("CRTT_CLAMP_TAPS", None)
        return run

    src64, dst64 = torch.empty((H, W, 16), device=dev), torch.empty((H, W, 16), device=dev)
    src40, dst40 = torch.empty((H, W, 10), device=dev), torch.empty((H, W, 10), device=dev)
    legs = {"copy64": lambda: dst64.copy_(src64), "copy40": lambda: dst40.copy_(src40)}
    BOTH = _lib.CRTT_CLAMP | _lib.CRTT_MATCH_INSTANCE
    for move, (cur, color) in moves.items():
        legs[f"{move}/shipped"] = with_env(None, None, lambda cur=cur, color=color: fused(cur, color, 0))
        legs[f"{move}/shipped+clamp"] = with_env(None, None, lambda cur=cur, color=color: fused(cur, color, _lib.CRTT_CLAMP))
        legs[f"{move}/shipped+both"] = with_env(None, None, lambda cur=cur, color=color: fused(cur, color, BOTH))
        for taps in ("all", "gated"):
            legs[f"{move}/taps-{taps}"] = with_env(taps, None, lambda cur=cur, color=color: fused(cur, color, 0))
            for clamp_taps in ("l1", "lds"):
                legs[f"{move}/taps-{taps}+clamp-{clamp_taps}"] = with_env(taps, clamp_taps, lambda cur=cur, color=color: fused(cur, color, _lib.CRTT_CLAMP))
        legs[f"{move}/torch"] = lambda cur=cur, color=color: torch_accumulate(torch, color, cur["geometry"], sets[0], cur["camera"], frames[0]["camera"], False)
        legs[f"{move}/torch+clamp"] = lambda cur=cur, color=color: torch_accumulate(torch, color, cur["geometry"], sets[0], cur["camera"], frames[0]["camera"], True)
    for f in legs.values():
        leg(f)
    times = {name: [] for name in legs}
    for _ in range(opt.rounds):
        for name, f in legs.items():
            times[name].append(leg(f))
    rec = {"device": device_name, "hit_share": [round(fr["hit_share"], 4) for fr in frames], "hit_pixels_that_keep_history": {k: round(v, 4) for k, v in kept.items()},
           "agreement_with_torch": agreement,
           "legs_ms": {name: {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)} for name, ts in times.items()}}
    ms = rec["legs_ms"]
    show = lambda r: f"{r['median']:8.4f} ms ({r['min']:.4f} .. {r['max']:.4f})"
    emit(f"== {view_name}: {frames[0]['hit_share']:.1%} of the pixels are hits ({frames[1]['hit_share']:.1%} after the pan); {device_name}")
    emit("fused against the torch composition: " + "; ".join(
        f"{k}: largest difference {a['max_abs_diff']:.3g}, {a['pixels_with_other_bits']} pixels with other bits" for k, a in agreement.items()))
    for name, per_pixel in (("copy64", 64), ("copy40", 40)):
        emit(f"  copy of {per_pixel} B per pixel ({per_pixel} read + {per_pixel} written) {show(ms[name])} = {W * H * 2 * per_pixel / ms[name]['median'] * 1e-9:.2f} TB/s")
    for move in moves:
        emit(f"{move} camera: {kept[move]:.1%} of the hit pixels keep their history")
        emit(f"  as shipped: no flags {show(ms[move + '/shipped'])} = {ms[move + '/shipped']['median'] / ms['copy64']['median']:.2f} x copy64; "
             f"CRTT_CLAMP {show(ms[move + '/shipped+clamp'])}; both flags {show(ms[move + '/shipped+both'])}")
        emit(f"  torch ops:  no flags {show(ms[move + '/torch'])} = {ms[move + '/torch']['median'] / ms[move + '/shipped']['median']:.1f} x the fused call; "
             f"CRTT_CLAMP {show(ms[move + '/torch+clamp'])} = {ms[move + '/torch+clamp']['median'] / ms[move + '/shipped+clamp']['median']:.1f} x")
        for taps in ("all", "gated"):
            emit(f"  CRTT_TAPS={taps:5s}: no flags {show(ms[f'{move}/taps-{taps}'])}; CRTT_CLAMP with CRTT_CLAMP_TAPS=l1 {show(ms[f'{move}/taps-{taps}+clamp-l1'])}, "
                 f"=lds {show(ms[f'{move}/taps-{taps}+clamp-lds'])}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=10, help="calls per timed leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_rate.txt"))
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("temporal_rate: no GPU (this tool measures; it does not fall back)")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"temporal accumulation (crtt_accumulate) on {W}x{H} G-buffer frames of multi-1M, seeded noise on the colour; events on the stream, median of "
         f"{opt.rounds} alternating rounds of {opt.repeats} calls (min .. max)")
    result = {"metric": "temporal_rate", "frame": f"{W}x{H}", "rounds": opt.rounds, "repeats": opt.repeats,
              "views": {view_name: measure(torch, opt, view_name, emit) for view_name in ("multi-1M", "multi-1M-dense")}}
    emit(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
