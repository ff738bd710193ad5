#!/usr/bin/env python3
"""Rate of the chain's last step (libcrt_present.so) on the 1920x1080 frames of multi-1M: the headline camera and the dense camera.
The colour is the frame's own plain float frame, the AO plane crt_frame_ao's.

    forms        ms of crtp_present for each of the eight sets of UNORM8 / POST / FXAA with both outputs (16 B read, 16 + 4 B written per pixel),
                 and of three more: bytes only, with an AO plane and an exposure, with HEAL on top; against a device copy of half the bytes the
                 form must move (the floor); the non-FXAA forms also against the same definition composed from torch ops, which is checked
                 against the fused result first (the same bytes and floats within 1e-6 without POST, within the frame's rule with it)
    fxaa taps    the FXAA forms under CRTP_TAPS=lds (S staged over the tile and a halo of 5 in LDS) and CRTP_TAPS=l1 (S made again at every tap
                 through L1): the two measured variants (the library's default, lds, is the faster on every form but FXAA+POST, where they tie)
    frame path   crt_last_kernel_ms(3) of crt_render with FXAA (crt_fxaa_kernel, which applies POST and UNORM8 in its epilogue) and, in a
                 session under CRT_KERNEL=wavefront, with POSTPROCESS alone (crt_postprocess_kernel as a launch of its own): what the same
                 stages cost inside the frame
    views        ms of crtp_view per mode, both outputs

Every leg is timed with events on the stream around `--repeats` back-to-back calls (a fifth as many for the torch compositions); the legs
alternate for `--rounds` rounds after a warm-up of each; the median round is reported with min .. max. Needs a GPU: there is no fallback.

    python tools/present_rate.py [--rounds R] [--repeats K] [--out profiles/present_rate.txt]
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
N = W * H
U8, POST, FXAA, HEAL = _lib.CRTP_UNORM8, _lib.CRTP_POST, _lib.CRTP_FXAA, _lib.CRTP_HEAL
R_POST, R_UNORM8, R_FXAA = 1, 64, 512                           # crt_render's flags
AO_SAMPLES, AO_RADIUS_OF_CAMERA_DISTANCE = 8, 0.05


def name_of(flags):
    return "+".join(n for n, b in (("UNORM8", U8), ("FXAA", FXAA), ("POST", POST), ("HEAL", HEAL)) if flags & b) or "plain"


def torch_unorm8(torch, v):
    u = v * 255.0
    return torch.where(torch.isnan(u) | (u <= 0.0), torch.zeros_like(u), torch.where(u >= 255.0, torch.full_like(u, 255.0), torch.round(u)))


def torch_present(torch, color, flags, ao=None, strength=1.0, exposure=1.0):
    """steps 1-4 and 6-8 of include/crt_present.h from torch ops (no FXAA): the float image and the bytes as (H, W, 4) uint8"""
    c = color[..., :3]
    if flags & HEAL:
        c = torch.where(torch.isfinite(c), c, torch.zeros_like(c))
    if ao is not None:
        f = (1.0 - strength) + strength * ao
        if flags & HEAL:
            f = torch.where(torch.isfinite(f), f, torch.ones_like(f))
        c = c * f[..., None]
    if exposure != 1.0:
        c = c * exposure
    if flags & U8:
        c = torch_unorm8(torch, c) / 255.0
    if flags & POST:
        yy, xx = torch.meshgrid(torch.arange(H, device=c.device, dtype=torch.float32), torch.arange(W, device=c.device, dtype=torch.float32), indexing="ij")
        uvx, uvy = xx / float(W), yy / float(H)
        P = torch.sqrt((c[..., 0] * c[..., 0]) * 0.299 + ((c[..., 1] * c[..., 1]) * 0.587) + ((c[..., 2] * c[..., 2]) * 0.114))[..., None]
        c = P + (c - P) * 1.2
        lw = torch.tensor([0.2126, 0.7152, 0.0722], device=c.device)
        l = ((c[..., 0] * lw[0] + c[..., 1] * lw[1]) + c[..., 2] * lw[2])[..., None]
        c = c * ((l * (1.0 + (l / (0.8 * 0.8)))) / (1.0 + l) / l)
        c = torch.pow(torch.pow(c, 1.0 / 1.55), 1.0 / 1.2)
        vig = torch.pow(((uvx * (1.0 - uvy)) * (uvy * (1.0 - uvx))) * 15.0, 0.15)[..., None]
        c = c * vig
        if flags & U8:
            c = torch_unorm8(torch, c) / 255.0
    out = torch.cat([c, torch.ones_like(c[..., :1])], dim=-1)
    return out, torch_unorm8(torch, out).to(torch.uint8)


def measure(torch, opt, view_name, emit):
    dev = torch.device("cuda", 0)
    lib = _lib.present()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rec = {}

    def leg(call, repeats, taps=None):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        set_taps(taps)                  # once per leg, outside the timed window (the library reads it at every call)
        ev0.record()
        for _ in range(repeats):
            call()
        ev1.record()
        torch.cuda.current_stream().synchronize()
        return ev0.elapsed_time(ev1) / repeats

    def set_taps(taps):
        if taps is not None:
            os.environ["CRTP_TAPS"] = taps
        else:
            os.environ.pop("CRTP_TAPS", None)

    def run(legs):
        for f, _, *taps in legs.values():
            leg(f, 1, *taps)
        times = {name: [] for name in legs}
        for _ in range(opt.rounds):
            for name, (f, k, *taps) in legs.items():
                times[name].append(leg(f, k, *taps))
        return {name: {"median": round(statistics.median(ts), 5), "min": round(min(ts), 5), "max": round(max(ts), 5)} for name, ts in times.items()}

    def copy_leg(nbytes):
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        return (lambda: dst.copy_(src), opt.repeats)

    slow = max(1, opt.repeats // 5)
    frame_ms = {}
    with driver.Session(W, H, device=0) as s:
        s.load_scene(scenes.get(view_name))
        rec["device"] = s.hip.crt_device_name().decode()
        for label, flags in (("FXAA", R_FXAA), ("FXAA+POST", R_FXAA | R_POST), ("UNORM8+FXAA+POST", R_FXAA | R_POST | R_UNORM8), ("POST (fused into Trace)", R_POST)):
            ts = []
            for _ in range(opt.rounds + 1):
                s.render_raw(flags)
                ts.append(s.kernel_ms(3))
            frame_ms[label] = round(statistics.median(ts[1:]), 5)
        s.render(gbuffer=True)
        color = torch.from_numpy(np.array(s.output(), copy=True)).to(dev)
        t = s.read_gbuffer_raw()["geometry"]["t"]
        hit = t <= 99998.0
        rec["hit_share"] = round(float(hit.mean()), 4)
        radius = AO_RADIUS_OF_CAMERA_DISTANCE * float(np.median(t[hit]))
        ao = torch.from_numpy(np.array(s.ambient_occlusion(AO_SAMPLES, radius=radius, bias=1e-3 * radius), copy=True)).to(dev)
        out_f, out_b = torch.empty((H, W, 4), device=dev), torch.empty((H, W), dtype=torch.int32, device=dev)

        def present(flags, with_ao=False, exposure=1.0, floats=True):
            p = _lib.CrtpPresent(W, H, color.data_ptr(), ao.data_ptr() if with_ao else None, 0.8, exposure, flags)
            rc = lib.crtp_present(C.byref(p), out_f.data_ptr() if floats else None, out_b.data_ptr(), None, stream)
            if rc:
                raise SystemExit(f"present_rate: crtp_present failed with {rc}")

        # ---- the torch compositions agree with the fused result before anything is timed
        worst = {}
        for flags, with_ao, exposure in [(f, False, 1.0) for f in (0, U8, POST, U8 | POST)] + [(U8 | POST, True, 1.25), (U8 | POST | HEAL, True, 1.25)]:
            present(flags, with_ao, exposure)
            tf, tb = torch_present(torch, color, flags, ao if with_ao else None, 0.8, exposure)
            d = float((tf - out_f).abs().max())
            worst[name_of(flags) + ("+ao+exposure" if with_ao else "")] = d
            bytes_differ = int((tb.view(torch.int32).view(H, W) != out_b).sum())
            limit = ((1.0 / 255.0 + 1e-6) if flags & U8 else 2e-5) if flags & POST else 1e-6      # (torch divides by 255 as a multiply: one ulp)
            if d > limit or (not flags & POST and bytes_differ) or bytes_differ > 0.002 * N:
                raise SystemExit(f"present_rate: the torch composition of {name_of(flags)} differs from crtp_present: max abs {d}, {bytes_differ} pixels' bytes")
        rec["torch_max_abs_diff"] = worst
        set_taps("l1")
        present(FXAA | U8)
        a = (out_f.clone(), out_b.clone())
        set_taps("lds")
        present(FXAA | U8)
        set_taps(None)
        if not (torch.equal(a[0].view(torch.int32), out_f.view(torch.int32)) and torch.equal(a[1], out_b)):
            raise SystemExit("present_rate: the two FXAA variants disagree")

        both, only_bytes = N * (16 + 16 + 4), N * (16 + 4)
        legs = {}
        for flags in range(8):
            n = name_of(flags)
            legs[n] = (lambda f=flags: present(f), opt.repeats)
            if not flags & FXAA:
                legs["torch " + n] = (lambda f=flags: torch_present(torch, color, f), slow)
        legs["copy 36 B/pixel"] = copy_leg(both)
        legs["UNORM8+POST, bytes only"] = (lambda: present(U8 | POST, floats=False), opt.repeats)
        legs["copy 20 B/pixel"] = copy_leg(only_bytes)
        legs["UNORM8+POST, ao + exposure"] = (lambda: present(U8 | POST, True, 1.25), opt.repeats)
        legs["torch UNORM8+POST, ao + exposure"] = (lambda: torch_present(torch, color, U8 | POST, ao, 0.8, 1.25), slow)
        legs["UNORM8+POST+HEAL, ao + exposure"] = (lambda: present(U8 | POST | HEAL, True, 1.25), opt.repeats)
        legs["copy 40 B/pixel"] = copy_leg(N * 40)
        for flags in (FXAA, FXAA | U8, FXAA | POST, FXAA | U8 | POST):
            for taps in ("lds", "l1"):
                legs[f"{name_of(flags)} taps {taps}"] = (lambda f=flags: present(f), opt.repeats, taps)
        legs["UNORM8+FXAA+POST, ao + exposure, taps lds"] = (lambda: present(FXAA | U8 | POST, True, 1.25), opt.repeats, "lds")
        legs["UNORM8+FXAA+POST, ao + exposure, taps l1"] = (lambda: present(FXAA | U8 | POST, True, 1.25), opt.repeats, "l1")
        rec["legs_ms"] = run(legs)
        os.environ.pop("CRTP_TAPS", None)

        # ---- views
        g = [s.hip.crt_gbuffer_device_ptr(p) for p in (_lib.CRT_GBUFFER_GEOMETRY, _lib.CRT_GBUFFER_IDS, _lib.CRT_GBUFFER_ALBEDO)]
        state = torch.randint(0, 4, (H, W), dtype=torch.int32, device=dev)

        def view(mode):
            plane = ao if mode == "scalar" else state if mode == "state" else None
            v = _lib.CrtpView(W, H, _lib.CRTP_GUIDES_PLANES, _lib.CRTP_VIEW_MODES[mode], g[0], g[1], g[2], plane.data_ptr() if plane is not None else None, 10.0, 0.0, 1.0)
            rc = lib.crtp_view(C.byref(v), out_f.data_ptr(), out_b.data_ptr(), stream)
            if rc:
                raise SystemExit(f"present_rate: crtp_view failed with {rc}")

        rec["view_legs_ms"] = run({mode: (lambda m=mode: view(m), opt.repeats) for mode in _lib.CRTP_VIEW_MODES})
        torch.cuda.synchronize()
    # crt_postprocess_kernel as a launch of its own: the wavefront variant keeps every per-pixel stage out of its kernels
    os.environ["CRT_KERNEL"] = "wavefront"
    try:
        with driver.Session(W, H, device=0) as s:
            s.load_scene(scenes.get(view_name))
            ts = []
            for _ in range(opt.rounds + 1):
                s.render_raw(R_POST)
                ts.append(s.kernel_ms(3))
            frame_ms["POST (crt_postprocess_kernel, CRT_KERNEL=wavefront)"] = round(statistics.median(ts[1:]), 5)
    finally:
        os.environ.pop("CRT_KERNEL", None)
    rec["frame_path_ms"] = frame_ms

    fmt = lambda r: f"{r['median']:8.4f} ms ({r['min']:.4f} .. {r['max']:.4f})"
    L = rec["legs_ms"]
    emit(f"== {view_name}: {rec['hit_share']:.1%} of the pixels are hits; {rec['device']}")
    c36 = L["copy 36 B/pixel"]["median"]
    emit(f"  device copy of half of 36 B/pixel ({both / 1e6:.1f} MB moved): {fmt(L['copy 36 B/pixel'])}; of 20 B/pixel: {fmt(L['copy 20 B/pixel'])}; of 40 B/pixel: {fmt(L['copy 40 B/pixel'])}")
    for flags in range(8):
        n = name_of(flags)
        line = f"  {n:18s} float + bytes: {fmt(L[n])} = {L[n]['median'] / c36:.2f} x copy"
        if not flags & FXAA:
            line += f"; torch ops {fmt(L['torch ' + n])} (torch / fused {L['torch ' + n]['median'] / L[n]['median']:.1f})"
        emit(line)
    emit(f"  UNORM8+POST, bytes only: {fmt(L['UNORM8+POST, bytes only'])} = {L['UNORM8+POST, bytes only']['median'] / L['copy 20 B/pixel']['median']:.2f} x copy")
    emit(f"  UNORM8+POST, ao + exposure: {fmt(L['UNORM8+POST, ao + exposure'])} = {L['UNORM8+POST, ao + exposure']['median'] / L['copy 40 B/pixel']['median']:.2f} x copy; "
         f"torch ops {fmt(L['torch UNORM8+POST, ao + exposure'])}; with HEAL {fmt(L['UNORM8+POST+HEAL, ao + exposure'])}")
    for flags in (FXAA, FXAA | U8, FXAA | POST, FXAA | U8 | POST):
        n = name_of(flags)
        emit(f"  FXAA taps, {n:18s}: lds {fmt(L[n + ' taps lds'])}; l1 {fmt(L[n + ' taps l1'])} (l1 / lds {L[n + ' taps l1']['median'] / L[n + ' taps lds']['median']:.2f})")
    emit(f"  FXAA taps, UNORM8+FXAA+POST with ao + exposure: lds {fmt(L['UNORM8+FXAA+POST, ao + exposure, taps lds'])}; l1 {fmt(L['UNORM8+FXAA+POST, ao + exposure, taps l1'])}")
    emit("  the frame path, crt_last_kernel_ms(3), median: " + "; ".join(f"{k} {v:.4f} ms" for k, v in frame_ms.items()))
    emit("  crtp_view, float + bytes: " + "; ".join(f"{m} {r['median']:.4f} ms" for m, r in rec["view_legs_ms"].items()))
    emit("  torch compositions against the fused result, max abs difference: " + "; ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=100, help="calls per timed leg (a fifth as many of the torch compositions)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "present_rate.txt"))
    ap.add_argument("--views", default="multi-1M,multi-1M-dense")
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("present_rate: no GPU (this tool measures; it does not fall back)")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"the chain's last step (crtp_present, crtp_view) on {W}x{H} frames of multi-1M; events on the stream, median of {opt.rounds} alternating rounds of "
         f"{opt.repeats} calls (min .. max); x copy = times the device copy of as many bytes as the form must move (the floor)")
    result = {"metric": "present_rate", "frame": f"{W}x{H}", "rounds": opt.rounds, "repeats": opt.repeats,
              "views": {v: measure(torch, opt, v, emit) for v in opt.views.split(",")}}
    emit(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
