#!/usr/bin/env python3
"""Rate of the metering step (libcrt_meter.so) on the 1920x1080 frames of multi-1M -- the headline camera and the dense camera --
and on a constant image, the case in which all 64 lanes of a wave add to one LDS address.

    forms        ms of crtx_meter (both launches) under CRTX_BINS=plain and CRTX_BINS=leader with the library's groups, no AO plane, no outHist
    groups       the same over groups = 32 .. 2048 under both forms: the sweep the library's default is chosen from
    extras       with an AO plane; with outHist; with both and CRTX_HEAL; trimmed fractions (0.5, 0.9)
    resolve      crtx_meter over a rectangle of one pixel with the library's groups and with 2048: the histogram launch has next to nothing to
                 do, so this is the two launches' overhead and the resolve over that many partial records
    expose       crtx_expose without and with an AO plane
    copy         a device copy that moves as many bytes as the call must: 16 B/pixel for the meter (read only), 32 B/pixel for expose
    torch        the same definition composed from torch ops (bit manipulation, bincount, cumsum), both the exact and the trimmed mean; its
                 record is checked against the kernel's first: the integer words and the histogram exactly, the exposure to 1e-6

Every leg is timed with events on the stream around `--repeats` back-to-back calls (a fifth as many for the torch compositions); the legs
alternate for `--rounds` rounds after a warm-up of each; the median round is reported with min .. max. Needs a GPU: there is no fallback.

    python tools/meter_rate.py [--rounds R] [--repeats K] [--out profiles/meter_rate.txt]
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
GROUPS = (32, 64, 128, 256, 512, 1024, 2048)
FORMS = ("plain", "leader")
AO_SAMPLES, AO_RADIUS_OF_CAMERA_DISTANCE = 8, 0.05
KEY, LO, HI = 0.18, 2.0 ** -8, 2.0 ** 8


def torch_meter(torch, color, low=0.0, high=1.0):
    """include/crt_meter.h from torch ops, whole frame, no AO plane, no heal: (record words as a list, hist)"""
    c = color[..., :3]
    l = (c[..., 0] * 0.2126 + c[..., 1] * 0.7152) + c[..., 2] * 0.0722
    valid = (l >= 0.0) & (l < float("inf"))
    q = l.view(torch.int32) >> 7
    q = torch.where(l < 2.0 ** -20, torch.full_like(q, _lib.CRTX_QMIN), torch.where(l >= 2.0 ** 12, torch.full_like(q, _lib.CRTX_QMAX - 1), q))
    n = valid.sum()
    q64 = torch.where(valid, q, torch.zeros_like(q)).to(torch.int64)
    bins = torch.where(valid, (q - _lib.CRTX_QMIN) >> 13, torch.full_like(q, 256))
    hist = torch.bincount(bins.reshape(-1), minlength=257)[:256]
    min_q = torch.where(valid, q, torch.full_like(q, 2 ** 31 - 1)).min()
    max_q = q64.max()
    if low == 0.0 and high == 1.0:
        mean_q = q64.sum() // n
    else:
        lo = torch.floor(n.double() * float(np.float32(low))).long()
        hi = torch.minimum(n, torch.ceil(n.double() * float(np.float32(high))).long())
        cum = torch.cumsum(hist, 0)
        take = (torch.minimum(cum, hi) - torch.maximum(cum - hist, lo)).clamp(min=0)
        centres = _lib.CRTX_QMIN + (torch.arange(256, device=color.device) << 13) + 4096
        mean_q = (take * centres).sum() // (hi - lo)
    average = (mean_q << 7).to(torch.int32).view(torch.float32)
    exposure = (torch.tensor(KEY, dtype=torch.float32, device=color.device) / average).clamp(LO, HI)
    return [exposure, average, mean_q, n, N - n, min_q, max_q], hist


def measure(torch, opt, name, color, ao, emit):
    dev = color.device
    lib = _lib.meter()
    stream = torch.cuda.current_stream(dev).cuda_stream
    record = torch.empty(8, dtype=torch.float32, device=dev)
    hist = torch.empty(256, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.crtx_scratch_bytes(W, H, _lib.CRTX_MAX_GROUPS) // 4, dtype=torch.int32, device=dev)
    out = torch.empty((H, W, 4), dtype=torch.float32, device=dev)

    def meter(groups=0, with_ao=False, with_hist=False, heal=False, fractions=(0.0, 1.0), rect=(0, 0, W, H)):
        m = _lib.CrtxMeter(W, H, color.data_ptr(), ao.data_ptr() if with_ao else None, 0.8, _lib.CRTX_HEAL if heal else 0, *rect, KEY, fractions[0],
                           fractions[1], LO, HI, 1.0, 1.0, groups, None)
        rc = lib.crtx_meter(C.byref(m), record.data_ptr(), hist.data_ptr() if with_hist else None, scratch.data_ptr(), stream)
        if rc:
            raise SystemExit(f"meter_rate: crtx_meter failed with {rc}")

    def expose(with_ao=False):
        e = _lib.CrtxExpose(W, H, color.data_ptr(), ao.data_ptr() if with_ao else None, record.data_ptr(), 0.8, 0)
        rc = lib.crtx_expose(C.byref(e), out.data_ptr(), stream)
        if rc:
            raise SystemExit(f"meter_rate: crtx_expose failed with {rc}")

    def set_form(form):
        if form is not None:
            os.environ["CRTX_BINS"] = form
        else:
            os.environ.pop("CRTX_BINS", None)

    def leg(call, repeats, form=None):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        set_form(form)                  # once per leg, outside the timed window (the library reads it at every call)
        ev0.record()
        for _ in range(repeats):
            call()
        ev1.record()
        torch.cuda.current_stream().synchronize()
        return ev0.elapsed_time(ev1) / repeats

    def run(legs):
        for f, _, *form in legs.values():
            leg(f, 1, *form)
        times = {k: [] for k in legs}
        for _ in range(opt.rounds):
            for k, (f, n, *form) in legs.items():
                times[k].append(leg(f, n, *form))
        return {k: {"median": round(statistics.median(ts), 5), "min": round(min(ts), 5), "max": round(max(ts), 5)} for k, ts in times.items()}

    def copy_leg(moved):
        src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        return (lambda: dst.copy_(src), opt.repeats)

    # ---- the two forms agree, and the torch composition agrees with them, before anything is timed
    words = {}
    for fractions in ((0.0, 1.0), (0.5, 0.9)):
        for form in FORMS:
            set_form(form)
            meter(with_hist=True, fractions=fractions)
            torch.cuda.synchronize()
            words[form] = (record.cpu().numpy().view(np.uint32).copy(), hist.cpu().numpy().copy())
        set_form(None)
        if not (np.array_equal(words["plain"][0], words["leader"][0]) and np.array_equal(words["plain"][1], words["leader"][1])):
            raise SystemExit(f"meter_rate: the two CRTX_BINS forms disagree on {name}")
        t, th = torch_meter(torch, color, *fractions)
        got = words["plain"][0]
        ints = [int(v) for v in t[2:]]
        if ints != [int(v) for v in got[3:]] or not np.array_equal(th.cpu().numpy(), words["plain"][1]):
            raise SystemExit(f"meter_rate: the torch composition differs from crtx_meter on {name}, fractions {fractions}: {ints} against {got[3:].tolist()}")
        e, a = float(t[0]), float(t[1])
        if abs(e - float(got[:1].view(np.float32)[0])) > 1e-6 * e or a != float(got[2:3].view(np.float32)[0]):
            raise SystemExit(f"meter_rate: the torch composition's exposure differs from crtx_meter's on {name}")
    rec = {"record": [float(v) for v in got[:3].view(np.float32)] + [int(v) for v in got[3:]]}

    slow = max(1, opt.repeats // 5)
    legs = {}
    for form in FORMS:
        legs[f"meter {form}"] = (lambda: meter(), opt.repeats, form)
        for g in GROUPS:
            legs[f"meter {form} groups {g}"] = (lambda g=g: meter(groups=g), opt.repeats, form)
        legs[f"meter {form} ao"] = (lambda: meter(with_ao=True), opt.repeats, form)
        legs[f"meter {form} outHist"] = (lambda: meter(with_hist=True), opt.repeats, form)
        legs[f"meter {form} ao outHist heal"] = (lambda: meter(with_ao=True, with_hist=True, heal=True), opt.repeats, form)
        legs[f"meter {form} trimmed"] = (lambda: meter(fractions=(0.5, 0.9)), opt.repeats, form)
    legs["one pixel"] = (lambda: meter(rect=(W // 2, H // 2, W // 2 + 1, H // 2 + 1)), opt.repeats)
    legs["one pixel groups 2048"] = (lambda: meter(groups=2048, rect=(W // 2, H // 2, W // 2 + 1, H // 2 + 1)), opt.repeats)
    legs["expose"] = (lambda: expose(), opt.repeats)
    legs["expose ao"] = (lambda: expose(True), opt.repeats)
    legs["copy 16 B/pixel"] = copy_leg(N * 16)
    legs["copy 20 B/pixel"] = copy_leg(N * 20)
    legs["copy 32 B/pixel"] = copy_leg(N * 32)
    legs["torch exact"] = (lambda: torch_meter(torch, color), slow)
    legs["torch trimmed"] = (lambda: torch_meter(torch, color, 0.5, 0.9), slow)
    L = rec["legs_ms"] = run(legs)
    set_form(None)
    torch.cuda.synchronize()

    fmt = lambda r: f"{r['median']:8.4f} ms ({r['min']:.4f} .. {r['max']:.4f})"
    c16, c20, c32 = (L[f"copy {b} B/pixel"]["median"] for b in (16, 20, 32))
    emit(f"== {name}: exposure {rec['record'][0]:.4f}, average {rec['record'][2]:.5f}, valid {rec['record'][4]}, invalid {rec['record'][5]}, "
         f"{int(np.count_nonzero(words['plain'][1]))} bins in use")
    emit(f"  device copies: 16 B/pixel {fmt(L['copy 16 B/pixel'])}; 20 B/pixel {fmt(L['copy 20 B/pixel'])}; 32 B/pixel {fmt(L['copy 32 B/pixel'])}")
    for form in FORMS:
        m = L[f"meter {form}"]
        emit(f"  crtx_meter {form:6s}: {fmt(m)} = {m['median'] / c16:.2f} x copy; torch ops exact {fmt(L['torch exact'])} (torch / fused "
             f"{L['torch exact']['median'] / m['median']:.1f}); trimmed {fmt(L[f'meter {form} trimmed'])}, torch {fmt(L['torch trimmed'])} (torch / fused "
             f"{L['torch trimmed']['median'] / L[f'meter {form} trimmed']['median']:.1f})")
        emit(f"    groups: " + "; ".join(f"{g} {L[f'meter {form} groups {g}']['median']:.4f}" for g in GROUPS) + " ms")
        emit(f"    with ao {fmt(L[f'meter {form} ao'])} = {L[f'meter {form} ao']['median'] / c20:.2f} x copy; with outHist {fmt(L[f'meter {form} outHist'])}; "
             f"ao + outHist + heal {fmt(L[f'meter {form} ao outHist heal'])}")
    emit(f"  leader / plain: {L['meter leader']['median'] / L['meter plain']['median']:.2f}")
    emit(f"  a rectangle of one pixel (two launches and the resolve): {fmt(L['one pixel'])}; with 2048 groups {fmt(L['one pixel groups 2048'])}")
    emit(f"  crtx_expose: {fmt(L['expose'])} = {L['expose']['median'] / c32:.2f} x copy; with ao {fmt(L['expose ao'])}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=100, help="calls per timed leg (a fifth as many of the torch compositions)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meter_rate.txt"))
    ap.add_argument("--views", default="multi-1M,multi-1M-dense")
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("meter_rate: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"metering (crtx_meter, crtx_expose) on {W}x{H} images; events on the stream, median of {opt.rounds} alternating rounds of {opt.repeats} calls "
         f"(min .. max); x copy = times the device copy that moves as many bytes as the call must (the floor); library groups "
         f"{min(_lib.CRTX_DEFAULT_GROUPS, ((W + 31) // 32) * ((H + 7) // 8))}")
    result = {"metric": "meter_rate", "frame": f"{W}x{H}", "rounds": opt.rounds, "repeats": opt.repeats, "images": {}}
    for view in opt.views.split(","):
        with driver.Session(W, H, device=0) as s:
            s.load_scene(scenes.get(view))
            device = s.hip.crt_device_name().decode()
            s.render(gbuffer=True)
            color = torch.from_numpy(np.array(s.output(), copy=True)).to(dev)
            t = s.read_gbuffer_raw()["geometry"]["t"]
            hit = t <= 99998.0
            radius = AO_RADIUS_OF_CAMERA_DISTANCE * float(np.median(t[hit]))
            ao = torch.from_numpy(np.array(s.ambient_occlusion(AO_SAMPLES, radius=radius, bias=1e-3 * radius), copy=True)).to(dev)
        result["device"] = device
        result["images"][view] = measure(torch, opt, f"{view} ({device})", color, ao, emit)
    color = torch.full((H, W, 4), 0.5, dtype=torch.float32, device=dev)
    ao = torch.full((H, W), 0.75, dtype=torch.float32, device=dev)
    result["images"]["constant"] = measure(torch, opt, "a constant image (0.5)", color, ao, emit)
    emit(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
