#!/usr/bin/env python3
"""Rate of temporal accumulation that follows moving instances (libcrt_motion.so) on 1920x1080 G-buffer frames of multi-1M with
seeded noise on their colour: the headline camera (a third of the pixels are hits) and the dense camera (nearly all are). Frame 0 is the
scene as it stands and makes the history; before frame 1 every instance turns by 0.002 rad about its own y axis (about a pixel on the screen)
and is uploaded again; every timed call accumulates frame 1 into the history of frame 0, without flags and with CRTT_CLAMP.

    crtt            crtt_accumulate (libcrt_temporal.so): the baseline of the same run
    null            crtm_accumulate with a NULL table              } against crtt: what the second library costs where it has nothing to do
    static          ... with a table whose every entry is CRTM_STATIC: the cost of the table fetch (the kind, per lane)
    moving          ... with the table of the turn, every entry CRTM_MOVING: against static, the cost of the matrices and their arithmetic
    +vectors        each crtm leg again with the motion-vector plane: the cost of its 16-B store per pixel
    --variant NAME=PATH   the static and moving legs again through another build of the library (the fetch variants that
                    tools/experiments/motion_fetch_variants.patch brings back, built with make PATH MOTION_SO=PATH EXTRA_HIPFLAGS=-DCRTM_FETCH=n);
                    its results are first compared bit for bit with the shipped build's

Every leg is timed with events on the stream around `--repeats` back-to-back calls; the legs alternate for `--rounds` rounds after a warm-up of
each; the median round is reported with min .. max. Needs a GPU: there is no fallback.

    python tools/motion_rate.py [--rounds R] [--repeats K] [--variant NAME=PATH ...] [--out profiles/motion_rate.txt]
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
TURN = 0.002                                # radians about each instance's own y axis between the two frames


def turned(records):
    """the records with every instance turned by TURN about its local y axis: p_local = (p_world * inv) * R^-1"""
    c, s = np.cos(TURN), np.sin(TURN)
    back = np.array([[c, 0.0, s, 0.0], [0.0, 1.0, 0.0, 0.0], [-s, 0.0, c, 0.0], [0.0, 0.0, 0.0, 1.0]])
    out = records.copy()
    out["inv"] = (records["inv"].astype(np.float64) @ back).astype(np.float32)
    return out


def measure(torch, opt, view_name, variants, emit):
    """every leg on one view; prints through emit() and returns the view's record"""
    dev = torch.device("cuda", 0)
    sc = scenes.get(view_name)
    frames = []
    with driver.Session(W, H, device=0) as s:
        s.load_scene(sc)
        device_name = s.hip.crt_device_name().decode()
        records = [s.arenas()["instances"]]
        records.append(turned(records[0]))
        for i in range(2):
            if i:
                s.upload_instances(records[1])
            s.render(gbuffer=True)
            g = s.read_gbuffer_raw()
            frame = s.read_output()
            noisy = (frame + np.random.RandomState(1 + i).normal(0, 0.2, frame.shape) * np.array([1, 1, 1, 0])).astype(np.float32)
            frames.append({"color": torch.from_numpy(noisy).to(dev),
                           "geometry": torch.from_numpy(np.concatenate([g["geometry"]["normal"], g["geometry"]["t"][..., None]], axis=-1)).to(dev),
                           "ids": torch.from_numpy(g["ids"].view(np.int32).reshape(H, W, 4).copy()).to(dev),
                           "camera": _lib.crtt_camera(*s.camera(), W, H), "hit_share": float((g["geometry"]["t"] <= 99998.0).mean())})
    host_tables = {"moving": _lib.crtm_motions(records[0], records[1]), "static": _lib.crtm_motions(records[0], records[0])}
    assert (host_tables["moving"]["kind"] == _lib.CRTM_MOVING).all() and (host_tables["static"]["kind"] == _lib.CRTM_STATIC).all()
    tables = {k: torch.from_numpy(v.view(np.uint8)).to(dev) for k, v in host_tables.items()}
    sets = [{"color": torch.empty((H, W, 4), device=dev), "moments": torch.empty((H, W, 4), device=dev), "geometry": torch.empty((H, W, 4), device=dev),
             "instance": torch.empty((H, W), dtype=torch.int32, device=dev)} for _ in range(2)]
    vectors = torch.empty((H, W, 4), device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    libs = {"": _lib.motion()}
    for name, path in variants.items():
        libs[name] = _lib._bind(path, _lib.MOTION_API)
    cur = frames[1]

    def history(i, cam):
        return _lib.CrttHistory(*[sets[i][k].data_ptr() for k in ("color", "moments", "geometry", "instance")], cam)

    def call(which, flags, table=None, with_vectors=False, reset=False, lib=""):
        fr = frames[0] if reset else cur
        f = _lib.CrttFrame(W, H, fr["color"].data_ptr(), _lib.CRTT_GUIDES_PLANES, fr["geometry"].data_ptr(), fr["ids"].data_ptr(), fr["camera"])
        p = _lib.CrttParams(flags, PARAMS["alpha"], PARAMS["moments_alpha"], PARAMS["max_history"], PARAMS["depth_tol"], PARAMS["normal_cos"])
        prev, nxt = history(0, frames[0]["camera"]), history(0 if reset else 1, fr["camera"])
        if which == "crtt":
            rc = _lib.temporal().crtt_accumulate(C.byref(f), None if reset else C.byref(prev), C.byref(nxt), C.byref(p), stream)
        else:
            t = tables[table] if table else None
            m = _lib.CrtmMotionArgs(t.data_ptr() if t is not None else None, len(records[0]) if t is not None else 0, vectors.data_ptr() if with_vectors else None)
            rc = libs[lib].crtm_accumulate(C.byref(f), None if reset else C.byref(prev), C.byref(nxt), C.byref(p), C.byref(m), stream)
        if rc:
            raise SystemExit(f"motion_rate: {which} failed with {rc}: {_lib.motion().crtm_error_string(rc).decode()}")

    # set 0: the history of frame 0 after one frame; every timed call reads it and writes set 1
    call("crtt", 0, reset=True)
    snapshot = lambda: torch.cat([sets[1]["color"].view(torch.int32), sets[1]["moments"].view(torch.int32)], dim=-1).clone()
    hit = cur["geometry"][..., 3] <= 99998.0
    kept, agreement = {}, {}
    for flags in (0, _lib.CRTT_CLAMP):
        call("crtt", flags); base = snapshot()
        kept["crtt"] = float((sets[1]["moments"][..., 2][hit] > 1.0).float().mean())
        for table in (None, "static"):
            call("crtm", flags, table, with_vectors=True)
            if not bool((snapshot() == base).all()):
                raise SystemExit(f"motion_rate: crtm_accumulate with table={table} differs from crtt_accumulate (flags {flags})")
        call("crtm", flags, "moving", with_vectors=True); moved = snapshot()
        kept["moving"] = float((sets[1]["moments"][..., 2][hit] > 1.0).float().mean())
        agreement[f"flags {flags}"] = {"pixels where following the turn changes the result": int((moved != base).any(dim=-1).sum())}
        for name in variants:
            for table, want in (("static", base), ("moving", moved)):
                call("crtm", flags, table, with_vectors=True, lib=name)
                if not bool((snapshot() == want).all()):
                    raise SystemExit(f"motion_rate: variant {name} differs from the shipped build (table={table}, flags {flags})")

    def leg(f):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(opt.repeats):
            f()
        ev1.record()
        torch.cuda.current_stream().synchronize()
        return ev0.elapsed_time(ev1) / opt.repeats

    legs = {}
    for flags, tag in ((0, ""), (_lib.CRTT_CLAMP, "+clamp")):
        legs[f"crtt{tag}"] = lambda flags=flags: call("crtt", flags)
        for table, name in ((None, "null"), ("static", "static"), ("moving", "moving")):
            for wv in (False, True):
                legs[f"{name}{tag}{'+vectors' if wv else ''}"] = lambda flags=flags, table=table, wv=wv: call("crtm", flags, table, with_vectors=wv)
        for v in variants:
            for table in ("static", "moving"):
                legs[f"{v}:{table}{tag}"] = lambda flags=flags, table=table, v=v: call("crtm", flags, table, lib=v)
    for f in legs.values():
        leg(f); leg(f)
    times = {name: [] for name in legs}
    for _ in range(opt.rounds):
        for name, f in legs.items():
            times[name].append(leg(f))
    rec = {"device": device_name, "hit_share": [round(fr["hit_share"], 4) for fr in frames], "hit_pixels_that_keep_history": {k: round(v, 4) for k, v in kept.items()},
           "agreement": agreement,
           "legs_ms": {name: {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)} for name, ts in times.items()}}
    ms = rec["legs_ms"]
    show = lambda r: f"{r['median']:8.4f} ms ({r['min']:.4f} .. {r['max']:.4f})"
    emit(f"== {view_name}: {cur['hit_share']:.1%} of the pixels are hits; {len(records[0])} instances; {device_name}")
    emit(f"  with a NULL table and with an all-static one crtm_accumulate equals crtt_accumulate in every bit; following the turn changes "
         f"{agreement['flags 0']['pixels where following the turn changes the result']} pixels; hit pixels that keep their history: "
         f"camera-only {kept['crtt']:.1%}, following {kept['moving']:.1%}")
    for tag in ("", "+clamp"):
        b = ms[f"crtt{tag}"]
        emit(f"  {'no flags' if not tag else 'CRTT_CLAMP'}: crtt_accumulate {show(b)}, spread {b['max'] - b['min']:.4f}")
        for name in ("null", "static", "moving"):
            a, av = ms[f"{name}{tag}"], ms[f"{name}{tag}+vectors"]
            emit(f"    crtm {name:6s} {show(a)} = {a['median'] / b['median']:.3f} x crtt; with vectors {show(av)} (+{av['median'] - a['median']:.4f})")
        emit(f"    table fetch (static - crtt) {ms[f'static{tag}']['median'] - b['median']:+.4f} ms; matrices (moving - static) "
             f"{ms[f'moving{tag}']['median'] - ms[f'static{tag}']['median']:+.4f} ms")
        for v in variants:
            emit(f"    variant {v}: static {show(ms[f'{v}:static{tag}'])}, moving {show(ms[f'{v}:moving{tag}'])}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=10, help="calls per timed leg")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=PATH", help="another build of libcrt_motion.so to time beside the shipped one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_rate.txt"))
    opt = ap.parse_args()
    variants = {}
    for v in opt.variant:
        name, _, path = v.partition("=")
        if not name or not os.path.exists(path):
            raise SystemExit(f"motion_rate: --variant {v}: NAME=PATH of a built library is required")
        variants[name] = os.path.abspath(path)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("motion_rate: no GPU (this tool measures; it does not fall back)")
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    emit(f"temporal accumulation following moving instances (crtm_accumulate) on {W}x{H} G-buffer frames of multi-1M, seeded noise on the colour, every "
         f"instance turned by {TURN} rad between the frames; events on the stream, median of {opt.rounds} alternating rounds of {opt.repeats} calls (min .. max)")
    result = {"metric": "motion_rate", "frame": f"{W}x{H}", "rounds": opt.rounds, "repeats": opt.repeats, "variants": sorted(variants),
              "views": {view_name: measure(torch, opt, view_name, variants, emit) for view_name in ("multi-1M", "multi-1M-dense")}}
    emit(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
