#!/usr/bin/env python3
"""Supersampling rate: multi-1M at the headline camera and the dense view, the SAME 3840x2160 ray set traced three ways --
plain 3840x2160, CRT_RENDER_SSAA2 at 1920x1080 and CRT_RENDER_SSAA4 at 960x540 (explicit matrices of the 3840x2160 camera) -- each as
frames in flight (the default slots) and as synchronous frames. Prints one JSON line: Mrays/s, ms per frame and the Trace kernel's name
of every leg. Run on the GPU box.

    python tools/ssaa_rate.py [--frames K] [--warmup W]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clraytracer_amd import _lib, driver, scenes

ASYNC, COUNT, SSAA2, SSAA4 = 4, 8, 2048, 4096
LEGS = (("plain_3840x2160", 0, 3840, 2160), ("ssaa2_1920x1080", SSAA2, 1920, 1080), ("ssaa4_960x540", SSAA4, 960, 540))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    opt = ap.parse_args()
    hip = _lib.hip()
    fp = C.POINTER(C.c_float)
    result = {"metric": "ssaa_rate", "unit": "Mrays/s", "frames": opt.frames, "views": {}}
    for view_name in ("multi-1M", "multi-1M-dense"):
        sc = scenes.get(view_name)
        legs = {}
        with driver.Session(3840, 2160, device=0) as s:
            s.load_scene(sc)
            iv, ip, pos = s.camera()                     # the 3840x2160 camera: every leg traces its ray set
            for name, ss, w, h in LEGS:
                s.resize(w, h)
                s.render_raw(ss | COUNT, view=(iv, ip, pos))
                rays = s.counters()["rays"]
                a, _, _ = s.trace_args()
                a.cameraPos[0], a.cameraPos[1], a.cameraPos[2] = (float(x) for x in pos)
                args = (C.byref(a), iv.ctypes.data_as(fp), ip.ctypes.data_as(fp))
                leg = {"rays": rays}
                for mode, flags in (("in_flight", ss | ASYNC), ("synchronous", ss)):
                    for _ in range(opt.warmup):
                        _lib.check(hip.crt_render(*args, flags), "crt_render")
                    _lib.check(hip.crt_sync(), "crt_sync")
                    t0 = time.perf_counter()
                    for _ in range(opt.frames):
                        _lib.check(hip.crt_render(*args, flags), "crt_render")
                    _lib.check(hip.crt_sync(), "crt_sync")
                    dt = (time.perf_counter() - t0) / opt.frames
                    leg[mode] = {"ms_per_frame": round(dt * 1e3, 4), "mrays_per_s": round(rays / dt / 1e6, 1), "kernel": s.last_kernel()}
                legs[name] = leg
        for mode in ("in_flight", "synchronous"):
            base = legs["plain_3840x2160"][mode]["mrays_per_s"]
            for name in ("ssaa2_1920x1080", "ssaa4_960x540"):
                legs[name][mode]["vs_plain"] = round(legs[name][mode]["mrays_per_s"] / base, 4)
        result["views"][view_name] = legs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
