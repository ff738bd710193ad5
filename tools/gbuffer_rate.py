#!/usr/bin/env python3
"""Cost of CRT_RENDER_GBUFFER: multi-1M at 1920x1080, the headline camera and the dense view, as synchronous frames and
as frames in flight (the default three slots), with and without the flag -- the two alternate leg by leg, `--rounds` times, and the
median leg is reported -- and, in the same process, what the flag replaces: a plain frame with CRT_RENDER_WRITE_RAYS, crt_read_rays
and crt_query_hits over the same view (which yields t, u, v, triangle and instance, but neither normal nor albedo), next to a
G-buffer frame with crt_read_gbuffer of all three planes, and one crt_pick_pixel. Prints a table and one JSON line. Run on the GPU box.

    python tools/gbuffer_rate.py [--frames K] [--warmup W] [--rounds R] > profiles/gbuffer_rate.txt
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clraytracer_amd import _lib, driver, scenes

WRITE_RAYS, ASYNC, COUNT, GBUFFER = 2, 4, 8, 8192
W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    opt = ap.parse_args()
    hip = _lib.hip()
    fp = C.POINTER(C.c_float)
    result = {"metric": "gbuffer_rate", "frame": f"{W}x{H}", "frames_per_leg": opt.frames, "rounds": opt.rounds, "views": {}}
    for view_name in ("multi-1M", "multi-1M-dense"):
        sc = scenes.get(view_name)
        with driver.Session(W, H, device=0) as s:
            s.load_scene(sc)
            s.render_raw(COUNT)
            rays = s.counters()["rays"]
            a, iv, ip = s.trace_args()
            args = (C.byref(a), iv.ctypes.data_as(fp), ip.ctypes.data_as(fp))

            def leg(flags):
                for _ in range(opt.warmup):
                    _lib.check(hip.crt_render(*args, flags), "crt_render")
                _lib.check(hip.crt_sync(), "crt_sync")
                t0 = time.perf_counter()
                for _ in range(opt.frames):
                    _lib.check(hip.crt_render(*args, flags), "crt_render")
                _lib.check(hip.crt_sync(), "crt_sync")
                return (time.perf_counter() - t0) / opt.frames * 1e3

            view = {"rays_per_frame": rays}
            for mode, base in (("synchronous", 0), ("in_flight", ASYNC)):
                ms = {"plain": [], "gbuffer": []}
                kern = {}
                for _ in range(opt.rounds):
                    for name, flags in (("plain", base), ("gbuffer", base | GBUFFER)):
                        ms[name].append(leg(flags))
                        kern[name] = s.last_kernel()
                med = {k: statistics.median(v) for k, v in ms.items()}
                view[mode] = {"plain_ms": round(med["plain"], 4), "gbuffer_ms": round(med["gbuffer"], 4),
                              "plain_ms_min_max": [round(min(ms["plain"]), 4), round(max(ms["plain"]), 4)],
                              "gbuffer_ms_min_max": [round(min(ms["gbuffer"]), 4), round(max(ms["gbuffer"]), 4)],
                              "gbuffer_vs_plain": round(med["gbuffer"] / med["plain"], 4),
                              "plain_gray_s": round(rays / med["plain"] / 1e6, 2), "gbuffer_gray_s": round(rays / med["gbuffer"] / 1e6, 2),
                              "kernels": kern}
            # what the flag replaces: the hit records of the frame's primary rays on the host, by the only route without it
            rays_buf = np.empty((H * W, 3), np.float32)
            origins = np.tile(s.camera()[2], (H * W, 1)).astype(np.float32)
            rec = np.zeros(H * W, _lib.RAYHIT_DTYPE)
            planes = {n: np.empty((H, W), d) for n, (_, d) in _lib.GBUFFER_PLANE_DTYPES.items()}
            pix = np.zeros(1, _lib.GBUFFER_PIXEL_DTYPE)
            old, new, pick = [], [], []
            for _ in range(max(3, opt.rounds)):
                t0 = time.perf_counter()
                _lib.check(hip.crt_render(*args, WRITE_RAYS), "crt_render")
                _lib.check(hip.crt_read_rays(rays_buf.ctypes.data, rays_buf.size), "crt_read_rays")
                _lib.check(hip.crt_query_hits(origins.ctypes.data, rays_buf.ctypes.data, H * W, a.numMeshes, rec.ctypes.data), "crt_query_hits")
                old.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                _lib.check(hip.crt_render(*args, GBUFFER), "crt_render")
                for n, (plane, _) in _lib.GBUFFER_PLANE_DTYPES.items():
                    _lib.check(hip.crt_read_gbuffer(plane, planes[n].ctypes.data, planes[n].nbytes), "crt_read_gbuffer")
                new.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                _lib.check(hip.crt_render(*args, GBUFFER), "crt_render")
                _lib.check(hip.crt_pick_pixel(W // 2, H // 2, pix.ctypes.data), "crt_pick_pixel")
                pick.append((time.perf_counter() - t0) * 1e3)
            ids = planes["ids"].reshape(-1)
            same = bool(np.array_equal(ids["instance"], rec["instance"]) and np.array_equal(ids["tri"], rec["tri"])
                        and np.array_equal(planes["geometry"]["t"].reshape(-1).view(np.uint32), rec["t"].view(np.uint32)))
            view["records_on_the_host"] = {"write_rays_read_rays_query_hits_ms": round(statistics.median(old), 3),
                                           "gbuffer_frame_read_three_planes_ms": round(statistics.median(new), 3),
                                           "gbuffer_frame_pick_one_pixel_ms": round(statistics.median(pick), 3),
                                           "same_records": same, "hit_share": round(float((ids["instance"] >= 0).mean()), 4)}
        result["views"][view_name] = view
        print(f"{view_name} {W}x{H}, {rays} rays per frame, {opt.frames} frames per leg, median of {opt.rounds} alternating legs")
        for mode in ("synchronous", "in_flight"):
            v = view[mode]
            print(f"  {mode:12s} plain {v['plain_ms']:.4f} ms [{v['plain_ms_min_max'][0]:.4f}, {v['plain_ms_min_max'][1]:.4f}]  {v['kernels']['plain']}")
            print(f"  {'':12s} gbuf  {v['gbuffer_ms']:.4f} ms [{v['gbuffer_ms_min_max'][0]:.4f}, {v['gbuffer_ms_min_max'][1]:.4f}]  {v['kernels']['gbuffer']}  x{v['gbuffer_vs_plain']:.4f}")
        r = view["records_on_the_host"]
        print(f"  hit records on the host: WRITE_RAYS frame + crt_read_rays + crt_query_hits {r['write_rays_read_rays_query_hits_ms']:.3f} ms; "
              f"G-buffer frame + crt_read_gbuffer x 3 {r['gbuffer_frame_read_three_planes_ms']:.3f} ms; G-buffer frame + crt_pick_pixel "
              f"{r['gbuffer_frame_pick_one_pixel_ms']:.3f} ms; same records: {r['same_records']}; hit share {r['hit_share']}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
