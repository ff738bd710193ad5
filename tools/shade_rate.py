#!/usr/bin/env python3
"""Rate of the shaded ray queries on device buffers, on the rays, views and orders of tools/ray_query_rate.py: multi-1M at
1920x1080 from the headline and the dense camera, the frame's own primary rays (one CRT_RENDER_WRITE_RAYS frame + crt_read_rays) uploaded
once as torch tensors, in pixel order and in a seeded shuffle. Legs, alternating leg by leg for `--rounds` rounds after a warm-up of every leg:

    radiance         Session.shade_rays(radiance=True)                  two traversals, the shading of both bounces
    surface          Session.shade_rays(radiance=False, surface=True)   one traversal, the first hit's record
    both             Session.shade_rays(radiance=True, surface=True)
    closest          Session.trace_rays(mode="closest") on the same rays: the floor -- one traversal, no shading
    frame            one synchronous frame without flags, its Trace time (crt_last_kernel_ms(2)): the same rays dealt by tiles (pixel order only)

Device legs are timed by HIP events around `--repeats` launches. No rate is promised: the tool reports every leg's median, its spread over
the rounds (min .. max) and the ratios against the two yardsticks of the same run. Needs a GPU: there is no fallback.

    python tools/shade_rate.py [--rounds R] [--repeats K] [--out profiles/shade_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clraytracer_amd import driver, scenes

WRITE_RAYS = 2
W, H = 1920, 1080
LEGS = ("radiance", "surface", "both", "closest")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5, help="queries per timed leg")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "shade_rate.txt"))
    opt = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("shade_rate: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda", 0)
    result = {"metric": "shade_rate", "frame": f"{W}x{H}", "rays": W * H, "rounds": opt.rounds, "repeats": opt.repeats, "views": {}}
    for view_name in ("multi-1M", "multi-1M-dense"):
        sc = scenes.get(view_name)
        with driver.Session(W, H, device=0) as s:
            s.load_scene(sc)
            result["device"] = s.hip.crt_device_name().decode()
            s.render_raw(WRITE_RAYS)
            dirs = s.read_rays().reshape(-1, 3)
            _, _, pos = s.camera()
            n = len(dirs)
            origins = np.tile(pos.astype(np.float32), (n, 1))
            perm = np.random.RandomState(11).permutation(n)
            orders = {"pixel": (origins, dirs), "shuffled": (origins[perm].copy(), dirs[perm].copy())}
            s.render_raw(0)
            frame = torch.from_numpy(s.read_output().reshape(-1, 4)).to(dev)
            view = {}
            for order, (o, d) in orders.items():
                to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
                rad, surf = s.shade_rays(to, td, surface=True)
                hits = int((surf.instance >= 0).sum().item())
                # what is timed is what the frame computes: the radiance, bit for bit
                want = frame if order == "pixel" else frame[torch.from_numpy(perm).to(dev)]
                same = bool(torch.equal(rad.view(torch.int32), want.view(torch.int32)))
                torch.cuda.synchronize()

                def device_leg(call):
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                    for _ in range(opt.repeats):
                        call()
                    ev1.record()
                    torch.cuda.current_stream().synchronize()
                    return ev0.elapsed_time(ev1) / opt.repeats

                def frame_leg():
                    s.render_raw(0)
                    s.sync()
                    return s.kernel_ms(2)

                legs = {"radiance": lambda: device_leg(lambda: s.shade_rays(to, td)),
                        "surface": lambda: device_leg(lambda: s.shade_rays(to, td, radiance=False, surface=True)),
                        "both": lambda: device_leg(lambda: s.shade_rays(to, td, surface=True)),
                        "closest": lambda: device_leg(lambda: s.trace_rays(to, td))}
                if order == "pixel":
                    legs["frame"] = frame_leg
                for f in legs.values():                       # warm-up: every leg once
                    f()
                times = {k: [] for k in legs}
                for _ in range(opt.rounds):
                    for k, f in legs.items():
                        times[k].append(f())
                chunks, no_cull, groups = s.shade_stats()
                rec = {"rays": n, "hits": hits, "radiance_equals_frame": same, "chunks": chunks, "chunks_without_cull": no_cull, "workgroups": groups}
                for k, ts in times.items():
                    rec[k] = {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                              "mrays_per_s": round(n / statistics.median(ts) * 1e-3, 1)}
                view[order] = rec
            result["views"][view_name] = view
    lines = []

    def emit(text):
        print(text)
        lines.append(text)

    emit(f"shaded ray queries on device buffers, {W}x{H} primary rays of multi-1M ({W * H} rays per query), median of {opt.rounds} alternating rounds "
         f"(min .. max), {opt.repeats} queries per leg, device events; {result['device']}")
    for view_name, view in result["views"].items():
        for order, rec in view.items():
            emit(f"{view_name}, {order} order: {rec['hits']} rays hit; radiance equals the frame bit for bit: {rec['radiance_equals_frame']}; "
                 f"{rec['chunks']} chunks claimed by {rec['workgroups']} workgroups, {rec['chunks_without_cull']} without the cull")
            for k in LEGS + (("frame",) if "frame" in rec else ()):
                r = rec[k]
                emit(f"  {k:9s} {r['ms_median']:8.3f} ms ({r['ms_min']:.3f} .. {r['ms_max']:.3f}) = {r['mrays_per_s']:8.1f} Mrays/s")
            c = rec["closest"]["ms_median"]
            emit("  against crt_trace_rays closest (one traversal, no shading): " + ", ".join(f"{k} {rec[k]['ms_median'] / c:.2f} x the time" for k in ("radiance", "surface", "both")))
            if "frame" in rec:
                f = rec["frame"]["ms_median"]
                emit("  against the synchronous frame's Trace (the same rays dealt by tiles): " + ", ".join(f"{k} {rec[k]['ms_median'] / f:.2f} x the time" for k in ("radiance", "both")))
        emit(f"  pixel order against shuffled order (radiance): {view['shuffled']['radiance']['ms_median'] / view['pixel']['radiance']['ms_median']:.2f} x the time")
    emit(json.dumps(result))
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
