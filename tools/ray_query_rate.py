#!/usr/bin/env python3
"""Rate of the ray queries on device buffers: multi-1M at 1920x1080 from the headline and the dense camera. The rays are
the frame's own primary rays (one CRT_RENDER_WRITE_RAYS frame + crt_read_rays), uploaded once as torch tensors, in pixel order and in a
seeded shuffle. Legs, alternating leg by leg for `--rounds` rounds after a warm-up of every leg:

    closest          Session.trace_rays(mode="closest")
    occluded         Session.trace_rays(mode="occluded")
    occluded-half    the same with tmax = half the closest t (no ray is occluded: what a bounded visibility query costs)
    query_hits       crt_query_hits on the same rays from host memory (24 B per ray in, 20 B out over the host link, synchronous)

Every leg is timed by a host clock around a stream synchronise (end to end); the device legs also by HIP events around the launch (the
device route's own time). Reports the median leg in Mrays/s, the run-to-run spread of every leg (min .. max over the rounds), pixel
order against the shuffled order and the device route against crt_query_hits. Needs a GPU: there is no fallback. Run on the GPU box.

    python tools/ray_query_rate.py [--rounds R] [--repeats K] [--out profiles/ray_query_rate.txt]

--inclusive: the inclusive box test against the plain mode of the same build, on the same rays, alternating leg by leg --
closest, closest-inclusive, occluded, occluded-inclusive -- for two ray sets: the camera rays in pixel order (they start outside every box:
the rule should cost about nothing) and "surface" rays, the workload the mode exists for: the frame's first hits (G-buffer) as origins,
stepped 1e-3 of their t back towards the camera, with the camera ray reflected about the stored normal as direction. Writes its section of
profiles/inclusive_rate.txt (tools/ao_rate.py --inclusive writes the other).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clraytracer_amd import driver, scenes

WRITE_RAYS = 2
W, H = 1920, 1080


def write_section(path, head, lines):
    """replace the section of `path` that starts with a line beginning with `head` (sections start with "== ") by `lines`, or append it"""
    kept, skip = [], False
    if os.path.exists(path):
        for line in open(path).read().splitlines():
            if line.startswith("== "):
                skip = line.startswith(head)
            if not skip:
                kept.append(line)
    with open(path, "w") as f:
        f.write("\n".join(kept + lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5, help="queries per timed leg (device legs)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ray_query_rate.txt"))
    ap.add_argument("--inclusive", action="store_true", help="the inclusive box test against the plain mode (see above)")
    opt = ap.parse_args()
    if opt.inclusive and opt.out == ap.get_default("out"):
        opt.out = os.path.join(os.path.dirname(opt.out), "inclusive_rate.txt")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ray_query_rate: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda", 0)
    result = {"metric": "ray_query_rate", "frame": f"{W}x{H}", "rays": W * H, "rounds": opt.rounds, "repeats": opt.repeats, "views": {}}
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
            if opt.inclusive:
                s.render(gbuffer=True)
                g = s.read_gbuffer()["geometry"].reshape(-1)
                hit = ~(g["t"] > np.float32(99998.0))
                nrm, t = np.ascontiguousarray(g["normal"], np.float32)[hit], g["t"].astype(np.float32)[hit]
                dh = dirs[hit]
                refl = dh - 2.0 * (dh * nrm).sum(axis=1, keepdims=True) * nrm
                orders = {"camera": (origins, dirs), "surface": (np.ascontiguousarray(origins[hit] + dh * (t * np.float32(1.0 - 1e-3))[:, None], np.float32),
                                                                 np.ascontiguousarray(refl, np.float32))}
            view = {}
            for order, (o, d) in orders.items():
                n = len(d)
                to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
                closest = s.trace_rays(to, td)
                half = (closest.t * 0.5).contiguous()
                hits = int((closest.instance >= 0).sum().item())
                occluded_at_half = int(s.trace_rays(to, td, tmax=half, mode="occluded").sum().item())
                torch.cuda.synchronize()

                def device_leg(mode, tmax=None, inclusive=False):
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    ev0.record()
                    for _ in range(opt.repeats):
                        s.trace_rays(to, td, tmax=tmax, mode=mode, inclusive=inclusive)
                    ev1.record()
                    torch.cuda.current_stream().synchronize()
                    host = (time.perf_counter() - t0) / opt.repeats
                    return host, ev0.elapsed_time(ev1) * 1e-3 / opt.repeats

                def host_leg():
                    t0 = time.perf_counter()
                    s.query_hits(o, d)
                    return time.perf_counter() - t0, None

                legs = {"closest": lambda: device_leg("closest"), "occluded": lambda: device_leg("occluded"),
                        "occluded-half": lambda: device_leg("occluded", half), "query_hits": host_leg}
                if opt.inclusive:
                    legs = {"closest": lambda: device_leg("closest"), "closest-inclusive": lambda: device_leg("closest", inclusive=True),
                            "occluded": lambda: device_leg("occluded"), "occluded-inclusive": lambda: device_leg("occluded", inclusive=True)}
                    hits_inclusive = int((s.trace_rays(to, td, inclusive=True).instance >= 0).sum().item())
                for f in legs.values():                       # warm-up: every leg once
                    f()
                times = {k: [] for k in legs}
                for _ in range(opt.rounds):
                    for k, f in legs.items():
                        times[k].append(f())
                chunks, no_cull, groups = s.rays_stats()
                rec = {"rays": n, "hits": hits, "occluded_at_half_t": occluded_at_half, "chunks": chunks, "chunks_without_cull": no_cull, "workgroups": groups}
                if opt.inclusive:
                    rec["hits_inclusive"] = hits_inclusive
                for k, ts in times.items():
                    host = [t[0] for t in ts]
                    rec[k] = {"host_ms_median": round(statistics.median(host) * 1e3, 4), "host_ms_min": round(min(host) * 1e3, 4), "host_ms_max": round(max(host) * 1e3, 4),
                              "mrays_per_s_end_to_end": round(n / statistics.median(host) * 1e-6, 1)}
                    if ts[0][1] is not None:
                        evt = [t[1] for t in ts]
                        rec[k].update({"event_ms_median": round(statistics.median(evt) * 1e3, 4), "event_ms_min": round(min(evt) * 1e3, 4), "event_ms_max": round(max(evt) * 1e3, 4),
                                       "mrays_per_s_device": round(n / statistics.median(evt) * 1e-6, 1)})
                view[order] = rec
            result["views"][view_name] = view
    lines = []

    def emit(text):
        print(text)
        lines.append(text)

    if opt.inclusive:
        emit(f"== ray_query_rate --inclusive: the inclusive box test against the plain mode, same build, same rays; multi-1M at {W}x{H}, median of {opt.rounds} alternating rounds, "
             f"{opt.repeats} queries per leg, device events; {result['device']}")
        for view_name, view in result["views"].items():
            for order, rec in view.items():
                emit(f"{view_name}, {order} rays: {rec['rays']} rays, {rec['hits']} hit under upstream's rule, {rec['hits_inclusive']} under the inclusive rule; {rec['chunks_without_cull']} chunks without the cull")
                for k in ("closest", "closest-inclusive", "occluded", "occluded-inclusive"):
                    r = rec[k]
                    emit(f"  {k:19s} {r['event_ms_median']:8.3f} ms ({r['event_ms_min']:.3f} .. {r['event_ms_max']:.3f}) = {r['mrays_per_s_device']:8.1f} Mrays/s")
                emit(f"  inclusive against plain: closest {rec['closest-inclusive']['event_ms_median'] / rec['closest']['event_ms_median']:.3f} x the time, "
                     f"occluded {rec['occluded-inclusive']['event_ms_median'] / rec['occluded']['event_ms_median']:.3f} x")
        emit(json.dumps(result))
        write_section(opt.out, "== ray_query_rate", lines)
        return
    emit(f"ray queries on device buffers, {W}x{H} primary rays of multi-1M ({W * H} rays per query), median of {opt.rounds} alternating rounds, {opt.repeats} queries per device leg; {result['device']}")
    for view_name, view in result["views"].items():
        for order, rec in view.items():
            emit(f"{view_name}, {order} order: {rec['hits']} rays hit ({rec['occluded_at_half_t']} occluded within half their t); {rec['chunks']} chunks claimed by {rec['workgroups']} workgroups, {rec['chunks_without_cull']} without the cull")
            for k in ("closest", "occluded", "occluded-half", "query_hits"):
                r = rec[k]
                line = f"  {k:14s} end to end {r['host_ms_median']:9.3f} ms ({r['host_ms_min']:.3f} .. {r['host_ms_max']:.3f}) = {r['mrays_per_s_end_to_end']:8.1f} Mrays/s"
                if "event_ms_median" in r:
                    line += f"; device events {r['event_ms_median']:8.3f} ms ({r['event_ms_min']:.3f} .. {r['event_ms_max']:.3f}) = {r['mrays_per_s_device']:8.1f} Mrays/s"
                emit(line)
            emit(f"  device route against crt_query_hits, end to end: {rec['query_hits']['host_ms_median'] / rec['closest']['host_ms_median']:.1f} x")
        emit(f"  pixel order against shuffled order (closest, device events): {view['shuffled']['closest']['event_ms_median'] / view['pixel']['closest']['event_ms_median']:.2f} x the time")
    emit(json.dumps(result))
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
