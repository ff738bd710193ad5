#!/usr/bin/env python3
"""Rate of ambient occlusion on a G-buffer frame: multi-1M at 1920x1080 from the headline and the dense camera, N = 8 sample
rays per pixel, radius = 0.1 x the diagonal of the bounding box of the frame's first-hit points. Two legs on the same sample rays, in the same
run, alternating leg by leg for `--rounds` rounds after a warm-up of both:

    fused          crt_frame_ao: the rays are generated in registers, traced and reduced per pixel by one kernel (4 B per pixel written)
    materialised   the route of the API before: the same rays (tests/ao_ref.py's restatement of the definition, uploaded once as torch
                   tensors: 28 B per ray) through Session.trace_rays(mode="occluded") -- the query alone is timed, neither the generation of
                   the rays nor the reduction of the answers, which that route needs too

Both legs are timed with events on the stream around `--repeats` back-to-back calls; reports the median leg in ms per frame and sample rays per
second (the rays of the pixels that trace: a pixel of sky has none), and the run-to-run spread of every leg (min .. max over the rounds). The
fused plane is checked against the composition of the materialised answers before anything is timed. Needs a GPU: there is no fallback.

    python tools/ao_rate.py [--rounds R] [--repeats K] [--out profiles/ao_rate.txt]

--inclusive: the fused kernel under CRT_AO_INCLUSIVE against the plain fused kernel of the same build on the same frame,
alternating leg by leg; the inclusive plane is checked against the composition of the inclusive occlusion query first. Writes its section of
profiles/inclusive_rate.txt (tools/ray_query_rate.py --inclusive writes the other).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from clraytracer_amd import _lib, driver, scenes
import ao_ref

WRITE_RAYS = 2
W, H, SAMPLES, BIAS_OF_RADIUS, RADIUS_OF_EXTENT = 1920, 1080, 8, 1e-3, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3, help="calls per timed leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ao_rate.txt"))
    ap.add_argument("--inclusive", action="store_true", help="CRT_AO_INCLUSIVE against the plain fused kernel (see above)")
    opt = ap.parse_args()
    if opt.inclusive and opt.out == ap.get_default("out"):
        opt.out = os.path.join(ROOT, "profiles", "inclusive_rate.txt")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ao_rate: no GPU (this tool measures; it does not fall back)")
    dev = torch.device("cuda", 0)
    table = ao_ref.table()
    result = {"metric": "ao_rate", "frame": f"{W}x{H}", "samples": SAMPLES, "rounds": opt.rounds, "repeats": opt.repeats, "views": {}}
    for view_name in ("multi-1M", "multi-1M-dense"):
        sc = scenes.get(view_name)
        with driver.Session(W, H, device=0) as s:
            s.load_scene(sc)
            result["device"] = s.hip.crt_device_name().decode()
            s.render_raw(WRITE_RAYS)
            dirs = s.read_rays()
            _, _, pos = s.camera()
            s.render(gbuffer=True)
            P, n, k = ao_ref.frame_items(s.read_gbuffer(), dirs, pos)
            traces = (n != 0).any(axis=1)
            box = P[traces].astype(np.float64)
            extent = float(np.linalg.norm(box.max(axis=0) - box.min(axis=0)))
            radius = RADIUS_OF_EXTENT * extent
            par = {"samples": SAMPLES, "radius": radius, "bias": BIAS_OF_RADIUS * radius, "seed": 0}
            o, d, w = ao_ref.rays(P, n, k, par, table)
            to = torch.from_numpy(np.repeat(o, SAMPLES, axis=0)).to(dev)
            td = torch.from_numpy(np.ascontiguousarray(d.reshape(-1, 3))).to(dev)
            tt = torch.full((len(to),), radius, dtype=torch.float32, device=dev)
            cp = _lib.CrtAoParams(SAMPLES, radius, par["bias"], 0, 0, 0.0, 0.0)
            stream = torch.cuda.current_stream(dev).cuda_stream
            # the two routes agree, bit for bit, before either is timed
            fused = s.ambient_occlusion(SAMPLES, radius=radius, bias=par["bias"])
            occ = s.trace_rays(to, td, tmax=tt, mode="occluded").cpu().numpy().reshape(-1, SAMPLES)
            if not np.array_equal(fused.reshape(-1).view(np.uint32), ao_ref.compose(w, occ).view(np.uint32)):
                raise SystemExit(f"ao_rate: {view_name}: the fused plane differs from the composition of the materialised answers")
            rays = int(traces.sum()) * SAMPLES

            def leg(call):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(opt.repeats):
                    call()
                ev1.record()
                torch.cuda.current_stream().synchronize()
                return ev0.elapsed_time(ev1) * 1e-3 / opt.repeats

            legs = {"fused": lambda: _lib.check(s.hip.crt_frame_ao(C.byref(cp), stream), "crt_frame_ao"),
                    "materialised": lambda: s.trace_rays(to, td, tmax=tt, mode="occluded")}
            if opt.inclusive:
                cpi = _lib.CrtAoParams(SAMPLES, radius, par["bias"], 0, _lib.CRT_AO_INCLUSIVE, 0.0, 0.0)
                fused_inc = s.ambient_occlusion(SAMPLES, radius=radius, bias=par["bias"], inclusive=True).copy()
                occ_inc = s.trace_rays(to, td, tmax=tt, mode="occluded", inclusive=True).cpu().numpy().reshape(-1, SAMPLES)
                if not np.array_equal(fused_inc.reshape(-1).view(np.uint32), ao_ref.compose(w, occ_inc).view(np.uint32)):
                    raise SystemExit(f"ao_rate: {view_name}: the inclusive fused plane differs from the composition of the inclusive occlusion answers")
                legs = {"fused": legs["fused"], "fused-inclusive": lambda: _lib.check(s.hip.crt_frame_ao(C.byref(cpi), stream), "crt_frame_ao")}
            for f in legs.values():                           # warm-up: every leg once
                leg(f)
            times = {name: [] for name in legs}
            for _ in range(opt.rounds):
                for name, f in legs.items():
                    times[name].append(leg(f))
            rec = {"radius": round(radius, 4), "extent": round(extent, 3), "tracing_pixels": int(traces.sum()), "sample_rays": rays,
                   "materialised_rays": len(to), "occluded_share": round(float(occ[traces].mean()), 4), "mean_ao": round(float(fused.mean()), 4),
                   "ao_stats": s.ao_stats()}
            if opt.inclusive:
                rec.update({"occluded_share_inclusive": round(float(occ_inc[traces].mean()), 4), "mean_ao_inclusive": round(float(fused_inc.mean()), 4)})
            for name, ts in times.items():
                med = statistics.median(ts)
                rec[name] = {"ms_median": round(med * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4), "ms_max": round(max(ts) * 1e3, 4),
                             "grays_per_s": round(rays / med * 1e-9, 3)}
            result["views"][view_name] = rec
    lines = []

    def emit(text):
        print(text)
        lines.append(text)

    if opt.inclusive:
        from ray_query_rate import write_section
        emit(f"== ao_rate --inclusive: crt_frame_ao under CRT_AO_INCLUSIVE against the plain fused kernel, same build, same {W}x{H} G-buffer frame of multi-1M, {SAMPLES} sample rays per pixel; "
             f"events on the stream, median of {opt.rounds} alternating rounds of {opt.repeats} calls; {result['device']}")
        for view_name, rec in result["views"].items():
            emit(f"{view_name}: radius {rec['radius']}, {rec['sample_rays']} sample rays; occluded share {rec['occluded_share']} (mean AO {rec['mean_ao']}) under upstream's rule, "
                 f"{rec['occluded_share_inclusive']} (mean AO {rec['mean_ao_inclusive']}) under the inclusive rule")
            for name in ("fused", "fused-inclusive"):
                r = rec[name]
                emit(f"  {name:16s} {r['ms_median']:9.3f} ms per frame ({r['ms_min']:.3f} .. {r['ms_max']:.3f}) = {r['grays_per_s']:7.3f} G sample rays/s")
            emit(f"  inclusive against plain: {rec['fused-inclusive']['ms_median'] / rec['fused']['ms_median']:.3f} x the time")
        emit(json.dumps(result))
        write_section(opt.out, "== ao_rate", lines)
        return
    emit(f"ambient occlusion of a {W}x{H} G-buffer frame of multi-1M, {SAMPLES} sample rays per pixel, radius = {RADIUS_OF_EXTENT} x the extent of the frame's hit points, "
         f"bias = {BIAS_OF_RADIUS} x the radius; events on the stream, median of {opt.rounds} alternating rounds of {opt.repeats} calls; {result['device']}")
    for view_name, rec in result["views"].items():
        emit(f"{view_name}: radius {rec['radius']} (extent {rec['extent']}), {rec['tracing_pixels']} pixels trace {rec['sample_rays']} sample rays, {rec['occluded_share']} of them occluded, "
             f"mean AO {rec['mean_ao']}; {rec['ao_stats'][0]} tiles claimed by {rec['ao_stats'][2]} workgroups, {rec['ao_stats'][1]} without the cull")
        for name in ("fused", "materialised"):
            r = rec[name]
            emit(f"  {name:13s} {r['ms_median']:9.3f} ms per frame ({r['ms_min']:.3f} .. {r['ms_max']:.3f}) = {r['grays_per_s']:7.3f} G sample rays/s")
        emit(f"  the materialised query ({rec['materialised_rays']} rays, 28 B each, in HBM; their generation and the reduction not timed) takes "
             f"{rec['materialised']['ms_median'] / rec['fused']['ms_median']:.2f} x the fused kernel's time")
    emit(json.dumps(result))
    with open(opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
