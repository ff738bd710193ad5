#!/usr/bin/env python3
"""How many instances the wave test of the staged cull (crt_device.h: wave_cone, cone_rejects) leaves per tile on the camera bounce, set against
the union of the per-lane masks. Needs no GPU: a host-only session for the scene's arenas and camera, the oracle's RayGen for the rays, and the
float32 numpy restatement the tests use (tests/wave_cull_ref.py).

    python tools/count_wave_cull.py [--scene multi-1M] [--width 1920 --height 1080] > profiles/wave_cull_counts.txt

Per 8 x 8 tile (a wave; lanes in Morton order, lane 0 the tile's first pixel): `survivors` = the instances the wave test does not reject,
`union` = the instances some lane's own predicate (candidate_mask's) lets through. Output: the histogram of both, the totals, and both sets per tile. A partial tile takes no wave test: all survive. Every instance
is taken as cullable, as in tools/count_box_pretest.py. The tool also checks the lemma in float64: no rejected (tile, instance) pair has a lane
whose ray comes within sqrt(1.02 w^2 + 2.8e-6 x^2) of fl(c), and no rejected pair lies in a lane's own mask.
The gate (exit status 1 if missed): mean survivors per tile <= 6."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32


def morton_xy(m):
    return (m & 1) | ((m >> 1) & 2) | ((m >> 2) & 4), ((m >> 1) & 1) | ((m >> 2) & 2) | ((m >> 3) & 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="multi-1M")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    from clraytracer_amd import driver, scenes
    import oracle_lib
    import wave_cull_ref as ref
    from count_box_pretest import table_sphere
    W, H = args.width, args.height
    sc = scenes.get(args.scene)
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        iv, ip, pos = s.camera()
        rays = np.ascontiguousarray(oracle_lib.Oracle(a, nthreads=args.threads).raygen(W, H, iv, ip), F).reshape(H, W, 3)
    cf, w = [], []
    for inst in a["instances"]:
        node = a["nodes"][int(a["roots"][inst["meshIndex"]])]
        kids = a["nodes"][int(node["leftFirst"]):int(node["leftFirst"]) + 2] if node["triCount"] == 0 else [node, node]
        fwd = np.linalg.inv(np.ascontiguousarray(inst["inv"], F).astype(np.float64))
        lo = np.minimum(kids[0]["min"], kids[1]["min"]).astype(np.float64)
        hi = np.maximum(kids[0]["max"], kids[1]["max"]).astype(np.float64)
        _, c32, w32 = table_sphere(lo, hi, fwd)
        cf.append(c32); w.append(w32)
    cf, w = np.array(cf, F), np.array(w, F)
    K = len(w)
    th, tw = H // 8, W // 8                                         # whole tiles; the rest are partial
    partial = ((H + 7) // 8) * ((W + 7) // 8) - th * tw
    lx, ly = morton_xy(np.arange(64))
    d = rays[:th * 8, :tw * 8].reshape(th, 8, tw, 8, 3).transpose(0, 2, 1, 3, 4)[:, :, ly, lx, :].reshape(th * tw, 64, 3)
    T = len(d)
    o = np.broadcast_to(np.asarray(pos, F), (T, 3))
    cfT, wT = np.broadcast_to(cf, (T, K, 3)), np.broadcast_to(w, (T, K))
    rej = np.zeros((T, K), bool)
    union = np.zeros((T, K), bool)
    worst, unsound, inmask, guarded = np.inf, 0, 0, 0
    for t0 in range(0, T, 2048):
        sl = slice(t0, t0 + 2048)
        r = ref.wave_rejects(o[sl], d[sl], cfT[sl], wT[sl])
        lane = ~ref.lane_culls(o[sl], d[sl], cfT[sl], wT[sl])       # (t, L, K): let through
        margin = ref.lemma_margin64(o[sl], d[sl], cfT[sl], wT[sl])
        rej[sl], union[sl] = r, lane.any(1)
        hit = np.broadcast_to(r[:, None, :], margin.shape)
        if hit.any():
            worst = min(worst, float(margin[hit].min()))
        unsound += int((hit & ~(margin > 0)).sum())
        inmask += int((hit & lane).sum())
        guarded += int((~ref.wave_cone(d[sl])["ok"]).sum())
    surv = K - rej.sum(1)
    un = union.sum(1)
    print(f"# python tools/count_wave_cull.py   (CPU only; float32 numpy restatement tests/wave_cull_ref.py, lemma in float64)")
    print(f"{args.scene} {W}x{H}, camera {tuple(float(v) for v in pos)}, {K} instances, {T} whole tiles, {partial} partial (no wave test: all survive)")
    print(f"waves whose guard turned the test off            {guarded}")
    print("instances  tiles(survivors)  tiles(union of lane masks)")
    for n in range(K + 1):
        print(f"{n:9d}  {int((surv == n).sum()):16d}  {int((un == n).sum()):26d}")
    tot_s, tot_u = int(surv.sum()) + partial * K, int(un.sum())
    print(f"(tile, instance) pairs the wave test leaves      {tot_s}   mean {tot_s / (T + partial):.3f} of {K} per tile")
    print(f"(tile, instance) pairs in the union of the masks {tot_u}   mean {tot_u / max(T, 1):.3f} of {K} per tile (whole tiles)")
    print(f"rejected pairs                                   {int(rej.sum())}")
    print(f"rejected pairs inside some lane's own mask       {inmask}  (must be 0)")
    print(f"rejected (pair, lane) that miss the lemma's bound {unsound}  (must be 0)")
    print(f"smallest (dist^2 - bound) / bound over rejected  {worst:.3e}")
    mean = tot_s / (T + partial)
    print(f"gate: mean survivors per tile <= 6               {'met' if mean <= 6 else 'MISSED'} ({mean:.3f})")
    # per tile: the sets themselves, one line per tile row (top to bottom), one hexadecimal mask per tile (bit k = instance k)
    digits = (K + 3) // 4
    weights = 1 << np.arange(K, dtype=object)
    for title, keep in (("instances the wave test leaves", ~rej), ("union of the per-lane masks", union)):
        print(f"per tile, {title}: {th} rows of {tw} masks")
        masks = (keep.astype(object) * weights).sum(1).reshape(th, tw)
        for row in masks:
            print(" ".join(f"{int(m):0{digits}x}" for m in row))
    return 0 if (unsound == 0 and inmask == 0 and mean <= 6) else 1


if __name__ == "__main__":
    sys.exit(main())
