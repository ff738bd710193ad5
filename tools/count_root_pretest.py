#!/usr/bin/env python3
"""What the exact root pre-test of the camera bounce (crt_device.h: root_pretest_misses) removes, counted on the CPU: a host-only session for the
scene's arenas and camera, the oracle's RayGen for the rays, and the float32 restatements of tools/count_box_pretest.py (the sphere cull, the
traversal's root step at the bound 99999).

    python tools/count_root_pretest.py [--scene multi-1M] [--width 1920 --height 1080]

Prints, per instance and in total, the primary-ray entries the sphere cull lets through and the ones the pre-test removes; the wave-level
(tile, instance) pairs before and after (a pair stays while any lane of the 8 x 8 tile keeps the instance); and how many instances a lane is left
with. An instance whose root is a leaf has no box to test and keeps all its entries."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from count_box_pretest import F, dot3, root_step_passes, sphere_lets_through, table_sphere      # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="multi-1M")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    from clraytracer_amd import driver, scenes
    import oracle_lib
    W, H = args.width, args.height
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(scenes.get(args.scene))
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        iv, ip, pos = s.camera()
        d = np.ascontiguousarray(oracle_lib.Oracle(a, nthreads=args.threads).raygen(W, H, iv, ip), F).reshape(-1, 3)
    o = np.asarray(pos, F)
    dd = dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
    th, tw = (H + 7) // 8, (W + 7) // 8

    def tiles(mask):                                   # any pixel of the 8 x 8 tile
        m = np.zeros((th * 8, tw * 8), bool)
        m[:H, :W] = mask.reshape(H, W)
        return m.reshape(th, 8, tw, 8).any((1, 3))

    n = len(a["instances"])
    entries = removed = pairs_before = pairs_after = 0
    left = np.zeros(len(d), np.int32)                  # instances a lane still enters
    before = np.zeros(len(d), np.int32)
    print(f"{args.scene} {W}x{H}, {len(d)} primary rays, {n} instances, {th * tw} tiles")
    print("instance  sphere-entries   removed  removed/entries  tile pairs before -> after")
    with np.errstate(all="ignore"):
        for i, inst in enumerate(a["instances"]):
            node = a["nodes"][int(a["roots"][inst["meshIndex"]])]
            if node["triCount"] != 0:
                keep = np.ones(len(d), bool)           # never culled, never cleared
                left += 1; before += 1
                entries += len(d); pairs_before += th * tw; pairs_after += th * tw
                print(f"{i:8d}  {len(d):14d}  {0:8d}  (the root is a leaf: no box to test)")
                continue
            kids = a["nodes"][int(node["leftFirst"]):int(node["leftFirst"]) + 2]
            m = np.ascontiguousarray(inst["inv"], F)
            fwd = np.linalg.inv(m.astype(np.float64))
            lo = np.minimum(kids[0]["min"], kids[1]["min"]).astype(np.float64)
            hi = np.maximum(kids[0]["max"], kids[1]["max"]).astype(np.float64)
            _, cf, w = table_sphere(lo, hi, fwd)
            sph = sphere_lets_through(cf, w, o, d, dd)
            keep = sph & root_step_passes(m, o, d, kids)
            n_s, n_k = int(sph.sum()), int(keep.sum())
            pb, pa = int(tiles(sph).sum()), int(tiles(keep).sum())
            entries += n_s; removed += n_s - n_k; pairs_before += pb; pairs_after += pa
            before += sph; left += keep
            print(f"{i:8d}  {n_s:14d}  {n_s - n_k:8d}  {100.0 * (n_s - n_k) / max(n_s, 1):6.1f} %          {pb:8d} -> {pa:8d}")
    print(f"entries let through by the sphere cull      {entries}   ({entries / len(d):.2f} per lane)")
    print(f"entries the root pre-test removes           {removed}   ({100.0 * removed / max(entries, 1):.1f} %)")
    print(f"entries left                                {entries - removed}   ({(entries - removed) / len(d):.2f} per lane)")
    print(f"wave-level (tile, instance) pairs           {pairs_before} -> {pairs_after}   ({pairs_before / (th * tw):.2f} -> {pairs_after / (th * tw):.2f} per tile)")
    print("instances per lane                 before the pre-test         after")
    for k in range(int(before.max()) + 1):
        print(f"  {k:3d}                              {100.0 * (before == k).mean():6.2f} %               {100.0 * (left == k).mean():6.2f} %")
    return 0


if __name__ == "__main__":
    sys.exit(main())
