#!/usr/bin/env python3
"""How many instance entries of the PRIMARY rays a world-space box pre-test would remove (the lead left open beside the
staged sphere cull). Needs no GPU: a host-only session for the scene's arenas and camera, the oracle's RayGen for the rays, and numpy.

    python tools/count_box_pretest.py [--scene multi-1M] [--width 1920 --height 1080] [--frame-entries 5580000]

Per instance with an inner root (a root that is a leaf is entered without a box test and is left out):
  sphere   the cull of candidate_mask (crt_device.h) in float32, operation by operation, on the table entry (fl(c), w) restated from
           crt_instances.h (image_sphere, fp32_sphere; every instance is taken as cullable, which holds for the stock scenes' cameras)
  useful   the exact float32 root step of the traversal: xform_xyz, 1.0f / md, intersect_aabb on both children with the 99999 the first
           instance starts with as "closest so far" (an upper bound of the entries that pass: a closer hit only turns passes into misses)
  box      a float64 slab test of the world ray against the world AABB of the two child boxes' images, grown by
           sqrt(1.02 w^2 + 2.8e-6 x^2) - w (the sphere cull's own slack at distance x = |c - o|, which covers the fp32 error of the
           traversal's test over the admitted range) and by a relative 1e-5; entered when tnear <= tfar and tfar >= 0, any NaN: entered
A (tile, instance) pair is a wave-level entry when any pixel of the 8 x 8 tile is let through. `--frame-entries`: the entries of the whole
frame, secondary rays included (5.58 M on multi-1M), for the share the bar is set against (a tenth of all entries)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def table_sphere(lo, hi, fwd):
    """(fl(c), w) of crt_instances.h: the sphere around the image of the box [lo, hi] under fwd (4 x 4, row vectors), as the kernel reads it"""
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    c = mid @ fwd[:3, :3] + fwd[3, :3]
    r2 = 0.0
    for sy in (1.0, -1.0):
        for sz in (1.0, -1.0):
            v = half[0] * fwd[0, :3] + sy * half[1] * fwd[1, :3] + sz * half[2] * fwd[2, :3]
            r2 = max(r2, float(v @ v))
    cf = c.astype(F)
    w = F((np.sqrt(r2) * (1.0 + 1e-4) + np.linalg.norm(c - cf.astype(np.float64))) * (1.0 + 1e-6))
    return c, cf, w


def sphere_lets_through(cf, w, o, d, dd):
    ocx, ocy, ocz = F(cf[0] - o[0]), F(cf[1] - o[1]), F(cf[2] - o[2])
    oc2 = dot3(ocx, ocy, ocz, ocx, ocy, ocz)
    b = dot3(ocx, ocy, ocz, d[:, 0], d[:, 1], d[:, 2])
    r2 = w * w * F(1.0201) + F(4e-6) * oc2
    cull = (w >= 0) & ((oc2 * dd - b * b > r2 * dd) | ((b < 0) & (oc2 > r2)))
    return ~cull


def slab_f32(mo, inv, bmin, bmax, best):
    """intersect_aabb of crt_device.h (upstream's rule)"""
    tmin = [(F(bmin[k]) - mo[k]) * inv[k] for k in range(3)]
    tmax = [(F(bmax[k]) - mo[k]) * inv[k] for k in range(3)]
    tnear = np.fmax(np.fmax(np.fmin(tmin[0], tmax[0]), np.fmin(tmin[1], tmax[1])), np.fmin(tmin[2], tmax[2]))
    tfar = np.fmin(np.fmin(np.fmax(tmin[0], tmax[0]), np.fmax(tmin[1], tmax[1])), np.fmax(tmin[2], tmax[2]))
    return (tnear < tfar) & (tnear > 0) & (tnear < best)


def root_step_passes(m, o, d, kids):
    """does the ray pass a child box of the root as the traversal computes it: Traversal::enter + the first inner step"""
    mo = [F(((m[0, j] * o[0] + m[1, j] * o[1]) + m[2, j] * o[2]) + m[3, j] * F(1.0)) for j in range(3)]
    md = [((m[0, j] * d[:, 0] + m[1, j] * d[:, 1]) + m[2, j] * d[:, 2]) + m[3, j] * F(0.0) for j in range(3)]
    inv = [F(1.0) / md[j] for j in range(3)]
    return slab_f32(mo, inv, kids[0]["min"], kids[0]["max"], F(99999.0)) | slab_f32(mo, inv, kids[1]["min"], kids[1]["max"], F(99999.0))


def world_box_lets_through(kids, fwd, c, w, o, d):
    corners = []
    for kid in kids:
        lo, hi = kid["min"].astype(np.float64), kid["max"].astype(np.float64)
        for k in range(8):
            p = np.array([hi[0] if k & 1 else lo[0], hi[1] if k & 2 else lo[1], hi[2] if k & 4 else lo[2]])
            corners.append(p @ fwd[:3, :3] + fwd[3, :3])
    corners = np.array(corners)
    wlo, whi = corners.min(0), corners.max(0)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    x = np.linalg.norm(c - o64)
    grow = np.sqrt(1.02 * float(w) ** 2 + 2.8e-6 * x * x) - float(w)
    rel = 1e-5 * np.maximum(np.abs(wlo), np.abs(whi))
    wlo, whi = wlo - grow - rel, whi + grow + rel
    t1, t2 = (wlo[None] - o64[None]) / d64, (whi[None] - o64[None]) / d64
    tnear, tfar = np.fmin(t1, t2).max(1), np.fmax(t1, t2).min(1)
    return ~(tnear > tfar) & ~(tfar < 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="multi-1M")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frame-entries", type=float, default=5.58e6, help="instance entries of the whole frame, all bounces (DESIGN.md 9)")
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    from clraytracer_amd import driver, scenes
    import oracle_lib
    W, H = args.width, args.height
    sc = scenes.get(args.scene)
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        iv, ip, pos = s.camera()
        rays = np.ascontiguousarray(oracle_lib.Oracle(a, nthreads=args.threads).raygen(W, H, iv, ip), F).reshape(H, W, 3)
    o = np.asarray(pos, F)
    d = rays.reshape(-1, 3)
    dd = dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
    th, tw = (H + 7) // 8, (W + 7) // 8

    def tiles(mask):                                   # any pixel of the 8 x 8 tile
        m = np.zeros((th * 8, tw * 8), bool)
        m[:H, :W] = mask.reshape(H, W)
        return m.reshape(th, 8, tw, 8).any((1, 3))

    tot = dict(sphere=0, useful=0, both=0, unsound=0, w_sphere=0, w_both=0, w_useful=0)
    print(f"{args.scene} {W}x{H}, {len(d)} primary rays from {tuple(float(v) for v in o)}, {len(a['instances'])} instances")
    print("instance  sphere-entries    useful  sphere&box   removed  removed/entries")
    with np.errstate(all="ignore"):
        for i, inst in enumerate(a["instances"]):
            node = a["nodes"][int(a["roots"][inst["meshIndex"]])]
            if node["triCount"] != 0:
                print(f"{i:8d}  (the root is a leaf: entered without a box test, left out)")
                continue
            kids = a["nodes"][int(node["leftFirst"]):int(node["leftFirst"]) + 2]
            m = np.ascontiguousarray(inst["inv"], F)
            fwd = np.linalg.inv(m.astype(np.float64))
            lo = np.minimum(kids[0]["min"], kids[1]["min"]).astype(np.float64)
            hi = np.maximum(kids[0]["max"], kids[1]["max"]).astype(np.float64)
            c, cf, w = table_sphere(lo, hi, fwd)
            sph = sphere_lets_through(cf, w, o, d, dd)
            use = root_step_passes(m, o, d, kids)
            box = world_box_lets_through(kids, fwd, c, w, o, d)
            both = sph & box
            n_s, n_u, n_b = int(sph.sum()), int((use & sph).sum()), int(both.sum())
            tot["sphere"] += n_s; tot["useful"] += n_u; tot["both"] += n_b
            tot["unsound"] += int((use & ~both).sum())
            tot["w_sphere"] += int(tiles(sph).sum()); tot["w_both"] += int(tiles(both).sum()); tot["w_useful"] += int(tiles(use & sph).sum())
            print(f"{i:8d}  {n_s:14d}  {n_u:8d}  {n_b:10d}  {n_s - n_b:8d}  {100.0 * (n_s - n_b) / max(n_s, 1):6.1f} %")
    removed, wasted = tot["sphere"] - tot["both"], tot["sphere"] - tot["useful"]
    print(f"entries let through by the sphere cull          {tot['sphere']}")
    print(f"entries that pass a root child box              {tot['useful']}  ({100.0 * wasted / max(tot['sphere'], 1):.1f} % are wasted)")
    print(f"entries left after sphere and box               {tot['both']}")
    print(f"removed by the box pre-test                     {removed}")
    print(f"removed, share of primary entries               {100.0 * removed / max(tot['sphere'], 1):.1f} %")
    print(f"removed, share of wasted primary entries        {100.0 * removed / max(wasted, 1):.1f} %")
    print(f"removed, share of the frame's {args.frame_entries / 1e6:.2f} M entries      {100.0 * removed / args.frame_entries:.1f} %  (the bar: 10 %)")
    print(f"wave-level (tile, instance) entries, sphere only {tot['w_sphere']}")
    print(f"wave-level entries, sphere and box               {tot['w_both']}")
    print(f"wave-level entries that are useful               {tot['w_useful']}")
    print(f"useful entries the pre-test would have removed   {tot['unsound']}  (must be 0: the pre-test is conservative)")
    return 0 if tot["unsound"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
