#!/usr/bin/env python3
"""How many instance entries of the REFLECTION bounce's rays the exact root step per wave would remove (the camera bounce's
pre-test, root_pretest_misses, asked of bounce 1, where every lane has its own origin). Needs no GPU: a host-only session for the scene's
arenas and camera, the oracle's RayGen and closest_hits for the primary hits, and numpy.

    python tools/count_bounce_pretest.py [--scene multi-1M] [--width 1920 --height 1080] > profiles/bounce_pretest_counts.txt

bounce_rays() restates shade_bounce's continuing ray (crt_device.h) in float32, one IEEE operation per numpy operation in the kernel's order:
the half-float vertex normals through mat3mul, their barycentric sum through normalize3, point = mo + md t, o' = point + 0.01 n,
d' = reflect3(d, n). The cull (candidate_mask) and the root step (Traversal::enter + the root's inner step at the bound 99999) are
tools/count_box_pretest.py's restatements, given one origin per ray. A wave is an 8 x 8 tile of the frame; its live lanes at bounce 1 are the
pixels whose path continued. An instance whose root is a leaf is entered without a box test: its entries count as passing.

Exit status 1 when the gate of the kernel work fails: fewer than half of the bounce's entries removed, or a mean union per tile above 4."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from count_box_pretest import dot3, root_step_passes, sphere_lets_through, table_sphere  # noqa: E402

F = np.float32
SKY = F(99998.0)             # shade_bounce: a hit beyond it is shaded as sky and the path ends


def mat3mul(m, vx, vy, vz):
    """mat3mul(CrtDevInstance, v): (m0 vx + m1 vy) + m2 vz per column of the inverse transform (row vectors)"""
    return [(m[:, 0, j] * vx + m[:, 1, j] * vy) + m[:, 2, j] * vz for j in range(3)]


def xform(m, vx, vy, vz, vw):
    """xform_xyz: ((m0 vx + m1 vy) + m2 vz) + m3 vw per column"""
    return [((m[:, 0, j] * vx + m[:, 1, j] * vy) + m[:, 2, j] * vz) + m[:, 3, j] * vw for j in range(3)]


def bounce_rays(arenas, o, d, hits):
    """(alive, o', d'): which rays continue after the first hit, and shade_bounce's reflected ray for those (float32, (n, 3) each).
    o: (3,) or (n, 3) origins, d: (n, 3) directions, hits: the oracle's closest_hits records of those rays."""
    d = np.asarray(d, F).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(o, F), d.shape)
    alive = (hits["instance"] >= 0) & ~(hits["t"] > SKY)
    h, o, d = hits[alive], o[alive], d[alive]
    m = np.ascontiguousarray(arenas["instances"]["inv"], F)[h["instance"]]
    n16 = np.ascontiguousarray(arenas["tris"]["n"][h["tri"]]).view(np.float16).astype(F).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        mo = xform(m, o[:, 0], o[:, 1], o[:, 2], F(1.0))
        md = xform(m, d[:, 0], d[:, 1], d[:, 2], F(0.0))
        u, v, t = h["u"].astype(F), h["v"].astype(F), h["t"].astype(F)
        b = [(F(1.0) - u) - v, u, v]
        nv = [mat3mul(m, n16[:, k, 0], n16[:, k, 1], n16[:, k, 2]) for k in range(3)]
        s = [(nv[0][j] * b[0] + nv[1][j] * b[1]) + nv[2][j] * b[2] for j in range(3)]
        inv = F(1.0) / np.sqrt(dot3(s[0], s[1], s[2], s[0], s[1], s[2]))
        n = [s[j] * inv for j in range(3)]
        point = [mo[j] + md[j] * t for j in range(3)]
        o1 = [point[j] + n[j] * F(0.01) for j in range(3)]
        nd = dot3(n[0], n[1], n[2], d[:, 0], d[:, 1], d[:, 2])
        d1 = [d[:, j] - (n[j] * nd) * F(2.0) for j in range(3)]
    return alive, np.stack(o1, 1).astype(F), np.stack(d1, 1).astype(F)


def instance_masks(arenas, o, d):
    """(sphere, useful): (n rays, n instances) bool each -- the entries candidate_mask lets through, and those of them that pass a root child box
    at the bound 99999 (an instance whose root is a leaf: all of them)"""
    a = arenas
    ot = np.ascontiguousarray(o.T)                     # (3, n): o[k] is the k-th component of every ray's origin
    dd = dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
    sph, use = [], []
    with np.errstate(all="ignore"):
        for inst in a["instances"]:
            node = a["nodes"][int(a["roots"][inst["meshIndex"]])]
            m = np.ascontiguousarray(inst["inv"], F)
            fwd = np.linalg.inv(m.astype(np.float64))
            if node["triCount"] != 0:
                lo, hi, kids = node["min"].astype(np.float64), node["max"].astype(np.float64), None
            else:
                kids = a["nodes"][int(node["leftFirst"]):int(node["leftFirst"]) + 2]
                lo = np.minimum(kids[0]["min"], kids[1]["min"]).astype(np.float64)
                hi = np.maximum(kids[0]["max"], kids[1]["max"]).astype(np.float64)
            _, cf, w = table_sphere(lo, hi, fwd)
            s = sphere_lets_through(cf, w, ot, d, dd)
            sph.append(s)
            use.append(s if kids is None else s & root_step_passes(m, ot, d, kids))
    return np.stack(sph, 1), np.stack(use, 1)


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
    sc = scenes.get(args.scene)
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        iv, ip, pos = s.camera()
        orc = oracle_lib.Oracle(a, nthreads=args.threads)
        rays = np.ascontiguousarray(orc.raygen(W, H, iv, ip), F).reshape(-1, 3)
        cam = np.asarray(pos, F)
        hits, _ = orc.closest_hits(np.broadcast_to(cam, rays.shape), rays)
    alive, o, d = bounce_rays(a, cam, rays, hits)
    sph, use = instance_masks(a, o, d)
    nI = sph.shape[1]
    th, tw = (H + 7) // 8, (W + 7) // 8

    def per_tile(rows):                                # (rays, nI) of the bounce rays -> (tiles, 64, nI) over the whole frame, dead lanes all false
        full = np.zeros((th * 8, tw * 8, nI), bool)
        frame = np.zeros((H * W, nI), bool)
        frame[alive] = rows
        full[:H, :W] = frame.reshape(H, W, nI)
        return full.reshape(th, 8, tw, 8, nI).transpose(0, 2, 1, 3, 4).reshape(th * tw, 64, nI)

    live = np.zeros((th * 8, tw * 8), bool)
    live[:H, :W] = alive.reshape(H, W)
    live = live.reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(th * tw, 64)
    has = live.any(1)
    tS, tU = per_tile(sph)[has], per_tile(use)[has]
    live = live[has]
    n_rays, n_tiles = int(alive.sum()), int(has.sum())
    print(f"{args.scene} {W}x{H}: {len(rays)} primary rays from {tuple(float(v) for v in cam)}, {nI} instances")
    print("instance  sphere-entries  pass-a-root-box    wasted  wasted/entries  tiles-holding-it  tiles-after")
    for i in range(nI):
        n_s, n_u = int(sph[:, i].sum()), int(use[:, i].sum())
        print(f"{i:8d}  {n_s:14d}  {n_u:15d}  {n_s - n_u:8d}  {100.0 * (n_s - n_u) / max(n_s, 1):12.1f} %  {int(tS[:, :, i].any(1).sum()):16d}  {int(tU[:, :, i].any(1).sum()):11d}")
    entries, useful = int(sph.sum()), int(use.sum())
    wasted = entries - useful
    union, union_after = tS.any(1).sum(1), tU.any(1).sum(1)
    removed_share = wasted / max(entries, 1)
    mean_union = float(union.mean()) if n_tiles else 0.0
    print(f"bounce rays                                           {n_rays}")
    print(f"tiles with bounce rays                                {n_tiles}")
    print(f"live lanes per such wave                              {live.sum() / max(n_tiles, 1):.1f}")
    print(f"instance entries the sphere cull lets through         {entries}  ({entries / max(n_rays, 1):.2f} per ray)")
    print(f"entries that pass a root child box at the bound 99999 {useful}")
    print(f"entries wasted                                        {wasted}  ({100.0 * removed_share:.1f} %)")
    print(f"union of a wave's candidates per tile                 {mean_union:.2f} of {nI}  (largest {int(union.max()) if n_tiles else 0})")
    print(f"  histogram of the union (0 .. {nI})                    {np.bincount(union, minlength=nI + 1).tolist()}")
    print(f"pre-tests executed (sum of the unions)                {int(union.sum())}")
    print(f"entries removed per executed pre-test                 {wasted / max(int(union.sum()), 1):.1f}")
    print(f"union after the exact root step                       {union_after.mean() if n_tiles else 0.0:.2f}")
    print(f"tiles left with no instance at all                    {int((union_after == 0).sum())} of {n_tiles}")
    print(f"lanes left with no instance                           {100.0 * float((use.sum(1) == 0).mean()) if n_rays else 0.0:.1f} %")
    print(f"most candidates held by one lane of a tile, before -> after   {tS.sum(2).max(1).mean() if n_tiles else 0.0:.2f} -> {tU.sum(2).max(1).mean() if n_tiles else 0.0:.2f}")
    ok = removed_share >= 0.5 and mean_union <= 4.0
    print(f"gate (at least half of the entries removed, mean union at most 4): {'met' if ok else 'NOT met'}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
