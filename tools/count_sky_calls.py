#!/usr/bin/env python3
"""How often a frame calls the skybox index (crt_device.h: sample_skybox / sample_skybox_guarded), per wave, and how much of that the guarded
float decision leaves to the double form. Needs no GPU: a host-only session for the scene's arenas and camera, the oracle's RayGen and closest
hits, the numpy restatement of the bounce set-up (tests/test_shading_independent.py) and of the float decision (tests/sky_fast_ref.py).

    python tools/count_sky_calls.py [--scene multi-1M] [--width 1920 --height 1080] > profiles/sky_index_calls.txt

A wave is an 8 x 8 pixel tile (Morton order inside: which lanes share a wave does not depend on the order). A wave calls the lookup at
bounce 0 if any of its pixels' primary rays misses, and again at bounce 1 if any of its bounce rays misses; a call runs the double form
if any lane taking part in it is undecided."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", default="multi-1M")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    from clraytracer_amd import driver, scenes
    import oracle_lib
    import sky_fast_ref
    from test_shading_independent import half, mat3_mul, normalize, reflect
    W, H = args.width, args.height
    sc = scenes.get(args.scene)
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(sc)
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        iv, ip, pos = s.camera()
    orc = oracle_lib.Oracle(a, nthreads=args.threads)
    d0 = np.ascontiguousarray(orc.raygen(W, H, iv, ip), F).reshape(-1, 3)
    n = len(d0)
    o0 = np.tile(np.asarray(pos, F), (n, 1))
    tw, th = int(a["textures"][2]["width"]), int(a["textures"][2]["height"])

    rec, _ = orc.closest_hits(o0, d0)
    miss0 = rec["t"] > F(99998.0)
    hit = np.flatnonzero(~miss0)
    hr = rec[hit]
    inst = a["instances"][hr["instance"]]
    m = np.ascontiguousarray(inst["inv"], F)
    tri = a["tris"][hr["tri"]]
    uu, vv = hr["u"].astype(F), hr["v"].astype(F)
    bx, by, bz = (F(1.0) - uu) - vv, uu, vv
    nh = half(tri["n"])
    with np.errstate(all="ignore"):
        normal = normalize((mat3_mul(m, nh[:, 0:3]) * bx[:, None] + mat3_mul(m, nh[:, 3:6]) * by[:, None]) + mat3_mul(m, nh[:, 6:9]) * bz[:, None])
        mo = ((m[:, 0, :3] * o0[hit, 0:1] + m[:, 1, :3] * o0[hit, 1:2]) + m[:, 2, :3] * o0[hit, 2:3]) + m[:, 3, :3] * F(1.0)
        md = ((m[:, 0, :3] * d0[hit, 0:1] + m[:, 1, :3] * d0[hit, 1:2]) + m[:, 2, :3] * d0[hit, 2:3]) + m[:, 3, :3] * F(0.0)
        o1 = (mo + hr["t"].astype(F)[:, None] * md) + normal * F(0.01)
        d1 = reflect(d0[hit], normal)
    rec1, _ = orc.closest_hits(o1, d1)
    miss1 = np.zeros(n, bool)
    miss1[hit] = rec1["t"] > F(99998.0)
    dirs1 = np.zeros((n, 3), F)
    dirs1[hit] = d1

    dec0 = sky_fast_ref.decide(d0, tw, th)[0]
    dec1 = sky_fast_ref.decide(dirs1, tw, th)[0]
    und0, und1 = miss0 & ~dec0, miss1 & ~dec1
    tH, tW = (H + 7) // 8, (W + 7) // 8

    def tiles(mask):
        t = np.zeros((tH * 8, tW * 8), bool)
        t[:H, :W] = mask.reshape(H, W)
        return t.reshape(tH, 8, tW, 8).any((1, 3))

    waves = tH * tW
    c0, c1, f0, f1 = int(tiles(miss0).sum()), int(tiles(miss1).sum()), int(tiles(und0).sum()), int(tiles(und1).sum())
    l0, l1 = int(miss0.sum()), int(miss1.sum())
    print(f"{args.scene} {W}x{H}: {n} primary rays, {waves} waves (8x8 tiles), sky {tw}x{th} texels")
    print(f"primary rays that miss                          {l0}  ({100.0 * l0 / n:.1f} % of the pixels)")
    print(f"bounce rays                                     {len(hit)}, of which miss {l1}  ({100.0 * l1 / max(len(hit), 1):.1f} %)")
    print(f"waves that call the sky lookup at bounce 0      {c0}  ({100.0 * c0 / waves:.1f} % of the waves), {l0 / max(c0, 1):.1f} lanes per call")
    print(f"waves that call the sky lookup at bounce 1      {c1}  ({100.0 * c1 / waves:.1f} % of the waves), {l1 / max(c1, 1):.1f} lanes per call")
    print(f"calls per frame                                 {c0 + c1}  ({(c0 + c1) / waves:.2f} per wave), lanes taking part {l0 + l1}")
    print(f"guard (CRT_SKY_KA {float(sky_fast_ref.K['KA']):.3g}, CRT_SKY_KC {float(sky_fast_ref.K['KC']):.3g}):")
    print(f"  lanes undecided at bounce 0                   {int(und0.sum())}  ({100.0 * und0.sum() / max(l0, 1):.3f} % of its lanes)")
    print(f"  lanes undecided at bounce 1                   {int(und1.sum())}  ({100.0 * und1.sum() / max(l1, 1):.3f} % of its lanes)")
    print(f"  calls that fall back to double at bounce 0    {f0}  ({100.0 * f0 / max(c0, 1):.1f} % of its calls)")
    print(f"  calls that fall back to double at bounce 1    {f1}  ({100.0 * f1 / max(c1, 1):.1f} % of its calls)")
    print(f"  lanes undecided, all                          {int(und0.sum() + und1.sum())}  ({100.0 * (und0.sum() + und1.sum()) / max(l0 + l1, 1):.3f} %)")
    print(f"  calls that fall back, all                     {f0 + f1}  ({100.0 * (f0 + f1) / max(c0 + c1, 1):.1f} %)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
