#!/usr/bin/env python3
"""What the committing form of the camera bounce's root pre-test (crt_device.h: root_pretest_enters) commits, counted on the CPU: a host-only session
for the scene's arenas and camera, the oracle's RayGen for the rays, and the float32 restatements of tests/root_pretest_ref.py,
tests/wave_cull_ref.py and tests/pretest_entry_ref.py (the sphere cull, the root step at the bound 99999, the commit and its order condition).

    python tools/count_pretest_entry.py [--scene multi-1M] [--width 1920 --height 1080]

Per full 8 x 8 tile (the waves that take the wave test and the pre-test): the lanes that commit; the distinct first instances among them -- one:
the trip loop's first enter block was wave-uniform (scalar loads of the instance record and the root pair), more: it was divergent (four vector
loads each); the share of tiles with any committing lane; the executed pre-tests per wave (instances some lane of the tile still holds after the
per-lane sphere cull). An instance the wave test rejects is one the pre-test would clear: the commits do not depend on it."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pretest_entry_ref as entry      # noqa: E402

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
    W, H = args.width, args.height
    with driver.Session(W, H, host_only=True) as s:
        s.load_scene(scenes.get(args.scene))
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in s.arenas().items()}
        iv, ip, pos = s.camera()
        d = np.ascontiguousarray(oracle_lib.Oracle(a, nthreads=args.threads).raygen(W, H, iv, ip), F).reshape(-1, 3)
    o = np.asarray(pos, F)
    n = len(a["instances"])
    terms = [entry.instance_terms(a, k) for k in range(n)]
    masks = entry.lane_masks(a, o, d)
    after, inside, pushed, _ = entry.wave_commits(masks, terms, o, d)
    th, tw = H // 8, W // 8

    def tiles(x):                                      # the full tiles, 64 lanes each
        return x.reshape(H, W)[:th * 8, :tw * 8].reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(th * tw, 64)

    ins, psh, msk, aft = tiles(inside), tiles(pushed), tiles(masks), tiles(after)
    lanes = (ins >= 0).sum(1)
    distinct = np.array([len(set(r[r >= 0])) for r in ins])
    executed = np.array([bin(int(np.bitwise_or.reduce(r))).count("1") for r in msk])
    have = np.array([(r != 0).sum() for r in msk])                  # lanes with any instance after the sphere cull
    left = np.array([((x != 0) | (y >= 0)).sum() for x, y in zip(aft, ins)])      # ... after the pre-test (inside one, or a bit left)
    T = th * tw
    print(f"{args.scene} {W}x{H}, {len(d)} primary rays, {n} instances, {T} full tiles of {((H + 7) // 8) * ((W + 7) // 8)}")
    print(f"lanes with an instance after the sphere cull      {int(have.sum()):9d}   {have.sum() / T:6.2f} per tile")
    print(f"lanes with an instance after the pre-test         {int(left.sum()):9d}   {left.sum() / T:6.2f} per tile   ({100.0 * left.sum() / (64 * T):.1f} % of lanes)")
    print(f"lanes that commit                                 {int(lanes.sum()):9d}   {lanes.sum() / T:6.2f} per tile   ({100.0 * lanes.sum() / max(left.sum(), 1):.1f} % of the lanes with an instance)")
    print(f"  of them with the far child pushed               {int(psh.sum()):9d}   ({100.0 * psh.sum() / max(lanes.sum(), 1):.1f} %)")
    print(f"tiles with a committing lane                      {int((lanes > 0).sum()):9d}   ({100.0 * (lanes > 0).mean():.1f} % of tiles)")
    print(f"  one first instance (the first enter was uniform)  {int((distinct == 1).sum()):7d}   ({100.0 * (distinct == 1).sum() / max((lanes > 0).sum(), 1):.1f} % of those)")
    print(f"  two or more (the first enter was divergent)       {int((distinct >= 2).sum()):7d}   ({100.0 * (distinct >= 2).sum() / max((lanes > 0).sum(), 1):.1f} %)")
    print(f"distinct first instances per tile                 {distinct.sum() / T:6.3f}   ({distinct.sum() / max((lanes > 0).sum(), 1):.3f} per tile with a committing lane)")
    print(f"executed pre-tests per wave                       {executed.sum() / T:6.3f}")
    print(f"lanes left to enter through the trip loop first   {int((left - lanes).sum()):9d}   {(left - lanes).sum() / T:6.2f} per tile (a lower single-leaf bit, or n1 == 1e30)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
