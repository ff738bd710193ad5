"""The guarded float skybox index (clraytracer_amd/csrc/crt_device.h: sky_index_float) restated in numpy float32, one IEEE operation per
statement as the header writes it, with the constants READ FROM THE HEADER. No tests in here: tests/test_sky_index_cpu.py and
tests/test_gpu_sky_index.py use it.

    constants()                 the header's CRT_SKY_* values
    poly_atan / fast_acos       p ~ atan(q) / pi on [0, 1] and ac~ ~ acos(y) / pi
    decide(d, tw, th)           (decided, theta, phi, index): the lane's float decision; theta, phi and index only mean something where decided
    recorded()                  the figures of profiles/sky_index_bounds.txt (tools/sky_index_bounds.c)
    edge_aimed_columns / rows   directions aimed at texel edges, stepped through the neighbouring floats
"""
import os
import re

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "clraytracer_amd", "csrc", "crt_device.h")).read()
BOUNDS = os.path.join(ROOT, "profiles", "sky_index_bounds.txt")


def constants():
    found = dict(re.findall(r"^#define CRT_SKY_(\w+) (-?[0-9.]+(?:e[-+]?\d+)?)f$", HEADER, re.M))
    assert len(found) == 22, "the constants' text changed: restate it here"
    c = {k: F(v) for k, v in found.items()}
    c["A"] = [c["A%d" % k] for k in range(9)]
    c["C"] = [c["C%d" % k] for k in range(8)]
    return c


K = constants()


def poly_atan(q):
    q = np.asarray(q, F)
    u = q * q
    p = np.full_like(q, K["A"][8])
    for k in range(7, -1, -1):
        p = p * u
        p = p + K["A"][k]
    return p * q


def fast_acos(y):
    y = np.asarray(y, F)
    ay = np.abs(y)
    r = np.sqrt(F(1.0) - ay)
    c = np.full_like(y, K["C"][7])
    for k in range(6, -1, -1):
        c = c * ay
        c = c + K["C"][k]
    c = c * r
    return np.where(y < 0, F(1.0) - c, c)


def decide(d, tw, th):
    d = np.asarray(d, F).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    fw, fh = F(tw), F(th)
    with np.errstate(all="ignore"):
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        steep = ax > az
        mn, mx = np.where(steep, az, ax), np.where(steep, ax, az)
        p = poly_atan(mn / mx)
        a = np.where(steep, F(0.5) - p, p)
        a = np.where(z > 0, F(1.0) - a, a)
        a = np.where(x < 0, -a, a)
        c = fast_acos(y)
        s = (a * F(0.5)) * fw
        sv = c * fh
        es, ev = np.abs(s - np.rint(s)), np.abs(sv - np.rint(sv))
        mw, mh = K["KA"] * np.abs(F(0.5) * fw), K["KC"] * np.abs(fh)
        decided = ((es > mw) & (ev > mh) & (np.abs(s) < K["MAX_SCALED"]) & (sv < K["MAX_SCALED"]) & (mn >= K["MIN_COMPONENT"]) & (mx <= K["MAX_COMPONENT"])
                   & (ay >= K["MIN_COMPONENT"]) & (ay < F(1.0)))
        assert s.dtype == F and sv.dtype == F and es.dtype == F and mw.dtype == F
        theta = np.where(decided, s, F(0)).astype(np.int64)
        phi = np.where(decided, sv, F(0)).astype(np.int64)
    return decided, theta, phi, phi * tw + (theta + 2)


def recorded():
    """{'E_p', 'E_c', 'K_a', 'K_c'} floats and {('y' | 'q' | 'q0', tw, th): decided} of profiles/sky_index_bounds.txt"""
    text = open(BOUNDS).read()
    vals = {k: float(v) for k, v in re.findall(r"^recorded (E_p|E_c|K_a|K_c) (\S+)$", text, re.M)}
    assert len(vals) == 4, "profiles/sky_index_bounds.txt changed its form"
    sweeps = {(k, int(w), int(h)): int(n) for k, w, h, n in re.findall(r"^sweep (\w+)\s.* sky (\d+)x(\d+): decided (\d+)", text, re.M)}
    fixed = re.search(r"\(d\.x, d\.z\) = \((\S+), (\S+)\)", text), re.search(r"d = \(q, (\S+), -1\)", text)
    vals["sweep_xz"] = (F(fixed[0].group(1)), F(fixed[0].group(2)))
    vals["sweep_y"] = F(fixed[1].group(1))
    return vals, sweeps


def _stepped(v, steps=8):
    """(len(v) * (2 steps + 1),) float32: every value and its `steps` neighbouring floats on either side (17 floats for steps = 8)"""
    v = np.asarray(v, F)
    out = [v]
    lo = hi = v
    for _ in range(steps):
        lo = np.nextafter(lo, F(-np.inf))
        hi = np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return np.stack(out, 1).reshape(-1)


def edge_aimed_columns(tw, elevation=0.3):
    """Directions whose azimuth is pi 2k / tw for every column edge k = -tw/2 .. tw/2 (s = k), d.x stepped through its 17 neighbouring floats"""
    k = np.arange(-(tw // 2), tw // 2 + 1)
    az = np.pi * 2.0 * k / tw
    ce = np.sqrt(1.0 - elevation * elevation)
    x, nz = (np.sin(az) * ce).astype(F), (np.cos(az) * ce).astype(F)
    xs = _stepped(x)
    n = len(xs) // len(x)
    return np.stack([xs, np.full(len(xs), elevation, F), np.repeat(-nz, n)], 1).astype(F)


def edge_aimed_rows(th, azimuth=0.7):
    """Directions with d.y = cos(pi k / th) for every row edge k = 0 .. th, d.y stepped through its 17 neighbouring floats"""
    k = np.arange(0, th + 1)
    y = np.cos(np.pi * k / th)
    ys = _stepped(y.astype(F))
    n = len(ys) // len(y)
    ce = np.repeat(np.sqrt(np.maximum(0.0, 1.0 - y * y)), n)
    return np.stack([(np.sin(azimuth) * ce).astype(F), ys, (-np.cos(azimuth) * ce).astype(F)], 1).astype(F)
