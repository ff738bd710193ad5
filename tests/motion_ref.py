"""A numpy float32 restatement of the definition in include/crt_motion.h: tests/temporal_ref.py's accumulate with the reprojection taken through
each pixel's instance's motion record, and the motion-vector plane. What crtm_accumulate must give, bit for bit. Everything the two definitions
share (dot3, the cameras, the hand-made inputs) is temporal_ref's. motion() is the independent statement of crtm_motion, in float64."""
import numpy as np

import temporal_ref
from temporal_ref import CLAMP, MATCH_INSTANCE, F, camera_pairs, dot3, guides, luma, noisy_color, pinhole, shifted, surface_records  # noqa: F401

STATIC, MOVING, NEW = 0, 1, 2
MOTION_DTYPE = np.dtype([("kind", "<u4"), ("point", "<f4", 12), ("normal", "<f4", 9)])


def affine(m):
    """a CrtMatrix4 (row-major, row vectors: p_local = p_world * m) as the trace kernel reads it: column 3 is never looked at"""
    m = np.array(m, np.float64).reshape(4, 4)
    m[:, 3] = (0.0, 0.0, 0.0, 1.0)
    return m


def motion(prev_inv, cur_inv):
    """(kind, point (12,), normal (9,)) in float64 from two inverse transforms (prev_inv None: NEW): with T = cur * prev^-1 a point at p now was
    at p * T; point[4k + j] = T[j][k], point[4k + 3] = T[3][k]; normal[3k + j] = (L^-1)[k][j], L the upper-left 3 x 3 of T."""
    eye_p, eye_n = np.eye(3, 4).reshape(-1), np.eye(3).reshape(-1)
    if prev_inv is None:
        return NEW, eye_p, eye_n
    a, b = np.ascontiguousarray(prev_inv, np.float32).reshape(-1), np.ascontiguousarray(cur_inv, np.float32).reshape(-1)
    if np.array_equal(a.view(np.uint32), b.view(np.uint32)):
        return STATIC, eye_p, eye_n
    T = affine(b) @ np.linalg.inv(affine(a))
    return MOVING, np.concatenate([T[:3, :3].T, T[3:4, :3].T], axis=1).reshape(-1), np.linalg.inv(T[:3, :3]).reshape(-1)


def table(entries):
    """a MOTION_DTYPE table from (kind, point, normal) triples, rounded to float32"""
    t = np.zeros(len(entries), MOTION_DTYPE)
    for i, (kind, point, normal) in enumerate(entries):
        t[i] = (kind, np.asarray(point, np.float64).astype(np.float32), np.asarray(normal, np.float64).astype(np.float32))
    return t


def accumulate(color, geometry, instance, cam, prev=None, motions=None, flags=0, alpha=0.2, moments_alpha=0.2, max_history=32.0, depth_tol=0.05,
               normal_cos=0.9, static_normal=False):
    """temporal_ref.accumulate's arguments and `motions`, a MOTION_DTYPE table or None. Returns (the next history, vectors (H, W, 4) float32).
    static_normal=True is NOT the definition: the moving pixels' v with the unrotated normal in the normal test, for the test that shows
    the rotated normal matters."""
    color = np.ascontiguousarray(color, np.float32)
    geometry = np.ascontiguousarray(geometry, np.float32)
    H, W = color.shape[:2]
    alpha, moments_alpha, max_history, depth_tol, normal_cos = F(alpha), F(moments_alpha), F(max_history), F(depth_tol), F(normal_cos)
    one, zero = F(1.0), F(0.0)
    vectors = np.zeros((H, W, 4), np.float32)
    with np.errstate(all="ignore"):
        n, t = geometry[..., :3], geometry[..., 3]
        hit = t <= F(99998.0)
        L = luma(color[..., :3])
        out = color.copy()
        moments = np.stack([L, L * L, np.where(hit, one, zero), np.zeros_like(L)], axis=-1).astype(np.float32)
        nxt = {"color": out, "moments": moments, "geometry": geometry.copy(), "instance": None if instance is None else np.array(instance, np.int32),
               "camera": cam}
        if prev is None:
            return nxt, vectors
        kind = np.zeros((H, W), np.uint32)
        rec = None
        if motions is not None and len(motions):
            listed = (instance >= 0) & (instance < len(motions))
            rec = motions[np.where(listed, instance, 0)]
            kind = np.where(listed, rec["kind"], np.uint32(STATIC))
        yy, xx = np.mgrid[0:H, 0:W]
        px, py = xx.astype(np.float32), yy.astype(np.float32)
        R, S = cam["toRay"], prev["camera"]["toScreen"]
        d = [dot3(R[r, 0], R[r, 1], R[r, 2], px, py, one) for r in range(3)]
        dl = np.sqrt(dot3(d[0], d[1], d[2], d[0], d[1], d[2]))
        d = [d[k] / dl for k in range(3)]
        v = [(cam["pos"][k] - prev["camera"]["pos"][k]) + d[k] * t for k in range(3)]
        nn = [n[..., k] for k in range(3)]
        moving = kind == MOVING
        if moving.any():
            P = [cam["pos"][k] + d[k] * t for k in range(3)]
            pt, nr = rec["point"], rec["normal"]
            Pp = [dot3(pt[..., 4 * k], pt[..., 4 * k + 1], pt[..., 4 * k + 2], P[0], P[1], P[2]) + pt[..., 4 * k + 3] for k in range(3)]
            v = [np.where(moving, Pp[k] - prev["camera"]["pos"][k], v[k]) for k in range(3)]
            m = [dot3(nr[..., 3 * k], nr[..., 3 * k + 1], nr[..., 3 * k + 2], n[..., 0], n[..., 1], n[..., 2]) for k in range(3)]
            ml = np.sqrt(dot3(m[0], m[1], m[2], m[0], m[1], m[2]))
            if not static_normal:
                nn = [np.where(moving, m[k] / ml, nn[k]) for k in range(3)]
        dist = np.sqrt(dot3(v[0], v[1], v[2], v[0], v[1], v[2]))
        u = [dot3(S[r, 0], S[r, 1], S[r, 2], v[0], v[1], v[2]) for r in range(3)]
        fx, fy = u[0] / u[2], u[1] / u[2]
        on_screen = (u[2] > zero) & (fx >= F(-1.0)) & (fx < F(W)) & (fy >= F(-1.0)) & (fy < F(H))
        want = hit & on_screen & (kind != NEW)
        flx, fly = np.floor(fx), np.floor(fy)
        ax, ay = fx - flx, fy - fly
        x0, y0 = np.where(want, flx, zero).astype(np.int64), np.where(want, fly, zero).astype(np.int64)
        dtol = depth_tol * dist
        pc, pm, pg = prev["color"], prev["moments"], prev["geometry"]
        sums = [np.zeros((H, W), np.float32) for _ in range(6)]           # colour r, g, b, m1, m2, N
        wsum = np.zeros((H, W), np.float32)
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = x0 + dx, y0 + dy
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx_, cy_ = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                gq, cq, mq = pg[cy_, cx_], pc[cy_, cx_], pm[cy_, cx_]
                ok = inside & (gq[..., 3] <= F(99998.0)) & (np.abs(gq[..., 3] - dist) <= dtol)
                ok &= dot3(gq[..., 0], gq[..., 1], gq[..., 2], nn[0], nn[1], nn[2]) >= normal_cos
                if flags & MATCH_INSTANCE:
                    ok &= prev["instance"][cy_, cx_] == instance
                ok &= mq[..., 2] >= one
                for a in (cq[..., 0], cq[..., 1], cq[..., 2], mq[..., 0], mq[..., 1]):
                    ok &= np.isfinite(a)
                b = (ax if dx else one - ax) * (ay if dy else one - ay)
                for s, a in zip(sums, (cq[..., 0], cq[..., 1], cq[..., 2], mq[..., 0], mq[..., 1], mq[..., 2])):
                    s[...] = np.where(ok, s + a * b, s)                    # selected away, never multiplied by zero
                wsum = np.where(ok, wsum + b, wsum)
        have = want & (wsum > F(0.01))
        h = [s / wsum for s in sums[:3]]
        m1h, m2h, Nh = sums[3] / wsum, sums[4] / wsum, sums[5] / wsum
        if flags & CLAMP:
            inf = F(np.inf)
            mn = [np.full((H, W), inf, np.float32) for _ in range(3)]
            mx = [np.full((H, W), -inf, np.float32) for _ in range(3)]
            for oy in (-1, 0, 1):
                for ox in (-1, 0, 1):
                    q, inside = shifted(color, ox, oy, 0)
                    for ch in range(3):
                        mn[ch] = np.where(inside, np.where(mn[ch] < q[..., ch], mn[ch], q[..., ch]), mn[ch])
                        mx[ch] = np.where(inside, np.where(mx[ch] > q[..., ch], mx[ch], q[..., ch]), mx[ch])
            for ch in range(3):
                hi = np.where(h[ch] > mn[ch], h[ch], mn[ch])               # max(h, mn)
                h[ch] = np.where(hi < mx[ch], hi, mx[ch])                   # min(that, mx)
        N = np.fmin(Nh + one, max_history)
        a, am = np.fmax(alpha, one / N), np.fmax(moments_alpha, one / N)
        for ch in range(3):
            out[..., ch] = np.where(have, h[ch] * (one - a) + color[..., ch] * a, color[..., ch])
        m1 = m1h * (one - am) + L * am
        m2 = m2h * (one - am) + (L * L) * am
        var = m2 - m1 * m1
        blended = np.stack([m1, m2, N, np.where(var > zero, var, zero)], axis=-1).astype(np.float32)
        moments[...] = np.where(have[..., None], blended, moments)
        state = np.where(have, F(2.0), one)
        vectors[...] = np.where(want[..., None], np.stack([fx - px, fy - py, dist, state], axis=-1), zero).astype(np.float32)
    return nxt, vectors


# ---- what tests/test_motion_cpu.py and tests/test_gpu_motion.py share ------------------------------------------------------------------------
def trs(translate=(0.0, 0.0, 0.0), axis=(0.0, 1.0, 0.0), angle=0.0, scale=(1.0, 1.0, 1.0)):
    """a forward transform in float64, row-vector convention: p_world = p_local * (S R) + t as a 4 x 4"""
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    Rm = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
    m = np.eye(4)
    m[:3, :3] = np.diag(np.asarray(scale, np.float64)) @ Rm.T
    m[3, :3] = translate
    return m


def inverse32(forward):
    """the float32 inverseTransform of a forward transform, as a CrtMeshInstance carries it"""
    return np.linalg.inv(forward).astype(np.float32)


# The hand-made table of tests/test_gpu_motion.py: guides()' instance plane remapped onto ids 0..4 (five bands along the diagonal), one entry of
# each kind and an id beyond the table's count. The moving entries are small: a shift of about a pixel and a half at guides()' near depth, and a
# rotation of 0.02 rad about an axis through the scene with a non-uniform scale within 2 %, so that most moving pixels stay on the screen.
def five_ids(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.minimum(5 * (xx + 2 * yy) // max(W + 2 * H, 1), 4).astype(np.int32)


def hand_made_inputs(H, W):
    """(planes, colour, previous history without its camera) of tests/test_gpu_temporal.py's inputs(), the instance planes of both remapped
    onto the five ids (a pixel that is no hit keeps its -1)"""
    planes, color = guides(H, W, seed=W), noisy_color(H, W, seed=W)
    hist = temporal_ref.history_content(H, W, None, seed=W)
    planes["ids"]["instance"] = np.where(planes["ids"]["instance"] < 0, -1, five_ids(H, W))
    hist["instance"] = np.where(hist["instance"] < 0, -1, five_ids(H, W)).astype(np.int32)
    return planes, color, hist


def hand_made_table():
    about = trs(translate=(0.0, 0.0, 25.0))
    turn = np.linalg.inv(about) @ trs(axis=(0.3, 1.0, 0.2), angle=0.02, scale=(1.02, 0.99, 1.01)) @ about
    base = trs(translate=(1.0, -2.0, 20.0), axis=(1.0, 0.0, 0.0), angle=0.4, scale=(2.0, 2.0, 2.0))
    entries = [motion(inverse32(base), inverse32(base)),
               motion(inverse32(base), inverse32(base @ trs(translate=(0.25, -0.125, 0.0)))),
               motion(inverse32(base), inverse32(base @ turn)),
               motion(None, inverse32(base))]
    assert [e[0] for e in entries] == [STATIC, MOVING, MOVING, NEW]
    return table(entries)                                              # id 4 lies beyond count = 4


# The Session test on `tiny` at 96 x 64: frame A, then instance SESSION_INSTANCE translated by SESSION_DELTA in world space -- along x, perpendicular
# to the camera's front (0, -0.447, -0.894) -- and frame B. Under this module the moved instance's pixels travel 2.5 pixels on the screen.
SESSION_SIZE = (96, 64)
SESSION_INSTANCE = 0
SESSION_DELTA = (0.6, 0.0, 0.0)


def translated(records, index, delta):
    """a copy of CrtMeshInstance records with instance `index` moved by `delta` in world space: p_local = (p_world - delta) * A + b"""
    out = records.copy()
    inv = out["inv"][index]
    inv[3, :3] -= np.asarray(delta, np.float32) @ inv[:3, :3]
    return out
