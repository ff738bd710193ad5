"""A numpy float32 restatement of the definition in include/crt_temporal.h: vectorised over the pixels, the four taps in the definition's order,
every operation a float32 operation of its own (numpy contracts nothing). What crtt_accumulate must give, bit for bit. The hand-made inputs are
those of tests/denoise_ref.py: guides(), noisy_color() and surface_records()."""
import numpy as np

from denoise_ref import guides, luma, noisy_color, shifted, surface_records  # noqa: F401 (the inputs are re-exported)

MATCH_INSTANCE, CLAMP = 1, 2
F = np.float32


def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def camera(pos, to_ray, to_screen=None):
    """a CrttCamera by hand: pos (3,), toRay and toScreen (3, 3) row-major, float32; toScreen defaults to the float32 rounding of toRay's
    inverse in double"""
    to_ray = np.asarray(to_ray, np.float64).reshape(3, 3)
    if to_screen is None:
        to_screen = np.linalg.inv(to_ray)
    return {"pos": np.asarray(pos, np.float32).reshape(3).copy(), "toRay": to_ray.astype(np.float32),
            "toScreen": np.asarray(to_screen, np.float64).reshape(3, 3).astype(np.float32)}


def pinhole(W, H, pos=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, fov=1.0):
    """a hand-made pinhole camera looking down +z, turned by yaw about y and then pitch about x (radians): toRay takes (i, j, 1) to a direction
    through the pixel's corner, in no normalisation in particular"""
    k = np.tan(fov / 2.0)
    base = np.array([[2.0 * k / W, 0.0, -k], [0.0, 2.0 * k * H / W / H, -k * H / W], [0.0, 0.0, 1.0]])
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    rot = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    return camera(pos, rot @ base)


def accumulate(color, geometry, instance, cam, prev=None, flags=0, alpha=0.2, moments_alpha=0.2, max_history=32.0, depth_tol=0.05, normal_cos=0.9):
    """color, geometry (H, W, 4) float32; instance (H, W) int32 or None; cam = the frame's camera(); prev = None (reset) or a history
    {"color", "moments", "geometry", "instance", "camera"}. Returns the next history, its camera = cam."""
    color = np.ascontiguousarray(color, np.float32)
    geometry = np.ascontiguousarray(geometry, np.float32)
    H, W = color.shape[:2]
    alpha, moments_alpha, max_history, depth_tol, normal_cos = F(alpha), F(moments_alpha), F(max_history), F(depth_tol), F(normal_cos)
    one, zero = F(1.0), F(0.0)
    with np.errstate(all="ignore"):
        n, t = geometry[..., :3], geometry[..., 3]
        hit = t <= F(99998.0)
        L = luma(color[..., :3])
        out = color.copy()
        moments = np.stack([L, L * L, np.where(hit, one, zero), np.zeros_like(L)], axis=-1).astype(np.float32)
        nxt = {"color": out, "moments": moments, "geometry": geometry.copy(), "instance": None if instance is None else np.array(instance, np.int32),
               "camera": cam}
        if prev is None:
            return nxt
        yy, xx = np.mgrid[0:H, 0:W]
        px, py = xx.astype(np.float32), yy.astype(np.float32)
        R, S = cam["toRay"], prev["camera"]["toScreen"]
        d = [dot3(R[r, 0], R[r, 1], R[r, 2], px, py, one) for r in range(3)]
        dl = np.sqrt(dot3(d[0], d[1], d[2], d[0], d[1], d[2]))
        d = [d[k] / dl for k in range(3)]
        v = [(cam["pos"][k] - prev["camera"]["pos"][k]) + d[k] * t for k in range(3)]
        dist = np.sqrt(dot3(v[0], v[1], v[2], v[0], v[1], v[2]))
        u = [dot3(S[r, 0], S[r, 1], S[r, 2], v[0], v[1], v[2]) for r in range(3)]
        fx, fy = u[0] / u[2], u[1] / u[2]
        on_screen = (u[2] > zero) & (fx >= F(-1.0)) & (fx < F(W)) & (fy >= F(-1.0)) & (fy < F(H))
        want = hit & on_screen
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
                ok &= dot3(gq[..., 0], gq[..., 1], gq[..., 2], n[..., 0], n[..., 1], n[..., 2]) >= normal_cos
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
    return nxt


# ---- hand-made camera pairs and inputs shared by tests/test_temporal_cpu.py and tests/test_gpu_temporal.py -------------------------------
def camera_pairs(W, H):
    """name -> (camera of the current frame, camera of the previous one), as CrttCamera values made by hand. A pixel is 2 tan(fov / 2) / W
    radians wide at the centre, so a yaw of k pixels' worth moves the picture by about k pixels: the pans are 4.5 and 2.5 pixels, no whole
    numbers, so that fx and fy of the pixels at the border fall into [-1, 0) and the taps leave the frame on every side."""
    px = 2.0 * np.tan(0.5) / W
    here = pinhole(W, H)
    behind = pinhole(W, H, pos=(0.0, 0.0, 200.0))                        # beyond every surface of guides() (t around 10 and 40), looking on: u.z <= 0
    nan_screen = pinhole(W, H)
    nan_screen["toScreen"][2, 1] = np.nan
    return {
        "identical": (here, pinhole(W, H)),
        "sub-pixel pan": (here, pinhole(W, H, yaw=0.3 * px, pitch=-0.45 * px)),
        "pan left": (here, pinhole(W, H, yaw=4.5 * px)),
        "pan right": (here, pinhole(W, H, yaw=-4.5 * px)),
        "pan up": (here, pinhole(W, H, pitch=2.5 * px)),
        "pan down": (here, pinhole(W, H, pitch=-2.5 * px)),
        "translation": (pinhole(W, H, pos=(-2.0, 0.5, 0.25)), pinhole(W, H, yaw=0.7 * px)),
        "previous camera behind the surface": (here, behind),
        "NaN in toScreen": (here, nan_screen),
    }


def reproject64(cam, prev_cam, geometry):
    """(fx, fy, u.z, dist) of every pixel in float64 from the float32 camera values: where the definition looks in the previous frame"""
    H, W = geometry.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    p = np.stack([xx, yy, np.ones_like(xx)], axis=-1).astype(np.float64)
    d = p @ cam["toRay"].astype(np.float64).T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        v = (cam["pos"].astype(np.float64) - prev_cam["pos"].astype(np.float64)) + d * geometry[..., 3:4].astype(np.float64)
        u = v @ prev_cam["toScreen"].astype(np.float64).T
        return u[..., 0] / u[..., 2], u[..., 1] / u[..., 2], u[..., 2], np.linalg.norm(v, axis=-1)


def history_content(H, W, cam, seed=0):
    """A previous history over guides(H, W, seed + 50) with everything the fetch looks at: N of 0 (also on hit pixels), 1, in between and 32,
    non-finite colours and moments, and the no-hit, far and NaN-t pixels of guides()."""
    rng = np.random.RandomState(3000 + seed)
    planes = guides(H, W, seed=seed + 50)
    hist = {"color": noisy_color(H, W, seed=seed + 60, nans=False), "geometry": planes["geometry"].copy(),
            "instance": planes["ids"]["instance"].astype(np.int32), "camera": cam}
    m = np.zeros((H, W, 4), np.float32)
    m[..., 0] = rng.uniform(0.2, 0.9, (H, W)); m[..., 1] = m[..., 0] ** 2 + rng.uniform(0.0, 0.1, (H, W))
    m[..., 2] = rng.choice(np.array([0.0, 0.5, 1.0, 1.0, 2.0, 7.25, 32.0, 32.0], np.float32), (H, W))
    m[..., 3] = rng.uniform(0.0, 0.1, (H, W))
    m[..., 2][~(planes["geometry"][..., 3] <= 99998.0)] = 0.0
    pick = lambda k: (rng.randint(0, H, k), rng.randint(0, W, k))
    k = max(1, H * W // 30)
    hist["color"][pick(k) + (rng.randint(0, 3, k),)] = np.nan
    hist["color"][pick(k) + (rng.randint(0, 3, k),)] = np.inf
    m[pick(k) + (0,)] = np.nan
    m[pick(k) + (1,)] = -np.inf
    m[pick(k) + (2,)] = np.nan
    m[pick(k) + (3,)] = np.nan                                        # the variance of a tap is never read
    hist["moments"] = m
    return hist


# The camera pair of the Session test on `tiny` at 160 x 96: the scene's own camera, then this one. tests/test_temporal_cpu.py requires that
# under the reference at least 5 % of the second frame's hit pixels keep their history and at least 5 % lose it.
SESSION_SIZE = (160, 96)
SESSION_MOVE = {"pos": (4.0, 2.0, -3.0), "front": (0.3, -0.2, 0.0)}    # added to the scene's camera_pos and camera_front (then normalised)
# the parameters of the Session test's moved frame (on a history of max_history frames already); the shares are required under these too
SESSION_MOVED_PARAMS = dict(flags=MATCH_INSTANCE, max_history=2.0, depth_tol=0.1, normal_cos=0.5, moments_alpha=0.5)


def session_second_camera(scene):
    pos = np.asarray(scene.camera_pos, np.float64) + SESSION_MOVE["pos"]
    front = np.asarray(scene.camera_front, np.float64) + SESSION_MOVE["front"]
    return pos.astype(np.float32), (front / np.linalg.norm(front)).astype(np.float32)


def camera_from_struct(c):
    """a _lib.CrttCamera as the dict this module works on"""
    return {"pos": np.array(c.pos[:], np.float32), "toRay": np.array(c.toRay[:], np.float32).reshape(3, 3),
            "toScreen": np.array(c.toScreen[:], np.float32).reshape(3, 3)}
