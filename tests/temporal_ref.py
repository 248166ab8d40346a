"""The numpy restatement of temporal reprojection (include/gdpt.h: gdpt_temporal_*, where the definition stands), and the synthetic
geometry its tests use: a pinhole camera looking at planes, with the depth, normal and coverage planes computed analytically.

The restatement takes M(camera) as an INPUT (the library's matrix on the GPU, numpy's inverses in the CPU tests): the per-pixel
arithmetic is defined on M alone, in the operations and the order of the definition, without fused multiply-adds.

Beside its outputs a push returns the smallest distance of every kind of decision from its threshold (`margins`), so that a test
can show that no discontinuous decision sits where a fused multiply-add could flip it between numpy and the kernel:
    w       w against 0
    guard   q against the guard -1 <= q <= W (H)
    floor   f against 0 and 1
    depth   | |d_prev - e| - tau_z e |
    normal  | n^ . n^_prev - tau_n |
    s       | S - s_min |
A kind no pixel reached is inf. MARGIN is what every case of every test must keep: a condition on the inputs, not a tolerance.
`floor` is the one kind with no discontinuity behind it: bilinear interpolation is continuous across an integer q (the tap that a
flipped floor brings in has weight f ~ 0), so under IDENTICAL cameras, where q is an integer up to rounding and f is 0 or 1 up to
an ulp, margin(m, identical=True) leaves it out; everywhere else it is held like the others."""
import numpy as np

MARGIN = 1e-9
DEFAULTS = dict(tau_z=0.05, tau_n=0.9, s_min=1e-3, max_history=32)
KINDS = ("w", "guard", "floor", "depth", "normal", "s")


def margin(m, identical=False):
    return min(v for k, v in m.items() if not (identical and k == "floor"))


# ---- cameras ------------------------------------------------------------------------------------------------------------------

def look_at(pos, target, up=(0.0, 1.0, 0.0)):
    """cam_to_world of a camera at `pos` looking at `target`: columns right, up, forward, position (the camera looks along +z)."""
    pos, target, up = (np.asarray(a, dtype=np.float64) for a in (pos, target, up))
    f = target - pos
    f /= np.linalg.norm(f)
    r = np.cross(up, f)
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, u, f, pos
    return m


def pinhole(W, H, fov_deg=40.0, near=0.1):
    """sample_to_cam of a pinhole: the inverse of (NDC -> [0, 1]^2, y down) . perspective; the sample (rx, ry, 0) lies on the near plane."""
    t = np.tan(np.radians(fov_deg) / 2)
    ty = t * H / W
    P = np.array([[1 / t, 0, 0, 0], [0, 1 / ty, 0, 0], [0, 0, 1.0, -near], [0, 0, 1.0, 0]])
    A = np.array([[0.5, 0, 0, 0.5], [0, -0.5, 0, 0.5], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])
    return np.linalg.inv(A @ P)


def camera(W, H, c2w, fov_deg=40.0):
    return dict(W=int(W), H=int(H), s2c=pinhole(W, H, fov_deg), c2w=np.array(c2w, dtype=np.float64))


def world_to_sample(cam):
    """M(camera) by numpy's inverses (the CPU tests; the GPU tests take the library's)."""
    return np.linalg.inv(cam["s2c"]) @ np.linalg.inv(cam["c2w"])


def origin(cam):
    m = cam["c2w"]
    return m[:3, 3] * (1.0 / m[3, 3])


def rays(cam):
    """(org (3,), dir (H, W, 3)): the camera rays through the pixel centres, in camera_ray's operations."""
    W, H, s, c = cam["W"], cam["H"], cam["s2c"], cam["c2w"]
    rx = ((np.arange(W) + 0.5) / W)[None, :] * np.ones((H, 1))
    ry = ((np.arange(H) + 0.5) / H)[:, None] * np.ones((1, W))
    row = lambda k: s[k, 0] * rx + s[k, 1] * ry + s[k, 2] * 0.0 + s[k, 3]      # noqa: E731
    inv_w = 1.0 / row(3)
    pt = np.stack([row(0) * inv_w, row(1) * inv_w, row(2) * inv_w], axis=-1)
    pt = pt * (1.0 / np.sqrt(pt[..., 0] * pt[..., 0] + pt[..., 1] * pt[..., 1] + pt[..., 2] * pt[..., 2]))[..., None]
    d = np.stack([c[k, 0] * pt[..., 0] + c[k, 1] * pt[..., 1] + c[k, 2] * pt[..., 2] for k in range(3)], axis=-1)
    d = d * (1.0 / np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]))[..., None]
    return origin(cam), d


# ---- synthetic geometry -------------------------------------------------------------------------------------------------------

def plane(point, normal, x_max=None):
    """A plane through `point`; with x_max only its part with world x <= x_max (the near plane of a step)."""
    return dict(p=np.asarray(point, dtype=np.float64), n=np.asarray(normal, dtype=np.float64), x_max=x_max)


def features(cam, planes, normal_scale=0.7):
    """The (8, H, W) planes of a feature render of `planes` at one sample a pixel, through the pixel centre: the nearest hit's normal
    (times normal_scale: the definition normalises), depth and coverage 1; all 0 on a miss. Also the index of the plane hit (-1: none)."""
    org, d = rays(cam)
    H, W = d.shape[:2]
    best_t, which = np.full((H, W), np.inf), np.full((H, W), -1)
    for k, pl in enumerate(planes):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((pl["p"] - org) @ pl["n"]) / (d @ pl["n"])
        hit = np.isfinite(t) & (t > 0)
        if pl["x_max"] is not None:
            hit &= (org[0] + np.where(hit, t, 0.0) * d[..., 0]) <= pl["x_max"]
        closer = hit & (t < best_t)
        best_t, which = np.where(closer, t, best_t), np.where(closer, k, which)
    f = np.zeros((8, H, W))
    for k, pl in enumerate(planes):
        m = which == k
        n = pl["n"] / np.linalg.norm(pl["n"]) * normal_scale
        f[0:3, m] = 0.5
        for c in range(3):
            f[3 + c, m] = n[c]
        f[6, m], f[7, m] = best_t[m], 1.0
    return f, which


# ---- the restatement ----------------------------------------------------------------------------------------------------------

class Temporal:
    """The handle: the history and the previous camera. push() is one gdpt_temporal_push."""

    def __init__(self, W, H):
        self.W, self.H = int(W), int(H)
        self.reset()

    def reset(self):
        self.hist = None

    def push(self, cam, M, u, v, feat, **params):
        """cam: camera(); M: M(cam), 4x4. Returns dict: out, var_out, length (N'), left_out, background, reset (the counts),
        sum_history, masks (left_out, background, reset: HxW bools), margins."""
        p = dict(DEFAULTS, **params)
        W, H = self.W, self.H
        u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
        mg = {k: np.inf for k in KINDS}

        def note(kind, values, where):
            if where.any():
                mg[kind] = min(mg[kind], float(np.abs(values[where]).min()))

        with np.errstate(all="ignore"):
            ok = (np.isfinite(u) & np.isfinite(v) & (v >= 0)).all(axis=-1)
            cov = feat[7]
            bg = ok & ~(cov > 0)
            surf = ok & (cov > 0)
            d = np.where(surf, feat[6] / np.where(surf, cov, 1.0), 0.0)
            nrm = np.stack([feat[3], feat[4], feat[5]], axis=-1)
            ln = np.sqrt(nrm[..., 0] * nrm[..., 0] + nrm[..., 1] * nrm[..., 1] + nrm[..., 2] * nrm[..., 2])
            nh = np.where((ln > 0)[..., None], nrm * (1.0 / np.where(ln > 0, ln, 1.0))[..., None], 0.0)
            nh = np.where(surf[..., None], nh, 0.0)
            facing = (nh != 0).any(axis=-1)
            out, var_out = u.copy(), v.copy()
            length = np.where(ok, 1.0, 0.0)
            blend = np.zeros((H, W), dtype=bool)
            if self.hist is not None:
                h = self.hist
                cand = surf & facing
                org, dirs = rays(cam)
                X = org[None, None, :] + d[..., None] * dirs
                Mp = h["M"]
                row = lambda k: Mp[k, 0] * X[..., 0] + Mp[k, 1] * X[..., 1] + Mp[k, 2] * X[..., 2] + Mp[k, 3]      # noqa: E731
                sx, sy, w = row(0), row(1), row(3)
                note("w", w, cand)
                cand = cand & (w > 0)
                ws = np.where(cand, w, 1.0)
                qx, qy = sx / ws * W - 0.5, sy / ws * H - 0.5
                for q, n in ((qx, W), (qy, H)):
                    note("guard", q + 1.0, cand)
                    note("guard", n - q, cand)
                cand = cand & (qx >= -1.0) & (qx <= W) & (qy >= -1.0) & (qy <= H)
                qx, qy = np.where(cand, qx, 0.0), np.where(cand, qy, 0.0)
                flx, fly = np.floor(qx), np.floor(qy)
                i0, j0 = flx.astype(np.int64), fly.astype(np.int64)
                fx, fy = qx - flx, qy - fly
                for f in (fx, fy):
                    note("floor", f, cand)
                    note("floor", 1.0 - f, cand)
                dX = X - h["org"][None, None, :]
                e = np.sqrt(dX[..., 0] * dX[..., 0] + dX[..., 1] * dX[..., 1] + dX[..., 2] * dX[..., 2])
                S, Ns = np.zeros((H, W)), np.zeros((H, W))
                Us, Vs = np.zeros((H, W, 3)), np.zeros((H, W, 3))
                for tb in (0, 1):
                    for ta in (0, 1):
                        tx, ty = i0 + ta, j0 + tb
                        t = cand & (tx >= 0) & (ty >= 0) & (tx < W) & (ty < H)
                        cx, cy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                        Nq = h["N"][cy, cx]
                        t = t & (Nq >= 1.0) & (h["cov"][cy, cx] > 0)
                        dz = np.abs(h["d"][cy, cx] - e)
                        note("depth", dz - p["tau_z"] * e, t)
                        t = t & (dz <= p["tau_z"] * e)
                        nq = h["n"][cy, cx]
                        t = t & (nq != 0).any(axis=-1)
                        dot = nh[..., 0] * nq[..., 0] + nh[..., 1] * nq[..., 1] + nh[..., 2] * nq[..., 2]
                        note("normal", dot - p["tau_n"], t)
                        t = t & (dot >= p["tau_n"])
                        bt = np.where(t, (fx if ta else 1.0 - fx) * (fy if tb else 1.0 - fy), 0.0)
                        S = S + bt
                        Us = Us + bt[..., None] * np.where(t[..., None], h["U"][cy, cx], 0.0)
                        Vs = Vs + (bt * bt)[..., None] * np.where(t[..., None], h["V"][cy, cx], 0.0)
                        Ns = Ns + bt * np.where(t, Nq, 0.0)
                note("s", S - p["s_min"], cand)
                blend = cand & (S >= p["s_min"])
                Sd = np.where(blend, S, 1.0)
                U, V, N = Us / Sd[..., None], Vs / (Sd * Sd)[..., None], Ns / Sd
                Np = np.minimum(N + 1.0, float(p["max_history"]))
                mix = blend & (Np > 1.0)
                alpha = 1.0 / np.where(mix, Np, 1.0)
                keep = 1.0 - alpha
                out = np.where(mix[..., None], U + alpha[..., None] * (u - U), u)
                var_out = np.where(mix[..., None], (keep * keep)[..., None] * V + (alpha * alpha)[..., None] * v, v)
                length = np.where(blend, Np, length)
            reset = surf & ~blend
        self.hist = dict(U=out.copy(), V=var_out.copy(), N=length.copy(), n=nh, d=d, cov=np.where(surf, cov, 0.0),
                         M=np.array(M, dtype=np.float64).reshape(4, 4), org=origin(cam))
        return dict(out=out, var_out=var_out, length=length, left_out=int((~ok).sum()), background=int(bg.sum()), reset=int(reset.sum()),
                    sum_history=float(length.sum()), masks=dict(left_out=~ok, background=bg, reset=reset), margins=mg)


# ---- the cases the tests share ------------------------------------------------------------------------------------------------

FOV = 40.0
Z_FAR, Z_NEAR = 10.0, 6.0
MOVES = ("identical", "subpixel_pan", "quarter_pan", "dolly", "rotation", "behind")


def step_scene(tilted=True):
    """A far plane z = Z_FAR that ends at world x = 2.5 (background to its right) and in front of it a near plane through z = Z_NEAR
    that ends at x = -0.3: a depth step, and with `tilted` a normal that fails tau_n = 0.9 against the far plane's."""
    return [plane((0, 0, Z_FAR), (0, 0, -1), x_max=2.5), plane((0, 0, Z_NEAR), (0.6, 0.1, -1) if tilted else (0, 0, -1), x_max=-0.3)]


def far_pixel(W):
    """the width of a pixel on the far plane, seen from z = 0"""
    return 2 * Z_FAR * np.tan(np.radians(FOV) / 2) / W


def move_cameras(W, H, move):
    """The three cameras of the consecutive pushes of `move`. Pans are k + 0.37 pixels (of the far plane) to the left, where the far plane goes on, and 0.29 down, never
    whole pixels, so that no fraction f sits at 0 or 1."""
    px = far_pixel(W)
    at = lambda pos, yaw=0.0: camera(W, H, look_at(pos, (pos[0] + np.sin(yaw), pos[1], pos[2] + np.cos(yaw))), FOV)      # noqa: E731
    if move == "identical":
        c = at((0, 0, 0))
        return [c, c, c]
    if move == "subpixel_pan":
        return [at((-0.37 * k * px, 0.29 * k * px, 0)) for k in range(3)]
    if move == "quarter_pan":
        return [at((-(W // 4 + 0.37) * k * px, 0.29 * k * px, 0)) for k in range(3)]
    if move == "dolly":
        return [at((0.013 + 0.0171 * k, 0.007 + 0.0093 * k, 0.8 * k)) for k in range(3)]      # (it drifts: the centre pixel moves too)
    if move == "rotation":
        return [at((0.011, 0.006 + 0.0113 * k, 0), np.radians(3.1 * k)) for k in range(3)]       # (and rises: a yaw alone keeps the middle row)
    if move == "behind":       # the middle camera stands behind the near plane: in the third push those points have w <= 0
        return [at((0.013, 0.007, 0)), at((0.021, 0.012, 8.0)), at((0.013, 0.007, 0))]
    raise ValueError(move)


def case(W, H, move, planted, seed=0):
    """Three frames of `move` on the step scene: [(camera, u, v, feat)] with u, v random and feat analytic. `planted`: a non-finite
    u, a non-finite v, a negative v, a zero coverage and a zero normal in frames 0 and 1, each on a pixel of its own (on a film of
    fewer than six pixels one NaN in frame 1)."""
    rng = np.random.default_rng(1000 * W + 10 * H + seed)
    cams, frames = move_cameras(W, H, move), []
    for k, cam in enumerate(cams):
        u, v = rng.uniform(0.5, 1.5, (H, W, 3)), rng.uniform(0.01, 0.02, (H, W, 3))
        feat, _ = features(cam, step_scene())
        if planted and W * H < 6 and k == 1:
            u[0, 0, 1] = np.nan
        elif planted and W * H >= 6 and k < 2:
            spots = [divmod(int(i), W) for i in (np.arange(5) * (W * H // 5) + (W * H // 11) + k) % (W * H)]
            (y0, x0), (y1, x1), (y2, x2), (y3, x3), (y4, x4) = spots
            u[y0, x0, 2] = np.nan
            v[y1, x1, 0] = np.inf
            v[y2, x2, 1] = -1e-3
            feat[3:8, y3, x3] = 0.0
            feat[3:6, y4, x4] = 0.0
        frames.append((cam, u, v, feat))
    return frames


def gdpt_camera(G, cam):
    """the GdptCamera of a camera() (box filter of width 1)"""
    c = G.GdptCamera()
    for i in range(16):
        c.sample_to_cam[i], c.cam_to_world[i] = float(cam["s2c"].flat[i]), float(cam["c2w"].flat[i])
    c.width, c.height, c.filter_type, c.filter_param = cam["W"], cam["H"], 0, 1.0
    return c
