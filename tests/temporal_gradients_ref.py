"""The numpy restatement of the temporal reprojection of GradPath gradients (include/gdpt.h: gdpt_temporal_push_gradients*, where the
definition stands). The primal is temporal_ref.Temporal's push, unchanged; this file adds the gradient history, its gather by the
primal's taps, the Jacobian of the reprojection and the blend, in the operations and the order of the definition, without fused
multiply-adds. M(camera) is an INPUT, as in temporal_ref.

Beside its outputs a push returns the pre-blend H_x, H_y (NaN where no gradient blends), the Jacobian, and `margins` extended by
the kinds of the gradient decisions, each the smallest distance of a decision from its threshold over the pixels that reach it:
    cos     | |c_k| - cos_min |
    side    c0 / c_k against 0
    wk      w_k against 0
    jmax    | |J entry| - j_max |
A kind no pixel reached is inf; temporal_ref.MARGIN is what every case keeps."""
import numpy as np

import temporal_ref as T

GRAD_DEFAULTS = dict(j_max=4.0, cos_min=0.02)
GRAD_KINDS = ("cos", "side", "wk", "jmax")


def rays_at(cam, ox, oy):
    """temporal_ref.rays through the samples ((x + ox) / W, (y + oy) / H): (org, dir (H, W, 3)), in camera_ray's operations"""
    W, H, s, c = cam["W"], cam["H"], cam["s2c"], cam["c2w"]
    rx = ((np.arange(W) + ox) / W)[None, :] * np.ones((H, 1))
    ry = ((np.arange(H) + oy) / H)[:, None] * np.ones((1, W))
    row = lambda k: s[k, 0] * rx + s[k, 1] * ry + s[k, 2] * 0.0 + s[k, 3]      # noqa: E731
    inv_w = 1.0 / row(3)
    pt = np.stack([row(0) * inv_w, row(1) * inv_w, row(2) * inv_w], axis=-1)
    pt = pt * (1.0 / np.sqrt(pt[..., 0] * pt[..., 0] + pt[..., 1] * pt[..., 1] + pt[..., 2] * pt[..., 2]))[..., None]
    d = np.stack([c[k, 0] * pt[..., 0] + c[k, 1] * pt[..., 1] + c[k, 2] * pt[..., 2] for k in range(3)], axis=-1)
    d = d * (1.0 / np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]))[..., None]
    return T.origin(cam), d


def dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def project(Mp, X, W, H):
    """(q_x, q_y, w) of the world points X under M(prev); the division is made with w as it is"""
    row = lambda k: Mp[k, 0] * X[..., 0] + Mp[k, 1] * X[..., 1] + Mp[k, 2] * X[..., 2] + Mp[k, 3]      # noqa: E731
    sx, sy, w = row(0), row(1), row(3)
    return sx / w * W - 0.5, sy / w * H - 0.5, w


class TemporalGradients:
    """The handle: a temporal_ref.Temporal for the primal, and the gradient history. push() is one gdpt_temporal_push_gradients,
    push_plain() one gdpt_temporal_push (which makes the gradient history stale)."""

    def __init__(self, W, H):
        self.W, self.H = int(W), int(H)
        self.primal = T.Temporal(W, H)
        self.ghist = None

    def reset(self):
        self.primal.reset()
        self.ghist = None

    def push_plain(self, cam, M, u, v, feat, **params):
        self.ghist = None
        return self.primal.push(cam, M, u, v, feat, **params)

    def push(self, cam, M, u, v, feat, gx, gx_var, gy, gy_var, j_max=GRAD_DEFAULTS["j_max"], cos_min=GRAD_DEFAULTS["cos_min"],
             force_identity=False, **params):
        """Returns temporal_ref.Temporal.push's dict extended by gx_out, gx_var_out, gy_out, gy_var_out, glength (N_g'), gradient_reset
        (the count), sum_gradient_history, masks["gradient_reset"], masks["gradient_blend"], Hx, Hy, J (Jxx, Jyx, Jxy, Jyy), q (the
        reprojected position, or None where no gradient history was read).
        `force_identity`: J taken as the identity (a plain gather of the gradients), for comparisons."""
        p = dict(T.DEFAULTS, **params)
        W, H = self.W, self.H
        u = np.asarray(u, dtype=np.float64)
        g = [np.asarray(a, dtype=np.float64) for a in (gx, gy)]
        gv = [np.asarray(a, dtype=np.float64) for a in (gx_var, gy_var)]
        with np.errstate(all="ignore"):
            gok = np.ones((H, W), dtype=bool)
            for k in range(2):
                gok &= (np.isfinite(g[k]) & np.isfinite(gv[k]) & (gv[k] >= 0)).all(axis=-1)
        # a pixel with an invalid gradient is LEFT OUT of the primal too: the primal sees a NaN there, and gets its input bits back
        u_in = u.copy()
        u_in[~gok, 0] = np.nan
        prev, gprev = self.primal.hist, self.ghist
        r = self.primal.push(cam, M, u_in, v, feat, **params)
        r["out"][~gok] = u[~gok]
        self.primal.hist["U"][~gok] = u[~gok]
        ok = ~r["masks"]["left_out"]
        blend = ok & ~r["masks"]["background"] & ~r["masks"]["reset"]
        mg = {k: np.inf for k in GRAD_KINDS}

        def note(kind, values, where):
            if where.any():
                mg[kind] = min(mg[kind], float(np.abs(values[where]).min()))

        outs = [g[0].copy(), g[1].copy()]
        vouts = [gv[0].copy(), gv[1].copy()]
        glength = np.where(ok, 1.0, 0.0)
        nan = np.full((H, W, 3), np.nan)
        Hk = [nan.copy(), nan.copy()]
        J = [np.full((H, W), np.nan) for _ in range(4)]
        greset = blend.copy()
        gblend = np.zeros((H, W), dtype=bool)
        q = None
        if blend.any() and gprev is not None:
            with np.errstate(all="ignore"):
                cov = np.where(blend, feat[7], 1.0)
                d = np.where(blend, feat[6] / cov, 0.0)
                nrm = np.stack([feat[3], feat[4], feat[5]], axis=-1)
                ln = np.sqrt(dot3(nrm, nrm))
                nh = np.where(blend[..., None], nrm * (1.0 / np.where(ln > 0, ln, 1.0))[..., None], 0.0)
                org, dirs = T.rays(cam)
                X = org[None, None, :] + d[..., None] * dirs
                Mp = prev["M"]
                qx, qy, w = project(Mp, X, W, H)
                qx, qy = np.where(blend, qx, 0.0), np.where(blend, qy, 0.0)
                flx, fly = np.floor(qx), np.floor(qy)
                i0, j0 = flx.astype(np.int64), fly.astype(np.int64)
                fx, fy = qx - flx, qy - fly
                q = (qx, qy)
                dX = X - prev["org"][None, None, :]
                e = np.sqrt(dot3(dX, dX))
                S, Ngs = np.zeros((H, W)), np.zeros((H, W))
                Gs = [np.zeros((H, W, 3)), np.zeros((H, W, 3))]
                VGs = [np.zeros((H, W, 3)), np.zeros((H, W, 3))]
                for tb in (0, 1):
                    for ta in (0, 1):
                        tx, ty = i0 + ta, j0 + tb
                        t = blend & (tx >= 0) & (ty >= 0) & (tx < W) & (ty < H)
                        cx, cy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                        t = t & (prev["N"][cy, cx] >= 1.0) & (prev["cov"][cy, cx] > 0)
                        t = t & (np.abs(prev["d"][cy, cx] - e) <= p["tau_z"] * e)
                        nq = prev["n"][cy, cx]
                        t = t & (nq != 0).any(axis=-1) & (dot3(nh, nq) >= p["tau_n"])
                        bt = np.where(t, (fx if ta else 1.0 - fx) * (fy if tb else 1.0 - fy), 0.0)
                        S = S + bt
                        for k in range(2):
                            Gs[k] = Gs[k] + bt[..., None] * np.where(t[..., None], gprev["G"][k][cy, cx], 0.0)
                            VGs[k] = VGs[k] + (bt * bt)[..., None] * np.where(t[..., None], gprev["VG"][k][cy, cx], 0.0)
                        Ngs = Ngs + bt * np.where(t, gprev["N"][cy, cx], 0.0)
                Sd = np.where(blend, S, 1.0)
                G = [Gs[k] / Sd[..., None] for k in range(2)]
                VG = [VGs[k] / (Sd * Sd)[..., None] for k in range(2)]
                Ng = Ngs / Sd
                # the Jacobian: the two neighbour rays cut with the tangent plane, projected by M(prev)
                c0 = dot3(nh, dirs)
                cand = blend.copy()
                for k, (ox, oy) in enumerate(((-0.5, 0.5), (0.5, -0.5))):
                    _, dk = rays_at(cam, ox, oy)
                    ck = dot3(nh, dk)
                    note("cos", np.abs(ck) - cos_min, cand)
                    cand = cand & ~(np.abs(ck) < cos_min)
                    ratio = c0 / np.where(cand, ck, 1.0)
                    note("side", ratio, cand)
                    cand = cand & (ratio > 0)
                    tk = d * ratio
                    Xk = org[None, None, :] + tk[..., None] * dk
                    row = lambda i: Mp[i, 0] * Xk[..., 0] + Mp[i, 1] * Xk[..., 1] + Mp[i, 2] * Xk[..., 2] + Mp[i, 3]      # noqa: E731
                    sxk, syk, wk = row(0), row(1), row(3)
                    note("wk", wk, cand)
                    cand = cand & (wk > 0)
                    ws = np.where(cand, wk, 1.0)
                    jx, jy = qx - (sxk / ws * W - 0.5), qy - (syk / ws * H - 0.5)
                    for j in (jx, jy):
                        note("jmax", np.abs(j) - j_max, cand)
                    cand = cand & (np.abs(jx) <= j_max) & (np.abs(jy) <= j_max)
                    J[2 * k], J[2 * k + 1] = jx, jy
                if force_identity:
                    J = [np.ones((H, W)), np.zeros((H, W)), np.zeros((H, W)), np.ones((H, W))]
                gblend = cand
                greset = blend & ~gblend
                Ngp = np.minimum(Ng + 1.0, float(p["max_history"]))
                mix = gblend & (Ngp > 1.0)
                alpha = 1.0 / np.where(mix, Ngp, 1.0)
                keep = 1.0 - alpha
                for k in range(2):
                    a, b = J[2 * k][..., None], J[2 * k + 1][..., None]
                    Hv = a * G[0] + b * G[1]
                    VH = (a * a) * VG[0] + (b * b) * VG[1]
                    Hk[k] = np.where(gblend[..., None], Hv, np.nan)
                    outs[k] = np.where(mix[..., None], Hv + alpha[..., None] * (g[k] - Hv), g[k])
                    vouts[k] = np.where(mix[..., None], (keep * keep)[..., None] * VH + (alpha * alpha)[..., None] * gv[k], gv[k])
                glength = np.where(gblend, Ngp, glength)
                J = [np.where(gblend, j, np.nan) for j in J]
        self.ghist = dict(G=[outs[0].copy(), outs[1].copy()], VG=[vouts[0].copy(), vouts[1].copy()], N=glength.copy())
        r["margins"] = dict(r["margins"], **mg)
        r["masks"] = dict(r["masks"], gradient_reset=greset, gradient_blend=gblend)
        r.update(gx_out=outs[0], gx_var_out=vouts[0], gy_out=outs[1], gy_var_out=vouts[1], glength=glength, gradient_reset=int(greset.sum()),
                 sum_gradient_history=float(glength.sum()), Hx=Hk[0], Hy=Hk[1], J=J, q=q)
        return r


# ---- the cases the tests share ------------------------------------------------------------------------------------------------

def case(W, H, move, planted, seed=0):
    """temporal_ref.case extended by random gradients and variances: [(camera, u, v, feat, gx, gx_var, gy, gy_var)]. `planted`
    additionally has a NaN gradient and a negative gradient variance in frames 0 and 1, each on a pixel of its own that
    temporal_ref.case leaves alone (on a film of fewer than eight pixels nothing is added)."""
    rng = np.random.default_rng(77000 + 1000 * W + 10 * H + seed)
    frames = []
    for k, (cam, u, v, feat) in enumerate(T.case(W, H, move, planted, seed)):
        gx, gy = rng.uniform(-0.5, 0.5, (H, W, 3)), rng.uniform(-0.5, 0.5, (H, W, 3))
        gxv, gyv = rng.uniform(0.01, 0.02, (H, W, 3)), rng.uniform(0.01, 0.02, (H, W, 3))
        if planted and W * H >= 8 and k < 2:
            taken = {int(i) for i in (np.arange(5) * (W * H // 5) + (W * H // 11) + k) % (W * H)}
            free = [i for i in range(W * H) if i not in taken]
            (y0, x0), (y1, x1) = divmod(free[len(free) // 3], W), divmod(free[2 * len(free) // 3], W)
            gy[y0, x0, 1] = np.nan
            gxv[y1, x1, 2] = -1e-3
        frames.append((cam, u, v, feat, gx, gxv, gy, gyv))
    return frames
