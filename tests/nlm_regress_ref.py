"""numpy restatement of the first-order feature regression on the non-local-means weights (include/gdpt.h:
gdpt_denoise_nlm_regress*), on the helpers of tests/nlm_ref.py and tests/nlm_guided_ref.py: the guided filter's weights, and a weighted
linear fit of the colour on the regressor planes in the place of the weighted mean. Not collected by pytest;
tests/test_nlm_regress_ref.py pins it, tests/test_gpu_nlm_regress.py holds the kernels against it.

    denoise(img, var, feat, fvar, groups, channels, scales, ridge, k_f, alpha_f, r, f, k, alpha, eps) -> the dict of nlm_ref.denoise
    brute_force(...)            the same pixel by pixel, for small films
    ldlt_solve(A, rhs)          the header's LDL^T on stacked matrices: A (..., d, d), rhs (..., d, n)
    feat, fvar: (channels, H, W) planes; groups: a list of (first_channel, num_channels, tau); channels, scales: the regressors
    synthetic_regression(seed)  the film of the quality test: nlm_guided_ref's textured film with a normal and a depth plane"""
import numpy as np

import nlm_guided_ref
import nlm_ref
from nlm_guided_ref import feature_distance
from nlm_ref import box, film_sums, shifted

REGRESS_DEFAULTS = dict(channels=(0, 1, 2, 3, 4, 5), scales=(1.0,) * 6, ridge=1e-2)


def valid_mask(img, var, feat, fvar, groups, channels):
    """HxW: valid for the guided filter, and every regressor plane is finite there with variance >= 0."""
    ok = nlm_guided_ref.valid_mask(img, var, feat, fvar, groups)
    for c in channels:
        with np.errstate(invalid="ignore"):
            ok = ok & np.isfinite(feat[c]) & np.isfinite(fvar[c]) & (fvar[c] >= 0)
    return ok


def ldlt_solve(A, rhs):
    """A x = rhs by LDL^T without pivoting, in the order of include/gdpt.h; only the lower triangle of A is read."""
    A, rhs = np.asarray(A, dtype=np.float64), np.asarray(rhs, dtype=np.float64)
    d = A.shape[-1]
    L = np.zeros_like(A)
    D = np.zeros(A.shape[:-1])
    for j in range(d):
        v = [L[..., j, k] * D[..., k] for k in range(j)]
        t = A[..., j, j].copy()
        for k in range(j):
            t = t - L[..., j, k] * v[k]
        D[..., j] = t
        for i in range(j + 1, d):
            t = A[..., i, j].copy()
            for k in range(j):
                t = t - L[..., i, k] * v[k]
            L[..., i, j] = t / D[..., j]
    x = np.zeros_like(rhs)
    for i in range(d):                      # L y = rhs
        t = rhs[..., i, :].copy()
        for k in range(i):
            t = t - L[..., i, k, None] * x[..., k, :]
        x[..., i, :] = t
    for i in range(d):                      # D z = y
        x[..., i, :] = x[..., i, :] / D[..., i, None]
    for i in range(d - 1, -1, -1):          # L^T x = z
        t = x[..., i, :].copy()
        for k in range(i + 1, d):
            t = t - L[..., k, i, None] * x[..., k, :]
        x[..., i, :] = t
    return x


def denoise(img, var, feat, fvar, groups=(), channels=(), scales=None, ridge=1e-2, k_f=0.6, alpha_f=1.0, r=10, f=3, k=0.45, alpha=1.0,
            eps=1e-10):
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    groups, channels = list(groups), list(channels)
    scales = [1.0] * len(channels) if scales is None else list(scales)
    m, d = len(channels), 1 + len(channels)
    if groups or channels:
        feat, fvar = np.asarray(feat, dtype=np.float64), np.asarray(fvar, dtype=np.float64)
    ok = valid_mask(img, var, feat, fvar, groups, channels)
    ok3 = ok[:, :, None]
    h, w = ok.shape
    u, v = np.where(ok3, img, 0.0), np.where(ok3, var, 0.0)
    if groups or channels:
        g, s = np.where(ok[None], feat, 0.0), np.where(ok[None], fvar, 0.0)
    k2 = k * k

    def weights(oy, ox):
        ub, vb, okb = shifted(u, oy, ox, 0.0), shifted(v, oy, ox, 0.0), shifted(ok, oy, ox, False)
        both = ok & okb
        with np.errstate(all="ignore"):
            dd = u - ub
            t = (dd * dd - alpha * (v + np.minimum(vb, v))) / (eps + k2 * (v + vb))
            e = np.where(both, ((t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]) / 3.0, 0.0)
            S, C = box(e, f), box(both.astype(np.int64), f)
            D = S / np.maximum(C, 1)
            D = np.where(D > 0, D, 0.0)
            if groups:
                gb = np.stack([shifted(p, oy, ox, 0.0) for p in g])
                sb = np.stack([shifted(p, oy, ox, 0.0) for p in s])
                D = np.fmax(D, feature_distance(g, s, gb, sb, groups, k_f, alpha_f))
            wgt = np.where(both, np.exp(-D), 0.0)
        z = [np.ones((h, w))] + [(shifted(g[c], oy, ox, 0.0) - g[c]) / scales[j] for j, c in enumerate(channels)]
        return wgt, z, ub, vb

    A, b = np.zeros((h, w, d, d)), np.zeros((h, w, d, 3))
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            wgt, z, ub, vb = weights(oy, ox)
            for i in range(d):
                wz = wgt * z[i]
                for j in range(i + 1):
                    A[:, :, i, j] += wz * z[j]
                b[:, :, i, :] += wz[:, :, None] * ub
    W = A[:, :, 0, 0].copy()
    for j in range(1, d):
        A[:, :, j, j] += ridge * W
    A[~ok] = np.eye(d)                       # (an invalid pixel has no equations; it keeps its input below)
    rhs = np.concatenate([b, np.zeros((h, w, d, 1))], axis=3)
    rhs[:, :, 0, 3] = 1.0
    x = ldlt_solve(A, rhs)
    beta0, q = x[:, :, 0, :3], x[:, :, :, 3]
    vacc = np.zeros_like(u)
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            wgt, z, ub, vb = weights(oy, ox)
            lin = q[:, :, 0].copy()
            for j in range(1, d):
                lin = lin + q[:, :, j] * z[j]
            t = wgt * lin
            vacc += (t * t)[:, :, None] * vb
    out, var_out = np.where(ok3, beta0, img), np.where(ok3, vacc, var)
    res = dict(out=out, var_out=var_out)
    res.update(film_sums(img, var, out, var_out, ok))
    return res


def brute_force(img, var, feat, fvar, groups=(), channels=(), scales=None, ridge=1e-2, k_f=0.6, alpha_f=1.0, r=10, f=3, k=0.45, alpha=1.0,
                eps=1e-10):
    """The definition read literally, pixel by pixel: the weights of nlm_guided_ref.brute_force, numpy's own solver for the fit."""
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    groups, channels = list(groups), list(channels)
    scales = [1.0] * len(channels) if scales is None else list(scales)
    d = 1 + len(channels)
    hh, ww = img.shape[:2]
    ok = valid_mask(img, var, feat, fvar, groups, channels)
    out, var_out = img.copy(), var.copy()
    inside = lambda x, y: 0 <= x < ww and 0 <= y < hh      # noqa: E731
    for y in range(hh):
        for x in range(ww):
            if not ok[y, x]:
                continue
            taps = []
            for oy in range(-r, r + 1):
                for ox in range(-r, r + 1):
                    qx, qy = x + ox, y + oy
                    if not inside(qx, qy) or not ok[qy, qx]:
                        continue
                    S, C = 0.0, 0
                    for ny in range(-f, f + 1):
                        for nx in range(-f, f + 1):
                            ax, ay = x + nx, y + ny
                            bx, by = ax + ox, ay + oy
                            if not (inside(ax, ay) and inside(bx, by) and ok[ay, ax] and ok[by, bx]):
                                continue
                            ua, va, ub, vb = img[ay, ax], var[ay, ax], img[by, bx], var[by, bx]
                            t = ((ua - ub) ** 2 - alpha * (va + np.minimum(vb, va))) / (eps + k * k * (va + vb))
                            S += t.sum() / 3.0
                            C += 1
                    Df = 0.0
                    for first, count, tau in groups:
                        phi = 0.0
                        for c in range(first, first + count):
                            gp, sp, gq, sq = feat[c, y, x], fvar[c, y, x], feat[c, qy, qx], fvar[c, qy, qx]
                            phi += ((gp - gq) ** 2 - alpha_f * (sp + min(sq, sp))) / (k_f * k_f * max(tau, sp + sq))
                        Df = max(Df, phi / count)
                    wgt = float(np.exp(-max(max(0.0, S / C), Df)))
                    z = np.array([1.0] + [(feat[c, qy, qx] - feat[c, y, x]) / scales[j] for j, c in enumerate(channels)])
                    taps.append((wgt, z, img[qy, qx], var[qy, qx]))
            A, b, W = np.zeros((d, d)), np.zeros((d, 3)), 0.0
            for wgt, z, uq, vq in taps:
                W += wgt
                A += wgt * np.outer(z, z)
                b += wgt * np.outer(z, uq)
            A[np.arange(1, d), np.arange(1, d)] += ridge * W
            beta = np.linalg.solve(A, b)
            e0 = np.zeros(d)
            e0[0] = 1.0
            q = np.linalg.solve(A, e0)
            out[y, x] = beta[0]
            var_out[y, x] = sum((wgt * float(q @ z)) ** 2 * vq for wgt, z, uq, vq in taps)
    res = dict(out=out, var_out=var_out)
    res.update(film_sums(img, var, out, var_out, ok))
    return res


def synthetic_regression(seed):
    """(truth, mean, variance of the mean, 7 feature planes (albedo, normal, depth), their variances): nlm_guided_ref's textured film;
    the normal turns with the right half's sinusoid, the depth ramps with the left half's; four samples of each with N(0, 0.01^2)
    noise (depth 0.005^2)."""
    truth, mean, var, alb, albv = nlm_guided_ref.synthetic_textured(seed)
    y, x = np.mgrid[0:nlm_ref.H_SYN, 0:nlm_ref.W_SYN].astype(float)
    disc = (x - 26.0) ** 2 + (y - 14.0) ** 2 < 49.0
    nx = np.where(disc, 0.0, np.where(x < 24, 0.0, 0.6 * np.sin(2 * np.pi * x / 12.0)))
    nz = np.sqrt(1 - nx * nx)
    ny = 0 * nx
    depth = np.where(disc, 1.0, np.where(x < 24, 2.0 + 1.5 * y / 39, 3.0))
    clean = np.stack([nx, ny, nz, depth])
    rng = np.random.default_rng(200 + seed)
    sig = np.array([0.01, 0.01, 0.01, 0.005])[:, None, None]
    fs = np.stack([clean + sig * rng.standard_normal(clean.shape) for _ in range(4)])
    feat = np.concatenate([alb, fs.mean(0)])
    fvar = np.concatenate([albv, fs.var(0, ddof=1) / 4])
    return truth, mean, var, feat, fvar
