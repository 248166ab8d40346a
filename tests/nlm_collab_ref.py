"""numpy restatement of the collaborative form of the first-order feature regression (include/gdpt.h: gdpt_denoise_nlm_collab*), on
the helpers of tests/nlm_regress_ref.py and tests/nlm_ref.py: the regression's weights and fit with the whole solution kept per pixel,
then every pixel's weighted average of all fits whose windows cover it. Not collected by pytest; tests/test_nlm_collab_ref.py pins
it, tests/test_gpu_nlm_collab.py holds the kernels against it.

    denoise(img, var, feat, fvar, groups, channels, scales, ridge, k_f, alpha_f, r, f, k, alpha, eps) -> dict: out (H, W, 3), coef
                                (3 d, H, W; plane c d + j holds beta_c,j), and the film sums of nlm_ref.film_sums, of which sum_var_out
                                and error_out are NaN: the estimator has no variance estimate
    brute_force(...)            the same by pixel, offset and tap with numpy's own solver, for small films
    feat, fvar: (channels, H, W) planes; groups: a list of (first_channel, num_channels, tau); channels, scales: the regressors"""
import numpy as np

from nlm_guided_ref import feature_distance
from nlm_ref import box, film_sums, shifted
from nlm_regress_ref import ldlt_solve, valid_mask


def _sums(img, var, out, ok):
    res = film_sums(img, var, out, np.zeros_like(out), ok)
    res["sum_var_out"] = res["error_out"] = float("nan")
    return res


def _planes(beta, img, ok):
    """(H, W, d, 3) solutions -> the coefficient film (3 d, H, W); an invalid pixel holds its input bits in plane c d and 0 elsewhere."""
    h, w, d, _ = beta.shape
    coef = np.zeros((3 * d, h, w))
    for c in range(3):
        for j in range(d):
            coef[c * d + j] = np.where(ok, beta[:, :, j, c], img[:, :, c] if j == 0 else 0.0)
    return coef


def denoise(img, var, feat, fvar, groups=(), channels=(), scales=None, ridge=1e-2, k_f=0.6, alpha_f=1.0, r=10, f=3, k=0.45, alpha=1.0,
            eps=1e-10):
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    groups, channels = list(groups), list(channels)
    scales = [1.0] * len(channels) if scales is None else list(scales)
    d = 1 + len(channels)
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
        """w_o(p), z(p, o) and u(p + o), indexed at p: nlm_regress_ref.denoise's"""
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
        return wgt, z, ub

    # the fit: nlm_regress_ref.denoise's normal equations, every solution kept
    A, b = np.zeros((h, w, d, d)), np.zeros((h, w, d, 3))
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            wgt, z, ub = weights(oy, ox)
            for i in range(d):
                wz = wgt * z[i]
                for j in range(i + 1):
                    A[:, :, i, j] += wz * z[j]
                b[:, :, i, :] += wz[:, :, None] * ub
    W = A[:, :, 0, 0].copy()
    for j in range(1, d):
        A[:, :, j, j] += ridge * W
    A[~ok] = np.eye(d)                       # (an invalid pixel has no equations; it keeps its input below)
    beta = ldlt_solve(A, b)                  # (h, w, d, 3)
    # the gather, in row-major order of t: q = p - t takes the fit of p, whose offset to q is o = -t
    num, den = np.zeros((h, w, 3)), np.zeros((h, w))
    for ty in range(-r, r + 1):
        for tx in range(-r, r + 1):
            wgt, z, _ = weights(-ty, -tx)
            pred = beta[:, :, 0, :].copy()
            for j in range(1, d):
                pred = pred + beta[:, :, j, :] * z[j][:, :, None]
            num += shifted(wgt[:, :, None] * pred, ty, tx, 0.0)
            den += shifted(wgt, ty, tx, 0.0)
    with np.errstate(all="ignore"):
        out = np.where(ok3, num / den[:, :, None], img)
    res = dict(out=out, coef=_planes(beta, img, ok))
    res.update(_sums(img, var, out, ok))
    return res


def brute_force(img, var, feat, fvar, groups=(), channels=(), scales=None, ridge=1e-2, k_f=0.6, alpha_f=1.0, r=10, f=3, k=0.45, alpha=1.0,
                eps=1e-10):
    """The definition read literally: every valid p's weights by pixel, offset and tap and its fit by numpy's own solver; then every
    valid q's average over the p = q + t of p's fit at q under the weight p gave q."""
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    groups, channels = list(groups), list(channels)
    scales = [1.0] * len(channels) if scales is None else list(scales)
    d = 1 + len(channels)
    hh, ww = img.shape[:2]
    ok = valid_mask(img, var, feat, fvar, groups, channels)
    inside = lambda x, y: 0 <= x < ww and 0 <= y < hh      # noqa: E731
    design = lambda px, py, qx, qy: np.array([1.0] + [(feat[c, qy, qx] - feat[c, py, px]) / scales[j] for j, c in enumerate(channels)])      # noqa: E731
    beta = np.zeros((hh, ww, d, 3))
    given = {}                                # (px, py, qx, qy) -> the weight the fit centred at p gave q
    for y in range(hh):
        for x in range(ww):
            if not ok[y, x]:
                continue
            A, b, W = np.zeros((d, d)), np.zeros((d, 3)), 0.0
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
                    z = design(x, y, qx, qy)
                    given[(x, y, qx, qy)] = wgt
                    W += wgt
                    A += wgt * np.outer(z, z)
                    b += wgt * np.outer(z, img[qy, qx])
            A[np.arange(1, d), np.arange(1, d)] += ridge * W
            beta[y, x] = np.linalg.solve(A, b)
    out = img.copy()
    for y in range(hh):
        for x in range(ww):
            if not ok[y, x]:
                continue
            num, den = np.zeros(3), 0.0
            for ty in range(-r, r + 1):
                for tx in range(-r, r + 1):
                    px, py = x + tx, y + ty
                    if not inside(px, py) or not ok[py, px]:
                        continue
                    wgt = given[(px, py, x, y)]
                    num += wgt * (design(px, py, x, y) @ beta[py, px])
                    den += wgt
            out[y, x] = num / den
    res = dict(out=out, coef=_planes(beta, img, ok))
    res.update(_sums(img, var, out, ok))
    return res
