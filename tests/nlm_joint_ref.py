"""numpy restatement of the joint non-local-means filter of include/gdpt.h (gdpt_denoise_nlm_joint*): nlm_guided_ref.denoise, whose
weights also average companion films. Not collected by pytest; tests/test_nlm_joint_ref.py pins it, tests/test_gpu_nlm_joint.py holds
the kernels against it.

    denoise(img, var, comps, comp_vars, feat, fvar, groups, k_f, alpha_f, r, f, k, alpha, eps)
        -> the dict of nlm_ref.denoise, and comp_out, comp_var_out (lists), comp_sum_var_in, comp_sum_var_out (lists of floats)
    brute_force(...)       the same by a loop over pixels, offsets, patch taps, groups and channels, for small films
    synthetic_gradients(seed, passes, grad_scale)   the film of the quality test: truth and the means and variances of c, gx, gy
    reconstruct(c, gx, gy, alpha)                   natural-boundary least squares (round 0 of recon_l1_ref.irls)"""
import numpy as np

import nlm_guided_ref
import nlm_ref
from nlm_ref import box, film_sums, shifted


def valid_mask(img, var, comps, comp_vars, feat, fvar, groups):
    """HxW: valid for nlm_guided_ref, and every companion triple finite with finite variances >= 0."""
    ok = nlm_guided_ref.valid_mask(img, var, feat, fvar, list(groups))
    for a, s in zip(comps, comp_vars):
        ok = ok & nlm_ref.valid_mask(a, s)
    return ok


def _companion_sums(res, comp_vars, comp_var_out, ok):
    res["comp_sum_var_in"] = [float(s[ok].sum()) for s in comp_vars]
    res["comp_sum_var_out"] = [float(s[ok].sum()) for s in comp_var_out]


def denoise(img, var, comps=(), comp_vars=(), feat=None, fvar=None, groups=(), k_f=0.6, alpha_f=1.0, r=10, f=3, k=0.45, alpha=1.0, eps=1e-10):
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    comps = [np.asarray(a, dtype=np.float64) for a in comps]
    comp_vars = [np.asarray(s, dtype=np.float64) for s in comp_vars]
    groups = list(groups)
    if groups:
        feat, fvar = np.asarray(feat, dtype=np.float64), np.asarray(fvar, dtype=np.float64)
    ok = valid_mask(img, var, comps, comp_vars, feat, fvar, groups)
    ok3 = ok[:, :, None]
    u, v = np.where(ok3, img, 0.0), np.where(ok3, var, 0.0)
    ca, csv = [np.where(ok3, a, 0.0) for a in comps], [np.where(ok3, s, 0.0) for s in comp_vars]
    if groups:
        g, s = np.where(ok[None], feat, 0.0), np.where(ok[None], fvar, 0.0)
    num, vnum, wsum = np.zeros_like(u), np.zeros_like(u), np.zeros(ok.shape)
    cnum, cvnum = [np.zeros_like(u) for _ in comps], [np.zeros_like(u) for _ in comps]
    k2 = k * k
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            ub, vb, okb = shifted(u, oy, ox, 0.0), shifted(v, oy, ox, 0.0), shifted(ok, oy, ox, False)
            both = ok & okb
            with np.errstate(all="ignore"):
                d = u - ub
                t = (d * d - alpha * (v + np.minimum(vb, v))) / (eps + k2 * (v + vb))
                e = np.where(both, ((t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]) / 3.0, 0.0)
                S, C = box(e, f), box(both.astype(np.int64), f)
                D = S / np.maximum(C, 1)
                D = np.where(D > 0, D, 0.0)
                if groups:
                    gb = np.stack([shifted(p, oy, ox, 0.0) for p in g])
                    sb = np.stack([shifted(p, oy, ox, 0.0) for p in s])
                    D = np.fmax(D, nlm_guided_ref.feature_distance(g, s, gb, sb, groups, k_f, alpha_f))
                wgt = np.where(both, np.exp(-D), 0.0)
            wsum += wgt
            num += wgt[:, :, None] * ub
            vnum += (wgt * wgt)[:, :, None] * vb
            for j in range(len(comps)):
                cnum[j] += wgt[:, :, None] * shifted(ca[j], oy, ox, 0.0)
                cvnum[j] += (wgt * wgt)[:, :, None] * shifted(csv[j], oy, ox, 0.0)
    with np.errstate(all="ignore"):
        out = np.where(ok3, num / wsum[:, :, None], img)
        var_out = np.where(ok3, vnum / (wsum * wsum)[:, :, None], var)
        comp_out = [np.where(ok3, cnum[j] / wsum[:, :, None], comps[j]) for j in range(len(comps))]
        comp_var_out = [np.where(ok3, cvnum[j] / (wsum * wsum)[:, :, None], comp_vars[j]) for j in range(len(comps))]
    res = dict(out=out, var_out=var_out, comp_out=comp_out, comp_var_out=comp_var_out)
    res.update(film_sums(img, var, out, var_out, ok))
    _companion_sums(res, comp_vars, comp_var_out, ok)
    return res


def brute_force(img, var, comps=(), comp_vars=(), feat=None, fvar=None, groups=(), k_f=0.6, alpha_f=1.0, r=10, f=3, k=0.45, alpha=1.0, eps=1e-10):
    """The definition read literally, pixel by pixel, offset by offset, tap by tap."""
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    comps = [np.asarray(a, dtype=np.float64) for a in comps]
    comp_vars = [np.asarray(s, dtype=np.float64) for s in comp_vars]
    groups = list(groups)
    n = len(comps)
    h, w = img.shape[:2]
    ok = valid_mask(img, var, comps, comp_vars, feat, fvar, groups)
    out, var_out = img.copy(), var.copy()
    comp_out, comp_var_out = [a.copy() for a in comps], [s.copy() for s in comp_vars]
    inside = lambda x, y: 0 <= x < w and 0 <= y < h      # noqa: E731
    for y in range(h):
        for x in range(w):
            if not ok[y, x]:
                continue
            num, vnum, wsum = np.zeros(3), np.zeros(3), 0.0
            cnum, cvnum = np.zeros((n, 3)), np.zeros((n, 3))
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
                    wsum += wgt
                    num += wgt * img[qy, qx]
                    vnum += wgt * wgt * var[qy, qx]
                    for j in range(n):
                        cnum[j] += wgt * comps[j][qy, qx]
                        cvnum[j] += wgt * wgt * comp_vars[j][qy, qx]
            out[y, x] = num / wsum
            var_out[y, x] = vnum / (wsum * wsum)
            for j in range(n):
                comp_out[j][y, x] = cnum[j] / wsum
                comp_var_out[j][y, x] = cvnum[j] / (wsum * wsum)
    res = dict(out=out, var_out=var_out, comp_out=comp_out, comp_var_out=comp_var_out)
    res.update(film_sums(img, var, out, var_out, ok))
    _companion_sums(res, comp_vars, comp_var_out, ok)
    return res


def true_gradients(truth):
    """Backward differences: gx(x, y) = t(x, y) - t(x - 1, y), 0 at x = 0; gy likewise in y."""
    gx, gy = np.zeros_like(truth), np.zeros_like(truth)
    gx[:, 1:] = truth[:, 1:] - truth[:, :-1]
    gy[1:] = truth[1:] - truth[:-1]
    return gx, gy


def box_mean(a, radius):
    """The mean over the (2 radius + 1)^2 window clipped to the film."""
    return box(a, radius) / box(np.ones(a.shape[:2]), radius)[:, :, None]


def synthetic_gradients(seed, passes, grad_scale):
    """nlm_ref's 48 x 40 film as a gradient-domain render of `passes` passes from default_rng(seed); per pass, in this order, a primal
    truth + 0.25 sqrt(truth) N(0,1), then gx and gy: the true backward differences + grad_scale 0.25 sqrt(truth) N(0,1).
    Returns (truth, (true gx, true gy), means (c, gx, gy), variances of those means); every variance is the sample variance of the
    passes / passes, the primal's box-averaged at radius 2."""
    truth = nlm_ref.synthetic_truth()
    tgx, tgy = true_gradients(truth)
    sigma = 0.25 * np.sqrt(truth)
    rng = np.random.default_rng(seed)
    cs, gxs, gys = [], [], []
    for _ in range(passes):
        cs.append(truth + sigma * rng.standard_normal(truth.shape))
        gxs.append(tgx + grad_scale * sigma * rng.standard_normal(truth.shape))
        gys.append(tgy + grad_scale * sigma * rng.standard_normal(truth.shape))
    means = tuple(np.stack(a).mean(axis=0) for a in (cs, gxs, gys))
    variances = [np.stack(a).var(axis=0, ddof=1) / passes for a in (cs, gxs, gys)]
    variances[0] = box_mean(variances[0], 2)
    return truth, (tgx, tgy), means, tuple(variances)


def reconstruct(c, gx, gy, alpha):
    """Natural-boundary least squares: round 0 of recon_l1_ref.irls."""
    import recon_l1_ref
    return recon_l1_ref.irls(c, gx, gy, alpha, 0)[0]


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))
