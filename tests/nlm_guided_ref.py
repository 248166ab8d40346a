"""numpy restatement of the feature-guided non-local-means filter of include/gdpt.h (gdpt_denoise_nlm_guided*), on the helpers of
tests/nlm_ref.py: that definition with a feature distance of the pixel pair capping the colour weight. Not collected by pytest;
tests/test_nlm_guided_ref.py pins it, tests/test_gpu_nlm_guided.py holds the kernels against it.

    denoise(img, var, feat, fvar, groups, k_f, alpha_f, r, f, k, alpha, eps)  -> the dict of nlm_ref.denoise
    brute_force(...)       the same by a loop over pixels, offsets, patch taps, groups and channels, for small films
    feat, fvar: (channels, H, W) planes; groups: a list of (first_channel, num_channels, tau)
    synthetic_textured(seed)   the film of the quality test: nlm_ref's film under a 15 % albedo checker, with a three-channel albedo"""
import numpy as np

import nlm_ref
from nlm_ref import box, film_sums, shifted

GUIDE_DEFAULTS = dict(k_f=0.6, alpha_f=1.0)


def used_channels(groups):
    return sorted({c for first, count, _ in groups for c in range(first, first + count)})


def valid_mask(img, var, feat, fvar, groups):
    """HxW: valid for nlm_ref, and every channel some group names is finite there with variance >= 0."""
    ok = nlm_ref.valid_mask(img, var)
    for c in used_channels(groups):
        with np.errstate(invalid="ignore"):
            ok = ok & np.isfinite(feat[c]) & np.isfinite(fvar[c]) & (fvar[c] >= 0)
    return ok


def feature_distance(g, s, gb, sb, groups, k_f, alpha_f):
    """D^f of every pixel against its partner (planes g, s against gb, sb): max(0, max_j phi_j)."""
    Df = np.zeros(g.shape[1:])
    kf2 = k_f * k_f
    for first, count, tau in groups:
        phi = np.zeros(g.shape[1:])
        for c in range(first, first + count):
            d = g[c] - gb[c]
            phi = phi + (d * d - alpha_f * (s[c] + np.minimum(sb[c], s[c]))) / (kf2 * np.maximum(tau, s[c] + sb[c]))
        Df = np.fmax(Df, phi / float(count))
    return Df


def denoise(img, var, feat, fvar, groups=(), k_f=0.6, alpha_f=1.0, r=10, f=3, k=0.45, alpha=1.0, eps=1e-10):
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    groups = list(groups)
    if groups:
        feat, fvar = np.asarray(feat, dtype=np.float64), np.asarray(fvar, dtype=np.float64)
    ok = valid_mask(img, var, feat, fvar, groups)
    ok3 = ok[:, :, None]
    u, v = np.where(ok3, img, 0.0), np.where(ok3, var, 0.0)
    if groups:
        g, s = np.where(ok[None], feat, 0.0), np.where(ok[None], fvar, 0.0)
    num, vnum, wsum = np.zeros_like(u), np.zeros_like(u), np.zeros(ok.shape)
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
                    D = np.fmax(D, feature_distance(g, s, gb, sb, groups, k_f, alpha_f))
                wgt = np.where(both, np.exp(-D), 0.0)
            wsum += wgt
            num += wgt[:, :, None] * ub
            vnum += (wgt * wgt)[:, :, None] * vb
    with np.errstate(all="ignore"):
        out = np.where(ok3, num / wsum[:, :, None], img)
        var_out = np.where(ok3, vnum / (wsum * wsum)[:, :, None], var)
    res = dict(out=out, var_out=var_out)
    res.update(film_sums(img, var, out, var_out, ok))
    return res


def brute_force(img, var, feat, fvar, groups=(), k_f=0.6, alpha_f=1.0, r=10, f=3, k=0.45, alpha=1.0, eps=1e-10):
    """The definition read literally, pixel by pixel."""
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    groups = list(groups)
    h, w = img.shape[:2]
    ok = valid_mask(img, var, feat, fvar, groups)
    out, var_out = img.copy(), var.copy()
    inside = lambda x, y: 0 <= x < w and 0 <= y < h      # noqa: E731
    for y in range(h):
        for x in range(w):
            if not ok[y, x]:
                continue
            num, vnum, wsum = np.zeros(3), np.zeros(3), 0.0
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
            out[y, x] = num / wsum
            var_out[y, x] = vnum / (wsum * wsum)
    res = dict(out=out, var_out=var_out)
    res.update(film_sums(img, var, out, var_out, ok))
    return res


def checker():
    y, x = np.mgrid[0:nlm_ref.H_SYN, 0:nlm_ref.W_SYN]
    return (((x // 3) + (y // 3)) % 2).astype(np.float64)


def synthetic_textured(seed):
    """(truth, mean, variance of the mean, albedo mean (3, H, W), variance of it): nlm_ref's film times 1 + 0.15 (chk - 0.5), four
    noisy passes as there; the albedo is three region colours times the same factor, four samples with N(0, 0.01^2) noise."""
    fac = 1.0 + 0.15 * (checker() - 0.5)
    truth = nlm_ref.synthetic_truth() * fac[..., None]
    rng = np.random.default_rng(seed)
    passes = np.stack([truth + 0.25 * np.sqrt(truth) * rng.standard_normal(truth.shape) for _ in range(nlm_ref.PASSES_SYN)])
    y, x = np.mgrid[0:nlm_ref.H_SYN, 0:nlm_ref.W_SYN].astype(np.float64)
    colour = np.where((x < 24)[..., None], np.array([0.7, 0.2, 0.2]), np.array([0.2, 0.7, 0.2]))
    colour = np.where((((x - 26.0) ** 2 + (y - 14.0) ** 2) < 49.0)[..., None], np.array([0.05, 0.05, 0.05]), colour)
    albedo = np.moveaxis(colour * fac[..., None], 2, 0)
    frng = np.random.default_rng(100 + seed)
    fs = np.stack([albedo + 0.01 * frng.standard_normal(albedo.shape) for _ in range(4)])
    return truth, passes.mean(axis=0), passes.var(axis=0, ddof=1) / nlm_ref.PASSES_SYN, fs.mean(axis=0), fs.var(axis=0, ddof=1) / 4
