"""numpy restatement of the edge-avoiding a-trous wavelet filter of include/gdpt.h (gdpt_denoise_atrous*), on the helpers of the
restatements before it: nlm_ref.shifted, nlm_guided_ref.feature_distance / valid_mask, nlm_demod_ref.effective_albedo / valid_mask.
Level by level, tap by tap, with whole-film array operations. Not collected by pytest; tests/test_atrous_ref.py pins it,
tests/test_gpu_atrous.py holds the kernels against it.

    denoise(img, var, feat, fvar, groups, demod, levels, first_level, k, alpha, eps, k_f, alpha_f)  -> the dict of nlm_ref.denoise
    brute_force(...)       the same by a loop over levels, pixels and taps, for small films
    feat, fvar: (channels, H, W) planes; groups: a list of (first_channel, num_channels, tau), empty: no feature term;
    demod: None, or (albedo_channel, coverage_channel, floor) with coverage_channel = -1 for none"""
import numpy as np

import nlm_demod_ref
import nlm_guided_ref
from nlm_ref import film_sums, shifted

DEFAULTS = dict(levels=5, first_level=0, k=2.0, alpha=1.0, eps=1e-10)
MAX_LEVELS = 6
SPLINE = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def valid_mask(img, var, feat, fvar, groups=(), demod=None):
    """HxW: valid for the guided filter on the groups' channels, and with a demod block the albedo and coverage values valid too."""
    if demod is None:
        return nlm_guided_ref.valid_mask(img, var, feat, fvar, list(groups))
    return nlm_demod_ref.valid_mask(img, var, feat, fvar, demod[0], demod[1], list(groups))


def denoise(img, var, feat=None, fvar=None, groups=(), demod=None, levels=5, first_level=0, k=2.0, alpha=1.0, eps=1e-10, k_f=0.6, alpha_f=1.0):
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    groups = list(groups)
    assert 1 <= levels and 0 <= first_level and first_level + levels <= MAX_LEVELS
    if groups or demod is not None:
        feat, fvar = np.asarray(feat, dtype=np.float64), np.asarray(fvar, dtype=np.float64)
    ok = valid_mask(img, var, feat, fvar, groups, demod)
    ok3 = ok[:, :, None]
    u, v = np.where(ok3, img, 0.0), np.where(ok3, var, 0.0)
    if demod is not None:
        al = np.where(ok3, nlm_demod_ref.effective_albedo(feat, *demod), 1.0)
        u, v = u / al, v / (al * al)
    if groups:
        g, s = np.where(ok[None], feat, 0.0), np.where(ok[None], fvar, 0.0)
    k2 = k * k
    for i in range(levels):
        step = 1 << (first_level + i)
        num, vnum, wsum = np.zeros_like(u), np.zeros_like(u), np.zeros(ok.shape)
        for a in range(-2, 3):
            for b in range(-2, 3):
                oy, ox = a * step, b * step
                ub, vb, okb = shifted(u, oy, ox, 0.0), shifted(v, oy, ox, 0.0), shifted(ok, oy, ox, False)
                both = ok & okb
                with np.errstate(all="ignore"):
                    d = u - ub
                    t = (d * d - alpha * (v + np.minimum(vb, v))) / (eps + k2 * (v + vb))
                    D = np.maximum(0.0, ((t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]) / 3.0)
                    if groups:
                        gb = np.stack([shifted(p, oy, ox, 0.0) for p in g])
                        sb = np.stack([shifted(p, oy, ox, 0.0) for p in s])
                        D = np.fmax(D, nlm_guided_ref.feature_distance(g, s, gb, sb, groups, k_f, alpha_f))
                    wgt = np.where(both, (SPLINE[a + 2] * SPLINE[b + 2]) * np.exp(-D), 0.0)
                wsum = wsum + wgt
                num = num + wgt[:, :, None] * ub
                vnum = vnum + (wgt * wgt)[:, :, None] * vb
        with np.errstate(all="ignore"):
            u = np.where(ok3, num / wsum[:, :, None], 0.0)
            v = np.where(ok3, vnum / (wsum * wsum)[:, :, None], 0.0)
    if demod is not None:
        u, v = u * al, v * (al * al)
    out, var_out = np.where(ok3, u, img), np.where(ok3, v, var)
    res = dict(out=out, var_out=var_out)
    res.update(film_sums(img, var, out, var_out, ok))
    return res


def brute_force(img, var, feat=None, fvar=None, groups=(), demod=None, levels=5, first_level=0, k=2.0, alpha=1.0, eps=1e-10, k_f=0.6,
                alpha_f=1.0):
    """The definition read literally: validity, division, every level and the multiplication pixel by pixel and tap by tap."""
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    groups = list(groups)
    h, w = img.shape[:2]
    fin = lambda x: bool(np.isfinite(x))      # noqa: E731
    named = sorted({c for first, count, _ in groups for c in range(first, first + count)})
    if demod is not None:
        named = named + list(range(demod[0], demod[0] + 3)) + ([demod[1]] if demod[1] >= 0 else [])
    ok = np.zeros((h, w), dtype=bool)
    al = np.ones((h, w, 3))
    u, v = np.zeros(img.shape), np.zeros(img.shape)
    for y in range(h):
        for x in range(w):
            good = all(fin(img[y, x, c]) and fin(var[y, x, c]) and var[y, x, c] >= 0 for c in range(3))
            good = good and all(fin(feat[c, y, x]) and fin(fvar[c, y, x]) and fvar[c, y, x] >= 0 for c in named)
            ok[y, x] = good
            if not good:
                continue
            if demod is not None:
                cov = feat[demod[1], y, x] if demod[1] >= 0 else 1.0
                for c in range(3):
                    al[y, x, c] = max(demod[2], feat[demod[0] + c, y, x] + (1.0 - cov))
            for c in range(3):
                u[y, x, c] = img[y, x, c] / al[y, x, c] if demod is not None else img[y, x, c]
                v[y, x, c] = var[y, x, c] / (al[y, x, c] * al[y, x, c]) if demod is not None else var[y, x, c]
    for i in range(levels):
        step = 1 << (first_level + i)
        un, vn = np.zeros_like(u), np.zeros_like(v)
        for y in range(h):
            for x in range(w):
                if not ok[y, x]:
                    continue
                num, vnum, wsum = np.zeros(3), np.zeros(3), 0.0
                for a in range(-2, 3):
                    for b in range(-2, 3):
                        qx, qy = x + b * step, y + a * step
                        if not (0 <= qx < w and 0 <= qy < h) or not ok[qy, qx]:
                            continue
                        ua, va, ub, vb = u[y, x], v[y, x], u[qy, qx], v[qy, qx]
                        t = ((ua - ub) ** 2 - alpha * (va + np.minimum(vb, va))) / (eps + k * k * (va + vb))
                        D = max(0.0, ((t[0] + t[1]) + t[2]) / 3.0)
                        Df = 0.0
                        for first, count, tau in groups:
                            phi = 0.0
                            for c in range(first, first + count):
                                gp, sp, gq, sq = feat[c, y, x], fvar[c, y, x], feat[c, qy, qx], fvar[c, qy, qx]
                                phi += ((gp - gq) ** 2 - alpha_f * (sp + min(sq, sp))) / (k_f * k_f * max(tau, sp + sq))
                            Df = max(Df, phi / count)
                        wgt = (SPLINE[a + 2] * SPLINE[b + 2]) * float(np.exp(-max(D, Df)))
                        wsum += wgt
                        num += wgt * ub
                        vnum += wgt * wgt * vb
                un[y, x] = num / wsum
                vn[y, x] = vnum / (wsum * wsum)
        u, v = un, vn
    out, var_out = img.copy(), var.copy()
    for y in range(h):
        for x in range(w):
            if ok[y, x]:
                for c in range(3):
                    out[y, x, c] = u[y, x, c] * al[y, x, c] if demod is not None else u[y, x, c]
                    var_out[y, x, c] = v[y, x, c] * (al[y, x, c] * al[y, x, c]) if demod is not None else v[y, x, c]
    res = dict(out=out, var_out=var_out)
    res.update(film_sums(img, var, out, var_out, ok))
    return res
