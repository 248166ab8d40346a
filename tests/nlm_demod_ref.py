"""numpy restatement of the albedo-demodulated non-local-means filter of include/gdpt.h (gdpt_denoise_nlm_demod*), on the two
restatements before it: tests/nlm_ref.py (no guide) or tests/nlm_guided_ref.py (a guide) run on the mean divided by the effective
albedo, and the albedo multiplied back. Not collected by pytest; tests/test_nlm_demod_ref.py pins it, tests/test_gpu_nlm_demod.py
holds the kernels against it.

    denoise(img, var, feat, fvar, albedo_channel, coverage_channel, floor, groups, k_f, alpha_f, r, f, k, alpha, eps)
                           -> the dict of nlm_ref.denoise; groups = None: no feature term (nlm_ref), a list: nlm_guided_ref
    brute_force(...)       the same pixel by pixel through the brute forces of the two restatements, for small films
    effective_albedo(feat, albedo_channel, coverage_channel, floor)   HxWx3: max(floor, a_c + (1 - cov))
    valid_mask(...)        HxW
    feat, fvar: (channels, H, W) planes; coverage_channel = -1: none (cov = 1)"""
import numpy as np

import nlm_guided_ref
import nlm_ref

DEMOD_DEFAULTS = dict(albedo_channel=0, coverage_channel=7, floor=1e-3)


def effective_albedo(feat, albedo_channel=0, coverage_channel=-1, floor=1e-3):
    a = np.moveaxis(np.asarray(feat, dtype=np.float64)[albedo_channel:albedo_channel + 3], 0, 2)
    with np.errstate(invalid="ignore"):
        if coverage_channel >= 0:
            a = a + (1.0 - np.asarray(feat, dtype=np.float64)[coverage_channel])[:, :, None]
        return np.maximum(floor, a)


def valid_mask(img, var, feat, fvar, albedo_channel=0, coverage_channel=-1, groups=None):
    """HxW: valid for the filter underneath, the albedo triple finite with variances finite and >= 0, and so the coverage if used."""
    ok = nlm_ref.valid_mask(img, var) if groups is None else nlm_guided_ref.valid_mask(img, var, feat, fvar, list(groups))
    named = list(range(albedo_channel, albedo_channel + 3)) + ([coverage_channel] if coverage_channel >= 0 else [])
    for c in named:
        with np.errstate(invalid="ignore"):
            ok = ok & np.isfinite(feat[c]) & np.isfinite(fvar[c]) & (fvar[c] >= 0)
    return ok


def _through(inner, img, var, feat, fvar, albedo_channel, coverage_channel, floor, groups, k_f, alpha_f, r, f, k, alpha, eps):
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    feat, fvar = np.asarray(feat, dtype=np.float64), np.asarray(fvar, dtype=np.float64)
    ok = valid_mask(img, var, feat, fvar, albedo_channel, coverage_channel, groups)
    ok3 = ok[:, :, None]
    al = effective_albedo(feat, albedo_channel, coverage_channel, floor)
    with np.errstate(all="ignore"):
        # an invalid pixel goes in as NaN: it is invalid for the filter underneath too, whatever made it invalid here
        ud = np.where(ok3, img / al, np.nan)
        vd = np.where(ok3, var / (al * al), np.nan)
    if groups is None:
        res = inner[0](ud, vd, r=r, f=f, k=k, alpha=alpha, eps=eps)
    else:
        res = inner[1](ud, vd, feat, fvar, groups=list(groups), k_f=k_f, alpha_f=alpha_f, r=r, f=f, k=k, alpha=alpha, eps=eps)
    with np.errstate(all="ignore"):
        out = np.where(ok3, res["out"] * al, img)
        var_out = np.where(ok3, res["var_out"] * (al * al), var)
    d = dict(out=out, var_out=var_out)
    d.update(nlm_ref.film_sums(img, var, out, var_out, ok))      # the colour domain: the original u, v and the remodulated outputs
    return d


def denoise(img, var, feat, fvar, albedo_channel=0, coverage_channel=-1, floor=1e-3, groups=None, k_f=0.6, alpha_f=1.0, r=10, f=3, k=0.45,
            alpha=1.0, eps=1e-10):
    return _through((nlm_ref.denoise, nlm_guided_ref.denoise), img, var, feat, fvar, albedo_channel, coverage_channel, floor, groups, k_f, alpha_f,
                    r, f, k, alpha, eps)


def brute_force(img, var, feat, fvar, albedo_channel=0, coverage_channel=-1, floor=1e-3, groups=None, k_f=0.6, alpha_f=1.0, r=10, f=3, k=0.45,
                alpha=1.0, eps=1e-10):
    """A literal per-pixel reading: validity, division and multiplication pixel by pixel here, the filter between them by the
    per-pixel loops of the restatement underneath."""
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    feat, fvar = np.asarray(feat, dtype=np.float64), np.asarray(fvar, dtype=np.float64)
    h, w = img.shape[:2]
    ok = np.zeros((h, w), dtype=bool)
    al = np.ones((h, w, 3))
    ud, vd = np.full(img.shape, np.nan), np.full(img.shape, np.nan)
    fin = lambda x: bool(np.isfinite(x))      # noqa: E731
    used = sorted({c for first, count, _ in (groups or ()) for c in range(first, first + count)})
    for y in range(h):
        for x in range(w):
            good = all(fin(img[y, x, c]) and fin(var[y, x, c]) and var[y, x, c] >= 0 for c in range(3))
            good = good and all(fin(feat[c, y, x]) and fin(fvar[c, y, x]) and fvar[c, y, x] >= 0 for c in used)
            good = good and all(fin(feat[albedo_channel + c, y, x]) and fin(fvar[albedo_channel + c, y, x]) and fvar[albedo_channel + c, y, x] >= 0
                                for c in range(3))
            cov = 1.0
            if coverage_channel >= 0:
                cov = feat[coverage_channel, y, x]
                good = good and fin(cov) and fin(fvar[coverage_channel, y, x]) and fvar[coverage_channel, y, x] >= 0
            ok[y, x] = good
            if not good:
                continue
            for c in range(3):
                al[y, x, c] = max(floor, feat[albedo_channel + c, y, x] + (1.0 - cov))
                ud[y, x, c] = img[y, x, c] / al[y, x, c]
                vd[y, x, c] = var[y, x, c] / (al[y, x, c] * al[y, x, c])
    if groups is None:
        res = nlm_ref.brute_force(ud, vd, r=r, f=f, k=k, alpha=alpha, eps=eps)
    else:
        res = nlm_guided_ref.brute_force(ud, vd, feat, fvar, groups=list(groups), k_f=k_f, alpha_f=alpha_f, r=r, f=f, k=k, alpha=alpha, eps=eps)
    out, var_out = img.copy(), var.copy()
    for y in range(h):
        for x in range(w):
            if ok[y, x]:
                for c in range(3):
                    out[y, x, c] = res["out"][y, x, c] * al[y, x, c]
                    var_out[y, x, c] = res["var_out"][y, x, c] * (al[y, x, c] * al[y, x, c])
    d = dict(out=out, var_out=var_out)
    d.update(nlm_ref.film_sums(img, var, out, var_out, ok))
    return d
