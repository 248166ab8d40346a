"""numpy restatement of the variance smoothing of include/gdpt.h (gdpt_variance_smooth*), on the helpers of tests/nlm_ref.py
(shifted, box) and tests/nlm_demod_ref.py (effective_albedo): the box mean, over the valid pixels of a (2s+1)^2 window, of the
variance of a mean, taken in the albedo-normalised domain when a demod block is given. Not collected by pytest;
tests/test_var_smooth_ref.py pins it, tests/test_gpu_var_smooth.py holds the kernel against it.

    smooth(img, var, radius, feat, fvar, albedo_channel, coverage_channel, floor)
                           -> dict(var_out, left_out, sum_var_in, sum_var_out); feat = None: no demod block (a~ = 1)
    brute_force(...)       the same pixel by pixel, tap by tap, for small films
    valid_mask(...)        HxW
    synthetic_passes(seed, passes)       nlm_ref.synthetic's recipe at a pass count (passes = 4: synthetic(seed) itself)
    synthetic_textured_strong(seed, passes)   nlm_ref's film under the checker of nlm_guided_ref at amplitude 1.2, a noise-free albedo
    feat, fvar: (channels, H, W) planes; coverage_channel = -1: none (cov = 1)"""
import numpy as np

import nlm_demod_ref
import nlm_guided_ref
import nlm_ref
from nlm_ref import box

MAX_RADIUS = 4
DEFAULT_RADIUS = 2


def valid_mask(img, var, feat=None, fvar=None, albedo_channel=0, coverage_channel=-1):
    """HxW: valid for nlm_ref; with planes also valid as the demodulated filter asks without a guide."""
    if feat is None:
        return nlm_ref.valid_mask(img, var)
    return nlm_demod_ref.valid_mask(img, var, feat, fvar, albedo_channel, coverage_channel, None)


def sums(var, var_out, ok):
    return dict(left_out=int((~ok).sum()), sum_var_in=float(var[ok].sum()), sum_var_out=float(var_out[ok].sum()))


def smooth(img, var, radius=DEFAULT_RADIUS, feat=None, fvar=None, albedo_channel=0, coverage_channel=-1, floor=1e-3):
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    ok = valid_mask(img, var, feat, fvar, albedo_channel, coverage_channel)
    ok3 = ok[:, :, None]
    with np.errstate(all="ignore"):
        if feat is None:
            n = np.where(ok3, var, 0.0)
        else:
            al = nlm_demod_ref.effective_albedo(feat, albedo_channel, coverage_channel, floor)
            al2 = al * al
            n = np.where(ok3, var / al2, 0.0)
        S, C = box(n, radius), box(ok.astype(np.int64), radius)
        mean = S / np.maximum(C, 1)[:, :, None]
        var_out = np.where(ok3, mean if feat is None else mean * al2, var)
    d = dict(var_out=var_out)
    d.update(sums(var, var_out, ok))
    return d


def brute_force(img, var, radius=DEFAULT_RADIUS, feat=None, fvar=None, albedo_channel=0, coverage_channel=-1, floor=1e-3):
    """The definition read literally, pixel by pixel: validity and a~ per pixel, the window tap by tap in row-major order (not
    separable: the last places may differ from smooth())."""
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    h, w = img.shape[:2]
    fin = lambda x: bool(np.isfinite(x))      # noqa: E731
    ok = np.zeros((h, w), dtype=bool)
    al2 = np.ones((h, w, 3))
    for y in range(h):
        for x in range(w):
            good = all(fin(img[y, x, c]) and fin(var[y, x, c]) and var[y, x, c] >= 0 for c in range(3))
            if feat is not None:
                named = [albedo_channel + c for c in range(3)] + ([coverage_channel] if coverage_channel >= 0 else [])
                good = good and all(fin(feat[c, y, x]) and fin(fvar[c, y, x]) and fvar[c, y, x] >= 0 for c in named)
                if good:
                    cov = feat[coverage_channel, y, x] if coverage_channel >= 0 else 1.0
                    for c in range(3):
                        a = max(floor, feat[albedo_channel + c, y, x] + (1.0 - cov))
                        al2[y, x, c] = a * a
            ok[y, x] = good
    var_out = var.copy()
    for y in range(h):
        for x in range(w):
            if not ok[y, x]:
                continue
            S, C = np.zeros(3), 0
            for qy in range(max(0, y - radius), min(h, y + radius + 1)):
                for qx in range(max(0, x - radius), min(w, x + radius + 1)):
                    if ok[qy, qx]:
                        S += var[qy, qx] / al2[qy, qx] if feat is not None else var[qy, qx]
                        C += 1
            var_out[y, x] = (S / C) * al2[y, x] if feat is not None else S / C
    d = dict(var_out=var_out)
    d.update(sums(var, var_out, ok))
    return d


def _passes(truth, sigma, seed, passes):
    rng = np.random.default_rng(seed)
    p = np.stack([truth + sigma * rng.standard_normal(truth.shape) for _ in range(passes)])
    return p.mean(axis=0), p.var(axis=0, ddof=1) / passes


def synthetic_passes(seed, passes=nlm_ref.PASSES_SYN):
    """(truth, mean of `passes` passes with noise 0.25 sqrt(truth), variance of that mean): nlm_ref.synthetic(seed) at passes = 4."""
    truth = nlm_ref.synthetic_truth()
    mean, var = _passes(truth, 0.25 * np.sqrt(truth), seed, passes)
    return truth, mean, var


def synthetic_textured_strong(seed, passes=2, amplitude=1.2):
    """(truth, mean, variance of the mean, feat (3, H, W), fvar): nlm_ref's film times fac = 1 + amplitude (checker - 0.5), noise
    0.25 sqrt(synthetic_truth) fac; the three planes hold the noise-free albedo, a colour per half of the film times fac, with
    variance 0; no coverage plane."""
    fac = 1.0 + amplitude * (nlm_guided_ref.checker() - 0.5)
    base = nlm_ref.synthetic_truth()
    truth = base * fac[..., None]
    mean, var = _passes(truth, 0.25 * np.sqrt(base) * fac[..., None], seed, passes)
    x = np.mgrid[0:nlm_ref.H_SYN, 0:nlm_ref.W_SYN][1]
    colour = np.where((x < nlm_ref.W_SYN // 2)[..., None], np.array([0.7, 0.2, 0.2]), np.array([0.2, 0.7, 0.2]))
    feat = np.moveaxis(colour * fac[..., None], 2, 0)
    return truth, mean, var, feat, np.zeros_like(feat)
