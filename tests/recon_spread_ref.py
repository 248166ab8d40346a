"""numpy restatement of the spread of N weighted images (include/gdpt.h: gdpt_recon_spread*; csrc/hip/recon_spread.hip): West's
weighted update in member order, the left-out rule of the film sums, and the clipped window mean with finite counts. Element-wise
and in the kernel's order of operations, so the GPU differs from it by FMA contraction alone. Not collected by pytest."""
import numpy as np


def spread(images, weights):
    """(mean, var) per component: W += W_i; d = f_i - mean; mean += (W_i / W) d; M2 += W_i d (f_i - mean_new); var = M2 / ((N-1) W)."""
    assert len(images) == len(weights) and len(images) >= 2
    mean = np.zeros_like(np.asarray(images[0], dtype=np.float64))
    m2 = np.zeros_like(mean)
    W = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for f, w in zip(images, weights):
            f, w = np.asarray(f, dtype=np.float64), float(w)
            W += w
            d = f - mean
            mean = mean + (w / W) * d
            m2 = m2 + w * d * (f - mean)
        var = m2 / (float(len(images) - 1) * W)
    return mean, var


def two_pass(images, weights):
    """The definition, not the update: fbar = sum W_i f_i / W, var = sum W_i (f_i - fbar)^2 / ((N-1) W)."""
    w = np.asarray(weights, dtype=np.float64)
    f = np.stack([np.asarray(x, dtype=np.float64) for x in images])
    W = w.sum()
    fbar = np.tensordot(w, f, axes=1) / W
    m2 = np.tensordot(w, (f - fbar) ** 2, axes=1)
    return fbar, m2 / ((len(w) - 1) * W)


def kept(images, total, var):
    """HxW mask of the pixels that enter the film sums: every member's triple, the total's triple and the var triple finite."""
    ok = np.isfinite(total).all(axis=-1) & np.isfinite(var).all(axis=-1)
    for f in images:
        ok &= np.isfinite(np.asarray(f)).all(axis=-1)
    return ok


def pixel_sum(var):
    """The raw error map: (v0 + v1) + v2 per pixel."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (var[..., 0] + var[..., 1]) + var[..., 2]


def estimate(images, weights, total=None):
    """dict: var, map (raw), sum_var, sum_sq, left_out, error. `total` None: the weighted mean."""
    mean, var = spread(images, weights)
    t = mean if total is None else np.asarray(total, dtype=np.float64)
    ok = kept(images, t, var)
    raw = pixel_sum(var)
    with np.errstate(invalid="ignore", over="ignore"):
        sq = (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]
    sum_var, sum_sq = float(raw[ok].sum()), float(sq[ok].sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        err = float(np.sqrt(np.float64(sum_var) / np.float64(sum_sq)))
    return dict(mean=mean, var=var, map=raw, sum_var=sum_var, sum_sq=sum_sq, left_out=int((~ok).sum()), error=err)


def window_mean(plane, r):
    """Mean of the finite entries of `plane` (HxW) in the (2r+1)^2 window clipped to the film, NaN where there is none; r = 0: the
    plane itself. Separable as box_kernel: row sums over x - r .. x + r in ascending x, then column sums of those in ascending y;
    entries outside the film or not finite count as 0 with count 0."""
    plane = np.asarray(plane, dtype=np.float64)
    if r == 0:
        return plane.copy()
    h, w = plane.shape
    fin = np.isfinite(plane)
    val = np.zeros((h + 2 * r, w + 2 * r))
    cnt = np.zeros((h + 2 * r, w + 2 * r), dtype=np.int64)
    val[r:r + h, r:r + w] = np.where(fin, plane, 0.0)
    cnt[r:r + h, r:r + w] = fin
    hv, hc = np.zeros((h + 2 * r, w)), np.zeros((h + 2 * r, w), dtype=np.int64)
    for k in range(2 * r + 1):
        hv = hv + val[:, k:k + w]
        hc = hc + cnt[:, k:k + w]
    s, c = np.zeros((h, w)), np.zeros((h, w), dtype=np.int64)
    for k in range(2 * r + 1):
        s = s + hv[k:k + h, :]
        c = c + hc[k:k + h, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(c > 0, s / np.maximum(c, 1), np.nan)


def window_counts(plane, r):
    """The number of finite in-film entries of every pixel's window (what window_mean divides by)."""
    fin = np.isfinite(np.asarray(plane, dtype=np.float64))
    h, w = fin.shape
    pad = np.zeros((h + 2 * r, w + 2 * r), dtype=np.int64)
    pad[r:r + h, r:r + w] = fin
    c = np.zeros((h, w), dtype=np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            c += pad[dy:dy + h, dx:dx + w]
    return c
