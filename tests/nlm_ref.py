"""numpy restatement of the non-local-means filter of include/gdpt.h (gdpt_denoise_nlm*): the definition there, offset by offset
with whole-film array operations. Not collected by pytest; tests/test_nlm_ref.py pins it, tests/test_gpu_nlm.py holds the kernels
against it.

    denoise(img, var, r, f, k, alpha, eps) -> dict(out, var_out, left_out, sum_var_in, sum_sq_in, sum_var_out, sum_sq_out,
                                                   error_in, error_out)
    brute_force(...)    the same by a double loop over pixels, offsets and patch taps (not separable), for small films
    synthetic(seed)     the 48 x 40 test film: truth, the mean of four noisy passes, the variance of that mean"""
import numpy as np

DEFAULTS = dict(r=10, f=3, k=0.45, alpha=1.0, eps=1e-10)


def valid_mask(img, var):
    """HxW: the pixel's three img and three var values are finite and the var values >= 0."""
    fin = np.isfinite(img).all(axis=2) & np.isfinite(var).all(axis=2)
    with np.errstate(invalid="ignore"):
        return fin & (var >= 0).all(axis=2)


def shifted(a, oy, ox, fill):
    """b[y, x] = a[y + oy, x + ox] where that lies in the film, `fill` elsewhere."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, xs = slice(max(0, -oy), min(h, h - oy)), slice(max(0, -ox), min(w, w - ox))
    yd, xd = slice(max(0, -oy) + oy, min(h, h - oy) + oy), slice(max(0, -ox) + ox, min(w, w - ox) + ox)
    if ys.start < ys.stop and xs.start < xs.stop:
        b[ys, xs] = a[yd, xd]
    return b


def box(a, f):
    """Sums over the (2f+1)^2 window clipped to the film: row sums of 2f + 1 taps, then column sums of the row sums."""
    rows = np.zeros_like(a)
    for n in range(-f, f + 1):
        rows = rows + shifted(a, 0, n, 0)
    out = np.zeros_like(a)
    for n in range(-f, f + 1):
        out = out + shifted(rows, n, 0, 0)
    return out


def film_sums(img, var, out, var_out, ok):
    d = dict(left_out=int((~ok).sum()))
    for name, a in (("sum_var_in", var), ("sum_sq_in", img * img), ("sum_var_out", var_out), ("sum_sq_out", out * out)):
        d[name] = float(a[ok].sum())
    with np.errstate(all="ignore"):
        d["error_in"] = float(np.sqrt(np.float64(d["sum_var_in"]) / np.float64(d["sum_sq_in"])))
        d["error_out"] = float(np.sqrt(np.float64(d["sum_var_out"]) / np.float64(d["sum_sq_out"])))
    return d


def denoise(img, var, r=10, f=3, k=0.45, alpha=1.0, eps=1e-10):
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    ok = valid_mask(img, var)
    ok3 = ok[:, :, None]
    u, v = np.where(ok3, img, 0.0), np.where(ok3, var, 0.0)
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


def brute_force(img, var, r=10, f=3, k=0.45, alpha=1.0, eps=1e-10):
    """The definition read literally, pixel by pixel; every patch distance is summed tap by tap where it is used."""
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    h, w = img.shape[:2]
    ok = valid_mask(img, var)
    out, var_out = img.copy(), var.copy()
    inside = lambda x, y: 0 <= x < w and 0 <= y < h      # noqa: E731
    for y in range(h):
        for x in range(w):
            if not ok[y, x]:
                continue
            num, vnum, wsum = np.zeros(3), np.zeros(3), 0.0
            for oy in range(-r, r + 1):
                for ox in range(-r, r + 1):
                    if not inside(x + ox, y + oy) or not ok[y + oy, x + ox]:
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
                    wgt = float(np.exp(-max(0.0, S / C)))
                    wsum += wgt
                    num += wgt * img[y + oy, x + ox]
                    vnum += wgt * wgt * var[y + oy, x + ox]
            out[y, x] = num / wsum
            var_out[y, x] = vnum / (wsum * wsum)
    res = dict(out=out, var_out=var_out)
    res.update(film_sums(img, var, out, var_out, ok))
    return res


W_SYN, H_SYN, PASSES_SYN = 48, 40, 4


def synthetic_truth():
    """48 x 40: a step edge (left / right halves), a vertical ramp on the left, a sinusoid on the right, a dark disc across the edge."""
    y, x = np.mgrid[0:H_SYN, 0:W_SYN].astype(np.float64)
    left = 0.25 + 0.5 * y / (H_SYN - 1)
    right = 1.0 + 0.3 * np.sin(2.0 * np.pi * x / 12.0)
    lum = np.where(x < W_SYN // 2, left, right)
    lum = np.where((x - 26.0) ** 2 + (y - 14.0) ** 2 < 7.0 ** 2, 0.05, lum)
    return lum[:, :, None] * np.array([1.0, 0.8, 0.6])


def synthetic(seed):
    """(truth, mean of four passes with noise 0.25 sqrt(truth), variance of that mean = sample variance of the four / 4)"""
    truth = synthetic_truth()
    rng = np.random.default_rng(seed)
    passes = np.stack([truth + 0.25 * np.sqrt(truth) * rng.standard_normal(truth.shape) for _ in range(PASSES_SYN)])
    return truth, passes.mean(axis=0), passes.var(axis=0, ddof=1) / PASSES_SYN
