"""numpy restatement of the multi-scale (pyramid) form of the non-local-means filters of include/gdpt.h (gdpt_nlm_pyramid_down*,
gdpt_nlm_pyramid_up*, gdpt_denoise_nlm_multiscale*), on the three restatements before it: tests/nlm_ref.py (kind "plain"),
tests/nlm_guided_ref.py ("guided") and tests/nlm_demod_ref.py ("demod"). Not collected by pytest; tests/test_nlm_pyramid_ref.py pins
it, tests/test_gpu_nlm_pyramid.py holds the kernels against it.

    kind_args(kind, groups, albedo_channel, coverage_channel, floor, k_f, alpha_f)   the kind's blocks as one dict `ka`
    valid_mask(ka, img, var, feat, fvar)                HxW, as the kind's filter defines validity
    down(ka, img, var, feat, fvar)                      -> (img', var', feat', fvar', n): the next level and the valid count of a cell
    up(ka, img, var, feat, fvar, F, coarse_out)         -> out: F plus the interpolated correction; invalid pixels keep img's bits
    filter_level(ka, img, var, feat, fvar, **nlm)       the kind's single-scale restatement (the dict of nlm_ref.denoise)
    denoise(ka, img, var, feat, fvar, levels, **nlm)    -> dict(out, var_out, left_out, levels, extents, level=[the levels' dicts])
    brute_down(...), brute_up(...)                      the two operators by a per-pixel double loop, for small films
    truth(h, w), passes(truth, seed, k), low_frequency_rmse(a, b)    the film and the figures of the quality test
    feat, fvar: (channels, H, W) planes (None for "plain")"""
import numpy as np

import nlm_demod_ref
import nlm_guided_ref
import nlm_ref

MAX_LEVELS = 4
DEFAULT_LEVELS = 2
DEFAULT_GROUPS = [(0, 3, 1e-3), (3, 3, 1e-3)]
WEIGHTS = (0.5625, 0.1875, 0.1875, 0.0625)
ORDER = ((0, 0), (1, 0), (0, 1), (1, 1))      # (dx, dy): the order of every sum over a cell


def kind_args(kind, groups=None, albedo_channel=0, coverage_channel=7, floor=1e-3, k_f=0.6, alpha_f=1.0):
    """"plain": no block. "guided": groups None = the default guide's. "demod": groups None = no feature term."""
    if kind not in ("plain", "guided", "demod"):
        raise ValueError(kind)
    if kind == "guided" and groups is None:
        groups = DEFAULT_GROUPS
    return dict(kind=kind, groups=None if groups is None else list(groups), albedo_channel=albedo_channel, coverage_channel=coverage_channel,
                floor=floor, k_f=k_f, alpha_f=alpha_f)


def valid_mask(ka, img, var, feat=None, fvar=None):
    if ka["kind"] == "plain":
        return nlm_ref.valid_mask(img, var)
    if ka["kind"] == "guided":
        return nlm_guided_ref.valid_mask(img, var, feat, fvar, ka["groups"])
    return nlm_demod_ref.valid_mask(img, var, feat, fvar, ka["albedo_channel"], ka["coverage_channel"], ka["groups"])


def filter_level(ka, img, var, feat=None, fvar=None, **nlm):
    if ka["kind"] == "plain":
        return nlm_ref.denoise(img, var, **nlm)
    if ka["kind"] == "guided":
        return nlm_guided_ref.denoise(img, var, feat, fvar, groups=ka["groups"], k_f=ka["k_f"], alpha_f=ka["alpha_f"], **nlm)
    return nlm_demod_ref.denoise(img, var, feat, fvar, ka["albedo_channel"], ka["coverage_channel"], ka["floor"], ka["groups"], ka["k_f"],
                                 ka["alpha_f"], **nlm)


def coarse_extent(h, w):
    return (h + 1) // 2, (w + 1) // 2


def cell_sums(ok, a):
    """a: HxWxC. The sums over the valid pixels of every 2 x 2 cell, from 0.0 in ORDER, and the valid counts."""
    h, w = ok.shape
    hc, wc = coarse_extent(h, w)
    okp = np.zeros((2 * hc, 2 * wc), dtype=bool)
    okp[:h, :w] = ok
    ap = np.zeros((2 * hc, 2 * wc, a.shape[2]))
    ap[:h, :w] = a
    acc, n = np.zeros((hc, wc, a.shape[2])), np.zeros((hc, wc), dtype=np.int64)
    for dx, dy in ORDER:
        sel = okp[dy::2, dx::2]
        acc = acc + np.where(sel[:, :, None], ap[dy::2, dx::2], 0.0)
        n = n + sel
    return acc, n


def cell_means(ok, a, power=1):
    """The Down mean (power 1: / n) or variance (power 2: / (n n)) of a, NaN where n = 0."""
    acc, n = cell_sums(ok, a)
    with np.errstate(all="ignore"):
        q = acc / (n if power == 1 else n * n).astype(np.float64)[:, :, None]
    return np.where((n > 0)[:, :, None], q, np.nan), n


def down(ka, img, var, feat=None, fvar=None):
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    ok = valid_mask(ka, img, var, feat, fvar)
    img2, n = cell_means(ok, img, 1)
    var2, _ = cell_means(ok, var, 2)
    feat2 = fvar2 = None
    if feat is not None:
        feat2 = np.moveaxis(cell_means(ok, np.moveaxis(np.asarray(feat, dtype=np.float64), 0, 2), 1)[0], 2, 0)
        fvar2 = np.moveaxis(cell_means(ok, np.moveaxis(np.asarray(fvar, dtype=np.float64), 0, 2), 2)[0], 2, 0)
    return img2, var2, feat2, fvar2, n


def correction(ok, F, coarse_out):
    """R of every coarse cell: coarse_out - (the Down mean of F), 0.0 where the cell has no valid pixel."""
    DF, n = cell_means(ok, F, 1)
    with np.errstate(all="ignore"):
        return np.where((n > 0)[:, :, None], coarse_out - DF, 0.0)


def up(ka, img, var, feat, fvar, F, coarse_out):
    img, F = np.asarray(img, dtype=np.float64), np.asarray(F, dtype=np.float64)
    ok = valid_mask(ka, img, np.asarray(var, dtype=np.float64), feat, fvar)
    h, w = ok.shape
    hc, wc = coarse_extent(h, w)
    R = correction(ok, F, np.asarray(coarse_out, dtype=np.float64))
    x, y = np.arange(w), np.arange(h)
    X, Y = x >> 1, y >> 1
    Xs, Ys = np.clip(X + np.where(x & 1, 1, -1), 0, wc - 1), np.clip(Y + np.where(y & 1, 1, -1), 0, hc - 1)
    r00, r10, r01, r11 = R[np.ix_(Y, X)], R[np.ix_(Y, Xs)], R[np.ix_(Ys, X)], R[np.ix_(Ys, Xs)]
    t = ((WEIGHTS[0] * r00 + WEIGHTS[1] * r10) + WEIGHTS[2] * r01) + WEIGHTS[3] * r11
    with np.errstate(all="ignore"):
        return np.where(ok[:, :, None], F + t, img)


def extents(h, w, levels):
    """[(h, w)] of the levels made: level l + 1 exists if l + 1 < levels and w_l h_l > 1."""
    ext = [(h, w)]
    while len(ext) < levels and ext[-1][0] * ext[-1][1] > 1:
        ext.append(coarse_extent(*ext[-1]))
    return ext


def denoise(ka, img, var, feat=None, fvar=None, levels=DEFAULT_LEVELS, **nlm):
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError("levels")
    img, var = np.asarray(img, dtype=np.float64), np.asarray(var, dtype=np.float64)
    ext = extents(img.shape[0], img.shape[1], levels)
    pyr = [(img, var, feat, fvar)]
    for _ in ext[1:]:
        pyr.append(down(ka, *pyr[-1])[:4])
    res = [filter_level(ka, *lv, **nlm) for lv in pyr]
    out = res[-1]["out"]
    for lv, r in zip(pyr[-2::-1], res[-2::-1]):
        out = up(ka, *lv, r["out"], out)
    return dict(out=out, var_out=res[0]["var_out"], left_out=res[0]["left_out"], levels=len(ext), extents=ext, level=res)


def _valid_pixel(ka, img, var, feat, fvar, y, x):
    fin = lambda v: bool(np.isfinite(v))      # noqa: E731
    good = all(fin(img[y, x, c]) and fin(var[y, x, c]) and var[y, x, c] >= 0 for c in range(3))
    named = []
    if ka["kind"] != "plain":
        named += nlm_guided_ref.used_channels(ka["groups"] or [])
    if ka["kind"] == "demod":
        named += [ka["albedo_channel"] + c for c in range(3)] + ([ka["coverage_channel"]] if ka["coverage_channel"] >= 0 else [])
    return good and all(fin(feat[c, y, x]) and fin(fvar[c, y, x]) and fvar[c, y, x] >= 0 for c in named)


def brute_down(ka, img, var, feat=None, fvar=None):
    """Down read literally, coarse pixel by coarse pixel."""
    h, w = img.shape[:2]
    hc, wc = coarse_extent(h, w)
    nc = 0 if feat is None else feat.shape[0]
    img2, var2 = np.full((hc, wc, 3), np.nan), np.full((hc, wc, 3), np.nan)
    feat2, fvar2 = np.full((nc, hc, wc), np.nan), np.full((nc, hc, wc), np.nan)
    n = np.zeros((hc, wc), dtype=np.int64)
    for Y in range(hc):
        for X in range(wc):
            su, sv, sg, ss, cnt = [0.0] * 3, [0.0] * 3, [0.0] * nc, [0.0] * nc, 0
            for dx, dy in ORDER:
                x, y = 2 * X + dx, 2 * Y + dy
                if x >= w or y >= h or not _valid_pixel(ka, img, var, feat, fvar, y, x):
                    continue
                cnt += 1
                for c in range(3):
                    su[c] += img[y, x, c]
                    sv[c] += var[y, x, c]
                for c in range(nc):
                    sg[c] += feat[c, y, x]
                    ss[c] += fvar[c, y, x]
            n[Y, X] = cnt
            if cnt:
                img2[Y, X] = [s / cnt for s in su]
                var2[Y, X] = [s / (cnt * cnt) for s in sv]
                feat2[:, Y, X] = [s / cnt for s in sg]
                fvar2[:, Y, X] = [s / (cnt * cnt) for s in ss]
    return (img2, var2, feat2, fvar2, n) if feat is not None else (img2, var2, None, None, n)


def brute_up(ka, img, var, feat, fvar, F, coarse_out):
    """Up and combine read literally, fine pixel by fine pixel; every R is formed where it is used."""
    h, w = img.shape[:2]
    hc, wc = coarse_extent(h, w)

    def R(X, Y, c):
        s, cnt = 0.0, 0
        for dx, dy in ORDER:
            x, y = 2 * X + dx, 2 * Y + dy
            if x < w and y < h and _valid_pixel(ka, img, var, feat, fvar, y, x):
                s += F[y, x, c]
                cnt += 1
        return coarse_out[Y, X, c] - s / cnt if cnt else 0.0

    out = img.copy()
    for y in range(h):
        for x in range(w):
            if not _valid_pixel(ka, img, var, feat, fvar, y, x):
                continue
            X, Y = x >> 1, y >> 1
            Xs = min(max(X + (1 if x & 1 else -1), 0), wc - 1)
            Ys = min(max(Y + (1 if y & 1 else -1), 0), hc - 1)
            for c in range(3):
                t = ((0.5625 * R(X, Y, c) + 0.1875 * R(Xs, Y, c)) + 0.1875 * R(X, Ys, c)) + 0.0625 * R(Xs, Ys, c)
                out[y, x, c] = F[y, x, c] + t
    return out


def truth(h, w):
    """The film of the quality test: a ramp on the left, a slow sinusoid on the right, a dark disc, a thin bright bar."""
    y, x = np.mgrid[0:h, 0:w].astype(float)
    lum = np.where(x < w // 2, 0.25 + 0.5 * y / (h - 1), 1.0 + 0.3 * np.sin(2 * np.pi * x / 48.0))
    lum = np.where((x - 0.55 * w) ** 2 + (y - 0.35 * h) ** 2 < (0.15 * h) ** 2, 0.05, lum)
    lum = np.where((np.abs(x - 0.25 * w) < 1.5) & (y > 0.6 * h), 1.5, lum)
    return lum[..., None] * np.array([1.0, .8, .6])


def passes(tr, seed, k=4):
    """(mean of k passes with noise 0.25 sqrt(truth), variance of that mean): the recipe of nlm_ref.synthetic."""
    rng = np.random.default_rng(seed)
    p = np.stack([tr + 0.25 * np.sqrt(tr) * rng.standard_normal(tr.shape) for _ in range(k)])
    return p.mean(axis=0), p.var(axis=0, ddof=1) / k


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def low_frequency_rmse(a, b):
    """The RMSE of the 8 x 8 block means: the Down mean applied three times to both (every pixel valid)."""
    for _ in range(3):
        ok = np.ones(a.shape[:2], dtype=bool)
        a, b = cell_means(ok, a)[0], cell_means(ok, b)[0]
    return rmse(a, b)
