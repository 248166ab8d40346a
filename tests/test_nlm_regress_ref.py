"""Pins tests/nlm_regress_ref.py, the numpy restatement of the first-order feature regression on the non-local-means weights
(include/gdpt.h: gdpt_denoise_nlm_regress*), on the CPU: a literal brute force with numpy's own solver, the identities (no regressor,
no window, a constant film, a film exactly affine in its regressors), what it leaves out, and what the fit buys on a synthetic film."""
import numpy as np
import pytest

import nlm_guided_ref as NG
import nlm_regress_ref as NR
from test_nlm_guided_ref import noisy_features
from test_nlm_ref import noisy_film

GROUPS = [(0, 3, 1e-3)]
REGRESSORS = {0: [], 1: [4], 3: [0, 1, 2], 7: [6, 0, 1, 2, 3, 4, 5]}      # m -> channels (7: not in plane order)
SCALES = {0: [], 1: [0.5], 3: [1.0, 2.0, 0.25], 7: [1.0] * 7}
SUMS = ("sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out")


def close(a, b, ok, tol):
    for key in ("out", "var_out"):
        assert np.array_equal(a[key][~ok], b[key][~ok], equal_nan=True), key
        if ok.any():
            assert np.abs(a[key][ok] - b[key][ok]).max() <= tol * np.abs(b[key][ok]).max(), key
    for key in SUMS:
        assert abs(a[key] - b[key]) <= tol * abs(b[key]), key
    assert a["left_out"] == b["left_out"]


@pytest.mark.parametrize("planted", [False, True], ids=["clean", "planted"])
@pytest.mark.parametrize("m", [0, 1, 3, 7])
@pytest.mark.parametrize("r,f", [(0, 0), (1, 0), (2, 1), (3, 1)])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (9, 7)])
def test_brute_force_agrees(w, h, r, f, m, planted):
    """The restatement's LDL^T against numpy's solver: condition numbers here stay below 1e4 (ridge 1e-3 on regressors of spread
    0.03 - 0.06 a pixel pair), so 1e-10 relative leaves six orders over eps cond."""
    img, var = noisy_film(w, h, 7 + r)
    feat, fvar = noisy_features(w, h, r)
    left = 0
    if planted:
        img[h // 2, w // 2, 0] = np.inf
        var[0, 0, 1] = -1.0
        feat[4, h - 1, w - 1] = np.nan        # a regressor plane at m = 1 and 7 that no group names
        fvar[7, 0, w - 1] = np.nan            # named by nothing
        left = len({(h // 2, w // 2), (0, 0)} | ({(h - 1, w - 1)} if m in (1, 7) else set()))
    kw = dict(groups=GROUPS, channels=REGRESSORS[m], scales=SCALES[m], ridge=1e-3, r=r, f=f, k=0.8)
    a = NR.denoise(img, var, feat, fvar, **kw)
    b = NR.brute_force(img, var, feat, fvar, **kw)
    ok = NR.valid_mask(img, var, feat, fvar, GROUPS, REGRESSORS[m])
    assert a["left_out"] == b["left_out"] == left == (~ok).sum()
    assert np.array_equal(a["out"][~ok], img[~ok], equal_nan=True) and np.array_equal(a["var_out"][~ok], var[~ok], equal_nan=True)
    close(a, b, ok, 1e-10)


def test_no_regressor_is_the_guided_filter():
    """m = 0: A = (W), out = (sum w u) / W, var_out = sum (w / W)^2 v: the guided filter up to the placing of the division."""
    img, var = noisy_film(19, 13, 3)
    img[2, 3, 1] = np.nan
    feat, fvar = noisy_features(19, 13, 3)
    feat[7, 5, 5] = np.nan
    for groups in ([], GROUPS, [(0, 3, 1e-3), (3, 3, 1e-3)]):
        for (r, f) in ((0, 0), (3, 1), (5, 3)):
            a = NR.denoise(img, var, feat, fvar, groups, [], r=r, f=f, k=0.8)
            b = NG.denoise(img, var, feat, fvar, groups, r=r, f=f, k=0.8)
            close(a, b, NG.valid_mask(img, var, feat, fvar, groups), 1e-14)
            assert np.array_equal(a["out"], b["out"], equal_nan=True) or r > 0


def test_no_window_returns_the_input():
    img, var = noisy_film(9, 7, 2)
    var[3, 3, 0] = np.inf
    feat, fvar = noisy_features(9, 7, 2)
    for m in (0, 3, 7):
        d = NR.denoise(img, var, feat, fvar, GROUPS, REGRESSORS[m], ridge=1e-2, r=0, f=0)
        assert np.array_equal(d["out"], img, equal_nan=True) and np.array_equal(d["var_out"], var, equal_nan=True) and d["left_out"] == 1


def test_a_constant_image_comes_back_constant():
    """b_c = A e_0 times the constant, so beta = (constant, 0, ...) whatever the regressors hold: to 1e-13 relative."""
    w, h = 14, 11
    _, var = noisy_film(w, h, 4)
    feat, fvar = noisy_features(w, h, 4)
    img = np.ones((h, w, 3)) * np.array([0.7, 1.3, 0.02])
    for m in (0, 1, 7):
        d = NR.denoise(img, var, feat, fvar, GROUPS, REGRESSORS[m], scales=SCALES[m], ridge=1e-2, r=4, f=1, k=0.8)
        assert np.abs(d["out"] - img).max() <= 1e-13 * 1.3 and d["left_out"] == 0


def test_an_image_affine_in_its_regressors_comes_back_as_the_ridge_goes():
    """u = c0 + sum a_j g_j exactly, the regressors' variances zero. The fit without a ridge is exact, and the ridge shrinks the
    slopes by about ridge W (A')^-1, an error linear in the ridge: at ridge 1e-9 it is 1e-3 of that at ridge 1e-6, within 20 %
    (the regressors' spread keeps the term well above rounding at both). With a colour variance of 1 every colour distance is
    negative and every weight exactly 1, so the whole window is fitted. With the colour variances zero too the weights of differing
    pixels underflow (epsilon alone is in the denominator), and the film comes back within the same bounds, trivially."""
    w, h = 12, 9
    feat, _ = noisy_features(w, h, 9, sigma=0.05)
    fvar = np.zeros_like(feat)
    coef = np.array([[0.5, -0.3, 0.2], [0.1, 0.4, -0.6], [-0.2, 0.3, 0.5]])         # (regressor, colour)
    img = 1.0 + np.tensordot(np.moveaxis(feat[:3], 0, 2), coef, axes=1)
    for colour_var in (1.0, 0.0):
        var = np.full_like(img, colour_var)
        errs = []
        for ridge in (1e-6, 1e-9):
            d = NR.denoise(img, var, feat, fvar, [], [0, 1, 2], ridge=ridge, r=3, f=1, k=0.8)
            errs.append(np.abs(d["out"] - img).max())
            assert d["left_out"] == 0
        print(f"affine film, colour variance {colour_var}: worst error {errs[0]:.3e} at ridge 1e-6, {errs[1]:.3e} at ridge 1e-9")
        assert errs[0] <= 1e-3 and errs[1] <= 1e-6
        if colour_var:
            assert errs[1] > 1e-12 and 0.8e-3 <= errs[1] / errs[0] <= 1.2e-3, errs
            plain = NR.denoise(img, var, feat, fvar, [], [], r=3, f=1, k=0.8)
            assert np.abs(plain["out"] - img).max() > 1e-2           # the weighted mean over the same window is biased


def test_an_invalid_regressor_leaves_the_pixel_out_and_an_unnamed_plane_changes_nothing():
    w, h = 14, 11
    img, var = noisy_film(w, h, 6)
    feat, fvar = noisy_features(w, h, 6)
    kw = dict(groups=GROUPS, channels=[3, 4], ridge=1e-2, r=3, f=1, k=0.8)
    clean = NR.denoise(img, var, feat, fvar, **kw)
    for n, bad in enumerate((np.nan, np.inf, -np.inf)):
        feat[5, n, n] = bad
        fvar[6, h - 1 - n, n] = bad
    fvar[7, 5, 5] = -1.0
    d = NR.denoise(img, var, feat, fvar, **kw)
    assert d["left_out"] == 0 and all(np.array_equal(d[k], clean[k]) for k in ("out", "var_out")) and all(d[k] == clean[k] for k in SUMS)
    feat[3, 2, 2] = np.nan
    fvar[4, 7, 9] = -1e-6
    d = NR.denoise(img, var, feat, fvar, **kw)
    assert d["left_out"] == 2
    for (y, x) in ((2, 2), (7, 9)):
        assert np.array_equal(d["out"][y, x], img[y, x]) and np.array_equal(d["var_out"][y, x], var[y, x])
    assert np.isfinite(d["out"]).all() and np.isfinite(d["var_out"]).all()


def test_the_fit_beats_the_best_guided_filter_on_the_synthetic_film():
    """The film of synthetic_regression (48 x 40; albedo checker, a turning normal, a depth ramp), r = 10, f = 3, the albedo group as
    the guide, k = 4, regressors planes 0 - 6 at scale 1, ridge 1e-2, seeds 0 - 4:
      RMSE <= 0.70 x the smallest RMSE of the guided filter (default two groups) over k in {4, 8, 16}
      RMSE <= 1.5 x sqrt(mean var_out)
    Measured, seeds 0 - 4: RMSE 0.0128, 0.0154, 0.0140, 0.0136, 0.0137; against the best guided filter (0.0250, 0.0263, 0.0248,
    0.0256, 0.0253) 0.513, 0.584, 0.563, 0.532, 0.541; against sqrt(mean var_out) 1.061, 1.287, 1.168, 1.119, 1.116."""
    for seed in range(5):
        truth, mean, var, feat, fvar = NR.synthetic_regression(seed)
        d = NR.denoise(mean, var, feat, fvar, [(0, 3, 1e-3)], list(range(7)), ridge=1e-2, r=10, f=3, k=4.0)
        rmse = np.sqrt(((d["out"] - truth) ** 2).mean())
        best = min(np.sqrt(((NG.denoise(mean, var, feat, fvar, [(0, 3, 1e-3), (3, 3, 1e-3)], r=10, f=3, k=k)["out"] - truth) ** 2).mean())
                   for k in (4.0, 8.0, 16.0))
        sd = np.sqrt(d["var_out"].mean())
        print(f"seed {seed}: RMSE regression {rmse:.4f}, best guided {best:.4f} (x{rmse / best:.3f}), sqrt(mean var_out) {sd:.4f} (x{rmse / sd:.3f})")
        assert d["left_out"] == 0
        assert rmse <= 0.70 * best
        assert rmse <= 1.5 * sd
