"""Pins tests/nlm_collab_ref.py, the numpy restatement of the collaborative form of the first-order feature regression
(include/gdpt.h: gdpt_denoise_nlm_collab*), on the CPU: a literal brute force with numpy's own solver, what is left out, the identities
(no window, the regression's own output in the coefficient film, a constant film, a film exactly affine in its regressors), and what
the averaging of overlapping fits buys on the synthetic film of the regression's quality test."""
import numpy as np
import pytest

import nlm_collab_ref as NC
import nlm_regress_ref as NR
from test_nlm_guided_ref import noisy_features
from test_nlm_ref import noisy_film

GROUPS = [(0, 3, 1e-3)]
REGRESSORS = {0: [], 1: [4], 3: [0, 1, 2], 7: [6, 0, 1, 2, 3, 4, 5]}      # m -> channels (7: not in plane order)
SCALES = {0: [], 1: [0.5], 3: [1.0, 2.0, 0.25], 7: [1.0] * 7}
SUMS = ("sum_var_in", "sum_sq_in", "sum_sq_out")


def close(a, b, ok, tol):
    for key in ("out", "coef"):
        bad = ~ok if key == "out" else np.broadcast_to(~ok, a[key].shape)
        good = ~bad
        assert np.array_equal(a[key][bad], b[key][bad], equal_nan=True), key
        if ok.any():
            assert np.abs(a[key][good] - b[key][good]).max() <= tol * np.abs(b[key][good]).max(), key
    for key in SUMS:
        assert abs(a[key] - b[key]) <= tol * abs(b[key]), key
    assert a["left_out"] == b["left_out"]
    for d in (a, b):
        assert np.isnan(d["sum_var_out"]) and np.isnan(d["error_out"])


def plant(img, var, feat, fvar, m):
    """NaN, +-Inf and a negative variance in img, var, a regressor plane and its variance; returns the pixels left out at m."""
    h, w = img.shape[:2]
    img[h // 2, w // 2, 0] = np.inf
    var[0, 0, 1] = -1.0
    feat[4, h - 1, w - 1] = np.nan        # a regressor plane at m = 1 and 7 that no group names
    fvar[4, h - 1, 0] = -np.inf           # its variance
    fvar[7, 0, w - 1] = np.nan            # named by nothing
    return {(h // 2, w // 2), (0, 0)} | ({(h - 1, w - 1), (h - 1, 0)} if m in (1, 7) else set())


@pytest.mark.parametrize("planted", [False, True], ids=["clean", "planted"])
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "unguided"])
@pytest.mark.parametrize("m", [0, 1, 3, 7])
@pytest.mark.parametrize("r,f", [(0, 0), (1, 0), (2, 1), (3, 1)])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (9, 7)])
def test_brute_force_agrees(w, h, r, f, m, guided, planted):
    """The restatement's LDL^T against numpy's solver, the whole solution and the gathered image: condition numbers here stay below
    1e4 (ridge 1e-3 on regressors of spread 0.03 - 0.06 a pixel pair), so 1e-10 relative to the largest value leaves six orders over
    eps cond; the gather is a convex combination of the fits' values and adds no more than its 49 roundings."""
    img, var = noisy_film(w, h, 7 + r)
    feat, fvar = noisy_features(w, h, r)
    left = plant(img, var, feat, fvar, m) if planted else set()
    groups = GROUPS if guided else []
    kw = dict(groups=groups, channels=REGRESSORS[m], scales=SCALES[m], ridge=1e-3, r=r, f=f, k=0.8)
    a = NC.denoise(img, var, feat, fvar, **kw)
    b = NC.brute_force(img, var, feat, fvar, **kw)
    ok = NR.valid_mask(img, var, feat, fvar, groups, REGRESSORS[m])
    assert a["left_out"] == b["left_out"] == len(left) == (~ok).sum()
    d = 1 + m
    assert a["coef"].shape == (3 * d, h, w)
    assert np.array_equal(a["out"][~ok], img[~ok], equal_nan=True)          # the planted pixel keeps its bits, counted once
    for c in range(3):
        assert np.array_equal(a["coef"][c * d][~ok], img[:, :, c][~ok], equal_nan=True) and not a["coef"][c * d + 1:(c + 1) * d][:, ~ok].any()
    close(a, b, ok, 1e-10)


def test_a_pixel_among_invalid_pixels_returns_its_own_fit():
    """Every other pixel of the centre's window is invalid: its fit has the tap o = 0 alone (W = 1, beta = (u, 0, ..)) and nobody
    else's fit reaches it, so Omega = 1 and out = u."""
    w, h = 5, 5
    img, var = noisy_film(w, h, 1)
    feat, fvar = noisy_features(w, h, 1)
    for (y, x) in ((1, 1), (1, 2), (1, 3), (2, 1), (2, 3), (3, 1), (3, 2), (3, 3)):
        img[y, x, (y + x) % 3] = (np.nan, np.inf, -np.inf)[(y * x) % 3]
    for m in (0, 3, 7):
        d = NC.denoise(img, var, feat, fvar, GROUPS, REGRESSORS[m], ridge=1e-2, r=1, f=1, k=0.8)
        assert d["left_out"] == 8 and np.array_equal(d["out"][2, 2], img[2, 2])
        planes = d["coef"][:, 2, 2].reshape(3, 1 + m)
        assert np.array_equal(planes[:, 0], img[2, 2]) and not planes[:, 1:].any()
        ok = NR.valid_mask(img, var, feat, fvar, GROUPS, REGRESSORS[m])
        assert np.array_equal(d["out"][~ok], img[~ok], equal_nan=True) and np.isfinite(d["out"][ok]).all()


def test_an_unnamed_plane_changes_nothing_and_an_invalid_regressor_leaves_the_pixel_out():
    w, h = 14, 11
    img, var = noisy_film(w, h, 6)
    feat, fvar = noisy_features(w, h, 6)
    kw = dict(groups=GROUPS, channels=[3, 4], ridge=1e-2, r=3, f=1, k=0.8)
    clean = NC.denoise(img, var, feat, fvar, **kw)
    for n, bad in enumerate((np.nan, np.inf, -np.inf)):
        feat[5, n, n] = bad
        fvar[6, h - 1 - n, n] = bad
    fvar[7, 5, 5] = -1.0
    d = NC.denoise(img, var, feat, fvar, **kw)
    assert d["left_out"] == 0 and all(np.array_equal(d[k], clean[k]) for k in ("out", "coef")) and all(d[k] == clean[k] for k in SUMS)
    feat[3, 2, 2] = np.nan
    fvar[4, 7, 9] = -1e-6
    d = NC.denoise(img, var, feat, fvar, **kw)
    assert d["left_out"] == 2
    for (y, x) in ((2, 2), (7, 9)):
        assert np.array_equal(d["out"][y, x], img[y, x])
    assert np.isfinite(d["out"]).all() and np.isfinite(d["coef"]).all()


def test_no_window_returns_the_input():
    img, var = noisy_film(9, 7, 2)
    var[3, 3, 0] = np.inf
    feat, fvar = noisy_features(9, 7, 2)
    for m in (0, 3, 7):
        d = NC.denoise(img, var, feat, fvar, GROUPS, REGRESSORS[m], ridge=1e-2, r=0, f=0)
        assert np.array_equal(d["out"], img, equal_nan=True) and d["left_out"] == 1


@pytest.mark.parametrize("planted", [False, True], ids=["clean", "planted"])
def test_the_first_coefficient_plane_is_the_regression_bit_for_bit(planted):
    w, h = 19, 13
    img, var = noisy_film(w, h, 3)
    feat, fvar = noisy_features(w, h, 3)
    for m in (0, 1, 3, 7):
        if planted:
            plant(img, var, feat, fvar, m)
        for groups, (r, f), ridge in (([], (0, 0), 1e-2), (GROUPS, (3, 1), 1e-3), ([(0, 3, 1e-3), (3, 3, 1e-3)], (5, 3), 1e-2)):
            kw = dict(groups=groups, channels=REGRESSORS[m], scales=SCALES[m], ridge=ridge, r=r, f=f, k=0.8)
            a, b = NC.denoise(img, var, feat, fvar, **kw), NR.denoise(img, var, feat, fvar, **kw)
            d = 1 + m
            assert np.array_equal(np.moveaxis(a["coef"][[0, d, 2 * d]], 0, 2), b["out"], equal_nan=True)
            assert a["left_out"] == b["left_out"] and a["sum_var_in"] == b["sum_var_in"] and a["sum_sq_in"] == b["sum_sq_in"]


def test_a_constant_image_comes_back_constant():
    """Every fit is (constant, 0, ...) to rounding whatever the regressors hold, and so is every average of them: to 1e-13 relative."""
    w, h = 14, 11
    _, var = noisy_film(w, h, 4)
    feat, fvar = noisy_features(w, h, 4)
    img = np.ones((h, w, 3)) * np.array([0.7, 1.3, 0.02])
    for m in (0, 1, 7):
        d = NC.denoise(img, var, feat, fvar, GROUPS, REGRESSORS[m], scales=SCALES[m], ridge=1e-2, r=4, f=1, k=0.8)
        assert np.abs(d["out"] - img).max() <= 1e-13 * 1.3 and d["left_out"] == 0


def test_an_image_affine_in_its_regressors_comes_back_as_the_ridge_goes():
    """The film and the bounds of the regression's own test (tests/test_nlm_regress_ref.py): u = c0 + sum a_j g_j exactly, the
    regressors' variances zero. Every window's fit is then exact everywhere in its window up to the ridge's shrinking of the slopes,
    an error linear in the ridge, so the average of the fits is as well: at ridge 1e-9 it is 1e-3 of that at ridge 1e-6, within 20 %."""
    w, h = 12, 9
    feat, _ = noisy_features(w, h, 9, sigma=0.05)
    fvar = np.zeros_like(feat)
    coef = np.array([[0.5, -0.3, 0.2], [0.1, 0.4, -0.6], [-0.2, 0.3, 0.5]])         # (regressor, colour)
    img = 1.0 + np.tensordot(np.moveaxis(feat[:3], 0, 2), coef, axes=1)
    for colour_var in (1.0, 0.0):
        var = np.full_like(img, colour_var)
        errs = []
        for ridge in (1e-6, 1e-9):
            d = NC.denoise(img, var, feat, fvar, [], [0, 1, 2], ridge=ridge, r=3, f=1, k=0.8)
            errs.append(np.abs(d["out"] - img).max())
            assert d["left_out"] == 0
        print(f"affine film, colour variance {colour_var}: worst error {errs[0]:.3e} at ridge 1e-6, {errs[1]:.3e} at ridge 1e-9")
        assert errs[0] <= 1e-3 and errs[1] <= 1e-6
        if colour_var:
            assert errs[1] > 1e-12 and 0.8e-3 <= errs[1] / errs[0] <= 1.2e-3, errs


# ridge -> the worst ratio RMSE(collaborative) / RMSE(point regression) this restatement gives over seeds 0 - 4 (see the test below)
WORST_MEASURED = {1e-2: 0.840, 1e-3: 0.733}
MARGIN = 0.08          # the project's allowance for a generator that draws differently


@pytest.mark.parametrize("ridge", [1e-2, 1e-3])
def test_the_collaborative_form_beats_the_point_regression_on_the_synthetic_film(ridge):
    """The film and configuration of test_the_fit_beats_the_best_guided_filter_on_the_synthetic_film (48 x 40, r = 10, f = 3, the albedo
    group as the guide, k = 4, regressors planes 0 - 6 at scale 1), seeds 0 - 4, at ridge 1e-2 and 1e-3:
      RMSE(collaborative) <= (worst measured ratio + 0.08) x RMSE(point regression), a bound that stays below 1
    The point regression is the coefficient film's plane c d (the regression's out bit for bit, checked above).
    Measured with this restatement, seeds 0 - 4:
      ridge 1e-2: RMSE point 0.0128, 0.0154, 0.0140, 0.0136, 0.0137; collaborative 0.0102, 0.0124, 0.0118, 0.0112, 0.0110;
                  ratios 0.799, 0.809, 0.840, 0.822, 0.804 (bound 0.92)
      ridge 1e-3: RMSE point 0.0132, 0.0154, 0.0134, 0.0139, 0.0135; collaborative 0.0094, 0.0106, 0.0098, 0.0102, 0.0096;
                  ratios 0.713, 0.690, 0.728, 0.733, 0.711 (bound 0.813)"""
    ratios = []
    for seed in range(5):
        truth, mean, var, feat, fvar = NR.synthetic_regression(seed)
        d = NC.denoise(mean, var, feat, fvar, [(0, 3, 1e-3)], list(range(7)), ridge=ridge, r=10, f=3, k=4.0)
        point = np.moveaxis(d["coef"][[0, 8, 16]], 0, 2)
        rmse_c, rmse_p = np.sqrt(((d["out"] - truth) ** 2).mean()), np.sqrt(((point - truth) ** 2).mean())
        ratios.append(rmse_c / rmse_p)
        print(f"ridge {ridge:g} seed {seed}: RMSE point regression {rmse_p:.4f}, collaborative {rmse_c:.4f} (x{ratios[-1]:.3f})")
        assert d["left_out"] == 0
    assert WORST_MEASURED[ridge] is not None, f"WORST_MEASURED[{ridge:g}] has not been recorded; this run measured {max(ratios):.3f}"
    bound = WORST_MEASURED[ridge] + MARGIN
    assert bound < 1.0
    assert max(ratios) <= bound, ratios
