"""Pins tests/nlm_ref.py, the numpy restatement of the non-local-means filter (include/gdpt.h: gdpt_denoise_nlm*), on the CPU: its
identities, what it leaves out, a brute-force double loop that is not separable, and what the filter does to a noisy synthetic film."""
import numpy as np

import nlm_ref as N


def noisy_film(w, h, seed, sigma=0.05):
    """A smooth film with noise of the scale its variance plane states: the weights come out between 0 and 1, not at either end."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 0.5 + 0.25 * np.sin(0.7 * x + 0.3 * y)
    img = base[:, :, None] * np.array([1.0, 0.7, 0.4]) + sigma * rng.standard_normal((h, w, 3))
    var = sigma * sigma * rng.uniform(0.5, 1.5, (h, w, 3))
    return img, var


def test_radius_zero_is_the_identity():
    img, var = noisy_film(9, 7, 0)
    for f in (0, 3):
        d = N.denoise(img, var, r=0, f=f)
        assert np.array_equal(d["out"], img) and np.array_equal(d["var_out"], var)
        assert d["left_out"] == 0 and d["sum_var_out"] == d["sum_var_in"] and d["sum_sq_out"] == d["sum_sq_in"]


def test_a_constant_image_comes_back_with_the_variance_of_a_window_mean():
    w, h, r = 9, 7, 2
    img, var = np.full((h, w, 3), 0.75), np.full((h, w, 3), 0.01)
    d = N.denoise(img, var, r=r, f=1)
    assert np.allclose(d["out"], img, rtol=1e-15, atol=0)
    y, x = np.mgrid[0:h, 0:w]
    count = (np.minimum(x + r, w - 1) - np.maximum(x - r, 0) + 1) * (np.minimum(y + r, h - 1) - np.maximum(y - r, 0) + 1)
    assert np.allclose(d["var_out"], var / count[:, :, None], rtol=1e-14, atol=0)


def test_what_is_not_valid_is_left_out():
    img, var = noisy_film(12, 10, 1)
    clean = N.denoise(img, var, r=3, f=1)
    img[4, 5, 1] = np.nan
    var[7, 2, 0] = -1e-3
    d = N.denoise(img, var, r=3, f=1)
    assert d["left_out"] == 2
    for (y, x) in ((4, 5), (7, 2)):
        assert np.array_equal(d["out"][y, x], img[y, x], equal_nan=True) and np.array_equal(d["var_out"][y, x], var[y, x], equal_nan=True)
    fin = np.isfinite(d["out"]) & np.isfinite(d["var_out"])
    assert (~fin).sum() == 1 and not fin[4, 5, 1]
    assert np.isfinite([d[k] for k in ("sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out", "error_in", "error_out")]).all()
    # far from the two planted pixels (further than r + f) nothing has changed
    far = np.ones((10, 12), dtype=bool)
    for (y, x) in ((4, 5), (7, 2)):
        far[max(0, y - 4):y + 5, max(0, x - 4):x + 5] = False
    assert far.any() and np.array_equal(d["out"][far], clean["out"][far])


def test_brute_force_agrees():
    for (w, h, r, f, seed) in ((7, 6, 2, 1, 2), (5, 8, 3, 2, 3), (6, 5, 1, 0, 4)):
        img, var = noisy_film(w, h, seed)
        img[h // 2, w // 2, 0] = np.inf
        var[0, w - 1, 2] = -1.0
        a, b = N.denoise(img, var, r=r, f=f), N.brute_force(img, var, r=r, f=f)
        ok = N.valid_mask(img, var)
        wgt_spread = a["var_out"][ok] / var[ok]
        assert wgt_spread.min() < 0.5                     # the filter averages here: the weights are not all at 0
        assert np.array_equal(a["out"][~ok], b["out"][~ok], equal_nan=True)
        for key in ("out", "var_out"):
            assert np.abs(a[key][ok] - b[key][ok]).max() <= 1e-12 * np.abs(b[key][ok]).max(), (w, h, r, f, key)
        for key in ("sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out"):
            assert abs(a[key] - b[key]) <= 1e-12 * abs(b[key])
        assert a["left_out"] == b["left_out"] == 2


def test_the_synthetic_film():
    """48 x 40: step edge, ramp, sinusoid, dark disc; four passes with noise 0.25 sqrt(truth), the variance of their mean from their
    sample variance. At the defaults the filtered RMSE against the truth is below 0.8 of the unfiltered one, and lies between 0.9
    and 1.3 of sqrt(mean var_out): error_out leaves out the filter's bias and the dependence of the weights on the data, and that is
    how far it is off. Measured over the seeds 0..4: ratios 0.58 - 0.65 and 1.03 - 1.08."""
    for seed in range(5):
        truth, mean, var = N.synthetic(seed)
        d = N.denoise(mean, var, **N.DEFAULTS)
        before, after = np.sqrt(((mean - truth) ** 2).mean()), np.sqrt(((d["out"] - truth) ** 2).mean())
        stated = np.sqrt(d["var_out"].mean())
        print(f"seed {seed}: RMSE {before:.4f} -> {after:.4f} (x{after / before:.3f}); true / stated {after / stated:.3f}; "
              f"error_in {d['error_in']:.4f}, error_out {d['error_out']:.4f}")
        assert d["left_out"] == 0
        assert after < 0.8 * before
        assert 0.9 * stated < after < 1.3 * stated
