"""The numpy restatement of the albedo-demodulated non-local-means filter (tests/nlm_demod_ref.py; include/gdpt.h:
gdpt_denoise_nlm_demod*): against a literal per-pixel brute force, the three exact properties of the definition, validity, the
effective albedo at its edges, and the quality claim on the textured film of tests/nlm_guided_ref.py. No GPU."""
import numpy as np
import pytest

import nlm_demod_ref as ND
import nlm_guided_ref as NG
import nlm_ref as N
from test_nlm_guided_ref import noisy_features
from test_nlm_ref import noisy_film

GROUPS = [(3, 3, 1e-3)]                        # a normal group beside the albedo triple at 0 and the coverage at 7


def albedo_features(w, h, seed):
    """Eight planes as a feature render lays them out: a textured albedo in 0-2 (0.2 .. 0.9), coverage in 7 (1, with partly covered
    pixels down one column), the others noisy_features'."""
    feat, fvar = noisy_features(w, h, seed)
    rng = np.random.default_rng(2000 + seed)
    y, x = np.mgrid[0:h, 0:w]
    chk = ((x // 2 + y // 2) % 2).astype(np.float64)
    for c in range(3):
        feat[c] = (0.3 + 0.2 * c) * (1.0 + 0.5 * (chk - 0.5)) + 0.01 * rng.standard_normal((h, w))
    feat[7] = 1.0
    fvar[7] = 0.0
    feat[7, :, w - 1] = rng.uniform(0.2, 0.9, h)
    fvar[7, :, w - 1] = 1e-3
    return feat, fvar


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("out", "var_out")) and \
        all(a[k] == b[k] for k in ("left_out", "sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out"))


@pytest.mark.parametrize("coverage", [-1, 7], ids=["nocov", "cov"])
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("w,h,r,f", [(9, 7, 2, 1), (13, 5, 3, 0)])
def test_brute_force_agrees(w, h, r, f, guided, coverage):
    img, var = noisy_film(w, h, 3 + r)
    feat, fvar = albedo_features(w, h, r)
    img[h // 2, w // 2, 0] = np.inf
    feat[1, 0, w - 1] = np.nan
    groups = GROUPS if guided else None
    kw = dict(albedo_channel=0, coverage_channel=coverage, floor=1e-3, groups=groups, r=r, f=f, k=0.8)
    a, b = ND.denoise(img, var, feat, fvar, **kw), ND.brute_force(img, var, feat, fvar, **kw)
    ok = ND.valid_mask(img, var, feat, fvar, 0, coverage, groups)
    assert a["left_out"] == b["left_out"] == 2 == (~ok).sum()
    for key in ("out", "var_out"):
        assert np.array_equal(a[key][~ok], b[key][~ok], equal_nan=True)
        assert np.array_equal(a[key][~ok], (img if key == "out" else var)[~ok], equal_nan=True)
        err = np.linalg.norm(a[key][ok] - b[key][ok]) / np.linalg.norm(b[key][ok])
        assert err < 1e-13, (key, err)
    for key in ("sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out"):
        assert abs(a[key] - b[key]) <= 1e-13 * abs(b[key])
    plain = N.denoise(img, var, r=r, f=f, k=0.8)
    assert not np.allclose(plain["out"][ok], a["out"][ok], rtol=1e-6)          # the division is at work


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_unit_divisor_is_the_undemodulated_filter_bit_for_bit(guided):
    w, h, r, f = 13, 9, 3, 1
    img, var = noisy_film(w, h, 1)
    img[2, 3, 1] = np.nan
    feat, fvar = noisy_features(w, h, 1)
    groups = GROUPS if guided else None
    want = NG.denoise(img, var, feat, fvar, GROUPS, r=r, f=f, k=0.8) if guided else N.denoise(img, var, r=r, f=f, k=0.8)
    for albedo, cov in ((1.0, 1.0), (0.0, 0.0)):
        ft, fv = feat.copy(), fvar.copy()
        ft[0:3], ft[7] = albedo, cov
        got = ND.denoise(img, var, ft, fv, 0, 7, 1e-3, groups, r=r, f=f, k=0.8)
        assert same(got, want), (albedo, cov)
    ft = feat.copy()
    ft[0:3] = 1.0
    assert same(ND.denoise(img, var, ft, fvar, 0, -1, 1e-3, groups, r=r, f=f, k=0.8), want)      # no coverage plane: cov = 1


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_power_of_two_scaling_bit_for_bit(guided):
    w, h, r, f = 13, 9, 3, 1
    img, var = noisy_film(w, h, 2)
    feat, fvar = albedo_features(w, h, 2)
    feat[7], fvar[7] = 1.0, 0.0
    y, x = np.mgrid[0:h, 0:w]
    m = np.where((x + y) % 2 == 0, 2.0, 0.5)
    groups = GROUPS if guided else None
    kw = dict(albedo_channel=0, coverage_channel=7, floor=1e-3, groups=groups, r=r, f=f, k=0.8)
    a = ND.denoise(img, var, feat, fvar, **kw)
    ft = feat.copy()
    ft[0:3] = feat[0:3] * m
    assert (ft[0:3] > 1e-3).all()
    b = ND.denoise(img * m[:, :, None], var * (m * m)[:, :, None], ft, fvar, **kw)
    assert np.array_equal(b["out"], a["out"] * m[:, :, None]) and np.array_equal(b["var_out"], a["var_out"] * (m * m)[:, :, None])
    assert not np.array_equal(b["out"], a["out"])


def test_radius_zero_is_divide_and_multiply():
    img, var = noisy_film(9, 7, 0)
    feat, fvar = albedo_features(9, 7, 0)
    d = ND.denoise(img, var, feat, fvar, 0, 7, 1e-3, None, r=0, f=0)
    al = ND.effective_albedo(feat, 0, 7, 1e-3)
    assert np.array_equal(d["out"], (img / al) * al) and np.array_equal(d["var_out"], (var / (al * al)) * (al * al))
    assert np.allclose(d["out"], img, rtol=1e-15, atol=0)
    assert d["sum_var_in"] == float(var.sum()) and d["sum_sq_in"] == float((img * img).sum())


PLANTS = [(0, "nan"), (2, "+inf"), (1, "-inf"), (0, "vnan"), (1, "vinf"), (2, "vneg"), (7, "nan"), (7, "vneg"), (7, "vinf")]


@pytest.mark.parametrize("channel,kind", PLANTS)
def test_a_planted_value_leaves_exactly_that_pixel_out(channel, kind):
    w, h, r, f = 11, 8, 2, 1
    img, var = noisy_film(w, h, 4)
    feat, fvar = albedo_features(w, h, 4)
    y, x = 3, 5
    value = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "vnan": np.nan, "vinf": np.inf, "vneg": -1e-9}[kind]
    (fvar if kind.startswith("v") else feat)[channel, y, x] = value
    d = ND.denoise(img, var, feat, fvar, 0, 7, 1e-3, None, r=r, f=f)
    assert d["left_out"] == 1
    assert np.array_equal(d["out"][y, x], img[y, x]) and np.array_equal(d["var_out"][y, x], var[y, x])
    others = np.ones((h, w), dtype=bool)
    others[y, x] = False
    assert np.isfinite(d["out"][others]).all() and not np.array_equal(d["out"][others], img[others])
    # the same value in a plane no field names changes nothing: the coverage plane of a call without one, and plane 5
    if channel == 7:
        clean_f, clean_v = albedo_features(w, h, 4)
        assert same(ND.denoise(img, var, feat, fvar, 0, -1, 1e-3, None, r=r, f=f), ND.denoise(img, var, clean_f, clean_v, 0, -1, 1e-3, None, r=r, f=f))
    clean_f, clean_v = albedo_features(w, h, 4)
    want = ND.denoise(img, var, clean_f, clean_v, 0, 7, 1e-3, None, r=r, f=f)
    (clean_v if kind.startswith("v") else clean_f)[5, y, x] = value
    assert same(ND.denoise(img, var, clean_f, clean_v, 0, 7, 1e-3, None, r=r, f=f), want)
    # ... unless a guide names it
    assert ND.denoise(img, var, clean_f, clean_v, 0, 7, 1e-3, GROUPS, r=r, f=f)["left_out"] == 1


def test_the_effective_albedo_follows_the_formula():
    feat = np.zeros((8, 1, 5))
    feat[0:3, 0, :] = np.array([0.5, 1e-4, -0.25, 0.0, 0.4])      # plain, below the floor, negative, a miss, partly covered
    feat[7, 0, :] = np.array([1.0, 1.0, 1.0, 0.0, 0.25])
    al = ND.effective_albedo(feat, 0, 7, 1e-3)[0, :, 0]
    assert np.array_equal(al, np.array([0.5, 1e-3, 1e-3, 1.0, 0.4 + (1.0 - 0.25)]))
    assert np.array_equal(ND.effective_albedo(feat, 0, -1, 1e-3)[0, :, 0], np.array([0.5, 1e-3, 1e-3, 1e-3, 0.4]))
    assert np.array_equal(ND.effective_albedo(feat, 0, 7, 0.6)[0, :, 1], np.array([0.6, 0.6, 0.6, 1.0, 1.15]))
    # and the filter divides by it: one pixel, r = 0
    img, var = np.full((1, 5, 3), 0.3), np.full((1, 5, 3), 0.01)
    d = ND.denoise(img, var, feat, np.zeros_like(feat), 0, 7, 1e-3, None, r=0, f=0)
    full = ND.effective_albedo(feat, 0, 7, 1e-3)
    assert np.array_equal(d["out"], (img / full) * full) and d["left_out"] == 0


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def test_quality_on_the_textured_film():
    """synthetic_textured(seed), seeds 0-4, r = 10, f = 3, coverage 1, floor 1e-3: the demodulated unguided RMSE against the plain
    filter's at k = 0.45 (<= 0.90; measured 0.772 - 0.826) and at k = 1.0 (<= 0.75; measured 0.626 - 0.673), and against the
    albedo-guided filter's at k = 1.0 (<= 1.0; measured 0.880 - 0.915)."""
    for seed in range(5):
        truth, mean, var, albedo, avar = NG.synthetic_textured(seed)
        feat = np.concatenate([albedo, np.ones((1,) + albedo.shape[1:])])
        fvar = np.concatenate([avar, np.zeros((1,) + albedo.shape[1:])])
        ratios = {}
        for k in (0.45, 1.0):
            dem = ND.denoise(mean, var, feat, fvar, 0, 3, 1e-3, None, r=10, f=3, k=k)
            assert dem["left_out"] == 0
            ratios[("plain", k)] = rmse(dem["out"], truth) / rmse(N.denoise(mean, var, r=10, f=3, k=k)["out"], truth)
            ratios[("unfiltered", k)] = rmse(dem["out"], truth) / rmse(mean, truth)
            if k == 1.0:
                guided = NG.denoise(mean, var, albedo, avar, [(0, 3, 1e-3)], r=10, f=3, k=k)
                ratios[("guided", k)] = rmse(dem["out"], truth) / rmse(guided["out"], truth)
        print(f"seed {seed}: demodulated / plain at k 0.45 {ratios[('plain', 0.45)]:.3f}, at k 1.0 {ratios[('plain', 1.0)]:.3f}; / guided by albedo at "
              f"k 1.0 {ratios[('guided', 1.0)]:.3f}; / unfiltered at k 0.45 {ratios[('unfiltered', 0.45)]:.3f}, at k 1.0 {ratios[('unfiltered', 1.0)]:.3f}")
        assert ratios[("plain", 0.45)] <= 0.90
        assert ratios[("plain", 1.0)] <= 0.75
        assert ratios[("guided", 1.0)] <= 1.0
