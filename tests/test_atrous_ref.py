"""Pins tests/atrous_ref.py, the numpy restatement of the edge-avoiding a-trous wavelet filter (include/gdpt.h: gdpt_denoise_atrous*),
on the CPU: a literal brute force over levels, pixels and taps, the three exact identities of the definition, a constant film, and
the quality bounds on the synthetic film of tests/nlm_regress_ref.py. No GPU."""
import itertools

import numpy as np
import pytest

import atrous_ref as A
import nlm_guided_ref as NG
import nlm_regress_ref as NR
from test_nlm_demod_ref import albedo_features
from test_nlm_ref import noisy_film

GROUP_SETS = {0: [], 1: [(3, 3, 1e-3)], 2: [(3, 3, 1e-3), (6, 1, 5e-2)]}
DEMOD = (0, 7, 1e-3)
SUMS = ("sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out")


def planted(w, h, seed):
    """NaN, +-Inf and a negative variance in img, var, a channel the groups name (4, 6) and the albedo (1, 0), where the film has room."""
    img, var = noisy_film(w, h, seed)
    feat, fvar = albedo_features(w, h, seed)
    img[0, 0, 1] = np.nan
    var[h - 1, w - 1, 0] = np.inf
    if w > 2:
        var[h // 2, 1, 2] = -1e-4
        img[h - 1, w // 2, 0] = -np.inf
        feat[4, h // 2, w - 2] = -np.inf
        fvar[6, 0, w // 2] = -1e-6
        feat[1, h - 1, 1] = np.nan
        fvar[0, 1, w - 1] = np.inf
    return img, var, feat, fvar


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("out", "var_out")) and \
        all(a[k] == b[k] for k in ("left_out",) + SUMS)


SMALL = list(itertools.product([(1, 1), (5, 3), (9, 7)], (1, 2, 3), (0, 1, 2), (False, True), (False, True)))
# 21 x 13: the taps of step 4 reach +-8 pixels inside the film
LARGE = [((21, 13), 3, 0, False, True), ((21, 13), 3, 2, True, True), ((21, 13), 3, 1, True, False), ((21, 13), 2, 2, False, False)]


@pytest.mark.parametrize("film,levels,ng,demod,plant", SMALL + LARGE, ids=lambda v: str(v).replace(" ", ""))
def test_brute_force_agrees(film, levels, ng, demod, plant):
    w, h = film
    if plant:
        img, var, feat, fvar = planted(w, h, 3 + levels)
    else:
        (img, var), (feat, fvar) = noisy_film(w, h, 3 + levels), albedo_features(w, h, 3 + levels)
    kw = dict(groups=GROUP_SETS[ng], demod=DEMOD if demod else None, levels=levels, k=1.0)
    a, b = A.denoise(img, var, feat, fvar, **kw), A.brute_force(img, var, feat, fvar, **kw)
    ok = A.valid_mask(img, var, feat, fvar, GROUP_SETS[ng], DEMOD if demod else None)
    assert a["left_out"] == b["left_out"] == (~ok).sum()
    if plant:
        assert a["left_out"] >= 1
        if w > 2:                         # what the feature planes hold counts exactly when a group or the demod block names it
            assert a["left_out"] == 4 + (1 if ng >= 1 else 0) + (1 if ng == 2 else 0) + (2 if demod else 0)
    for key, src in (("out", img), ("var_out", var)):
        assert np.array_equal(a[key][~ok], src[~ok], equal_nan=True) and np.array_equal(b[key][~ok], src[~ok], equal_nan=True)
        if ok.any():
            err = np.linalg.norm(a[key][ok] - b[key][ok]) / np.linalg.norm(b[key][ok])
            assert err < 1e-13, (key, err)
    for key in SUMS:
        assert abs(a[key] - b[key]) <= 1e-13 * abs(b[key])
    if ok.sum() > 1:
        assert not np.allclose(a["out"][ok], img[ok], rtol=1e-6)          # the filter is at work


def test_first_level_and_the_parameters_reach_the_brute_force():
    img, var, feat, fvar = planted(21, 13, 9)
    kw = dict(groups=GROUP_SETS[1], levels=2, first_level=1, k=0.7, alpha=0.5, eps=1e-6, k_f=0.9, alpha_f=0.3)
    a, b = A.denoise(img, var, feat, fvar, **kw), A.brute_force(img, var, feat, fvar, **kw)
    ok = A.valid_mask(img, var, feat, fvar, GROUP_SETS[1])
    for key in ("out", "var_out"):
        assert np.linalg.norm(a[key][ok] - b[key][ok]) / np.linalg.norm(b[key][ok]) < 1e-13
    for other in (dict(first_level=0), dict(k=0.8), dict(alpha=0.6), dict(eps=1e-3), dict(k_f=1.0), dict(alpha_f=0.4), dict(levels=3)):
        assert not np.array_equal(A.denoise(img, var, feat, fvar, **{**kw, **other})["out"], a["out"], equal_nan=True), other


@pytest.mark.parametrize("ng", [0, 2])
def test_n_levels_are_n_calls_of_one_level_bit_for_bit(ng):
    img, var, feat, fvar = planted(40, 19, 2)
    for levels, first in ((5, 0), (3, 2), (6, 0)):
        whole = A.denoise(img, var, feat, fvar, GROUP_SETS[ng], levels=levels, first_level=first, k=1.0)
        u, v = img, var
        for i in range(levels):
            step = A.denoise(u, v, feat, fvar, GROUP_SETS[ng], levels=1, first_level=first + i, k=1.0)
            u, v = step["out"], step["var_out"]
        assert np.array_equal(u, whole["out"], equal_nan=True) and np.array_equal(v, whole["var_out"], equal_nan=True)
        assert all(step[k] == whole[k] for k in ("left_out", "sum_var_out", "sum_sq_out"))


def test_no_group_or_constant_noise_free_features_are_the_unguided_filter_bit_for_bit():
    img, var, feat, fvar = planted(19, 13, 4)
    plain = A.denoise(img, var, levels=4)
    assert same_bits(A.denoise(img, var, feat, fvar, [], levels=4), plain)
    flat = np.stack([np.full((13, 19), 0.1 * (c + 1)) for c in range(8)])
    for groups in (GROUP_SETS[1], GROUP_SETS[2]):
        assert same_bits(A.denoise(img, var, flat, np.zeros_like(flat), groups, levels=4), plain)
        assert not same_bits(A.denoise(img, var, feat, fvar, groups, levels=4), plain)


@pytest.mark.parametrize("ng", [0, 2])
def test_a_unit_divisor_is_the_undemodulated_filter_bit_for_bit(ng):
    img, var = noisy_film(19, 13, 5)
    img[3, 4, 2] = np.nan
    feat, fvar = albedo_features(19, 13, 5)
    plain = A.denoise(img, var, feat, fvar, GROUP_SETS[ng], levels=4)
    for albedo, cov, channel in ((1.0, 1.0, 7), (0.0, 0.0, 7), (1.0, 0.3, -1)):
        ft = feat.copy()
        ft[0:3], ft[7] = albedo, cov
        assert same_bits(A.denoise(img, var, ft, fvar, GROUP_SETS[ng], (0, channel, 1e-3), levels=4), plain)
    assert not same_bits(A.denoise(img, var, feat, fvar, GROUP_SETS[ng], DEMOD, levels=4), plain)


def test_a_constant_film_comes_back_constant():
    h, w = 13, 21
    img = np.ones((h, w, 3)) * np.array([0.7, 0.4, 0.1])
    _, var = noisy_film(w, h, 6)
    feat, fvar = albedo_features(w, h, 6)
    for groups, demod in (([], None), (GROUP_SETS[2], None)):
        res = A.denoise(img, var, feat, fvar, groups, demod, levels=5)
        assert np.abs(res["out"] - img).max() <= 1e-13 * 0.7
        assert (res["var_out"] > 0).all() and (res["var_out"] < var.max()).all()
    # demodulated: the quotient is constant where the film is the albedo times a constant
    al = np.moveaxis(feat[0:3], 0, 2)
    res = A.denoise(0.5 * al, var, feat, fvar, GROUP_SETS[1], (0, -1, 1e-3), levels=5)
    assert np.abs(res["out"] - 0.5 * al).max() <= 1e-13


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


@pytest.mark.parametrize("seed", range(5))
def test_quality_on_the_synthetic_film(seed):
    """At the defaults (k = 2, 5 levels). Measured, seeds 0 - 4: guided by albedo and normal 0.0311, 0.0310, 0.0312, 0.0299, 0.0308
    against the noisy mean's 0.0928, 0.0914, 0.0930, 0.0901, 0.0920; demodulated under the normal guide 0.0208, 0.0215, 0.0208, 0.0191,
    0.0199."""
    truth, mean, var, feat, fvar = NR.synthetic_regression(seed)
    both = [(0, 3, 1e-3), (3, 3, 1e-3)]
    noisy = rmse(mean, truth)
    guided = rmse(A.denoise(mean, var, feat, fvar, both)["out"], truth)
    nlm = rmse(NG.denoise(mean, var, feat, fvar, both, k=1.0)["out"], truth)
    demod = rmse(A.denoise(mean, var, feat, fvar, [(3, 3, 1e-3)], (0, -1, 1e-3))["out"], truth)
    print(f"seed {seed}: noisy {noisy:.4f}, a-trous guided {guided:.4f} (x{guided / noisy:.3f}), guided nlm at k = 1 {nlm:.4f} (x{guided / nlm:.3f} of it), "
          f"a-trous demodulated {demod:.4f} (x{demod / noisy:.3f})")
    assert guided <= 0.40 * noisy
    assert guided <= 0.90 * nlm
    assert demod <= 0.28 * noisy
