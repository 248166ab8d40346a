"""Pins tests/nlm_guided_ref.py, the numpy restatement of the feature-guided non-local-means filter (include/gdpt.h:
gdpt_denoise_nlm_guided*), on the CPU: a literal brute force, its identities with the unguided restatement (tests/nlm_ref.py), what
it leaves out, and what the guide buys on a textured synthetic film."""
import numpy as np
import pytest

import nlm_guided_ref as NG
import nlm_ref as N
from test_nlm_ref import noisy_film

GROUP_SETS = {0: [], 1: [(0, 3, 1e-3)], 3: [(0, 3, 1e-3), (3, 3, 2e-3), (6, 1, 5e-2)]}
PLANTED = (np.nan, np.inf, -np.inf)


def noisy_features(w, h, seed, channels=8, sigma=0.03):
    """Planes that vary over the film on the scale of their stated variances, so that the feature weights lie between 0 and 1."""
    rng = np.random.default_rng(1000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    feat = np.stack([0.5 + 0.05 * np.sin(0.9 * x + 0.4 * c) * np.cos(0.6 * y - 0.2 * c) for c in range(channels)])
    feat = feat + sigma * rng.standard_normal(feat.shape)
    fvar = sigma * sigma * rng.uniform(0.25, 1.0, feat.shape)
    return feat, fvar


@pytest.mark.parametrize("ngroups", [0, 1, 3])
@pytest.mark.parametrize("r,f", [(0, 0), (2, 1), (3, 2)])
@pytest.mark.parametrize("w,h", [(9, 7), (17, 17)])
def test_brute_force_agrees(w, h, r, f, ngroups):
    img, var = noisy_film(w, h, 7 + r)
    feat, fvar = noisy_features(w, h, r)
    img[h // 2, w // 2, 0] = np.inf
    fvar[1, 0, w - 1] = -1.0                 # channel 1 is used by every group set but the empty one
    groups = GROUP_SETS[ngroups]
    a = NG.denoise(img, var, feat, fvar, groups, r=r, f=f, k=0.8)
    b = NG.brute_force(img, var, feat, fvar, groups, r=r, f=f, k=0.8)
    ok = NG.valid_mask(img, var, feat, fvar, groups)
    assert a["left_out"] == b["left_out"] == (2 if ngroups else 1)
    assert np.array_equal(a["out"][~ok], b["out"][~ok], equal_nan=True)
    for key in ("out", "var_out"):
        assert np.abs(a[key][ok] - b[key][ok]).max() <= 1e-12 * np.abs(b[key][ok]).max(), key
    for key in ("sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out"):
        assert abs(a[key] - b[key]) <= 1e-12 * abs(b[key])
    if ngroups and r:
        plain = N.denoise(img, var, r=r, f=f, k=0.8)
        okp = ok & N.valid_mask(img, var)
        assert np.abs(a["out"][okp] - plain["out"][okp]).max() > 1e-4       # the guide is at work on this film


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("out", "var_out")) and \
        all(a[k] == b[k] for k in ("left_out", "sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out"))


def test_zero_groups_is_the_unguided_filter_bit_for_bit():
    img, var = noisy_film(19, 13, 3)
    img[2, 3, 1] = np.nan
    feat, fvar = noisy_features(19, 13, 3)
    feat[0, 5, 5] = np.nan                   # no group names it
    for (r, f) in ((0, 0), (3, 1), (5, 3)):
        assert same_bits(NG.denoise(img, var, feat, fvar, [], r=r, f=f), N.denoise(img, var, r=r, f=f))
        assert same_bits(NG.denoise(img, var, None, None, [], r=r, f=f), N.denoise(img, var, r=r, f=f))


def test_constant_noise_free_features_are_the_unguided_filter_bit_for_bit():
    img, var = noisy_film(19, 13, 4)
    var[6, 6, 2] = -1.0
    feat = np.stack([np.full((13, 19), 0.1 * (c + 1)) for c in range(8)])
    fvar = np.zeros_like(feat)
    for groups in (GROUP_SETS[1], GROUP_SETS[3]):
        assert same_bits(NG.denoise(img, var, feat, fvar, groups, r=4, f=2, k=0.7), N.denoise(img, var, r=4, f=2, k=0.7))


def step_films(w=20, h=12):
    """Two colour films that agree left of column w / 2 and differ right of it (by amounts the colour weights survive), a noise-free
    feature that steps from 0 to 1 there, and the mask of the left side."""
    img, var = noisy_film(w, h, 5, sigma=0.2)
    other = img.copy()
    other[:, w // 2:] = 1.1 * img[::-1, w // 2:] + 0.05
    feat = np.zeros((1, h, w))
    feat[0, :, w // 2:] = 1.0
    left = np.zeros((h, w), dtype=bool)
    left[:, :w // 2] = True
    return img, other, var, feat, np.zeros_like(feat), left


def test_a_feature_step_separates_the_two_sides_whatever_the_colours():
    """A step of height 1 in a noise-free feature (tau 1e-3, k_f 0.6): phi = 1 / (0.36 x 1e-3) across it, and exp(-2778) underflows
    to 0. With pixel-wise colour distances (f = 0) the left side's output then is a function of the left side alone: the same bits
    whatever colours the right side holds. The unguided filter does see them."""
    img, other, var, feat, fvar, left = step_films()
    kw = dict(r=6, f=0, k=1.0)
    assert np.exp(-1.0 / (0.36 * 1e-3)) == 0.0
    a = NG.denoise(img, var, feat, fvar, [(0, 1, 1e-3)], k_f=0.6, **kw)
    b = NG.denoise(other, var, feat, fvar, [(0, 1, 1e-3)], k_f=0.6, **kw)
    assert np.array_equal(a["out"][left], b["out"][left]) and np.array_equal(a["var_out"][left], b["var_out"][left])
    assert not np.array_equal(a["out"][~left], b["out"][~left])
    pa, pb = N.denoise(img, var, **kw), N.denoise(other, var, **kw)
    near = left.copy()
    near[:, :left.shape[1] // 2 - 6] = False
    assert (pa["out"][near] != pb["out"][near]).all()


@pytest.mark.parametrize("bad", PLANTED + ("negvar",), ids=["nan", "inf", "-inf", "negvar"])
def test_an_invalid_used_feature_leaves_the_pixel_out(bad):
    w, h = 14, 11
    img, var = noisy_film(w, h, 6)
    feat, fvar = noisy_features(w, h, 6)
    groups = GROUP_SETS[3]
    spots = ((0, 0, 0), (4, 0, 7), (6, 5, 5), (2, h - 1, w - 1))     # (channel, y, x)
    for n, (c, y, x) in enumerate(spots):
        if bad == "negvar":
            fvar[c, y, x] = -1e-6
        elif n % 2:
            fvar[c, y, x] = bad if bad != -np.inf else np.inf
        else:
            feat[c, y, x] = bad
    if bad == -np.inf:
        fvar[3, 2, 2] = -np.inf
        spots = spots + ((3, 2, 2),)
    d = NG.denoise(img, var, feat, fvar, groups, r=3, f=1, k=0.8)
    assert d["left_out"] == len(spots)
    for (_, y, x) in spots:
        assert np.array_equal(d["out"][y, x], img[y, x]) and np.array_equal(d["var_out"][y, x], var[y, x])
    assert np.isfinite(d["out"]).all() and np.isfinite(d["var_out"]).all()
    assert np.isfinite([d[k] for k in ("sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out", "error_in", "error_out")]).all()


def test_an_invalid_feature_no_group_names_changes_nothing():
    w, h = 14, 11
    img, var = noisy_film(w, h, 8)
    feat, fvar = noisy_features(w, h, 8)
    groups = [(0, 3, 1e-3), (5, 2, 1e-3)]              # channels 3, 4 and 7 are named by no group
    clean = NG.denoise(img, var, feat, fvar, groups, r=3, f=1, k=0.8)
    for n, bad in enumerate(PLANTED):
        feat[3, n, n] = bad
        fvar[4, h - 1 - n, n] = bad
    fvar[7, 5, 5] = -1.0
    d = NG.denoise(img, var, feat, fvar, groups, r=3, f=1, k=0.8)
    assert d["left_out"] == 0 and same_bits(d, clean)


def test_the_guide_keeps_a_texture_the_colour_filter_smooths_away():
    """The film of tests/nlm_ref.py under a 15 % albedo checker of 3 x 3 pixel cells, carried by a nearly noise-free albedo. At colour
    k = 1.0 the guided RMSE is at most 0.85 of the unguided one at the same k, for each of five seeds. Measured: 0.711 - 0.737."""
    ratios = []
    for seed in range(5):
        truth, mean, var, feat, fvar = NG.synthetic_textured(seed)
        guided = NG.denoise(mean, var, feat, fvar, [(0, 3, 1e-3)], k_f=0.6, alpha_f=1.0, r=10, f=3, k=1.0, alpha=1.0, eps=1e-10)
        plain = N.denoise(mean, var, r=10, f=3, k=1.0, alpha=1.0, eps=1e-10)
        rg, rp = np.sqrt(((guided["out"] - truth) ** 2).mean()), np.sqrt(((plain["out"] - truth) ** 2).mean())
        print(f"seed {seed}: RMSE unguided {rp:.4f}, guided {rg:.4f} (x{rg / rp:.3f})")
        ratios.append(rg / rp)
        assert guided["left_out"] == 0
    assert all(q <= 0.85 for q in ratios), ratios
