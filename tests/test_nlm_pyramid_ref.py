"""The numpy restatement of the multi-scale non-local-means filters (tests/nlm_pyramid_ref.py) pinned: the two operators against a
per-pixel double loop, the exact properties of the definition bit for bit, planted values, and the quality claim of DESIGN.md 4.11:
two levels against one on the 96 x 128 film, seeds 0 - 4. No GPU."""
import numpy as np
import pytest

import nlm_pyramid_ref as P
import var_smooth_ref as VS
from test_nlm_demod_ref import albedo_features
from test_nlm_ref import noisy_film
from test_var_smooth_ref import planted

FILMS = [(1, 1), (2, 2), (3, 3), (1, 7), (7, 1), (17, 9)]      # W x H
# every kind; "demod" without and with a coverage plane, without and with a guide
KINDS = {"plain": P.kind_args("plain"), "guided": P.kind_args("guided"), "demod": P.kind_args("demod", coverage_channel=-1),
         "demod-cov-guide": P.kind_args("demod", groups=[(3, 3, 1e-3)], coverage_channel=7)}


def level(ka, w, h, seed, dirty):
    """(img, var, feat, fvar) of one level, clean or planted; a planted film of 4 x 4 or more also has a whole 2 x 2 cell invalid."""
    img, var, feat, fvar = planted(w, h, seed) if dirty else noisy_film(w, h, seed) + albedo_features(w, h, seed)
    if dirty and w >= 4 and h >= 4:
        y0, x0 = 2 * ((h - 1) // 4), 2 * ((w - 1) // 4)
        img[y0, x0, 0], var[y0, x0 + 1, 1], img[y0 + 1, x0, 2], var[y0 + 1, x0 + 1, 0] = np.nan, -1.0, np.inf, -np.inf
    return (img, var, None, None) if ka["kind"] == "plain" else (img, var, feat, fvar)


def same(a, b):
    return (a is None and b is None) or np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "planted"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_down_and_up_against_the_double_loop(kind, dirty):
    ka = KINDS[kind]
    for (w, h) in FILMS:
        lv = level(ka, w, h, 10 * w + h, dirty)
        ok = P.valid_mask(ka, *lv)
        got, want = P.down(ka, *lv), P.brute_down(ka, *lv)
        assert all(same(g, b) for g, b in zip(got, want)), (w, h)
        img2, var2, feat2, fvar2, n = got
        assert img2.shape == ((h + 1) // 2, (w + 1) // 2, 3) and n.sum() == ok.sum()
        assert np.array_equal(np.isnan(img2).all(axis=2), n == 0) and np.array_equal(np.isnan(var2).any(axis=2), n == 0)
        # a coarse pixel without a valid fine pixel is invalid for the kind, every other one valid: no mask is carried
        assert np.array_equal(P.valid_mask(ka, img2, var2, feat2, fvar2), n > 0), (w, h)
        rng = np.random.default_rng(w + 100 * h)
        F = np.where(ok[:, :, None], lv[0] + 0.01 * rng.standard_normal(lv[0].shape), lv[0])
        coarse = np.where((n > 0)[:, :, None], img2 + 0.01 * rng.standard_normal(img2.shape), np.nan)
        out, want = P.up(ka, *lv, F, coarse), P.brute_up(ka, *lv, F, coarse)
        assert same(out, want), (w, h)
        assert same(out[~ok], lv[0][~ok]) and np.isfinite(out[ok]).all(), (w, h)
        if ok.any():
            assert not same(out, F)


def test_a_whole_cell_invalid_has_no_correction_and_keeps_its_bits():
    ka = KINDS["plain"]
    img, var, _, _ = level(ka, 17, 9, 3, True)
    ok = P.valid_mask(ka, img, var)
    n = P.down(ka, img, var)[4]
    Y, X = (9 - 1) // 4, (17 - 1) // 4                    # the cell level() plants; the film's last pixel is a cell of its own, also invalid
    assert n[Y, X] == 0 and n[4, 8] == 0 and (n == 0).sum() == 2 and (n[n > 0] < 4).any()
    F = np.where(ok[:, :, None], img + 1.0, img)
    coarse = np.where((n > 0)[:, :, None], 5.0, np.nan)
    R = P.correction(ok, F, coarse)
    assert np.array_equal(R[Y, X], [0.0, 0.0, 0.0]) and np.isfinite(R).all()
    out = P.up(ka, img, var, None, None, F, coarse)
    assert same(out[2 * Y:2 * Y + 2, 2 * X:2 * X + 2], img[2 * Y:2 * Y + 2, 2 * X:2 * X + 2])
    # the neighbours of the cell interpolate towards its R = 0: their correction is smaller than that of pixels far from it
    assert abs(out[2 * Y, 2 * X - 1, 0] - F[2 * Y, 2 * X - 1, 0]) < abs(out[2 * Y, 2 * X - 4, 0] - F[2 * Y, 2 * X - 4, 0])


@pytest.mark.parametrize("kind", list(KINDS))
def test_one_level_is_the_single_scale_filter_bit_for_bit(kind):
    ka = KINDS[kind]
    lv = level(ka, 17, 9, 5, True)
    one, ref = P.denoise(ka, *lv, levels=1, r=3, f=1), P.filter_level(ka, *lv, r=3, f=1)
    assert same(one["out"], ref["out"]) and same(one["var_out"], ref["var_out"]) and one["left_out"] == ref["left_out"] > 0
    assert one["levels"] == 1 and one["extents"] == [(9, 17)] and all(one["level"][0][k] == ref[k] for k in ("sum_var_in", "sum_sq_out"))
    two = P.denoise(ka, *lv, levels=2, r=3, f=1)
    assert same(two["var_out"], ref["var_out"]) and two["left_out"] == ref["left_out"] and not same(two["out"], ref["out"])
    assert same(P.denoise(ka, *lv, levels=2, r=3, f=1)["out"], two["out"])              # the same call gives the same bits


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_dyadic_constant_film_comes_back_unchanged_at_every_level_count(kind):
    ka = KINDS[kind]
    for (w, h) in ((17, 9), (7, 1), (1, 1)):
        _, _, feat, fvar = level(ka, w, h, 1, False)
        for value, variance in ((0.375, 2.0 ** -10), (-3.0, 0.0)):
            img, var = np.full((h, w, 3), value), np.full((h, w, 3), variance)
            if feat is not None:            # dyadic constant planes without variance: every weight is 1, the quotient and the product by the albedo exact
                feat[:], fvar[:], feat[7] = 0.5, 0.0, 1.0
            for levels in range(1, P.MAX_LEVELS + 1):
                d = P.denoise(ka, img, var, feat, fvar, levels=levels, r=2, f=1)
                assert np.array_equal(d["out"], img), (w, h, levels)
                assert d["levels"] == len(P.extents(h, w, levels)) <= levels


def test_the_levels_made_and_their_extents():
    assert P.extents(9, 17, 4) == [(9, 17), (5, 9), (3, 5), (2, 3)] and P.extents(9, 17, 1) == [(9, 17)]
    assert P.extents(1, 7, 4) == [(1, 7), (1, 4), (1, 2), (1, 1)] and P.extents(2, 2, 4) == [(2, 2), (1, 1)] and P.extents(1, 1, 4) == [(1, 1)]
    for bad in (0, 5):
        with pytest.raises(ValueError):
            P.denoise(KINDS["plain"], np.ones((2, 2, 3)), np.ones((2, 2, 3)), levels=bad)


# The claim of DESIGN.md 4.11, as this restatement measures it on seeds 0 - 4 (K = 4 passes, variance box-smoothed at s = 2, the
# filter's defaults): the ratio two levels / one level of the low-frequency RMSE is 0.654 - 0.767, of the full-resolution RMSE
# 0.938 - 0.969. The bounds are those of the proposal, which every seed passes with the reference alone.
LOW_FREQUENCY_BOUND, FULL_RESOLUTION_BOUND = 0.85, 1.0


def test_two_levels_remove_low_frequency_noise_one_level_cannot_reach():
    tr = P.truth(96, 128)
    ka = KINDS["plain"]
    lows, fulls = [], []
    for seed in range(5):
        img, var = P.passes(tr, seed, 4)
        sm = VS.smooth(img, var, 2)["var_out"]
        one, two = (P.denoise(ka, img, sm, levels=levels)["out"] for levels in (1, 2))
        lows.append(P.low_frequency_rmse(two, tr) / P.low_frequency_rmse(one, tr))
        fulls.append(P.rmse(two, tr) / P.rmse(one, tr))
        # today's filter leaves most of the low-frequency error in place: that is the weakness
        assert P.low_frequency_rmse(one, tr) > 0.8 * P.low_frequency_rmse(img, tr) and P.rmse(one, tr) < 0.25 * P.rmse(img, tr)
    print("two levels / one level, seeds 0 - 4: low-frequency RMSE " + " ".join(f"{v:.3f}" for v in lows) + "; full-resolution RMSE " +
          " ".join(f"{v:.3f}" for v in fulls))
    assert max(lows) <= LOW_FREQUENCY_BOUND and max(fulls) <= FULL_RESOLUTION_BOUND
