"""The numpy restatement of the joint non-local-means filter (tests/nlm_joint_ref.py; include/gdpt.h: gdpt_denoise_nlm_joint*) against
the definition read literally, its three exact identities, and what the joint filter buys on a synthetic gradient-domain film. CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nlm_guided_ref  # noqa: E402
import nlm_joint_ref as J  # noqa: E402
import nlm_ref  # noqa: E402

FILMS = [(1, 1), (5, 3), (9, 7), (21, 13)]
RADII = [(0, 0), (1, 0), (2, 1), (4, 3)]
COUNTS = [0, 1, 2, 4]
GROUPS = [(0, 2, 1e-3), (2, 1, 1e-2)]
FILTER = dict(k=0.7, alpha=1.0, eps=1e-10)
GUIDE = dict(k_f=0.6, alpha_f=1.0)


def film(w, h, seed, n=4):
    """A noisy step film with its variance, three feature planes with theirs, and n companions with theirs."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.where(x < w / 2, 0.3, 1.0)[:, :, None] * np.array([1.0, 0.8, 0.6])
    var = 0.01 * base * (0.5 + rng.random((h, w, 3)))
    img = base + np.sqrt(var) * rng.standard_normal((h, w, 3))
    feat = np.stack([np.where(x < w / 2, 0.2, 0.7), y / max(1, h - 1), 0.1 * x]) + 0.01 * rng.standard_normal((3, h, w))
    fvar = 1e-4 * (0.5 + rng.random((3, h, w)))
    comps = [0.2 * rng.standard_normal((h, w, 3)) + j for j in range(n)]
    comp_vars = [0.02 * (0.5 + rng.random((h, w, 3))) for _ in range(n)]
    return img, var, feat, fvar, comps, comp_vars


def run(fn, fl, n, guided, r, f):
    img, var, feat, fvar, comps, comp_vars = fl
    return fn(img, var, comps[:n], comp_vars[:n], feat if guided else None, fvar if guided else None, GROUPS if guided else (), r=r, f=f, **GUIDE,
              **FILTER)


def assert_close(res, ref, n, what):
    """The restatement sums in another association than the literal loops: a few ulps of sums of at most 81 positive terms."""
    tol = dict(rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(res["out"], ref["out"], err_msg=what, **tol)
    np.testing.assert_allclose(res["var_out"], ref["var_out"], err_msg=what, **tol)
    for j in range(n):
        np.testing.assert_allclose(res["comp_out"][j], ref["comp_out"][j], err_msg=f"{what} companion {j}", **tol)
        np.testing.assert_allclose(res["comp_var_out"][j], ref["comp_var_out"][j], err_msg=f"{what} companion variance {j}", **tol)
        for key in ("comp_sum_var_in", "comp_sum_var_out"):
            assert res[key][j] == pytest.approx(ref[key][j], rel=1e-11), (what, key, j)
    assert res["left_out"] == ref["left_out"], what
    for key in ("sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out"):
        assert res[key] == pytest.approx(ref[key], rel=1e-11, abs=1e-300), (what, key)


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("r,f", RADII)
@pytest.mark.parametrize("w,h", FILMS)
def test_restatement_matches_brute_force_clean(w, h, r, f, guided):
    """On a clean film every pixel is valid whatever n is, so one literal run with four companions is the reference of every count."""
    fl = film(w, h, 11 * w + h)
    ref = run(J.brute_force, fl, 4, guided, r, f)
    assert ref["left_out"] == 0
    for n in COUNTS:
        assert_close(run(J.denoise, fl, n, guided, r, f), ref, n, f"n={n}")


KINDS = ["img", "var", "feat", "fvar", "comp", "comp_var"]
# every film, radius pair and count appears; the literal loops at (4, 3) stay on the films where they take a second or two
PLANTED = [((1, 1), (1, 0), 1), ((5, 3), (0, 0), 2), ((5, 3), (4, 3), 4), ((9, 7), (2, 1), 1), ((9, 7), (4, 3), 2), ((21, 13), (1, 0), 4),
           ((21, 13), (2, 1), 2)]


def plant(fl, kind, n):
    """A non-finite value (value planes) or a negative and a non-finite variance (variance planes) in one kind of input, at two pixels;
    for the companions in the last of the n."""
    img, var, feat, fvar, comps, comp_vars = [np.copy(a) if isinstance(a, np.ndarray) else [np.copy(b) for b in a] for a in fl]
    h, w = img.shape[:2]
    p0, p1 = (h // 2, w // 2), (h - 1, 0)
    if kind == "img":
        img[p0][1] = np.nan; img[p1][0] = np.inf
    elif kind == "var":
        var[p0][2] = -1e-3; var[p1][0] = np.inf
    elif kind == "feat":
        feat[(1,) + p0] = np.nan; feat[(0,) + p1] = -np.inf
    elif kind == "fvar":
        fvar[(2,) + p0] = -1e-6; fvar[(0,) + p1] = np.nan
    elif kind == "comp":
        comps[n - 1][p0][0] = np.nan; comps[n - 1][p1][2] = np.inf
    else:
        comp_vars[n - 1][p0][1] = -1e-3; comp_vars[n - 1][p1][0] = np.nan
    return img, var, feat, fvar, comps, comp_vars


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("case", PLANTED, ids=lambda c: f"{c[0][0]}x{c[0][1]}-r{c[1][0]}f{c[1][1]}-n{c[2]}")
def test_restatement_matches_brute_force_planted(case, guided, kind):
    (w, h), (r, f), n = case
    fl = plant(film(w, h, 7 * w + h), kind, n)
    ref, res = run(J.brute_force, fl, n, guided, r, f), run(J.denoise, fl, n, guided, r, f)
    planted_counts = kind not in ("feat", "fvar") or guided          # (unguided: the feature planes are not read)
    assert ref["left_out"] == ((1 if w * h == 1 else 2) if planted_counts else 0)
    assert_close(res, ref, n, kind)
    # an invalid pixel keeps every input triple bit for bit
    img, var, _, _, comps, comp_vars = fl
    bad = ~J.valid_mask(img, var, comps[:n], comp_vars[:n], fl[2] if guided else None, fl[3] if guided else None, GROUPS if guided else ())
    assert int(bad.sum()) == ref["left_out"]
    for got, src in [(res["out"], img), (res["var_out"], var)] + list(zip(res["comp_out"], comps)) + list(zip(res["comp_var_out"], comp_vars)):
        assert got[bad].tobytes() == src[bad].tobytes()


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
def test_identity_valid_companions_change_nothing(guided):
    fl = film(21, 13, 5)
    img, var, feat, fvar, _, _ = fl
    ref = nlm_guided_ref.denoise(img, var, feat, fvar, GROUPS if guided else (), r=4, f=3, **GUIDE, **FILTER)
    for n in COUNTS:
        res = run(J.denoise, fl, n, guided, 4, 3)
        assert same_bits(res["out"], ref["out"]) and same_bits(res["var_out"], ref["var_out"])
        for key in ("left_out", "sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out", "error_in", "error_out"):
            assert res[key] == ref[key], (n, key)
    if not guided:
        plain = nlm_ref.denoise(img, var, r=4, f=3, **FILTER)
        res = run(J.denoise, fl, 2, False, 4, 3)
        assert same_bits(res["out"], plain["out"]) and same_bits(res["var_out"], plain["var_out"])


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
def test_identity_guide_film_as_companion(guided):
    img, var, feat, fvar, comps, comp_vars = film(21, 13, 6)
    res = J.denoise(img, var, [comps[0], img], [comp_vars[0], var], feat if guided else None, fvar if guided else None, GROUPS if guided else (),
                    r=4, f=3, **GUIDE, **FILTER)
    assert same_bits(res["comp_out"][1], res["out"]) and same_bits(res["comp_var_out"][1], res["var_out"])
    assert res["comp_sum_var_in"][1] == res["sum_var_in"] and res["comp_sum_var_out"][1] == res["sum_var_out"]


@pytest.mark.parametrize("f", [0, 3])
def test_identity_radius_zero_returns_every_input(f):
    fl = plant(film(9, 7, 8), "comp", 2)
    img, var, _, _, comps, comp_vars = fl
    res = run(J.denoise, fl, 2, True, 0, f)
    assert same_bits(res["out"], img) and same_bits(res["var_out"], var)
    for j in range(2):
        assert same_bits(res["comp_out"][j], comps[j]) and same_bits(res["comp_var_out"][j], comp_vars[j])


# Quality on synthetic_gradients, seeds 0 - 4, the filter at its defaults (10, 3, 0.45), unguided. R = RMSE(joint filter + L2
# reconstruction) / min(RMSE(plain L2 reconstruction), RMSE(NLM of the primal alone)), each reconstruction at the better of dataCost
# 0.04 and 1. MEASURED_WORST[(K, g)] is the worst R of the five seeds as measured with this file (DESIGN.md 4.15 has the table); the
# bound is that + 0.08, the project's margin for a generator that draws differently.
MEASURED_WORST = {(4, 0.3): 0.7066, (4, 1.0): 0.6387, (16, 0.3): 0.6396, (16, 1.0): 0.6074}
DATA_COSTS = (0.04, 1.0)


@pytest.mark.parametrize("K,g", sorted(MEASURED_WORST))
def test_joint_filter_beats_both_alternatives(K, g):
    worst = 0.0
    for seed in range(5):
        truth, (tgx, tgy), (c, gx, gy), (vc, vgx, vgy) = J.synthetic_gradients(seed, K, g)
        res = J.denoise(c, vc, [gx, gy], [vgx, vgy])
        fc, (fgx, fgy) = res["out"], res["comp_out"]
        plain = min(J.rmse(J.reconstruct(c, gx, gy, a), truth) for a in DATA_COSTS)
        joint = min(J.rmse(J.reconstruct(fc, fgx, fgy, a), truth) for a in DATA_COSTS)
        nlm_alone = J.rmse(fc, truth)
        ratio = joint / min(plain, nlm_alone)
        raw_g = np.sqrt(J.rmse(gx, tgx) ** 2 + J.rmse(gy, tgy) ** 2)
        fil_g = np.sqrt(J.rmse(fgx, tgx) ** 2 + J.rmse(fgy, tgy) ** 2)
        print(f"K={K} g={g} seed={seed}: mean {J.rmse(c, truth):.4f} plain {plain:.4f} nlm {nlm_alone:.4f} joint {joint:.4f} R {ratio:.4f} "
              f"gradients filtered/raw {fil_g / raw_g:.4f}")
        assert fil_g < raw_g
        worst = max(worst, ratio)
    assert worst <= MEASURED_WORST[(K, g)] + 0.08, worst
