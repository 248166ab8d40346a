"""Pins tests/filter_select_ref.py, the numpy restatement of the per-pixel filter selection (include/gdpt.h: gdpt_filter_select*), on
the CPU: a literal brute force by pixel, candidate and tap, clean and with a non-finite value planted in each kind of input, the five
exact identities of the definition, and the quality of the selection among six restated filters on the synthetic film of
tests/nlm_regress_ref.py. No GPU."""
import itertools

import numpy as np
import pytest

import atrous_ref as A
import filter_select_ref as FS
import nlm_regress_ref as NR
import var_smooth_ref as VS

FILMS = [(1, 1), (5, 3), (9, 7), (21, 13)]
CASES = list(itertools.product(FILMS, (1, 2, 3), (0, 1, 4, 8)))


def close(a, b, tol=1e-12):
    """E of the two restatements: the same NaNs, and finite values within tol of the film's largest magnitude (the brute force adds
    the window row-major, the restatement separably)."""
    assert np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(a)
    scale = max(1e-300, np.abs(a[m]).max()) if m.any() else 1.0
    assert (np.abs(a[m] - b[m]) <= tol * scale).all()


def agree(a, b, n):
    """select() against brute_force(): E close; the exact parts equal wherever the two smallest E of the restatement are not within
    the tolerance of each other."""
    close(a["E"], b["E"])
    assert np.array_equal(a["e"], b["e"]) and a["left_out"] == b["left_out"] and a["sum_e"] == b["sum_e"]
    ok = a["sel"] >= 0
    assert np.array_equal(ok, b["sel"] >= 0)
    clear = ok.copy()
    if n > 1 and ok.any():
        srt = np.sort(np.where(ok[None], a["E"], 0.0), axis=0)
        clear &= (srt[1] - srt[0]) > 1e-11 * np.abs(a["E"][:, ok]).max()
    assert clear[ok].mean() >= 0.99 if ok.any() else True
    assert np.array_equal(a["sel"][clear], b["sel"][clear]) and np.array_equal(a["out"][clear], b["out"][clear])
    assert np.array_equal(a["sel"][~ok], b["sel"][~ok]) and np.array_equal(a["out"][~ok], b["out"][~ok], equal_nan=True)
    for d in (a, b):                                         # each is consistent with its own E, exactly
        E = np.where(ok[None], d["E"], np.inf)
        assert np.array_equal(d["sel"][ok], np.argmin(E, axis=0)[ok])
        assert np.array_equal(d["mse"][ok], np.min(E, axis=0)[ok]) and np.isnan(d["mse"][~ok]).all()
        assert sum(d["chosen"]) == ok.sum()


@pytest.mark.parametrize("film,n,s", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_brute_force_agrees(film, n, s):
    w, h = film
    clean = FS.fields(w, h, n, 100 * w + h)
    a, b = FS.select(*clean, radius=s), FS.brute_force(*clean, radius=s)
    assert a["left_out"] == 0
    agree(a, b, n)
    for i, kind in enumerate(FS.KINDS):
        dirty = FS.plant(clean, kind, 7 + i)
        a, b = FS.select(*dirty, radius=s), FS.brute_force(*dirty, radius=s)
        assert 1 <= a["left_out"] <= 3, kind
        agree(a, b, n)
        bad = a["sel"] < 0
        assert np.array_equal(a["out"][bad], dirty[2][0][bad], equal_nan=True) and np.isnan(a["E"][:, bad]).all()


def identities(select, w, h, s, seed):
    """The five identities of include/gdpt.h, bit for bit, on `select` (the restatement's signature): shared with the GPU test."""
    FA, FB, T, uA, vA, uB, vB = FS.plant(FS.fields(w, h, 3, seed), "uB", seed)
    half = (uA, vA, uB, vB)
    base = select(FA, FB, T, *half, radius=s)
    ok = base["sel"] >= 0
    assert (~ok).any() and base["left_out"] == (~ok).sum()
    # n = 1 returns T[0]
    one = select(FA[:1], FB[:1], T[:1], *half, radius=s)
    assert np.array_equal(one["out"], T[0], equal_nan=True) and (one["sel"][ok] == 0).all() and (one["sel"][~ok] == -1).all()
    # a candidate listed twice never loses to its copy
    twice = select(FA + FA[1:2], FB + FB[1:2], T + [T[1] + 1.0], *half, radius=s)
    assert (twice["sel"] != 3).all() and np.array_equal(twice["sel"], base["sel"]) and np.array_equal(twice["out"], base["out"], equal_nan=True)
    assert np.array_equal(twice["E"][3], twice["E"][1], equal_nan=True)
    # permuting the candidates permutes sel and leaves out alone (continuous inputs: no two E_j are equal)
    perm = [2, 0, 1]
    moved = select([FA[i] for i in perm], [FB[i] for i in perm], [T[i] for i in perm], *half, radius=s)
    assert np.array_equal(np.array(perm)[moved["sel"][ok]], base["sel"][ok]) and np.array_equal(moved["out"][ok], base["out"][ok])
    assert np.array_equal(moved["out"][~ok], T[perm[0]][~ok], equal_nan=True)      # (an invalid pixel takes the first candidate listed)
    assert np.array_equal(moved["mse"], base["mse"], equal_nan=True)
    # s = 0 gives E = e
    if s == 0:
        assert np.array_equal(base["E"][:, ok], FS.select(FA, FB, T, *half, radius=0)["e"][:, ok])
    # every image times 2^m and every variance times 4^m: sel alone, mse times 4^m
    for m in (3, -5):
        f, f2 = 2.0 ** m, 4.0 ** m
        scaled = select([a * f for a in FA], [a * f for a in FB], [a * f for a in T], uA * f, vA * f2, uB * f, vB * f2, radius=s)
        assert np.array_equal(scaled["sel"], base["sel"]) and np.array_equal(scaled["mse"], base["mse"] * f2, equal_nan=True)
        assert np.array_equal(scaled["out"], base["out"] * f, equal_nan=True)
    return base


@pytest.mark.parametrize("s", [0, 1, 4, 8])
def test_exact_identities_bit_for_bit(s):
    identities(FS.select, 21, 13, s, 5)


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def half_films(seed, passes):
    """The prototype's generator: `passes` passes truth + 0.25 sqrt(truth) N(0, 1) on the film of nlm_regress_ref; half A the even
    passes, half B the odd ones, and the total; each (mean, box mean at radius 2 of the variance of the mean)."""
    truth, _, _, feat, fvar = NR.synthetic_regression(seed)
    rng = np.random.default_rng(1000 + seed)
    p = np.stack([truth + 0.25 * np.sqrt(truth) * rng.standard_normal(truth.shape) for _ in range(passes)])

    def part(q):
        mean, var = q.mean(axis=0), q.var(axis=0, ddof=1) / len(q)
        return mean, VS.smooth(mean, var, 2)["var_out"]
    return truth, feat, fvar, part(p[0::2]), part(p[1::2]), part(p)


def candidates(mean, var, feat, fvar, regression=True):
    """The six candidates of DESIGN.md 4.14, in its order; without the last with regression=False."""
    both, normal = [(0, 3, 1e-3), (3, 3, 1e-3)], [(3, 3, 1e-3)]
    five = [mean,
            A.denoise(mean, var, feat, fvar, both)["out"],
            A.denoise(mean, var, feat, fvar, normal, (0, -1, 1e-3), levels=5)["out"],
            A.denoise(mean, var, feat, fvar, normal, (0, -1, 1e-3), levels=3)["out"],
            A.denoise(mean, var)["out"]]
    if not regression:
        return five
    return five + [NR.denoise(mean, var, feat, fvar, [(0, 3, 1e-3)], list(range(7)), ridge=1e-2, r=10, f=3, k=4.0)["out"]]


@pytest.mark.parametrize("passes", [4, 8, 16])
@pytest.mark.parametrize("seed", range(5))
def test_quality_on_the_synthetic_film(seed, passes):
    """Six candidates, selected at radius 4 and at radius 0, against the best single candidate on the total.
    The proposal's prototype had the selection at 0.74 - 0.82 of the best single candidate and set the bound 0.90. The committed
    restatements draw differently: here the regression is the best single candidate at every pass count (0.0138 - 0.0153 at 4 passes,
    0.0117 - 0.0129 at 8, 0.0102 - 0.0112 at 16, where the prototype had 0.0199 - 0.0213, 0.0175 - 0.0184, 0.0149 - 0.0155) and wins
    68 - 86 % of the pixels, and the selection does NOT beat it: measured over seeds 0 - 4 and 4, 8, 16 passes, selected at s = 4 /
    best single = 1.007 - 1.130 (RMSE 0.0140 - 0.0158, 0.0125 - 0.0136, 0.0106 - 0.0118), below every other candidate's (0.0149 at the least).
    By the proposal's rule for this case the bound is the measured worst + 0.08 = 1.21. Selected at s = 0 is 2.61 - 4.00 of the best
    single candidate, so s = 4 < s = 0 holds with a wide margin."""
    truth, feat, fvar, a, b, t = half_films(seed, passes)
    FA, FB, T = (candidates(*h, feat, fvar) for h in (a, b, t))
    single = [rmse(x, truth) for x in T]
    s4 = FS.select(FA, FB, T, a[0], a[1], b[0], b[1], radius=4)
    s0 = FS.select(FA, FB, T, a[0], a[1], b[0], b[1], radius=0)
    r4, r0, best = rmse(s4["out"], truth), rmse(s0["out"], truth), min(single)
    print(f"seed {seed}, {passes} passes: single {' '.join(f'{x:.4f}' for x in single)}; selected s=4 {r4:.4f} (x{r4 / best:.3f} of the best), "
          f"s=0 {r0:.4f} (x{r0 / best:.3f}); won {s4['chosen']}; sum_mse {s4['sum_mse']:.3e}")
    assert s4["left_out"] == 0
    assert r4 <= 1.21 * best
    assert r4 < r0


@pytest.mark.parametrize("passes", [4, 8, 16])
@pytest.mark.parametrize("seed", range(5))
def test_quality_without_the_dominant_candidate(seed, passes):
    """The same film with the regression taken out of the bank, so that no candidate dominates (the three guided a-trous candidates
    lie within 25 % of each other). Measured over seeds 0 - 4 and 4, 8, 16 passes: selected at s = 4 / best single = 0.916 - 1.032
    (below 1 in 10 of the 15 runs), selected at s = 0 = 1.89 - 2.58. So here the selection is level with the best single candidate,
    with a gain of a few per cent more often than a loss; the gain of a fifth that the proposal's prototype reported is not shown on
    this film either. No bound on the ratio to the best candidate is asserted, because none follows from the definition: asserted is
    what a selector must do to be of any use without knowing the best candidate, namely beat the bank's median candidate, and the
    proposal's s = 4 < s = 0."""
    truth, feat, fvar, a, b, t = half_films(seed, passes)
    FA, FB, T = (candidates(*h, feat, fvar, regression=False) for h in (a, b, t))
    single = [rmse(x, truth) for x in T]
    r4, r0 = (rmse(FS.select(FA, FB, T, a[0], a[1], b[0], b[1], radius=s)["out"], truth) for s in (4, 0))
    print(f"seed {seed}, {passes} passes, no regression: single {' '.join(f'{x:.4f}' for x in single)}; selected s=4 {r4:.4f} "
          f"(x{r4 / min(single):.3f} of the best), s=0 x{r0 / min(single):.3f}")
    assert r4 < float(np.median(single))
    assert r4 < r0
