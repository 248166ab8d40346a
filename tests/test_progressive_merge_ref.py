"""The merge of progressive sessions, restated in numpy (tests/progressive_merge_ref.py), against the fold it must equal
(tests/progressive_ref.py): no GPU. The merge of sessions over disjoint passes is the state of the one session that folded all of
them: same means, same M2, same error estimate, same left-out count."""
import numpy as np
import pytest

import progressive_merge_ref as M
import progressive_ref as R

H, W = 12, 20
TOL = 1e-13          # relative L2, means and M2: a handful of roundings per component (5 seeds of this case give <= 1.5e-16)


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def passes(seed, sizes):
    """Skewed non-negative pass means, five buffers: a pass of n samples is the mean of n draws of a gamma-distributed radiance with
    a few bright pixels (what a path tracer's pass looks like to the fold)."""
    rng = np.random.default_rng(seed)
    scale = rng.gamma(0.5, 2.0, size=(H, W, 3)) + 1e-3
    out = []
    for n in sizes:
        p = {}
        for k in R.BUFS:
            draws = rng.gamma(0.3, 1.0, size=(n, H, W, 3)) * scale
            m = draws.mean(axis=0)
            p[k] = m if k == "img" else m - scale * 0.3       # gradients take both signs
        out.append(p)
    return out


GROUPS = [
    ([1, 2, 4], [4, 5]),
    ([1, 2, 4], [4], [5]),
    ([3], [1, 1], [2, 7, 1]),
]


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("groups", GROUPS)
def test_merge_of_folds_is_the_fold_of_all_passes(seed, groups):
    sizes = [n for g in groups for n in g]
    ps = passes(seed, sizes)
    whole = R.fold(ps, sizes)
    parts, at = [], 0
    for g in groups:
        parts.append(R.fold(ps[at:at + len(g)], g))
        at += len(g)
    got = M.merged(parts)
    assert got.W == whole.W and got.K == whole.K
    for k in R.BUFS:
        assert rel(got.mean[k], whole.mean[k]) < TOL, k
        assert rel(got.M2[k], whole.M2[k]) < TOL, k
    e_got, out_got = got.error_estimate()
    e_all, out_all = whole.error_estimate()
    assert out_got == out_all == 0
    assert abs(e_got - e_all) <= TOL * e_all
    # chained instead of into an empty accumulator: parts[0] takes in the others
    chain = parts[0]
    for p in parts[1:]:
        M.merge(chain, p)
    for k in R.BUFS:
        assert np.array_equal(chain.mean[k], got.mean[k]) and np.array_equal(chain.M2[k], got.M2[k])


def test_merge_into_an_empty_fold_is_the_identity():
    ps = passes(7, [2, 3, 1])
    src = R.fold(ps, [2, 3, 1])
    keep = {k: (src.mean[k].copy(), src.M2[k].copy()) for k in R.BUFS}
    acc = M.merge(R.Fold(), src)
    assert acc.W == src.W == 6.0 and acc.K == src.K == 3
    for k in R.BUFS:
        assert np.array_equal(acc.mean[k], src.mean[k]) and np.array_equal(acc.M2[k], src.M2[k])
        assert acc.mean[k] is not src.mean[k]
        assert np.array_equal(src.mean[k], keep[k][0]) and np.array_equal(src.M2[k], keep[k][1])     # src is unchanged
    assert acc.error_estimate() == src.error_estimate()
    # and an empty src is a no-op
    before = {k: acc.mean[k].copy() for k in R.BUFS}
    M.merge(acc, R.Fold())
    assert acc.K == 3 and all(np.array_equal(acc.mean[k], before[k]) for k in R.BUFS)


def test_state_round_trip():
    src = R.fold(passes(3, [1, 4]), [1, 4])
    again = M.state(src.mean, src.M2, src.W, src.K)
    assert again.norm() == src.norm() and again.error_estimate() == src.error_estimate()


def test_estimate_and_left_out_count_with_a_nan_in_a_pass():
    sizes_a, sizes_b = [1, 2, 4], [4, 5]
    ps = passes(11, sizes_a + sizes_b)
    ps[1]["img"][3, 5, 1] = np.nan                  # in the first half
    ps[4]["img"][8, 2, 0] = np.inf                  # in the second half
    ps[3]["cx0"][0, 0, 0] = np.nan                  # not in img: counted by nobody
    whole = R.fold(ps, sizes_a + sizes_b)
    got = M.merged([R.fold(ps[:3], sizes_a), R.fold(ps[3:], sizes_b)])
    e_got, out_got = got.error_estimate()
    e_all, out_all = whole.error_estimate()
    assert out_got == out_all == 2
    assert np.isfinite(e_all) and abs(e_got - e_all) <= TOL * e_all
    bad_got, bad_all = ~np.isfinite(got.mean["img"]), ~np.isfinite(whole.mean["img"])
    assert np.array_equal(bad_got, bad_all) and bad_all.sum() == 2
    ok = ~bad_all
    assert rel(got.mean["img"][ok], whole.mean["img"][ok]) < TOL
    ok2 = np.isfinite(whole.M2["img"])
    assert np.array_equal(np.isfinite(got.M2["img"]), ok2)
    assert rel(got.M2["img"][ok2], whole.M2["img"][ok2]) < TOL
