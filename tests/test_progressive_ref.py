"""tests/progressive_ref.py — the numpy restatement the GPU fold is checked against (test_gpu_progressive.py) — pinned by the
defining properties of the weighted running mean / M2 update, and the ctypes mirrors of the new structs by their sizes."""
import ctypes as C
import subprocess

import numpy as np

import progressive_ref as R
from helpers import ROOT, rel_l2

SIZES = [1, 1, 2, 4, 8, 16]


def batches(rng, shape, sizes, sigma=3.0, mu=1.5):
    """Pass means of `sizes` Gaussian samples each, drawn directly: N(mu, sigma^2 / n)."""
    return [mu + sigma / np.sqrt(n) * rng.standard_normal(shape) for n in sizes]


def test_means_are_the_weighted_average_and_m2_the_weighted_squared_deviations():
    rng = np.random.default_rng(7)
    ps = batches(rng, (40, 30, 3), SIZES)
    f = R.fold(ps, SIZES)
    mean = np.average(np.stack(ps), axis=0, weights=SIZES)
    assert rel_l2(f.mean["img"], mean) < 1e-14
    m2 = sum(n * (p - mean) ** 2 for p, n in zip(ps, SIZES))
    assert rel_l2(f.M2["img"], m2) < 1e-12          # (the update cancels in d; the direct sum does not)
    assert f.W == sum(SIZES) and f.K == len(SIZES)
    # after every prefix, too (a session is read between passes)
    g = R.Fold()
    for k, (p, n) in enumerate(zip(ps, SIZES)):
        g.add({"img": p}, n)
        pm = np.average(np.stack(ps[:k + 1]), axis=0, weights=SIZES[:k + 1])
        assert rel_l2(g.mean["img"], pm) < 1e-14
        if k:
            assert rel_l2(g.M2["img"], sum(m * (q - pm) ** 2 for q, m in zip(ps, SIZES[:k + 1]))) < 1e-12


def test_m2_over_k_minus_1_is_unbiased_for_unequal_batches():
    """E[M2] = (K-1) sigma^2 whatever the batch sizes. M2 / sigma^2 is chi-square with K-1 degrees of freedom per pixel, so the mean
    of M2 / (K-1) over P pixels has relative standard error sqrt(2 / (P (K-1))); the bound is five of them."""
    rng = np.random.default_rng(11)
    pixels, sigma, K = 200_000, 3.0, len(SIZES)
    f = R.fold(batches(rng, (pixels,), SIZES, sigma=sigma), SIZES)
    est = (f.M2["img"] / (K - 1)).mean()
    dev = abs(est / sigma ** 2 - 1.0)
    bound = 5.0 / np.sqrt(pixels * (K - 1) / 2.0)
    print(f"sigma^2 estimate {est:.5f} against {sigma ** 2}: relative deviation {dev:.2e}, bound {bound:.2e}")
    assert dev < bound
    # and the variance of the mean: var_mean = M2 / ((K-1) W) against sigma^2 / W
    vm = f.var_mean()["img"].mean()
    assert abs(vm / (sigma ** 2 / sum(SIZES)) - 1.0) < bound


def test_equal_passes_may_come_in_any_order():
    rng = np.random.default_rng(3)
    ps = batches(rng, (16, 16, 3), [4] * 8)
    a = R.fold(ps, [4] * 8)
    perm = rng.permutation(8)
    b = R.fold([ps[i] for i in perm], [4] * 8)
    assert rel_l2(b.mean["img"], a.mean["img"]) < 1e-14
    assert rel_l2(b.M2["img"], a.M2["img"]) < 1e-12
    ea, eb = a.error_estimate()[0], b.error_estimate()[0]
    assert abs(ea - eb) <= 1e-12 * ea


def test_assembled_variances_and_error_estimate():
    rng = np.random.default_rng(5)
    sizes = [2, 2, 4]
    ps = [{k: rng.standard_normal((6, 5, 3)) + 2.0 for k in R.BUFS} for _ in sizes]
    f = R.fold(ps, sizes)
    v, a = f.var_mean(), f.assembled_var()
    assert np.array_equal(a["c"], v["img"])
    assert np.array_equal(a["cx"][:, 0], v["cx0"][:, 0]) and np.array_equal(a["cy"][0], v["cy0"][0])
    assert np.array_equal(a["cx"][2, 3], v["cx0"][2, 3] + v["cx1"][2, 2])
    assert np.array_equal(a["cy"][4, 1], v["cy0"][4, 1] + v["cy1"][3, 1])
    e, out = f.error_estimate()
    assert out == 0 and abs(e - np.sqrt(v["img"].sum() / (f.mean["img"] ** 2).sum())) < 1e-15
    # a non-finite pass value propagates into the mean; its pixel leaves both sums and is counted
    ps[1]["img"][2, 2, 1] = np.inf
    g = R.fold(ps, sizes)
    assert not np.isfinite(g.mean["img"][2, 2, 1]) and np.isfinite(g.mean["img"][2, 2, 0])
    e2, out2 = g.error_estimate()
    ok = np.ones((6, 5), bool)
    ok[2, 2] = False
    assert out2 == 1 and abs(e2 - np.sqrt(v["img"][ok].sum() / (f.mean["img"][ok] ** 2).sum())) < 1e-15
    assert np.isnan(R.fold(ps[:1], sizes[:1]).error_estimate()[0])


def test_progressive_struct_layouts_match_the_header(G, tmp_path):
    src = tmp_path / "sz.c"
    structs = ["GdptSampleWindow", "GdptProgressiveConfig", "GdptProgressiveStatus"]
    body = "\n".join(f'printf("{s} %zu\\n", sizeof({s}));' for s in structs)
    body += 'printf("totals %zu\\n", offsetof(GdptProgressiveStatus, totals));'
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/gdpt.h"\nint main(){{{body} return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    sizes = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for s in structs:
        assert int(sizes[s]) == C.sizeof(getattr(G, s)), s
    assert int(sizes["GdptSampleWindow"]) == 8
    assert int(sizes["totals"]) == G.GdptProgressiveStatus.totals.offset
    assert (G.STOP_NONE, G.STOP_TARGET, G.STOP_BUDGET, G.STOP_MAX_PASSES) == (0, 1, 2, 3)
