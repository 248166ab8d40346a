"""The numpy restatement of the spread of N weighted images (tests/recon_spread_ref.py) against what it must mean: the closed form
for two images, the two-pass definition, unbiasedness, the left-out rule, the clipped window with finite counts; and the C ABI of the
feature (include/gdpt.h: gdpt_recon_spread*, gdpt_progressive_group_reconstruct_error, _run_recon): exports and struct sizes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import recon_spread_ref as S
from helpers import ROOT


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_two_images_closed_form():
    """N = 2: var = (W_a W_b / W^2) (f_a - f_b)^2, to 1e-15 relative per element."""
    rng = np.random.default_rng(1)
    fa, fb = rng.normal(1.0, 0.3, (6, 7, 3)), rng.normal(1.0, 0.3, (6, 7, 3))
    for wa, wb in ((1.0, 1.0), (3.0, 13.0), (1000.0, 1.0)):
        _, var = S.spread([fa, fb], [wa, wb])
        want = (wa * wb / (wa + wb) ** 2) * (fa - fb) ** 2
        assert np.abs(var - want).max() <= 1e-15 * np.abs(want).max(), (wa, wb)


def test_equal_images_have_no_spread():
    f = np.random.default_rng(2).normal(0.5, 1.0, (5, 4, 3))
    for n in (2, 3, 16):
        mean, var = S.spread([f] * n, np.arange(1, n + 1, dtype=np.float64))
        assert np.array_equal(var, np.zeros_like(f)) and np.array_equal(mean, f)


@pytest.mark.parametrize("n", [3, 16])
def test_update_against_the_two_pass_formula(n):
    """West's update in member order against the definition, skewed weights: 1e-13 relative on the mean and on var."""
    rng = np.random.default_rng(3 + n)
    images = [rng.normal(2.0, 0.5, (9, 11, 3)) for _ in range(n)]
    weights = [float(2 ** (k % 7)) + 0.25 * k for k in range(n)]
    mean, var = S.spread(images, weights)
    mean2, var2 = S.two_pass(images, weights)
    assert rel(mean, mean2) < 1e-13 and rel(var, var2) < 1e-13


def test_unbiased():
    """N = 4, film 64x48x3, iid Gaussian members of variance sigma^2 / W_i: sum var / (count sigma^2 / W) within 5 %. The ratio is
    a chi-square with 3 x 9216 degrees of freedom over that number: standard deviation sqrt(2 / (3 * 9216)) = 0.85 %, so the
    bound is 5 sigma plus slack."""
    rng = np.random.default_rng(4)
    sigma, weights = 0.7, [2.0, 5.0, 8.0, 17.0]
    images = [rng.normal(0.0, sigma / np.sqrt(w), (48, 64, 3)) for w in weights]
    e = S.estimate(images, weights, total=np.ones((48, 64, 3)))
    ratio = e["sum_var"] / (48 * 64 * 3 * sigma ** 2 / sum(weights))
    print(f"sum var / expectation = {ratio:.4f}")
    assert e["left_out"] == 0 and abs(ratio - 1.0) < 0.05


def test_non_finite_pixels_are_left_out():
    """NaN and Inf planted in one member and in the total: the count and both sums are those of the same input with the affected
    pixels removed."""
    rng = np.random.default_rng(5)
    h, w = 7, 9
    images = [rng.normal(1.0, 0.2, (h, w, 3)) for _ in range(3)]
    weights = [4.0, 9.0, 3.0]
    total = rng.normal(1.0, 0.05, (h, w, 3))
    clean = S.estimate(images, weights, total)
    assert clean["left_out"] == 0
    bad = [(0, 0), (3, 4), (6, 8), (2, 2)]
    planted, tot = [x.copy() for x in images], total.copy()
    planted[1][0, 0, 1] = np.nan
    planted[1][3, 4, 2] = np.inf
    tot[6, 8, 0] = -np.inf
    tot[2, 2, 1] = np.nan
    e = S.estimate(planted, weights, tot)
    keep = np.ones((h, w), dtype=bool)
    for y, x in bad:
        keep[y, x] = False
    sq = (total ** 2)
    want_var = S.pixel_sum(clean["var"])[keep].sum()
    want_sq = ((sq[..., 0] + sq[..., 1]) + sq[..., 2])[keep].sum()
    assert e["left_out"] == len(bad)
    assert abs(e["sum_var"] - want_var) <= 1e-15 * want_var and abs(e["sum_sq"] - want_sq) <= 1e-15 * want_sq
    assert np.isfinite(e["error"]) and np.array_equal(e["var"][keep], clean["var"][keep])
    # a member that is not finite makes var non-finite there; a total that is not finite leaves var alone
    assert not np.isfinite(e["var"][0, 0, 1]) and not np.isfinite(e["var"][3, 4, 2]) and np.isfinite(e["var"][6, 8]).all()


def test_window():
    """r = 2 on a 5x3 film: the corners average 9 entries; a planted NaN lowers the count of every window that holds it (all
    windows within 2 pixels of it, clipped to the film) by one, and the means are those of the surviving values."""
    rng = np.random.default_rng(6)
    h, w, r = 3, 5, 2
    plane = rng.uniform(0.5, 2.0, (h, w))
    cnt = S.window_counts(plane, r)
    assert cnt[0, 0] == cnt[0, 4] == cnt[2, 0] == cnt[2, 4] == 9 and cnt[1, 2] == 15
    got = S.window_mean(plane, r)
    for y in range(h):
        for x in range(w):
            win = plane[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1]
            assert win.size == cnt[y, x] and abs(got[y, x] - win.mean()) <= 1e-15 * win.mean()
    assert np.array_equal(S.window_mean(plane, 0), plane)
    holed = plane.copy()
    holed[0, 1] = np.nan
    cnt2, got2 = S.window_counts(holed, r), S.window_mean(holed, r)
    for y in range(h):
        for x in range(w):
            near = abs(y - 0) <= r and abs(x - 1) <= r
            assert cnt2[y, x] == cnt[y, x] - (1 if near else 0)
            win = holed[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1]
            alive = win[np.isfinite(win)]
            assert abs(got2[y, x] - alive.mean()) <= 1e-15 * alive.mean()
            if not near:
                assert got2[y, x] == got[y, x]
    assert np.isfinite(got2[0, 1])                    # the map has a value where the raw plane has none
    assert np.isnan(S.window_mean(np.full((h, w), np.nan), r)).all()
    lone = np.full((h, w), np.inf)
    lone[2, 4] = 3.0
    m = S.window_mean(lone, 1)
    assert m[2, 4] == m[1, 3] == 3.0 and np.isnan(m[0, 0])


def test_exports_and_struct_sizes(G, tmp_path):
    """The new symbols are exported, the new structs have the header's sizes, and no existing struct grew."""
    new = {"GdptReconSpreadStats": 48, "GdptGroupReconParams": 128}
    old = {"GdptProgressiveConfig": 16, "GdptProgressiveStatus": 136, "GdptSampleWindow": 8, "GdptReconParams": 48, "GdptReconStats": 48,
           "GdptWeightedReconParams": 64, "GdptWeightedReconStats": 80, "GdptRenderStats": 96}
    structs = {**new, **old}
    body = "\n".join(f'printf("{s} %zu\\n", sizeof({s}));' for s in structs)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include "{ROOT}/include/gdpt.h"\nint main(){{{body} return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    sizes = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for s, want in structs.items():
        assert int(sizes[s]) == C.sizeof(getattr(G, s)) == want, (s, sizes[s], C.sizeof(getattr(G, s)))
    for name in ("gdpt_recon_spread", "gdpt_recon_spread_device", "gdpt_progressive_group_reconstruct_error", "gdpt_progressive_group_run_recon"):
        assert hasattr(G.lib(), name), name
    for name in ("recon_spread", "recon_spread_device", "group_recon_params"):
        assert callable(getattr(G, name)), name
    assert callable(G.ProgressiveGroup.reconstruct_error)


def test_refusals_come_before_the_device(G):
    """What gdpt_recon_spread refuses is refused with its message on any machine; a well-formed call needs a GPU (no CPU fallback)."""
    f = np.ones((2, 3, 3))
    for images, weights, radius, match in (([f], [1.0], 0, r"\[2, 16\]"), ([f] * 17, [1.0] * 17, 0, r"\[2, 16\]"),
                                           ([f, f], [1.0, 0.0], 0, "weight 1"), ([f, f], [np.inf, 1.0], 0, "weight 0"),
                                           ([f, f], [1.0, np.nan], 0, "weight 1"), ([f, f], [1.0, 1.0], 9, "radius"),
                                           ([f, f], [1.0, 1.0], -1, "radius")):
        with pytest.raises(G.GdptError, match=match):
            G.recon_spread(images, weights, radius=radius)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(G.GdptError, match="(?i)hip"):
            G.recon_spread([f, f], [1.0, 2.0])
