"""The collaborative form of the first-order feature regression on the GPU (include/gdpt.h: gdpt_denoise_nlm_collab*,
gdpt_progressive_denoise_collab): both kernel forms against the numpy restatement (tests/nlm_collab_ref.py), the image and the
coefficient film, so that a wrong answer says which pass made it; what is left out; the identities that hold bit for bit (the
regression's own output in the coefficient film, no window, the same bits twice, on a second stream, from the host and the device
entries, enqueue-only, with and without a caller's coefficient film); a film past the block cap; the sessions (Path, GradPath, a
group's total) and the CLI."""
import hashlib
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import hip_rt
import nlm_collab_ref as NC
import nlm_regress_ref as NR
from helpers import ROOT, scene_variant
from test_gpu_nlm import CBOX, FORMS, masked_rel_l2, planted_film, rel_diff
from test_gpu_nlm_guided import planted_features
from test_gpu_progressive import read_pfm
from test_nlm_guided_ref import noisy_features
from test_nlm_ref import noisy_film

pytestmark = pytest.mark.gpu

# measured on an MI355X: the worst figure (masked relative L2 of out and of the coefficient film, relative difference of the three film
# sums) between either kernel form and the restatement and between the two forms, over every case of the tests below. The sides differ
# as the regression's do (tests/test_gpu_nlm_regress.py: FMA contraction in the normal equations, the LDL^T and here in the fits'
# values too, the order of the patch sums, the last place of exp, carried through a solve whose condition number stays below about
# 1.5e3 at ridge >= 1e-3); 100 x the measured value is the margin, never looser than 1e-9. Measured: 5.320e-15 (tiled) and 5.982e-15
# (direct) against the restatement over the 128 cases, 4.915e-15 between the forms, 6.171e-16 on the film past the block cap.
NLM_COLLAB_MEASURED = 6.0e-15
NLM_COLLAB_BOUND = min(100 * NLM_COLLAB_MEASURED, 1e-9) if NLM_COLLAB_MEASURED else None

FILMS = [(1, 1), (16, 16), (17, 17), (33, 9), (40, 19)]      # W x H: 16 x 16 is one tile, 17 x 17 one pixel into the next each way
RADII = [(0, 0), (1, 0), (2, 1), (10, 3)]                    # (10, 3): the full LDS stage
GROUPS = {0: [], 1: [(0, 3, 1e-3)], 2: [(0, 3, 1e-3), (3, 3, 1e-3)]}
# m -> (channels, scales): plane 6 is named by no group, plane 7 by nothing; scale 1 skips the division in the kernel, the others do not
REGRESSORS = {0: ([], []), 1: ([6], [0.25]), 3: ([6, 3, 4], [1.0, 0.5, 2.0]), 7: ([6, 0, 1, 2, 3, 4, 5], [1.0] * 7)}
RIDGES = (1e-3, 1e-2)
COMBOS = list(itertools.product((0, 1, 3, 7), (0, 1, 2)))      # (m, number of groups)
SUMS = ("sum_var_in", "sum_sq_in", "sum_sq_out")
KW = dict(k=0.8)


def regress_of(G, m, ridge):
    return G.nlm_regress(channels=REGRESSORS[m][0], scales=REGRESSORS[m][1], ridge=ridge)


def figure(out, coef, st, want):
    """The worst figure of one call against `want` (the restatement's dict, or another call's); the exact parts are asserted here."""
    figs = [masked_rel_l2(out, want["out"]), masked_rel_l2(coef, want["coef"])]
    figs += [rel_diff(getattr(st, k), want[k]) for k in SUMS]
    assert st.pixels_left_out == want["left_out"]
    assert math.isnan(st.sum_var_out) and math.isnan(st.error_out)          # not estimated
    with np.errstate(all="ignore"):
        assert np.array_equal(st.error_in, np.sqrt(np.float64(st.sum_var_in) / np.float64(st.sum_sq_in)), equal_nan=True)
    return max(figs)


def as_dict(out, coef, st):
    d = dict(out=out, coef=coef, left_out=st.pixels_left_out)
    d.update({k: getattr(st, k) for k in SUMS})
    return d


def same_bits(a, b):
    """(out, coef, stats) of two calls"""
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True) and \
        [getattr(a[2], k) for k in SUMS] == [getattr(b[2], k) for k in SUMS] and a[2].pixels_left_out == b[2].pixels_left_out


@pytest.fixture(scope="module")
def cases(G):
    """Films x (r, f) x (m, groups), clean and planted: the restatement's result (computed once, left unchanged) and both forms'.
    Every (m, groups) pair at (2, 1) and (10, 3) on the two films of more than one tile, one pair in turn elsewhere; the ridge
    alternates."""
    out = []
    n = 0
    for planted in (False, True):
        for (w, h) in FILMS:
            img, var = planted_film(w, h, 10 * w + h) if planted else noisy_film(w, h, 10 * w + h)
            feat, fvar = planted_features(w, h, w + h) if planted else noisy_features(w, h, w + h)
            for (r, f) in RADII:
                every = (r, f) in ((2, 1), (10, 3)) and (w, h) in ((17, 17), (40, 19))
                for (m, ng) in (COMBOS if every else (COMBOS[n % len(COMBOS)],)):
                    ridge = RIDGES[n % 2]
                    want = NC.denoise(img, var, feat, fvar, GROUPS[ng], REGRESSORS[m][0], REGRESSORS[m][1], ridge, r=r, f=f, **KW)
                    guide, regress = G.nlm_guide(groups=GROUPS[ng]), regress_of(G, m, ridge)
                    got = []
                    for direct in FORMS:
                        with G.debug_knobs(nlm_direct=direct):
                            got.append(G.denoise_nlm_collab(img, var, feat, fvar, guide=guide, regress=regress, coef=True, window_radius=r,
                                                            patch_radius=f, **KW))
                        assert (got[-1][2].window_radius, got[-1][2].patch_radius) == (r, f) and got[-1][2].filter_ms > 0
                    out.append(((w, h, r, f, m, ng, ridge, planted), img, var, feat, fvar, want, got))
                    n += 1
    return out


def test_both_forms_against_the_restatement(cases):
    worst = {0: 0.0, 1: 0.0}
    left = 0
    seen = set()
    for key, img, var, feat, fvar, want, got in cases:
        w, h, r, f, m, ng, ridge, planted = key
        seen.add((m, ng))
        ok = NR.valid_mask(img, var, feat, fvar, GROUPS[ng], REGRESSORS[m][0])
        assert want["left_out"] == (~ok).sum() and (not planted or want["left_out"] >= 1)
        left += want["left_out"]
        d = 1 + m
        for direct in FORMS:
            o, coef, st = got[direct]
            assert coef.shape == (3 * d, h, w), key
            assert np.array_equal(o[~ok], img[~ok], equal_nan=True), key
            for c in range(3):          # an invalid pixel's planes: its input bits and zeros, in both the restatement and the kernels
                assert np.array_equal(coef[c * d][~ok], img[:, :, c][~ok], equal_nan=True) and not coef[c * d + 1:(c + 1) * d][:, ~ok].any(), key
            if r == 0:
                assert np.array_equal(o, img, equal_nan=True), key
            worst[direct] = max(worst[direct], figure(o, coef, st, want))
    assert left > 50 and seen == set(COMBOS)
    print(f"nlm collaborative regression against the restatement: worst figure tiled {worst[0]:.3e}, direct {worst[1]:.3e} over {len(cases)} "
          f"cases (bound {NLM_COLLAB_BOUND})")
    assert NLM_COLLAB_BOUND is not None, f"NLM_COLLAB_MEASURED has not been recorded; this run measured {max(worst.values()):.3e}"
    assert max(worst.values()) < NLM_COLLAB_BOUND


def test_the_two_forms_agree(cases):
    worst = 0.0
    for key, img, var, feat, fvar, want, got in cases:
        worst = max(worst, figure(*got[0], as_dict(*got[1])))
    print(f"nlm collaborative regression tiled against direct: worst figure {worst:.3e} (bound {NLM_COLLAB_BOUND})")
    assert NLM_COLLAB_BOUND is not None, f"NLM_COLLAB_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < NLM_COLLAB_BOUND


@pytest.mark.parametrize("direct", FORMS, ids=["tiled", "direct"])
def test_the_first_coefficient_plane_is_the_regression_bit_for_bit(G, direct):
    """The same sweep, the same Fit::add and the same Ldlt: plane c d + 0 is gdpt_denoise_nlm_regress's out channel c."""
    w, h = 40, 19
    img, var = planted_film(w, h, 3)
    feat, fvar = planted_features(w, h, 3)
    with G.debug_knobs(nlm_direct=direct):
        for (m, ng), (r, f), ridge in zip(COMBOS, itertools.cycle(((3, 1), (10, 3), (1, 0), (2, 1))), itertools.cycle(RIDGES)):
            kw = dict(guide=G.nlm_guide(groups=GROUPS[ng]), regress=regress_of(G, m, ridge), window_radius=r, patch_radius=f, **KW)
            o, coef, st = G.denoise_nlm_collab(img, var, feat, fvar, coef=True, **kw)
            ro, _, rst = G.denoise_nlm_regress(img, var, feat, fvar, **kw)
            d = 1 + m
            assert np.array_equal(np.moveaxis(coef[[0, d, 2 * d]], 0, 2), ro, equal_nan=True), (m, ng, r, f)
            assert (st.pixels_left_out, st.sum_var_in, st.sum_sq_in) == (rst.pixels_left_out, rst.sum_var_in, rst.sum_sq_in) and st.pixels_left_out > 0
            assert not np.array_equal(o, ro, equal_nan=True)          # the gather is at work


def test_host_and_device_entries_same_bits_second_stream_enqueue_only_and_a_callers_film(G):
    w, h, r, f = 40, 19, 3, 1
    img, var = planted_film(w, h, 5)
    feat, fvar = planted_features(w, h, 5)
    guide, regress = G.nlm_guide(groups=GROUPS[2]), regress_of(G, 7, 1e-2)
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (img, var, feat, fvar))
    cshape = (24, h, w)
    d_out, d_coef = hip_rt.alloc(G, img.nbytes), hip_rt.alloc(G, 8 * img.nbytes)
    side = hip_rt.stream(G)
    kw = dict(guide=guide, regress=regress, window_radius=r, patch_radius=f, **KW)
    zero = lambda p, n: hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(n)))      # noqa: E731
    for direct in FORMS:
        with G.debug_knobs(nlm_direct=direct):
            first = G.denoise_nlm_collab(img, var, feat, fvar, coef=True, **kw)             # the host entry
            assert first[2].pixels_left_out > 4 and first[2].sum_sq_out > 0 and first[2].filter_ms > 0
            o, st = G.denoise_nlm_collab(img, var, feat, fvar, **kw)                        # ... without the film
            assert same_bits((o, first[1], st), first)
            for stream in (None, None, side):
                st = G.denoise_nlm_collab_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, d_coef, stream=stream, **kw)
                assert same_bits((hip_rt.to_host(G, d_out, img.shape), hip_rt.to_host(G, d_coef, cshape), st), first)
            # enqueue-only against blocking
            zero(d_out, img.nbytes), zero(d_coef, 8 * img.nbytes)
            assert G.denoise_nlm_collab_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, d_coef, stats=False, **kw) is None
            assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True)
            assert np.array_equal(hip_rt.to_host(G, d_coef, cshape), first[1], equal_nan=True)
            # without a caller's film: the library's own, on either stream
            for stream in (None, side):
                zero(d_out, img.nbytes)
                st = G.denoise_nlm_collab_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, stream=stream, **kw)
                assert same_bits((hip_rt.to_host(G, d_out, img.shape), first[1], st), first)
            zero(d_out, img.nbytes)
            assert G.denoise_nlm_collab_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, stats=False, **kw) is None
            assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True)
    # a film that overlaps an input or out is refused, whichever end it overlaps at
    for bad in (d_out, d_img, d_var - 8, d_feat + 8, d_fvar):
        with pytest.raises(G.GdptError, match="coef must not overlap"):
            G.denoise_nlm_collab_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, bad, **kw)
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    for p in (d_img, d_var, d_feat, d_fvar, d_out, d_coef):
        hip_rt.free(G, p)


def test_a_film_past_the_block_cap(G):
    """1025 x 345: 65 x 22 = 1430 tiles on 1024 blocks, so 406 blocks take a second tile (and stage it afresh) in both passes."""
    w, h, r, f = 1025, 345, 1, 0
    img, var = noisy_film(w, h, 11)
    feat, fvar = noisy_features(w, h, 11, channels=3)
    img[200, 1000, 0] = np.nan
    fvar[1, 344, 1024] = -1.0
    channels, scales = [1, 2], [1.0, 0.5]
    want = NC.denoise(img, var, feat, fvar, [(0, 1, 1e-3)], channels, scales, 1e-2, r=r, f=f, **KW)
    assert want["left_out"] == 2
    guide, regress = G.nlm_guide(num_channels=3, groups=[(0, 1, 1e-3)]), G.nlm_regress(channels=channels, scales=scales, ridge=1e-2)
    worst = 0.0
    for direct in FORMS:
        with G.debug_knobs(nlm_direct=direct):
            worst = max(worst, figure(*G.denoise_nlm_collab(img, var, feat, fvar, guide=guide, regress=regress, coef=True, window_radius=r,
                                                            patch_radius=f, **KW), want))
    print(f"nlm collaborative regression past the block cap: worst figure {worst:.3e} (bound {NLM_COLLAB_BOUND})")
    assert NLM_COLLAB_BOUND is not None, f"NLM_COLLAB_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < NLM_COLLAB_BOUND


def session_body(G, ses, scene, budget):
    """`ses` holds at least two passes: denoise_collab() is Scene.features with the window {budget, 0} fed to
    denoise_nlm_collab_device with the planes read() returns, bit for bit, in host and in device memory."""
    h, w, _ = ses.shape
    fspp = 4
    kw = dict(window_radius=4, patch_radius=2, k=2.0)
    guide, regress = G.nlm_guide(groups=GROUPS[1], k_f=0.7), G.nlm_regress(channels=[0, 1, 2, 3, 4, 5, 6], scales=[1.0] * 6 + [4.0], ridge=1e-2)
    out, fm, fv, st = ses.denoise_collab(fspp, guide=guide, regress=regress, features=True, **kw)
    want_fm, want_fv = scene.features(fspp, window=(budget, 0))
    assert np.array_equal(fm, want_fm) and np.array_equal(fv, want_fv) and fv.any()
    means, vars_, _ = ses.read()
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (means["img"], vars_["img"], fm, fv))
    d_out = hip_rt.alloc(G, out.nbytes)
    st2 = G.denoise_nlm_collab_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, guide=guide, regress=regress, **kw)
    assert np.array_equal(hip_rt.to_host(G, d_out, out.shape), out) and [getattr(st2, k) for k in SUMS] == [getattr(st, k) for k in SUMS]
    assert st.pixels_left_out == 0 and np.isfinite(out).all() and math.isnan(st.sum_var_out) and math.isnan(st.error_out)
    point = ses.denoise_regress(fspp, guide=guide, regress=regress, **kw)
    assert not np.array_equal(point[0], out)                      # the gather is at work
    # everything in device memory
    d_fm, d_fv = hip_rt.alloc(G, fm.nbytes), hip_rt.alloc(G, fm.nbytes)
    hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(out.nbytes)))
    st3 = ses.denoise_collab(fspp, guide=guide, regress=regress, out_ptr=d_out, features_ptrs=(d_fm, d_fv), **kw)
    assert np.array_equal(hip_rt.to_host(G, d_out, out.shape), out) and st3.sum_sq_out == st.sum_sq_out
    assert np.array_equal(hip_rt.to_host(G, d_fm, fm.shape), fm) and np.array_equal(hip_rt.to_host(G, d_fv, fm.shape), fv)
    again = ses.denoise_collab(fspp, guide=guide, regress=regress, **kw)
    assert np.array_equal(again[0], out) and again[1].sum_sq_out == st.sum_sq_out
    for bad in (1, budget + 1):
        with pytest.raises(G.GdptError, match="feature_spp"):
            ses.denoise_collab(bad)
    with pytest.raises(G.GdptError, match="ridge"):
        ses.denoise_collab(fspp, regress=G.nlm_regress(ridge=0.0))
    with pytest.raises(G.GdptError, match="num_channels"):
        ses.denoise_collab(fspp, guide=G.nlm_guide(num_channels=7, groups=GROUPS[1]))
    for p in (d_img, d_var, d_feat, d_fvar, d_out, d_fm, d_fv):
        hip_rt.free(G, p)


@pytest.mark.parametrize("path", [True, False], ids=["path", "gradpath"])
def test_session(G, scene_tmp, path):
    """cbox 40 x 24, budget 32 in eight passes of 4: refused before the second pass, then the collaborative regression on what read()
    returns."""
    sd = G.parse_scene(scene_variant(scene_tmp, CBOX, width=40, height=24, integrator="path" if path else None))
    sc = G.Scene(sd)
    ses = G.Progressive(sc, 32, path=path)
    ses.add_pass(4)
    with pytest.raises(G.GdptError, match="at least 2 passes"):
        ses.denoise_collab(4)
    ses.run(pass_spp=4)
    assert ses.status()["passes"] == 8
    session_body(G, ses, sc, 32)
    ses.close()
    sc.close()


def test_group_total(G, scene_tmp):
    sd = G.parse_scene(scene_variant(scene_tmp, CBOX, width=40, height=24))
    grp = G.ProgressiveGroup(sd, (0, 0), 32)
    grp.run(pass_spp=4)
    assert grp.total.status()["passes"] == 8
    sc = G.Scene(sd)
    session_body(G, grp.total, sc, 32)
    sc.close()
    grp.close()


EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")


def test_cli_collaborative(G, scene_tmp, tmp_path):
    xml = scene_variant(scene_tmp, CBOX, width=40, height=24, integrator="path")
    out, den, cden = tmp_path / "o.pfm", tmp_path / "d.pfm", tmp_path / "c.pfm"
    base = [EXE, "--spp", "32", "--pass-spp", "4", "--nlm-window", "4", "--nlm-patch", "2", "--nlm-regress", "albedo,normal", "--feature-spp", "4"]
    r0 = subprocess.run([*base, "--denoised", str(den), "-o", str(out), xml], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stderr
    sha = hashlib.sha256(open(out, "rb").read()).hexdigest()
    r1 = subprocess.run([*base, "--nlm-collaborative", "--denoised", str(cden), "-o", str(out), xml], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == sha          # -o does not know of the flag
    sc = G.Scene(G.parse_scene(xml))
    ses = G.Progressive(sc, 32, path=True)
    ses.run(pass_spp=4)
    kw = dict(guide=G.nlm_guide(groups=GROUPS[1]), window_radius=4, patch_radius=2, k=4.0)
    want, st = ses.denoise_collab(4, **kw)
    assert np.array_equal(read_pfm(cden, 40, 24), want.astype(np.float32))
    point = ses.denoise_regress(4, **kw)[0]
    assert np.array_equal(read_pfm(den, 40, 24), point.astype(np.float32)) and not np.array_equal(point.astype(np.float32), want.astype(np.float32))
    line = [l for l in r1.stdout.splitlines() if l.startswith("[gdpt] denoised:")]
    assert len(line) == 1 and "first-order regression on albedo,normal (ridge 0.010000), collaborative (no variance estimate)" in line[0]
    assert "collaborative (" not in r0.stdout
    ses.close()
    sc.close()
