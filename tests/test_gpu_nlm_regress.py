"""The first-order feature regression on the non-local-means weights on the GPU (include/gdpt.h: gdpt_denoise_nlm_regress*,
gdpt_progressive_denoise_regress): both kernel forms against the numpy restatement (tests/nlm_regress_ref.py) and against each other,
what is left out, the guided filter at no regressor, the host and device entries, a film past the block cap, the sessions (Path,
GradPath, a group's total) and the CLI."""
import hashlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import hip_rt
import nlm_regress_ref as NR
from helpers import ROOT, scene_variant
from test_gpu_nlm import CBOX, FORMS, SUMS, as_dict, figure, planted_film
from test_gpu_nlm_guided import planted_features, same_bits
from test_gpu_progressive import read_pfm
from test_nlm_guided_ref import noisy_features
from test_nlm_ref import noisy_film

pytestmark = pytest.mark.gpu

# measured on an MI355X: the worst figure of tests/test_gpu_nlm.py (masked relative L2 of out and of var_out, relative difference of
# the four film sums) between either kernel form and the restatement, between the two forms, and between the m = 0 regression and
# the guided filter, over every case of the tests below. The sides differ by FMA contraction (in the accumulation of the normal
# equations and in the LDL^T too), the order of the patch sums and the last place of exp, carried through a solve whose condition
# number stays below about 1.5e3 at ridge >= 1e-3; 100 x the measured value is the margin, never looser than 1e-9. Measured: 1.835e-15
# (tiled) and 2.412e-15 (direct) against the restatement over the 138 cases, 2.590e-15 between the forms, 5.413e-16 against the guided
# filter at m = 0, 3.530e-16 on the film past the block cap.
NLM_REGRESS_MEASURED = 2.6e-15
NLM_REGRESS_BOUND = min(100 * NLM_REGRESS_MEASURED, 1e-9) if NLM_REGRESS_MEASURED else None

FILMS = [(1, 1), (16, 16), (17, 17), (33, 9), (40, 19)]      # W x H: 17 x 17 is one pixel past a 16 x 16 tile each way
RADII = [(0, 0), (1, 0), (2, 1), (5, 1), (10, 3)]
GROUPS = {0: [], 1: [(0, 3, 1e-3)], 2: [(0, 3, 1e-3), (3, 3, 1e-3)]}
# m -> (channels, scales): plane 6 is named by no group, plane 7 by nothing; scale 1 skips the division in the kernel, the others do not
REGRESSORS = {0: ([], []), 1: ([6], [0.25]), 3: ([6, 3, 4], [1.0, 0.5, 2.0]), 7: ([6, 0, 1, 2, 3, 4, 5], [1.0] * 7)}
RIDGES = (1e-3, 1e-2)
COMBOS = list(itertools.product((0, 1, 3, 7), (0, 1, 2)))      # (m, number of groups)
KW = dict(k=0.8)


def regress_of(G, m, ridge):
    return G.nlm_regress(channels=REGRESSORS[m][0], scales=REGRESSORS[m][1], ridge=ridge)


def restated(img, var, feat, fvar, m, ng, ridge, r, f, **kw):
    return NR.denoise(img, var, feat, fvar, GROUPS[ng], REGRESSORS[m][0], REGRESSORS[m][1], ridge, r=r, f=f, **kw)


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
                    want = restated(img, var, feat, fvar, m, ng, ridge, r, f, **KW)
                    guide, regress = G.nlm_guide(groups=GROUPS[ng]), regress_of(G, m, ridge)
                    got = []
                    for direct in FORMS:
                        with G.debug_knobs(nlm_direct=direct):
                            got.append(G.denoise_nlm_regress(img, var, feat, fvar, guide=guide, regress=regress, window_radius=r, patch_radius=f, **KW))
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
        if planted and m > 0 and ng == 0 and (w, h) != (1, 1):
            assert not ok[h // 2, w // 2]          # -Inf in plane 6, which only the regressors name
        left += want["left_out"]
        for direct in FORMS:
            o, vo, st = got[direct]
            assert np.array_equal(o[~ok], img[~ok], equal_nan=True) and np.array_equal(vo[~ok], var[~ok], equal_nan=True), key
            if r == 0:
                assert np.array_equal(o, img, equal_nan=True) and np.array_equal(vo, var, equal_nan=True), key
            worst[direct] = max(worst[direct], figure(o, vo, st, want))
    assert left > 50 and seen == set(COMBOS)
    print(f"nlm regression against the restatement: worst figure tiled {worst[0]:.3e}, direct {worst[1]:.3e} over {len(cases)} cases "
          f"(bound {NLM_REGRESS_BOUND})")
    assert NLM_REGRESS_BOUND is not None, f"NLM_REGRESS_MEASURED has not been recorded; this run measured {max(worst.values()):.3e}"
    assert max(worst.values()) < NLM_REGRESS_BOUND


def test_the_two_forms_agree(cases):
    worst = 0.0
    for key, img, var, feat, fvar, want, got in cases:
        worst = max(worst, figure(*got[0], as_dict(*got[1])))
    print(f"nlm regression tiled against direct: worst figure {worst:.3e} (bound {NLM_REGRESS_BOUND})")
    assert NLM_REGRESS_BOUND is not None, f"NLM_REGRESS_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < NLM_REGRESS_BOUND


@pytest.mark.parametrize("direct", FORMS, ids=["tiled", "direct"])
def test_no_regressor_is_the_guided_filter_and_an_unnamed_plane_changes_nothing(G, direct):
    w, h = 40, 19
    img, var = planted_film(w, h, 3)
    feat, fvar = planted_features(w, h, 3)
    worst = 0.0
    with G.debug_knobs(nlm_direct=direct):
        for ng, (r, f) in itertools.product((0, 1, 2), ((3, 1), (10, 3))):
            kw = dict(guide=G.nlm_guide(groups=GROUPS[ng]), window_radius=r, patch_radius=f, **KW)
            guided = G.denoise_nlm_guided(img, var, feat, fvar, **kw)
            assert guided[2].pixels_left_out > 0
            worst = max(worst, figure(*G.denoise_nlm_regress(img, var, feat, fvar, regress=G.nlm_regress(channels=[]), **kw), as_dict(*guided)))
        # no group and no regressor: the feature planes are not looked at, and need not be given
        kw = dict(guide=G.nlm_guide(groups=[]), regress=G.nlm_regress(channels=[]), window_radius=3, patch_radius=1, **KW)
        assert same_bits(G.denoise_nlm_regress(img, var, None, None, **kw), G.denoise_nlm_regress(img, var, feat, fvar, **kw))
        # planes 5 and 7 are named by neither a group nor a regressor: whatever they hold, the same bits
        kw = dict(guide=G.nlm_guide(groups=GROUPS[1]), regress=regress_of(G, 3, 1e-2), window_radius=3, patch_radius=1, **KW)
        clean_f, clean_v = feat.copy(), fvar.copy()
        clean_f[[5, 7]], clean_v[[5, 7]] = 0.5, 0.0
        assert not (np.isfinite(feat[[5, 7]]).all() and np.isfinite(fvar[[5, 7]]).all() and (fvar[[5, 7]] >= 0).all())
        a, b = G.denoise_nlm_regress(img, var, feat, fvar, **kw), G.denoise_nlm_regress(img, var, clean_f, clean_v, **kw)
        assert same_bits(a, b) and a[2].pixels_left_out > 0
    print(f"nlm regression with no regressor against the guided filter: worst figure {worst:.3e} (bound {NLM_REGRESS_BOUND})")
    assert NLM_REGRESS_BOUND is not None, f"NLM_REGRESS_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < NLM_REGRESS_BOUND


def test_host_and_device_entries_same_bits_second_stream_and_enqueue_only(G):
    w, h, r, f = 40, 19, 3, 1
    img, var = planted_film(w, h, 5)
    feat, fvar = planted_features(w, h, 5)
    guide, regress = G.nlm_guide(groups=GROUPS[2]), regress_of(G, 7, 1e-2)
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (img, var, feat, fvar))
    d_out, d_vout = hip_rt.alloc(G, img.nbytes), hip_rt.alloc(G, img.nbytes)
    side = hip_rt.stream(G)
    kw = dict(guide=guide, regress=regress, window_radius=r, patch_radius=f, **KW)
    for direct in FORMS:
        with G.debug_knobs(nlm_direct=direct):
            first = G.denoise_nlm_regress(img, var, feat, fvar, **kw)             # the host entry
            assert first[2].pixels_left_out > 4 and first[2].sum_var_out > 0 and first[2].filter_ms > 0
            for stream in (None, None, side):
                st = G.denoise_nlm_regress_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, d_vout, stream=stream, **kw)
                assert same_bits((hip_rt.to_host(G, d_out, img.shape), hip_rt.to_host(G, d_vout, img.shape), st), first)
            for p in (d_out, d_vout):
                hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(img.nbytes)))
            assert G.denoise_nlm_regress_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, d_vout, stats=False, **kw) is None
            assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True)
            assert np.array_equal(hip_rt.to_host(G, d_vout, img.shape), first[1], equal_nan=True)
            # var_out is optional: with the sums asked for the second sweep still runs, without them it is left out
            hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(img.nbytes)))
            st = G.denoise_nlm_regress_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, **kw)
            assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True) and st.sum_var_out == first[2].sum_var_out
            hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(img.nbytes)))
            assert G.denoise_nlm_regress_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, stats=False, **kw) is None
            assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True)
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    for p in (d_img, d_var, d_feat, d_fvar, d_out, d_vout):
        hip_rt.free(G, p)


def test_a_film_past_the_block_cap(G):
    """1025 x 345: 65 x 22 = 1430 tiles on 1024 blocks, so 406 blocks take a second tile (and stage it afresh)."""
    w, h, r, f = 1025, 345, 1, 0
    img, var = noisy_film(w, h, 11)
    feat, fvar = noisy_features(w, h, 11, channels=3)
    img[200, 1000, 0] = np.nan
    fvar[1, 344, 1024] = -1.0
    channels, scales = [1, 2], [1.0, 0.5]
    want = NR.denoise(img, var, feat, fvar, [(0, 1, 1e-3)], channels, scales, 1e-2, r=r, f=f, **KW)
    assert want["left_out"] == 2
    guide, regress = G.nlm_guide(num_channels=3, groups=[(0, 1, 1e-3)]), G.nlm_regress(channels=channels, scales=scales, ridge=1e-2)
    worst = 0.0
    for direct in FORMS:
        with G.debug_knobs(nlm_direct=direct):
            worst = max(worst, figure(*G.denoise_nlm_regress(img, var, feat, fvar, guide=guide, regress=regress, window_radius=r, patch_radius=f, **KW),
                                      want))
    print(f"nlm regression past the block cap: worst figure {worst:.3e} (bound {NLM_REGRESS_BOUND})")
    assert NLM_REGRESS_BOUND is not None, f"NLM_REGRESS_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < NLM_REGRESS_BOUND


def session_body(G, ses, scene, budget):
    """`ses` holds at least two passes: denoise_regress() is Scene.features with the window {budget, 0} fed to
    denoise_nlm_regress_device with the planes read() returns, bit for bit, in host and in device memory."""
    h, w, _ = ses.shape
    fspp = 4
    kw = dict(window_radius=4, patch_radius=2, k=2.0)
    guide, regress = G.nlm_guide(groups=GROUPS[1], k_f=0.7), G.nlm_regress(channels=[0, 1, 2, 3, 4, 5, 6], scales=[1.0] * 6 + [4.0], ridge=1e-2)
    out, var_out, fm, fv, st = ses.denoise_regress(fspp, guide=guide, regress=regress, features=True, **kw)
    want_fm, want_fv = scene.features(fspp, window=(budget, 0))
    assert np.array_equal(fm, want_fm) and np.array_equal(fv, want_fv) and fv.any()
    means, vars_, _ = ses.read()
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (means["img"], vars_["img"], fm, fv))
    d_out, d_vout = hip_rt.alloc(G, out.nbytes), hip_rt.alloc(G, out.nbytes)
    st2 = G.denoise_nlm_regress_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, d_vout, guide=guide, regress=regress, **kw)
    assert same_bits((hip_rt.to_host(G, d_out, out.shape), hip_rt.to_host(G, d_vout, out.shape), st2), (out, var_out, st))
    assert st.pixels_left_out == 0 and np.isfinite(out).all() and np.isfinite(var_out).all() and (var_out >= 0).all()
    guided = ses.denoise_guided(fspp, guide=guide, **kw)
    assert not np.array_equal(guided[0], out)                     # the fit is at work
    # everything in device memory
    nf = fm.nbytes
    d_fm, d_fv = hip_rt.alloc(G, nf), hip_rt.alloc(G, nf)
    hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(out.nbytes)))
    st3 = ses.denoise_regress(fspp, guide=guide, regress=regress, out_ptr=d_out, var_out_ptr=d_vout, features_ptrs=(d_fm, d_fv), **kw)
    assert np.array_equal(hip_rt.to_host(G, d_out, out.shape), out) and st3.sum_var_out == st.sum_var_out
    assert np.array_equal(hip_rt.to_host(G, d_fm, fm.shape), fm) and np.array_equal(hip_rt.to_host(G, d_fv, fm.shape), fv)
    assert same_bits(ses.denoise_regress(fspp, guide=guide, regress=regress, **kw), (out, var_out, st))
    for bad in (1, budget + 1):
        with pytest.raises(G.GdptError, match="feature_spp"):
            ses.denoise_regress(bad)
    with pytest.raises(G.GdptError, match="ridge"):
        ses.denoise_regress(fspp, regress=G.nlm_regress(ridge=0.0))
    with pytest.raises(G.GdptError, match="num_channels"):
        ses.denoise_regress(fspp, guide=G.nlm_guide(num_channels=7, groups=GROUPS[1]))
    for p in (d_img, d_var, d_feat, d_fvar, d_out, d_vout, d_fm, d_fv):
        hip_rt.free(G, p)


@pytest.mark.parametrize("path", [True, False], ids=["path", "gradpath"])
def test_session(G, scene_tmp, path):
    """cbox 24 x 24, budget 16 in four passes of 4: refused before the second pass, then the regression on what read() returns."""
    sd = G.parse_scene(scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path" if path else None))
    sc = G.Scene(sd)
    ses = G.Progressive(sc, 16, path=path)
    ses.add_pass(4)
    with pytest.raises(G.GdptError, match="at least 2 passes"):
        ses.denoise_regress(4)
    ses.run(pass_spp=4)
    assert ses.status()["passes"] == 4
    session_body(G, ses, sc, 16)
    ses.close()
    sc.close()


def test_group_total(G, scene_tmp):
    sd = G.parse_scene(scene_variant(scene_tmp, CBOX, width=24, height=24))
    grp = G.ProgressiveGroup(sd, (0, 0), 16)
    grp.run(pass_spp=4)
    assert grp.total.status()["passes"] == 4
    sc = G.Scene(sd)
    session_body(G, grp.total, sc, 16)
    sc.close()
    grp.close()


EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")
# sha256 of the files `lajolla --spp 16 --pass-spp 4 --denoised d.pfm --nlm-window 4 --nlm-patch 2 --nlm-guide albedo,normal -o o.pfm`
# wrote for the 24 x 24 Integrator::Path cbox of scene_variant when built from the commit before the regression, on an MI355X:
# (-o, --denoised)
PARENT_SHA256 = ("1466954794e183f3e89ce7596bc12d8768c2c4cac515a8b665b65fdeb547e67b", "52971c4cafba11a78390a7c22673eaefd395c322860ea1889fb71e1081061a49")


def test_cli_regress(G, scene_tmp, tmp_path):
    xml = scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path")
    out, den, rden = tmp_path / "o.pfm", tmp_path / "d.pfm", tmp_path / "r.pfm"
    base = [EXE, "--spp", "16", "--pass-spp", "4"]
    nlm = ["--nlm-window", "4", "--nlm-patch", "2"]
    r0 = subprocess.run([*base, "--denoised", str(den), *nlm, "--nlm-guide", "albedo,normal", "-o", str(out), xml], capture_output=True, text=True,
                        timeout=300)
    assert r0.returncode == 0, r0.stderr
    # without --nlm-regress, -o and --denoised are byte for byte what the parent build wrote
    sha = tuple(hashlib.sha256(open(p, "rb").read()).hexdigest() for p in (out, den))
    print("lajolla without --nlm-regress: sha256", sha)
    assert PARENT_SHA256 is not None, f"PARENT_SHA256 has not been recorded; this run wrote {sha}"
    assert sha == PARENT_SHA256
    # --nlm-regress: the session's regression; the albedo group alone and k = 4.0 when --nlm-guide and --nlm-k are not given
    r1 = subprocess.run([*base, "--denoised", str(rden), *nlm, "--nlm-regress", "albedo,normal", "--feature-spp", "4", "-o", str(out), xml],
                        capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == sha[0]
    sc = G.Scene(G.parse_scene(xml))
    ses = G.Progressive(sc, 16, path=True)
    ses.run(pass_spp=4)
    want, _, st = ses.denoise_regress(4, guide=G.nlm_guide(groups=GROUPS[1]), window_radius=4, patch_radius=2, k=4.0)
    assert np.array_equal(read_pfm(rden, 24, 24), want.astype(np.float32))
    line = [l for l in r1.stdout.splitlines() if l.startswith("[gdpt] denoised:")]
    assert len(line) == 1 and "first-order regression on albedo,normal (ridge 0.010000)" in line[0] and "guided by" not in line[0]
    # depth with its scale, a guide and a k of the caller's, another ridge
    r2 = subprocess.run([*base, "--denoised", str(rden), *nlm, "--nlm-regress", "albedo,normal,depth", "--nlm-depth-scale", "4", "--nlm-ridge", "0.001",
                         "--nlm-guide", "albedo,normal", "--nlm-k", "2", "--feature-spp", "4", "-o", str(out), xml], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr
    want, _, st = ses.denoise_regress(4, regress=G.nlm_regress(channels=range(7), scales=[1.0] * 6 + [4.0], ridge=1e-3), window_radius=4,
                                      patch_radius=2, k=2.0)
    assert np.array_equal(read_pfm(rden, 24, 24), want.astype(np.float32))
    ses.close()
    sc.close()
    for extra in (["--nlm-demodulate"], ["--nlm-var-smooth", "1"], ["--nlm-levels", "2"]):
        r = subprocess.run([*base, "--denoised", str(den), "--nlm-regress", "albedo,normal", *extra, "-o", str(out), xml], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 2 and "--nlm-regress is not combined with" in r.stderr, r.stderr
    r = subprocess.run([*base, "--denoised", str(den), "--nlm-regress", "depth", "-o", str(out), xml], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--nlm-depth-scale" in r.stderr, r.stderr
