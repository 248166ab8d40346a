"""The feature-guided non-local-means filter on the GPU (include/gdpt.h: gdpt_denoise_nlm_guided*, gdpt_progressive_denoise_guided):
both kernel forms against the numpy restatement (tests/nlm_guided_ref.py) and against each other, the identities with the unguided
filter bit for bit, the host and device entries, the sessions (Path, GradPath, a group's total) and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import hip_rt
import nlm_guided_ref as NG
from helpers import ROOT, scene_variant
from test_gpu_nlm import CBOX, FORMS, SUMS, as_dict, figure, planted_film
from test_gpu_progressive import read_pfm
from test_nlm_guided_ref import noisy_features, step_films
from test_nlm_ref import noisy_film

pytestmark = pytest.mark.gpu

# measured on an MI355X: the worst figure of tests/test_gpu_nlm.py (masked relative L2 of out and of var_out, relative difference of
# the four film sums) between either guided kernel form and the restatement, and between the two forms, over every case of the two
# tests below. The sides differ by FMA contraction (in the feature distance too), the order of the patch sums and the last place of
# exp; 100 x the measured value is the margin, never looser than 1e-9. Measured: 3.429e-16 for either form against the
# restatement, 2.643e-16 between the forms, over the 88 cases.
NLM_GUIDED_MEASURED = 3.5e-16
NLM_GUIDED_BOUND = min(100 * NLM_GUIDED_MEASURED, 1e-9) if NLM_GUIDED_MEASURED else None

FILMS = [(1, 1), (16, 16), (17, 17), (40, 19)]
RADII = [(0, 0), (1, 0), (2, 1), (3, 3), (10, 3)]
GROUPS = {0: [], 1: [(0, 3, 1e-3)], 2: [(0, 3, 1e-3), (3, 3, 1e-3)], 3: [(0, 3, 1e-3), (3, 3, 2e-3), (6, 1, 5e-2)]}      # 3: the 3 + 3 + 1 layout over 8 planes
KW = dict(k=0.8)


def planted_features(w, h, seed):
    """NaN, +-Inf and a negative variance in channels the groups name, at a corner, an edge, the middle and a tile's halo; and the
    same in channel 7, which no group names."""
    feat, fvar = noisy_features(w, h, seed)
    spots = [(0, 0, 0, "nan"), (4, 0, w // 2, "neg"), (6, h // 2, w // 2, "-inf"), (2, h - 1, w - 1, "+inf")]
    if w > 16:
        spots += [(1, min(5, h - 1), 16, "neg"), (5, h // 2, 15, "nan")]
    if h > 16:
        spots += [(3, 16, 3, "+inf")]
    spots += [(7, 0, w - 1, "nan"), (7, h - 1, 0, "neg"), (7, h // 2, w // 3, "+inf")]
    for c, y, x, kind in spots:
        if kind == "nan":
            feat[c, y, x] = np.nan
        elif kind == "+inf":
            fvar[c, y, x] = np.inf
        elif kind == "-inf":
            feat[c, y, x] = -np.inf
        else:
            fvar[c, y, x] = -1e-6
    return feat, fvar


@pytest.fixture(scope="module")
def cases(G):
    """Films x (r, f) x group sets, clean and planted: the restatement's result (computed once, left unchanged) and both forms'."""
    out = []
    n = 0
    for planted in (False, True):
        for (w, h) in FILMS:
            img, var = planted_film(w, h, 10 * w + h) if planted else noisy_film(w, h, 10 * w + h)
            feat, fvar = planted_features(w, h, w + h) if planted else noisy_features(w, h, w + h)
            for (r, f) in RADII:
                for ng in ((n % 4,) if (r, f) not in ((2, 1), (10, 3)) else (0, 1, 2, 3)):       # every group count at two radii, one in turn at the others
                    groups = GROUPS[ng]
                    want = NG.denoise(img, var, feat, fvar, groups, r=r, f=f, **KW)
                    guide = G.nlm_guide(groups=groups)
                    got = []
                    for direct in FORMS:
                        with G.debug_knobs(nlm_direct=direct):
                            got.append(G.denoise_nlm_guided(img, var, feat, fvar, guide=guide, window_radius=r, patch_radius=f, **KW))
                    out.append(((w, h, r, f, ng, planted), img, var, feat, fvar, want, got))
                n += 1
    return out


def test_both_forms_against_the_restatement(cases):
    worst = {0: 0.0, 1: 0.0}
    left = 0
    for key, img, var, feat, fvar, want, got in cases:
        w, h, r, f, ng, planted = key
        ok = NG.valid_mask(img, var, feat, fvar, GROUPS[ng])
        assert want["left_out"] == (~ok).sum()
        left += want["left_out"]
        for direct in FORMS:
            o, vo, st = got[direct]
            assert np.array_equal(o[~ok], img[~ok], equal_nan=True) and np.array_equal(vo[~ok], var[~ok], equal_nan=True), key
            if r == 0:
                assert np.array_equal(o, img, equal_nan=True) and np.array_equal(vo, var, equal_nan=True), key
            worst[direct] = max(worst[direct], figure(o, vo, st, want))
    assert left > 50
    print(f"guided nlm against the restatement: worst figure tiled {worst[0]:.3e}, direct {worst[1]:.3e} (bound {NLM_GUIDED_BOUND})")
    assert NLM_GUIDED_BOUND is not None, f"NLM_GUIDED_MEASURED has not been recorded; this run measured {max(worst.values()):.3e}"
    assert max(worst.values()) < NLM_GUIDED_BOUND


def test_the_two_forms_agree(cases):
    worst = 0.0
    for key, img, var, feat, fvar, want, got in cases:
        worst = max(worst, figure(*got[0], as_dict(*got[1])))
    print(f"guided nlm tiled against direct: worst figure {worst:.3e} (bound {NLM_GUIDED_BOUND})")
    assert NLM_GUIDED_BOUND is not None, f"NLM_GUIDED_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < NLM_GUIDED_BOUND


def same_bits(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True) and \
        [getattr(a[2], k) for k in SUMS] == [getattr(b[2], k) for k in SUMS] and a[2].pixels_left_out == b[2].pixels_left_out


@pytest.mark.parametrize("direct", FORMS, ids=["tiled", "direct"])
def test_identities_with_the_unguided_filter_bit_for_bit(G, direct):
    w, h = 40, 19
    img, var = planted_film(w, h, 3)
    feat, fvar = planted_features(w, h, 3)
    const = np.stack([np.full((h, w), 0.1 * (c + 1)) for c in range(8)])
    with G.debug_knobs(nlm_direct=direct):
        for (r, f) in ((3, 1), (10, 3)):
            kw = dict(window_radius=r, patch_radius=f, k=0.7)
            plain = G.denoise_nlm(img, var, **kw)
            assert plain[2].pixels_left_out > 0
            # no group: the feature planes are not looked at (they hold NaN), and need not be given
            assert same_bits(G.denoise_nlm_guided(img, var, feat, fvar, guide=G.nlm_guide(groups=[]), **kw), plain)
            assert same_bits(G.denoise_nlm_guided(img, var, None, None, guide=G.nlm_guide(groups=[]), **kw), plain)
            # features constant over the film, variance 0: every feature distance is 0
            for ng in (1, 3):
                assert same_bits(G.denoise_nlm_guided(img, var, const, np.zeros_like(const), guide=G.nlm_guide(groups=GROUPS[ng]), **kw), plain)
        # a feature step of height 1: the left side's output does not depend on the right side's colours
        a_img, b_img, s_var, s_feat, s_fvar, left = step_films()
        guide = G.nlm_guide(num_channels=1, groups=[(0, 1, 1e-3)], k_f=0.6)
        kw = dict(window_radius=6, patch_radius=0, k=1.0)
        a, b = (G.denoise_nlm_guided(x, s_var, s_feat, s_fvar, guide=guide, **kw) for x in (a_img, b_img))
        assert np.array_equal(a[0][left], b[0][left]) and np.array_equal(a[1][left], b[1][left])
        assert not np.array_equal(a[0][~left], b[0][~left])
        pa, pb = (G.denoise_nlm(x, s_var, **kw) for x in (a_img, b_img))
        assert not np.array_equal(pa[0][left], pb[0][left])


def test_host_and_device_entries_same_bits_second_stream_and_enqueue_only(G):
    w, h, r, f = 40, 19, 3, 1
    img, var = planted_film(w, h, 5)
    feat, fvar = planted_features(w, h, 5)
    guide = G.nlm_guide(groups=GROUPS[3])
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (img, var, feat, fvar))
    d_out, d_vout = hip_rt.alloc(G, img.nbytes), hip_rt.alloc(G, img.nbytes)
    side = hip_rt.stream(G)
    kw = dict(window_radius=r, patch_radius=f, **KW)
    for direct in FORMS:
        with G.debug_knobs(nlm_direct=direct):
            first = G.denoise_nlm_guided(img, var, feat, fvar, guide=guide, **kw)             # the host entry
            assert first[2].pixels_left_out > 4 and first[2].sum_var_out > 0 and first[2].filter_ms > 0
            for stream in (None, None, side):
                st = G.denoise_nlm_guided_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, d_vout, guide=guide, stream=stream, **kw)
                assert same_bits((hip_rt.to_host(G, d_out, img.shape), hip_rt.to_host(G, d_vout, img.shape), st), first)
            for p in (d_out, d_vout):
                hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(img.nbytes)))
            assert G.denoise_nlm_guided_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, d_vout, guide=guide, stats=False, **kw) is None
            assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True)
            assert np.array_equal(hip_rt.to_host(G, d_vout, img.shape), first[1], equal_nan=True)
            hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(img.nbytes)))
            st = G.denoise_nlm_guided_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, guide=guide, **kw)       # var_out is optional
            assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True) and st.sum_var_out == first[2].sum_var_out
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    for p in (d_img, d_var, d_feat, d_fvar, d_out, d_vout):
        hip_rt.free(G, p)


def session_body(G, ses, scene, budget):
    """`ses` holds at least two passes: denoise_guided() is Scene.features with the window {budget, 0} fed to denoise_nlm_guided_device
    with the planes read() returns, bit for bit, in host and in device memory."""
    h, w, _ = ses.shape
    fspp = 4
    kw = dict(window_radius=4, patch_radius=2, k=1.0)
    guide = G.nlm_guide(k_f=0.7)
    out, var_out, fm, fv, st = ses.denoise_guided(fspp, guide=guide, features=True, **kw)
    want_fm, want_fv = scene.features(fspp, window=(budget, 0))
    assert np.array_equal(fm, want_fm) and np.array_equal(fv, want_fv) and fv.any()
    means, vars_, _ = ses.read()
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (means["img"], vars_["img"], fm, fv))
    d_out, d_vout = hip_rt.alloc(G, out.nbytes), hip_rt.alloc(G, out.nbytes)
    st2 = G.denoise_nlm_guided_device(w, h, d_img, d_var, d_feat, d_fvar, d_out, d_vout, guide=guide, **kw)
    assert same_bits((hip_rt.to_host(G, d_out, out.shape), hip_rt.to_host(G, d_vout, out.shape), st2), (out, var_out, st))
    assert st.pixels_left_out == 0 and np.isfinite(out).all()
    plain = ses.denoise(**kw)
    assert not np.array_equal(plain[0], out)                      # the guide is at work
    # everything in device memory
    nf = fm.nbytes
    d_fm, d_fv = hip_rt.alloc(G, nf), hip_rt.alloc(G, nf)
    hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(out.nbytes)))
    st3 = ses.denoise_guided(fspp, guide=guide, out_ptr=d_out, var_out_ptr=d_vout, features_ptrs=(d_fm, d_fv), **kw)
    assert np.array_equal(hip_rt.to_host(G, d_out, out.shape), out) and st3.sum_var_out == st.sum_var_out
    assert np.array_equal(hip_rt.to_host(G, d_fm, fm.shape), fm) and np.array_equal(hip_rt.to_host(G, d_fv, fm.shape), fv)
    assert same_bits(ses.denoise_guided(fspp, guide=guide, **kw), (out, var_out, st))
    for bad in (1, budget + 1):
        with pytest.raises(G.GdptError, match="feature_spp"):
            ses.denoise_guided(bad)
    with pytest.raises(G.GdptError, match="k_f"):
        ses.denoise_guided(fspp, guide=G.nlm_guide(k_f=0.0))
    for p in (d_img, d_var, d_feat, d_fvar, d_out, d_vout, d_fm, d_fv):
        hip_rt.free(G, p)


@pytest.mark.parametrize("path", [True, False], ids=["path", "gradpath"])
def test_session(G, scene_tmp, path):
    """cbox 24 x 24, budget 16 in four passes of 4: refused before the second pass, then the guided filter on what read() returns."""
    sd = G.parse_scene(scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path" if path else None))
    sc = G.Scene(sd)
    ses = G.Progressive(sc, 16, path=path)
    ses.add_pass(4)
    with pytest.raises(G.GdptError, match="at least 2 passes"):
        ses.denoise_guided(4)
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
# sha256 of the files `lajolla --spp 16 --pass-spp 4 --denoised d.pfm --nlm-window 4 --nlm-patch 2 --nlm-k 0.5 -o o.pfm` wrote for the
# 24 x 24 Integrator::Path cbox of scene_variant when built from the commit before the guided filter, on an MI355X: (-o, --denoised)
PARENT_SHA256 = ("1466954794e183f3e89ce7596bc12d8768c2c4cac515a8b665b65fdeb547e67b", "cd92c8f698a65d1c4514da1ac3425a4af3a404f72115424dbd64f45737aec9ce")


def test_cli_features_and_guided(G, scene_tmp, tmp_path):
    import hashlib
    xml = scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path")
    out, den, gden, prefix = tmp_path / "o.pfm", tmp_path / "d.pfm", tmp_path / "g.pfm", tmp_path / "f"
    base = [EXE, "--spp", "16", "--pass-spp", "4"]
    nlm = ["--nlm-window", "4", "--nlm-patch", "2"]
    r0 = subprocess.run([*base, "--denoised", str(den), *nlm, "--nlm-k", "0.5", "-o", str(out), xml], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stderr
    # without --nlm-guide, -o and --denoised are byte for byte what the parent build wrote
    sha = tuple(hashlib.sha256(open(p, "rb").read()).hexdigest() for p in (out, den))
    print("lajolla without --nlm-guide: sha256", sha)
    assert PARENT_SHA256 is not None, f"PARENT_SHA256 has not been recorded; this run wrote {sha}"
    assert sha == PARENT_SHA256
    # --features: three readable files, the means of the feature render along the render's own camera rays
    r1 = subprocess.run([*base, "--features", str(prefix), "--feature-spp", "4", "--denoised", str(gden), *nlm, "--nlm-guide", "albedo,normal",
                         "--nlm-kf", "0.7", "-o", str(out), xml], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == sha[0]
    sc = G.Scene(G.parse_scene(xml))
    fm, fv = sc.features(4, window=(16, 0))
    depth = read_pfm(str(prefix) + "_depth.pfm", 24, 24)
    assert np.array_equal(depth, np.repeat(fm[6][:, :, None], 3, axis=2).astype(np.float32)) and (depth > 0).any()
    for name, lo in (("albedo", 0), ("normal", 3)):
        img = G.imread(str(prefix) + f"_{name}.exr")
        want = np.moveaxis(fm[lo:lo + 3], 0, 2)
        assert img.shape == (24, 24, 3) and np.abs(img - want).max() <= 2.0 ** -10 * max(1.0, np.abs(want).max())       # fp16 files
    # --nlm-guide: the session's guided filter, k = 1.0 when --nlm-k is not given
    ses = G.Progressive(sc, 16, path=True)
    ses.run(pass_spp=4)
    want, _, st = ses.denoise_guided(4, guide=G.nlm_guide(k_f=0.7), window_radius=4, patch_radius=2, k=1.0)
    assert np.array_equal(read_pfm(gden, 24, 24), want.astype(np.float32))
    line = [l for l in r1.stdout.splitlines() if l.startswith("[gdpt] denoised:")]
    assert len(line) == 1 and "guided by albedo,normal" in line[0]
    assert len([l for l in r1.stdout.splitlines() if l.startswith("[gdpt] features: 4 samples per pixel")]) == 1
    ses.close()
    sc.close()
    for extra, msg in ((["--nlm-guide", "albedo,depth"], "--nlm-depth-tau"), (["--nlm-guide", "albedo,colour"], "albedo, normal and depth"),
                       (["--nlm-kf", "0.5"], "need --nlm-guide")):
        r = subprocess.run([*base, "--denoised", str(den), *extra, "-o", str(out), xml], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, r.stderr
    r = subprocess.run([*base, "--nlm-guide", "albedo", "-o", str(out), xml], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--nlm-guide needs --denoised" in r.stderr
