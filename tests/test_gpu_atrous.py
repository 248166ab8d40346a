"""The edge-avoiding a-trous wavelet filter on the GPU (include/gdpt.h: gdpt_denoise_atrous*, gdpt_progressive_denoise_atrous): every
kernel route against the numpy restatement (tests/atrous_ref.py) and against each other, what is left out, the three exact
identities, the host and device entries, a film past the block cap, the sessions (Path, GradPath, a group's total) and the CLI."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import atrous_ref as A
import hip_rt
from helpers import ROOT, scene_variant
from test_gpu_nlm import CBOX, SUMS, as_dict, figure, planted_film
from test_gpu_nlm_demod import planted_features
from test_gpu_nlm_regress import PARENT_SHA256
from test_gpu_progressive import read_pfm
from test_nlm_demod_ref import albedo_features
from test_nlm_ref import noisy_film

pytestmark = pytest.mark.gpu

# measured on an MI355X: the worst figure of tests/test_gpu_nlm.py (masked relative L2 of out and of var_out, relative difference of
# the four film sums) between any kernel route and the restatement, and between the routes, over every case of the tests below. The
# sides differ by FMA contraction and the last place of exp and of the divisions, carried through up to six levels; 100 x the measured
# value is the margin, never looser than 1e-9. Measured: 2.534e-15 for every route against the restatement over the 128 cases, 0 between
# the routes (the staged and the direct form run the same arithmetic on the same values: the same bits), 3.525e-16 on the film past
# the block cap.
ATROUS_MEASURED = 2.6e-15
ATROUS_BOUND = min(100 * ATROUS_MEASURED, 1e-9) if ATROUS_MEASURED else None

# knob nlm_direct: 0 the product routes (staged up to the step profiles/atrous_times.txt names, direct beyond), 1 the direct form at
# every step, 2 the staged form wherever it exists (steps 1 - 8)
FORMS = (0, 1, 2)
# W x H: 17 x 17 is one pixel past a 16 x 16 tile each way; 70 x 37 is the smallest film here on which a tap at step 16 lands inside the
# film and in another tile; on the others the deep levels have the centre tap alone
FILMS = [(1, 1), (16, 16), (17, 17), (33, 9), (40, 19), (70, 37)]
LEVELS = [(1, 0), (2, 0), (3, 0), (5, 0), (6, 0), (1, 3), (2, 2)]      # (levels, first_level)
GROUPS = {0: None, 1: [(3, 3, 1e-3)], 2: [(3, 3, 1e-3), (6, 1, 5e-2)], 3: [(0, 3, 1e-3), (3, 3, 2e-3), (6, 1, 5e-2)]}
DEMODS = (None, -1, 7)                         # none; the albedo of planes 0 - 2 without a coverage plane, and with plane 7
OPTIONS = [(ng, cov) for ng in (0, 1, 2, 3) for cov in DEMODS]
KW = dict(k=1.0)


def guide_of(G, ng):
    return G.nlm_guide(groups=GROUPS[ng]) if ng else None


def demod_of(G, cov):
    return G.nlm_demod(coverage_channel=cov) if cov is not None else None


def restated(img, var, feat, fvar, ng, cov, levels, first, **kw):
    return A.denoise(img, var, feat, fvar, GROUPS[ng] or [], None if cov is None else (0, cov, 1e-3), levels=levels, first_level=first, **kw)


@pytest.fixture(scope="module")
def cases(G):
    """Films x (levels, first level) x (guide, demod), clean and planted: the restatement's result (computed once, left unchanged) and
    every route's. Every (guide, demod) pair at 5 levels on 70 x 37 and at 2 levels on 17 x 17, one pair in turn elsewhere."""
    out = []
    n = 0
    for planted in (False, True):
        for (w, h) in FILMS:
            img, var = planted_film(w, h, 10 * w + h) if planted else noisy_film(w, h, 10 * w + h)
            feat, fvar = planted_features(w, h, w + h) if planted else albedo_features(w, h, w + h)
            for (levels, first) in LEVELS:
                every = ((w, h), levels, first) in (((70, 37), 5, 0), ((17, 17), 2, 0))
                for ng, cov in (OPTIONS if every else (OPTIONS[n % len(OPTIONS)],)):
                    want = restated(img, var, feat, fvar, ng, cov, levels, first, **KW)
                    got = []
                    for form in FORMS:
                        with G.debug_knobs(nlm_direct=form):
                            got.append(G.denoise_atrous(img, var, feat, fvar, guide=guide_of(G, ng), demod=demod_of(G, cov), levels=levels,
                                                        first_level=first, **KW))
                        st = got[-1][2]
                        assert (st.window_radius, st.patch_radius) == (2 << (first + levels - 1), 0) and st.filter_ms > 0
                    out.append(((w, h, levels, first, ng, cov, planted), img, var, feat, fvar, want, got))
                    n += 1
    return out


def test_every_route_against_the_restatement(cases):
    worst = {f: 0.0 for f in FORMS}
    left = 0
    seen = set()
    for key, img, var, feat, fvar, want, got in cases:
        w, h, levels, first, ng, cov, planted = key
        seen.add((ng, cov))
        ok = A.valid_mask(img, var, feat, fvar, GROUPS[ng] or [], None if cov is None else (0, cov, 1e-3))
        assert want["left_out"] == (~ok).sum() and (not planted or want["left_out"] >= 1)
        left += want["left_out"]
        for form in FORMS:
            o, vo, st = got[form]
            assert np.array_equal(o[~ok], img[~ok], equal_nan=True) and np.array_equal(vo[~ok], var[~ok], equal_nan=True), key
            assert np.isfinite(o[ok]).all() and np.isfinite(vo[ok]).all(), key
            worst[form] = max(worst[form], figure(o, vo, st, want))
    assert left > 100 and seen == set(OPTIONS)
    print(f"a-trous against the restatement over {len(cases)} cases: worst figure product routes {worst[0]:.3e}, direct {worst[1]:.3e}, "
          f"staged {worst[2]:.3e} (bound {ATROUS_BOUND})")
    assert ATROUS_BOUND is not None, f"ATROUS_MEASURED has not been recorded; this run measured {max(worst.values()):.3e}"
    assert max(worst.values()) < ATROUS_BOUND


def test_the_routes_agree(cases):
    worst = 0.0
    for key, img, var, feat, fvar, want, got in cases:
        for form in (0, 2):
            worst = max(worst, figure(*got[form], as_dict(*got[1])))
    print(f"a-trous staged against direct: worst figure {worst:.3e} (bound {ATROUS_BOUND})")
    assert ATROUS_BOUND is not None, f"ATROUS_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < ATROUS_BOUND


def same_bits(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True) and \
        [getattr(a[2], k) for k in SUMS] == [getattr(b[2], k) for k in SUMS] and a[2].pixels_left_out == b[2].pixels_left_out


@pytest.mark.parametrize("form", FORMS, ids=["product", "direct", "staged"])
def test_identities_bit_for_bit(G, form):
    w, h = 70, 37
    img, var = planted_film(w, h, 3)
    feat, fvar = albedo_features(w, h, 3)
    with G.debug_knobs(nlm_direct=form):
        for ng in (0, 2):
            guide = guide_of(G, ng)
            # one call of n levels is n calls of one level, each fed the one before
            for (levels, first) in ((5, 0), (3, 2)):
                whole = G.denoise_atrous(img, var, feat, fvar, guide=guide, levels=levels, first_level=first, **KW)
                assert whole[2].pixels_left_out > 0
                u, v, st = img, var, None
                for i in range(levels):
                    u, v, st = G.denoise_atrous(u, v, feat, fvar, guide=guide, levels=1, first_level=first + i, **KW)
                    assert st.window_radius == 2 << (first + i)
                assert np.array_equal(u, whole[0], equal_nan=True) and np.array_equal(v, whole[1], equal_nan=True), (ng, levels, first)
                assert (st.sum_var_out, st.sum_sq_out, st.pixels_left_out) == (whole[2].sum_var_out, whole[2].sum_sq_out, whole[2].pixels_left_out)
                assert not np.array_equal(whole[0], G.denoise_atrous(img, var, feat, fvar, guide=guide, levels=levels - 1, first_level=first, **KW)[0],
                                          equal_nan=True)
        kw = dict(levels=5, **KW)
        plain = G.denoise_atrous(img, var, **kw)
        # no group: the planes are not looked at, and need not be given
        assert same_bits(G.denoise_atrous(img, var, feat, fvar, guide=G.nlm_guide(groups=[]), **kw), plain)
        assert same_bits(G.denoise_atrous(img, var, None, None, guide=G.nlm_guide(groups=[]), **kw), plain)
        # features that are constant over the film with variance 0
        flat = np.stack([np.full((h, w), 0.1 * (c + 1)) for c in range(8)])
        assert same_bits(G.denoise_atrous(img, var, flat, 0.0 * flat, guide=G.nlm_guide(groups=GROUPS[3]), **kw), plain)
        assert not same_bits(G.denoise_atrous(img, var, feat, fvar, guide=G.nlm_guide(groups=GROUPS[3]), **kw), plain)
        # a unit divisor: albedo 1 with coverage 1, albedo 0 with coverage 0, albedo 1 without a coverage plane
        for ng in (0, 2):
            guide = guide_of(G, ng)
            undemod = G.denoise_atrous(img, var, feat, fvar, guide=guide, **kw)
            for albedo, cov, channel in ((1.0, 1.0, 7), (0.0, 0.0, 7), (1.0, 0.3, -1)):
                ft = feat.copy()
                ft[0:3], ft[7] = albedo, cov
                assert same_bits(G.denoise_atrous(img, var, ft, fvar, guide=guide, demod=G.nlm_demod(coverage_channel=channel), **kw), undemod), (ng, albedo)
            dem = G.denoise_atrous(img, var, feat, fvar, guide=guide, demod=G.nlm_demod(), **kw)
            assert (dem[2].sum_var_in, dem[2].sum_sq_in, dem[2].pixels_left_out) == (undemod[2].sum_var_in, undemod[2].sum_sq_in, undemod[2].pixels_left_out)
            assert not np.array_equal(dem[0], undemod[0], equal_nan=True)


def test_host_and_device_entries_same_bits_second_stream_and_enqueue_only(G):
    w, h = 70, 37
    img, var = planted_film(w, h, 5)
    feat, fvar = planted_features(w, h, 5)
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (img, var, feat, fvar))
    d_out, d_vout = hip_rt.alloc(G, img.nbytes), hip_rt.alloc(G, img.nbytes)
    side = hip_rt.stream(G)
    for ng, cov, levels in ((0, None, 5), (2, 7, 5), (1, None, 2)):
        kw = dict(guide=guide_of(G, ng), demod=demod_of(G, cov), levels=levels, **KW)
        for form in FORMS:
            with G.debug_knobs(nlm_direct=form):
                first = G.denoise_atrous(img, var, feat, fvar, **kw)             # the host entry
                assert first[2].pixels_left_out > 4 and first[2].sum_var_out > 0 and first[2].filter_ms > 0
                for stream in (None, None, side):
                    st = G.denoise_atrous_device(w, h, d_img, d_var, d_feat, d_fvar, 8, d_out, d_vout, stream=stream, **kw)
                    assert same_bits((hip_rt.to_host(G, d_out, img.shape), hip_rt.to_host(G, d_vout, img.shape), st), first)
                for p in (d_out, d_vout):
                    hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(img.nbytes)))
                assert G.denoise_atrous_device(w, h, d_img, d_var, d_feat, d_fvar, 8, d_out, d_vout, stats=False, **kw) is None
                assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True)
                assert np.array_equal(hip_rt.to_host(G, d_vout, img.shape), first[1], equal_nan=True)
                hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(img.nbytes)))
                st = G.denoise_atrous_device(w, h, d_img, d_var, d_feat, d_fvar, 8, d_out, **kw)       # var_out is optional
                assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True) and st.sum_var_out == first[2].sum_var_out
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    for p in (d_img, d_var, d_feat, d_fvar, d_out, d_vout):
        hip_rt.free(G, p)


def test_a_film_past_the_block_cap(G):
    """1025 x 345: 65 x 22 = 1430 tiles on 1024 blocks, so 406 blocks take a second tile (and stage it afresh)."""
    w, h = 1025, 345
    img, var = noisy_film(w, h, 11)
    rng = np.random.default_rng(12)
    feat = 0.5 + 0.05 * rng.standard_normal((3, h, w))
    fvar = 0.03 * 0.03 * rng.uniform(0.25, 1.0, feat.shape)
    img[200, 1000, 0] = np.nan
    fvar[1, 344, 1024] = -1.0
    groups = [(0, 2, 1e-3)]
    want = A.denoise(img, var, feat, fvar, groups, levels=2, **KW)
    assert want["left_out"] == 2
    worst = 0.0
    for form in (0, 1):
        with G.debug_knobs(nlm_direct=form):
            worst = max(worst, figure(*G.denoise_atrous(img, var, feat, fvar, guide=G.nlm_guide(num_channels=3, groups=groups), levels=2, **KW), want))
    print(f"a-trous past the block cap: worst figure {worst:.3e} (bound {ATROUS_BOUND})")
    assert ATROUS_BOUND is not None, f"ATROUS_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < ATROUS_BOUND


def session_body(G, ses, scene, budget):
    """`ses` holds at least two passes: denoise_atrous() is Scene.features with the window {budget, 0} fed to denoise_atrous_device
    with the planes read() returns, bit for bit, in host and in device memory; with neither a guide nor a demod block no features."""
    h, w, _ = ses.shape
    fspp = 4
    kw = dict(levels=3, k=1.5)
    means, vars_, _ = ses.read()
    want_fm, want_fv = scene.features(fspp, window=(budget, 0))
    d_img, d_var = hip_rt.upload(G, means["img"]), hip_rt.upload(G, vars_["img"])
    d_out, d_vout = hip_rt.alloc(G, means["img"].nbytes), hip_rt.alloc(G, means["img"].nbytes)
    outs = []
    for guide, demod in ((G.nlm_guide(k_f=0.7), None), (G.nlm_guide(groups=[(3, 3, 1e-3)]), G.nlm_demod()), (None, G.nlm_demod(floor=0.05))):
        out, var_out, fm, fv, st = ses.denoise_atrous(fspp, guide=guide, demod=demod, features=True, **kw)
        assert np.array_equal(fm, want_fm) and np.array_equal(fv, want_fv) and fv.any()
        d_feat, d_fvar = hip_rt.upload(G, fm), hip_rt.upload(G, fv)
        st2 = G.denoise_atrous_device(w, h, d_img, d_var, d_feat, d_fvar, 8, d_out, d_vout, guide=guide, demod=demod, **kw)
        assert same_bits((hip_rt.to_host(G, d_out, out.shape), hip_rt.to_host(G, d_vout, out.shape), st2), (out, var_out, st))
        assert st.pixels_left_out == 0 and np.isfinite(out).all() and np.isfinite(var_out).all() and (var_out >= 0).all()
        assert (st.window_radius, st.patch_radius) == (8, 0)
        # everything in device memory
        d_fm, d_fv = hip_rt.alloc(G, fm.nbytes), hip_rt.alloc(G, fm.nbytes)
        hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(out.nbytes)))
        st3 = ses.denoise_atrous(fspp, guide=guide, demod=demod, out_ptr=d_out, var_out_ptr=d_vout, features_ptrs=(d_fm, d_fv), **kw)
        assert np.array_equal(hip_rt.to_host(G, d_out, out.shape), out) and st3.sum_var_out == st.sum_var_out
        assert np.array_equal(hip_rt.to_host(G, d_fm, fm.shape), fm) and np.array_equal(hip_rt.to_host(G, d_fv, fm.shape), fv)
        assert same_bits(ses.denoise_atrous(fspp, guide=guide, demod=demod, **kw), (out, var_out, st))
        outs.append(out)
        for p in (d_feat, d_fvar, d_fm, d_fv):
            hip_rt.free(G, p)
    # neither: no features are rendered and feature_spp is ignored
    for spp in (0, budget + 7):
        out, var_out, st = ses.denoise_atrous(spp, **kw)
        st2 = G.denoise_atrous_device(w, h, d_img, d_var, None, None, 0, d_out, d_vout, **kw)
        assert same_bits((hip_rt.to_host(G, d_out, out.shape), hip_rt.to_host(G, d_vout, out.shape), st2), (out, var_out, st))
    assert same_bits(ses.denoise_atrous(0, guide=G.nlm_guide(groups=[]), **kw), (out, var_out, st))
    hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(out.nbytes)))
    ses.denoise_atrous(out_ptr=d_out, **kw)
    assert np.array_equal(hip_rt.to_host(G, d_out, out.shape), out)
    outs.append(out)
    assert all(not np.array_equal(outs[i], outs[j]) for i in range(4) for j in range(i))      # every block reaches the kernel
    with pytest.raises(G.GdptError, match="features need"):
        ses.denoise_atrous(fspp, features=True, **kw)
    for bad in (1, budget + 1):
        with pytest.raises(G.GdptError, match="feature_spp"):
            ses.denoise_atrous(bad, guide=G.nlm_guide())
    with pytest.raises(G.GdptError, match="levels"):
        ses.denoise_atrous(fspp, levels=7)
    with pytest.raises(G.GdptError, match="floor"):
        ses.denoise_atrous(fspp, demod=G.nlm_demod(floor=0.0))
    with pytest.raises(G.GdptError, match="num_channels"):
        ses.denoise_atrous(fspp, guide=G.nlm_guide(num_channels=7, groups=[(3, 3, 1e-3)]))
    for p in (d_img, d_var, d_out, d_vout):
        hip_rt.free(G, p)


@pytest.mark.parametrize("path", [True, False], ids=["path", "gradpath"])
def test_session(G, scene_tmp, path):
    """cbox 24 x 24, budget 16 in four passes of 4: refused before the second pass, then the filter on what read() returns."""
    sd = G.parse_scene(scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path" if path else None))
    sc = G.Scene(sd)
    ses = G.Progressive(sc, 16, path=path)
    ses.add_pass(4)
    for guide in (None, G.nlm_guide()):
        with pytest.raises(G.GdptError, match="at least 2 passes"):
            ses.denoise_atrous(4, guide=guide)
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


def test_cli_atrous(G, scene_tmp, tmp_path):
    xml = scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path")
    out, den, aden = tmp_path / "o.pfm", tmp_path / "d.pfm", tmp_path / "a.pfm"
    base = [EXE, "--spp", "16", "--pass-spp", "4"]
    # without --atrous-levels, -o and --denoised are byte for byte what the parent build wrote: the command and the hashes of
    # tests/test_gpu_nlm_regress.py, which the parent commit passes
    r0 = subprocess.run([*base, "--denoised", str(den), "--nlm-window", "4", "--nlm-patch", "2", "--nlm-guide", "albedo,normal", "-o", str(out), xml],
                        capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stderr
    sha = tuple(hashlib.sha256(open(p, "rb").read()).hexdigest() for p in (out, den))
    print("lajolla without --atrous-levels: sha256", sha)
    assert sha == PARENT_SHA256
    sc = G.Scene(G.parse_scene(xml))
    ses = G.Progressive(sc, 16, path=True)
    ses.run(pass_spp=4)
    # --atrous-levels alone: the default guide (albedo, normal), k 2.0
    r1 = subprocess.run([*base, "--denoised", str(aden), "--atrous-levels", "3", "--feature-spp", "4", "-o", str(out), xml], capture_output=True, text=True,
                        timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == sha[0]
    want, _, st = ses.denoise_atrous(4, guide=G.nlm_guide(), levels=3)
    assert np.array_equal(read_pfm(aden, 24, 24), want.astype(np.float32))
    assert not np.array_equal(read_pfm(aden, 24, 24), read_pfm(den, 24, 24))
    line = [l for l in r1.stdout.splitlines() if l.startswith("[gdpt] denoised:")]
    assert len(line) == 1 and "a-trous wavelet filter over 3 levels" in line[0] and "window 8, patch 0" in line[0]
    # demodulated: the default guide drops the albedo group; another k and floor
    r2 = subprocess.run([*base, "--denoised", str(aden), "--atrous-levels", "2", "--atrous-k", "1.5", "--nlm-demodulate", "--nlm-albedo-floor", "0.05",
                         "--feature-spp", "4", "-o", str(out), xml], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr
    want, _, st = ses.denoise_atrous(4, guide=G.nlm_guide(groups=[(3, 3, 1e-3)]), demod=G.nlm_demod(floor=0.05), levels=2, k=1.5)
    assert np.array_equal(read_pfm(aden, 24, 24), want.astype(np.float32))
    # a guide of the caller's
    r3 = subprocess.run([*base, "--denoised", str(aden), "--atrous-levels", "5", "--nlm-guide", "normal", "--nlm-kf", "0.7", "--feature-spp", "4", "-o", str(out),
                         xml], capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0, r3.stderr
    want, _, st = ses.denoise_atrous(4, guide=G.nlm_guide(groups=[(3, 3, 1e-3)], k_f=0.7), levels=5)
    assert np.array_equal(read_pfm(aden, 24, 24), want.astype(np.float32))
    ses.close()
    sc.close()
