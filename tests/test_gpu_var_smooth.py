"""The variance smoothing on the GPU (include/gdpt.h: gdpt_variance_smooth*, gdpt_progressive_denoise_smoothed): the kernel against the
numpy restatement (tests/var_smooth_ref.py), the exact properties of the definition bit for bit, the same bits from two calls, a
second stream, the host and device entries and the enqueue-only form, the sessions (Path, GradPath, a group's total) against the
composed device calls, and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import hip_rt
import nlm_ref as N
import var_smooth_ref as VS
from helpers import ROOT, scene_variant
from test_gpu_nlm import CBOX, SUMS, masked_rel_l2, rel_diff
from test_gpu_nlm_demod import room_desc
from test_gpu_progressive import read_pfm
from test_nlm_demod_ref import albedo_features
from test_nlm_ref import noisy_film
from test_var_smooth_ref import planted

pytestmark = pytest.mark.gpu

# The worst figure (masked relative L2 of var_out, relative difference of the two film sums) between the kernel and the restatement
# over every case of the first test below. Both sides add the same terms in the same order and divide and multiply in single correctly
# rounded operations; the film sums differ by the order of their reduction. 100 x the measured value is the margin, never looser than
# 1e-9, as in tests/test_gpu_nlm.py. Measured on an MI355X over the 192 cases: 8.910e-16 (the test prints the two parts apart).
VAR_SMOOTH_MEASURED = 9.0e-16
VAR_SMOOTH_BOUND = min(100 * VAR_SMOOTH_MEASURED, 1e-9) if VAR_SMOOTH_MEASURED is not None else None

# W x H: 17 x 17 is one pixel beyond a 16 x 16 tile each way; 530 x 500 has 34 x 32 = 1088 tiles, beyond the cap of 1024 blocks
FILMS = [(1, 1), (1, 7), (7, 1), (16, 16), (17, 17), (33, 9), (40, 19), (530, 500)]
RADII = [0, 1, 2, 4]
BLOCKS = [None, -1, 7]                                     # no demod block; one without a coverage plane; one with


def film(w, h, seed, dirty):
    """(img, var, feat, fvar), clean or planted; a planted film beyond the block cap gets values in tile 1024 (the second trip of
    block 0) and on the border of the tile before it."""
    if not dirty:
        return noisy_film(w, h, seed) + albedo_features(w, h, seed)
    img, var, feat, fvar = planted(w, h, seed)
    tiles_x = (w + 15) // 16
    if tiles_x * ((h + 15) // 16) > 1024:
        y0, x0 = 16 * (1024 // tiles_x), 16 * (1024 % tiles_x)
        var[y0 + 1, x0, 1], img[y0 + 3, x0 - 1, 0], feat[1, y0, x0 + 15], fvar[7, y0 + 15, x0 + 2] = np.nan, np.inf, -np.inf, -1e-3
    return img, var, feat, fvar


def block_of(G, cov):
    return None if cov is None else G.nlm_demod(coverage_channel=cov)


def smooth(G, img, var, feat, fvar, cov, s):
    if cov is None:
        return G.variance_smooth(img, var, radius=s)
    return G.variance_smooth(img, var, feat, fvar, demod=block_of(G, cov), radius=s)


def restated(img, var, feat, fvar, cov, s):
    return VS.smooth(img, var, s) if cov is None else VS.smooth(img, var, s, feat, fvar, 0, cov, 1e-3)


def same_bits(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and \
        (a[1].sum_var_in, a[1].sum_var_out, a[1].pixels_left_out) == (b[1].sum_var_in, b[1].sum_var_out, b[1].pixels_left_out)


def test_against_the_restatement(G):
    """Every film x radius x block, clean and planted: the figure against the restatement, and the exact parts."""
    worst, worst_var, cases, left = 0.0, 0.0, 0, 0
    for dirty in (False, True):
        for (w, h) in FILMS:
            img, var, feat, fvar = film(w, h, 10 * w + h, dirty)
            for cov in BLOCKS:
                ok = VS.valid_mask(img, var) if cov is None else VS.valid_mask(img, var, feat, fvar, 0, cov)
                for s in RADII:
                    key = (w, h, s, cov, dirty)
                    want = restated(img, var, feat, fvar, cov, s)
                    got, st = smooth(G, img, var, feat, fvar, cov, s)
                    assert st.pixels_left_out == want["left_out"] == (~ok).sum() and (not dirty or st.pixels_left_out >= 1), key
                    assert np.array_equal(got[~ok], var[~ok], equal_nan=True), key
                    assert np.isfinite(got[ok]).all(), key                      # the set of kept pixels is exactly ~ok
                    assert st.radius == s and st.smooth_ms > 0, key
                    if s == 0 and cov is None:
                        assert np.array_equal(got, var, equal_nan=True) and st.sum_var_in == st.sum_var_out, key
                    fig_var = masked_rel_l2(got, want["var_out"])
                    fig = max(fig_var, rel_diff(st.sum_var_in, want["sum_var_in"]), rel_diff(st.sum_var_out, want["sum_var_out"]))
                    worst, worst_var, cases, left = max(worst, fig), max(worst_var, fig_var), cases + 1, left + want["left_out"]
    assert cases == 192 and left > 300
    print(f"variance smoothing against the restatement over {cases} cases: worst figure {worst:.3e}, of var_out alone {worst_var:.3e} "
          f"(bound {VAR_SMOOTH_BOUND})")
    assert VAR_SMOOTH_BOUND is not None, f"VAR_SMOOTH_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < VAR_SMOOTH_BOUND


@pytest.mark.parametrize("w,h", [(40, 19), (530, 500)])
def test_exact_properties_bit_for_bit(G, w, h):
    img, var, feat, fvar = film(w, h, 3, True)
    ok = N.valid_mask(img, var)
    for s in RADII:
        # a variance that is one dyadic constant over the valid pixels comes back unchanged
        for value in (0.375, 2.0 ** -20):
            v = np.where(ok[:, :, None], value, var)
            got, st = G.variance_smooth(img, v, radius=s)
            assert np.array_equal(got, v, equal_nan=True) and st.pixels_left_out == (~ok).sum() > 0, (s, value)
        # var times a per-film power of two multiplies var_out by it, with and without a block
        v = np.where(var < 0, np.nan, var)                 # (a negative variance stays negative under the factor: keep the valid sets equal)
        for cov in BLOCKS:
            a = smooth(G, img, v, feat, fvar, cov, s)
            for m in (2.0 ** 10, 2.0 ** -7):
                b = smooth(G, img, v * m, feat, fvar, cov, s)
                assert np.array_equal(b[0], a[0] * m, equal_nan=True) and b[1].pixels_left_out == a[1].pixels_left_out, (s, cov, m)
                assert (b[1].sum_var_in, b[1].sum_var_out) == (a[1].sum_var_in * m, a[1].sum_var_out * m), (s, cov, m)
            assert not np.array_equal(b[0], a[0], equal_nan=True)
    # the block reaches the kernel: another floor, another albedo triple
    base = smooth(G, img, var, feat, fvar, 7, 2)[0]
    assert not np.array_equal(G.variance_smooth(img, var, feat, fvar, demod=G.nlm_demod(floor=0.6), radius=2)[0], base, equal_nan=True)
    assert not np.array_equal(G.variance_smooth(img, var, feat, fvar, demod=G.nlm_demod(albedo_channel=3), radius=2)[0], base, equal_nan=True)
    assert not np.array_equal(smooth(G, img, var, feat, fvar, None, 2)[0], base, equal_nan=True)


@pytest.mark.parametrize("w,h", [(40, 19), (530, 500)])
def test_host_and_device_entries_same_bits_second_stream_and_enqueue_only(G, w, h):
    img, var, feat, fvar = film(w, h, 5, True)
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (img, var, feat, fvar))
    d_out = hip_rt.alloc(G, img.nbytes)
    side = hip_rt.stream(G)
    zero = lambda: hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(img.nbytes)))      # noqa: E731
    for cov in BLOCKS:
        planes = {} if cov is None else dict(feat_ptr=d_feat, feat_var_ptr=d_fvar, num_channels=8, demod=block_of(G, cov))
        for s in (1, 4):
            first = smooth(G, img, var, feat, fvar, cov, s)                      # the host entry
            assert first[1].pixels_left_out > 4 and first[1].sum_var_out > 0 and first[1].smooth_ms > 0
            assert same_bits(smooth(G, img, var, feat, fvar, cov, s), first)
            for stream in (None, None, side):
                zero()
                st = G.variance_smooth_device(w, h, d_img, d_var, d_out, stream=stream, radius=s, **planes)
                assert same_bits((hip_rt.to_host(G, d_out, img.shape), st), first), (cov, s, stream)
            zero()
            assert G.variance_smooth_device(w, h, d_img, d_var, d_out, stats=False, radius=s, **planes) is None
            assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True)
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    for p in (d_img, d_var, d_feat, d_fvar, d_out):
        hip_rt.free(G, p)


def filter_bits(a, b):
    """(out, var_out, GdptNlmStats) twice: the same bits."""
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True) and \
        [getattr(a[2], k) for k in SUMS] == [getattr(b[2], k) for k in SUMS] and a[2].pixels_left_out == b[2].pixels_left_out


def session_body(G, ses, scene, budget):
    """`ses` holds two passes: denoise_smoothed() is, bit for bit, read(), Scene.features with the window {budget, 0} where the kind
    needs it, variance_smooth_device and the kind's device filter on the smoothed variance; in host and in device memory."""
    h, w, _ = ses.shape
    assert ses.status()["passes"] == 2
    fspp = 4
    kw = dict(window_radius=4, patch_radius=2, k=0.8)
    means, vars_, _ = ses.read()
    img, var = means["img"], vars_["img"]
    fm, fv = scene.features(fspp, window=(budget, 0))
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (img, var, fm, fv))
    d_sm, d_out, d_vout = (hip_rt.alloc(G, img.nbytes) for _ in range(3))
    d_fm, d_fv = hip_rt.alloc(G, fm.nbytes), hip_rt.alloc(G, fm.nbytes)
    guide = G.nlm_guide(groups=[(3, 3, 1e-3)], k_f=0.7)
    block = G.nlm_demod(floor=0.05)
    for kind, radius, opts in (("plain", 2, {}), ("plain", 0, {}), ("guided", 2, dict(guide=guide)), ("guided", None, {}), ("demod", 2, {}),
                               ("demod", 4, dict(guide=guide, demod=block))):
        s = 2 if radius is None else radius
        # the chain
        if kind == "demod":
            sst2 = G.variance_smooth_device(w, h, d_img, d_var, d_sm, feat_ptr=d_feat, feat_var_ptr=d_fvar, num_channels=8,
                                            demod=opts.get("demod", G.nlm_demod()), radius=s)
            st2 = G.denoise_nlm_demod_device(w, h, d_img, d_sm, d_feat, d_fvar, 8, d_out, d_vout, guide=opts.get("guide"), demod=opts.get("demod"), **kw)
        else:
            sst2 = G.variance_smooth_device(w, h, d_img, d_var, d_sm, radius=s)
            if kind == "guided":
                st2 = G.denoise_nlm_guided_device(w, h, d_img, d_sm, d_feat, d_fvar, d_out, d_vout, guide=opts.get("guide"), **kw)
            else:
                st2 = G.denoise_nlm_device(w, h, d_img, d_sm, d_out, d_vout, **kw)
        want = (hip_rt.to_host(G, d_out, img.shape), hip_rt.to_host(G, d_vout, img.shape), st2)
        want_sm = (hip_rt.to_host(G, d_sm, img.shape), sst2)
        # the session, into host memory
        if kind == "plain":
            out, var_out, sm, st, sst = ses.denoise_smoothed(kind, radius=radius, **kw)
        else:
            out, var_out, sm, gfm, gfv, st, sst = ses.denoise_smoothed(kind, radius=radius, feature_spp=fspp, features=True, **opts, **kw)
            assert np.array_equal(gfm, fm) and np.array_equal(gfv, fv)
        assert filter_bits((out, var_out, st), want), (kind, radius)
        assert same_bits((sm, sst), want_sm) and sst.radius == s and sst.pixels_left_out == 0, (kind, radius)
        assert st.sum_var_in == sst.sum_var_out                                  # the filter's input sums are those of the smoothed variance
        if s == 0:
            assert np.array_equal(sm, var) and filter_bits((out, var_out, st), ses.denoise(**kw))
        else:
            assert not np.array_equal(sm, var)
            plain = ses.denoise(**kw) if kind == "plain" else ses.denoise_guided(fspp, guide=opts.get("guide"), **kw) if kind == "guided" else \
                ses.denoise_demod(fspp, guide=opts.get("guide"), demod=opts.get("demod"), **kw)
            assert not np.array_equal(plain[0], out)                             # the smoothing is at work
        # ... and into device memory
        for p in (d_out, d_vout, d_sm):
            hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(img.nbytes)))
        extra = {} if kind == "plain" else dict(feature_spp=fspp, features_ptrs=(d_fm, d_fv), **opts)
        st3, sst3 = ses.denoise_smoothed(kind, radius=radius, out_ptr=d_out, var_out_ptr=d_vout, smoothed_var_ptr=d_sm, **extra, **kw)
        assert filter_bits((hip_rt.to_host(G, d_out, img.shape), hip_rt.to_host(G, d_vout, img.shape), st3), want)
        assert same_bits((hip_rt.to_host(G, d_sm, img.shape), sst3), want_sm)
        if kind != "plain":
            assert np.array_equal(hip_rt.to_host(G, d_fm, fm.shape), fm) and np.array_equal(hip_rt.to_host(G, d_fv, fm.shape), fv)
    for bad in (1, budget + 1):
        with pytest.raises(G.GdptError, match="feature_spp"):
            ses.denoise_smoothed("guided", feature_spp=bad)
    with pytest.raises(G.GdptError, match="radius"):
        ses.denoise_smoothed("plain", radius=5)
    with pytest.raises(G.GdptError, match="guide must be null"):
        ses.denoise_smoothed("plain", guide=guide)
    with pytest.raises(G.GdptError, match="kind"):
        ses.denoise_smoothed("median")
    for p in (d_img, d_var, d_feat, d_fvar, d_sm, d_out, d_vout, d_fm, d_fv):
        hip_rt.free(G, p)


@pytest.mark.parametrize("path", [True, False], ids=["path", "gradpath"])
def test_session(G, path):
    """budget 16 in two passes of 8: refused before the second pass, then every kind against the composed device calls."""
    sc = G.Scene(room_desc(G))
    ses = G.Progressive(sc, 16, path=path)
    ses.add_pass(8)
    for kind in ("plain", "guided", "demod"):
        with pytest.raises(G.GdptError, match="at least 2 passes"):
            ses.denoise_smoothed(kind, feature_spp=4)
    ses.add_pass(8)
    session_body(G, ses, sc, 16)
    ses.close()
    sc.close()


def test_group_total(G):
    sd = room_desc(G)
    grp = G.ProgressiveGroup(sd, (0, 0), 16)
    grp.run(pass_spp=8)
    sc = G.Scene(sd)
    session_body(G, grp.total, sc, 16)
    sc.close()
    grp.close()


EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")


def test_cli_var_smooth(G, scene_tmp, tmp_path):
    xml = scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path")
    out, out2, den, den2, sden, dden = (tmp_path / n for n in ("o.pfm", "o2.pfm", "d.pfm", "d2.pfm", "sd.pfm", "dd.pfm"))
    base = [EXE, "--spp", "8", "--pass-spp", "4"]
    nlm = ["--nlm-window", "4", "--nlm-patch", "2"]
    runs = [([*base, "--denoised", str(den), *nlm, "-o", str(out), xml]), ([*base, "--denoised", str(den2), *nlm, "-o", str(out2), xml]),
            ([*base, "--denoised", str(sden), *nlm, "--nlm-var-smooth", "2", "-o", str(out2), xml]),
            ([*base, "--denoised", str(dden), *nlm, "--nlm-var-smooth", "1", "--nlm-demodulate", "--nlm-guide", "normal", "--feature-spp", "4", "-o",
              str(out2), xml])]
    done = []
    for cmd in runs:
        done.append(subprocess.run(cmd, capture_output=True, text=True, timeout=300))
        assert done[-1].returncode == 0, done[-1].stderr
        if len(done) > 1:
            assert open(out, "rb").read() == open(out2, "rb").read()            # -o is what it is without the flag
    data = lambda p: open(p, "rb").read()      # noqa: E731
    assert data(den) == data(den2)                                              # without the flag: the same bytes run after run
    assert data(sden) != data(den) and data(dden) != data(den) and data(dden) != data(sden)
    lines = [[l for l in r.stdout.splitlines() if l.startswith("[gdpt] denoised:")] for r in done]
    assert all(len(l) == 1 for l in lines)
    assert "variance smoothed" not in lines[0][0] and "variance smoothed over radius 2" in lines[2][0] and "variance smoothed over radius 1" in lines[3][0]
    sc = G.Scene(G.parse_scene(xml))
    ses = G.Progressive(sc, 8, path=True)
    ses.run(pass_spp=4)
    want = ses.denoise_smoothed("plain", radius=2, window_radius=4, patch_radius=2)[0]
    assert np.array_equal(read_pfm(sden, 24, 24), want.astype(np.float32))
    want = ses.denoise_smoothed("demod", radius=1, feature_spp=4, guide=G.nlm_guide(groups=[(3, 3, 1e-3)]), window_radius=4, patch_radius=2, k=1.0)[0]
    assert np.array_equal(read_pfm(dden, 24, 24), want.astype(np.float32))
    ses.close()
    sc.close()
