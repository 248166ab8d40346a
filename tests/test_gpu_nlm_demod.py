"""The albedo-demodulated non-local-means filter on the GPU (include/gdpt.h: gdpt_denoise_nlm_demod*, gdpt_progressive_denoise_demod):
both kernel forms against the numpy restatement (tests/nlm_demod_ref.py) and against each other, the exact properties of the
definition bit for bit, the host and device entries, the sessions (Path, GradPath, a group's total) and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import hip_rt
import nlm_demod_ref as ND
from helpers import ROOT, Built, room, scene_variant
from test_gpu_nlm import CBOX, FORMS, SUMS, as_dict, figure, planted_film
from test_gpu_progressive import read_pfm
from test_nlm_demod_ref import albedo_features
from test_nlm_ref import noisy_film

pytestmark = pytest.mark.gpu

# The worst figure of tests/test_gpu_nlm.py (masked relative L2 of out and of var_out, relative difference of the four film sums)
# between either demodulated kernel form and the restatement, and between the two forms, over every case of the two tests below. The
# sides differ by FMA contraction, the order of the patch sums and the last place of exp (the division and the multiplication are
# single correctly rounded operations on both sides); 100 x the measured value is the margin, as in the two modules before this
# one (the measurement started from a bound of 1e-12). Measured on an MI355X: 3.994e-16 for either form against the restatement,
# 3.550e-16 between the forms, over 150 cases: the cases below and every (guide, coverage) pair at (10, 3) on the two small films too.
NLM_DEMOD_MEASURED = 4.0e-16
NLM_DEMOD_BOUND = 100 * NLM_DEMOD_MEASURED

FILMS = [(1, 1), (16, 16), (17, 17), (33, 9), (40, 19)]      # W x H: 17 x 17 is one pixel beyond a 16 x 16 tile each way
RADII = [(0, 0), (1, 0), (2, 1), (5, 1), (10, 3)]
GROUPS = {0: None, 1: [(3, 3, 1e-3)], 2: [(3, 3, 1e-3), (6, 1, 5e-2)]}      # no guide; the normal; the normal and the depth
OPTIONS = [(ng, cov) for ng in (0, 1, 2) for cov in (-1, 7)]
KW = dict(k=0.8)


def planted_features(w, h, seed):
    """NaN, +-Inf and a negative variance in the albedo planes, the coverage plane and the planes the guides name, at a corner, an
    edge, the middle and a tile's halo."""
    feat, fvar = albedo_features(w, h, seed)
    spots = [(0, 0, w - 1, "nan"), (7, h - 1, 0, "neg"), (2, h // 2, w // 3, "-inf"), (1, h - 1, w // 2, "+inf"), (4, h // 3, 0, "nan")]
    if w > 16:
        spots += [(1, min(3, h - 1), 16, "neg"), (7, h // 2, 17 if w > 17 else 16, "nan"), (0, h // 2, 14, "+inf")]
    if h > 16:
        spots += [(2, 16, 5, "nan"), (7, 16, 9, "+inf"), (6, 16, 1, "neg")]
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


def guide_of(G, ng):
    return G.nlm_guide(groups=GROUPS[ng]) if ng else None


@pytest.fixture(scope="module")
def cases(G):
    """Films x (r, f) x (guide, coverage), clean and planted: the restatement's result (computed once, left unchanged) and both forms'.
    Every (guide, coverage) pair at (2, 1), and at (10, 3) on the films beyond one tile; one in turn elsewhere."""
    out = []
    n = 0
    for planted in (False, True):
        for (w, h) in FILMS:
            img, var = planted_film(w, h, 10 * w + h) if planted else noisy_film(w, h, 10 * w + h)
            feat, fvar = planted_features(w, h, w + h) if planted else albedo_features(w, h, w + h)
            for (r, f) in RADII:
                every = (r, f) == (2, 1) or ((r, f) == (10, 3) and w > 16)
                for ng, cov in (OPTIONS if every else (OPTIONS[n % len(OPTIONS)],)):
                    want = ND.denoise(img, var, feat, fvar, 0, cov, 1e-3, GROUPS[ng], r=r, f=f, **KW)
                    got = []
                    for direct in FORMS:
                        with G.debug_knobs(nlm_direct=direct):
                            got.append(G.denoise_nlm_demod(img, var, feat, fvar, guide=guide_of(G, ng), demod=G.nlm_demod(coverage_channel=cov),
                                                           window_radius=r, patch_radius=f, **KW))
                    out.append(((w, h, r, f, ng, cov, planted), img, var, feat, fvar, want, got))
                n += 1
    return out


def test_both_forms_against_the_restatement(cases):
    worst = {0: 0.0, 1: 0.0}
    left = 0
    for key, img, var, feat, fvar, want, got in cases:
        w, h, r, f, ng, cov, planted = key
        ok = ND.valid_mask(img, var, feat, fvar, 0, cov, GROUPS[ng])
        assert want["left_out"] == (~ok).sum()
        left += want["left_out"]
        al = ND.effective_albedo(feat, 0, cov, 1e-3)
        for direct in FORMS:
            o, vo, st = got[direct]
            assert np.array_equal(o[~ok], img[~ok], equal_nan=True) and np.array_equal(vo[~ok], var[~ok], equal_nan=True), key
            assert np.isfinite(o[ok]).all() and np.isfinite(vo[ok]).all(), key         # the set of kept pixels is exactly ~ok
            if r == 0:                       # (u / a~) a~, not the input bits
                assert np.array_equal(o[ok], ((img / al) * al)[ok]) and np.array_equal(vo[ok], ((var / (al * al)) * (al * al))[ok]), key
            worst[direct] = max(worst[direct], figure(o, vo, st, want))
    assert left > 100
    print(f"demodulated nlm against the restatement over {len(cases)} cases: worst figure tiled {worst[0]:.3e}, direct {worst[1]:.3e} "
          f"(bound {NLM_DEMOD_BOUND})")
    assert max(worst.values()) < NLM_DEMOD_BOUND


def test_the_two_forms_agree(cases):
    worst = 0.0
    for key, img, var, feat, fvar, want, got in cases:
        worst = max(worst, figure(*got[0], as_dict(*got[1])))
    print(f"demodulated nlm tiled against direct: worst figure {worst:.3e} (bound {NLM_DEMOD_BOUND})")
    assert worst < NLM_DEMOD_BOUND


def same_bits(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True) and \
        [getattr(a[2], k) for k in SUMS] == [getattr(b[2], k) for k in SUMS] and a[2].pixels_left_out == b[2].pixels_left_out


@pytest.mark.parametrize("ng", [0, 2], ids=["plain", "guided"])
@pytest.mark.parametrize("direct", FORMS, ids=["tiled", "direct"])
def test_exact_properties_bit_for_bit(G, direct, ng):
    w, h = 40, 19
    img, var = planted_film(w, h, 3)
    feat, fvar = albedo_features(w, h, 3)
    guide = guide_of(G, ng)
    with G.debug_knobs(nlm_direct=direct):
        for (r, f) in ((2, 1), (10, 3)):
            kw = dict(window_radius=r, patch_radius=f, k=0.7)
            plain = G.denoise_nlm_guided(img, var, feat, fvar, guide=guide, **kw) if ng else G.denoise_nlm(img, var, **kw)
            assert plain[2].pixels_left_out > 0
            # a unit divisor: albedo 1 with coverage 1, albedo 0 with coverage 0, albedo 1 without a coverage plane
            for albedo, cov, channel in ((1.0, 1.0, 7), (0.0, 0.0, 7), (1.0, 0.3, -1)):
                ft = feat.copy()
                ft[0:3], ft[7] = albedo, cov
                got = G.denoise_nlm_demod(img, var, ft, fvar, guide=guide, demod=G.nlm_demod(coverage_channel=channel), **kw)
                assert same_bits(got, plain), (r, f, albedo, cov)
            # the colour-domain input sums are the undemodulated filter's on the same film (the valid sets agree: the planes are clean)
            dem = G.denoise_nlm_demod(img, var, feat, fvar, guide=guide, **kw)
            assert (dem[2].sum_var_in, dem[2].sum_sq_in, dem[2].pixels_left_out) == (plain[2].sum_var_in, plain[2].sum_sq_in, plain[2].pixels_left_out)
            assert not np.array_equal(dem[0], plain[0], equal_nan=True)
            # a per-pixel power of two on img and albedo (squared on var) comes out of out and var_out
            clean_img, clean_var = noisy_film(w, h, 3)
            ft = feat.copy()
            ft[7], fv = 1.0, fvar.copy()
            fv[7] = 0.0
            y, x = np.mgrid[0:h, 0:w]
            m = np.where((x // 2 + y) % 2 == 0, 2.0, 0.5)
            a = G.denoise_nlm_demod(clean_img, clean_var, ft, fv, guide=guide, **kw)
            fm = ft.copy()
            fm[0:3] = ft[0:3] * m
            assert (fm[0:3] > 1e-3).all()
            b = G.denoise_nlm_demod(clean_img * m[:, :, None], clean_var * (m * m)[:, :, None], fm, fv, guide=guide, **kw)
            assert np.array_equal(b[0], a[0] * m[:, :, None]) and np.array_equal(b[1], a[1] * (m * m)[:, :, None]), (r, f)
            assert not np.array_equal(b[0], a[0])


def test_input_sums_equal_the_plain_device_entry(G):
    """sum_var_in and sum_sq_in of the device entry are gdpt_denoise_nlm_device's on the same film, bit for bit, in both forms."""
    w, h, r, f = 33, 9, 5, 1
    img, var = planted_film(w, h, 8)
    feat, fvar = albedo_features(w, h, 8)
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (img, var, feat, fvar))
    d_out = hip_rt.alloc(G, img.nbytes)
    for direct in FORMS:
        with G.debug_knobs(nlm_direct=direct):
            p = G.denoise_nlm_device(w, h, d_img, d_var, d_out, window_radius=r, patch_radius=f)
            d = G.denoise_nlm_demod_device(w, h, d_img, d_var, d_feat, d_fvar, 8, d_out, window_radius=r, patch_radius=f)
            assert (d.sum_var_in, d.sum_sq_in, d.pixels_left_out) == (p.sum_var_in, p.sum_sq_in, p.pixels_left_out) and p.pixels_left_out > 0
            assert (d.sum_var_out, d.sum_sq_out) != (p.sum_var_out, p.sum_sq_out)
    for ptr in (d_img, d_var, d_feat, d_fvar, d_out):
        hip_rt.free(G, ptr)


def test_host_and_device_entries_same_bits_second_stream_and_enqueue_only(G):
    w, h, r, f = 40, 19, 5, 1
    img, var = planted_film(w, h, 5)
    feat, fvar = planted_features(w, h, 5)
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (img, var, feat, fvar))
    d_out, d_vout = hip_rt.alloc(G, img.nbytes), hip_rt.alloc(G, img.nbytes)
    side = hip_rt.stream(G)
    kw = dict(window_radius=r, patch_radius=f, **KW)
    for ng in (0, 2):
        guide = guide_of(G, ng)
        for direct in FORMS:
            with G.debug_knobs(nlm_direct=direct):
                first = G.denoise_nlm_demod(img, var, feat, fvar, guide=guide, **kw)             # the host entry
                assert first[2].pixels_left_out > 8 and first[2].sum_var_out > 0 and first[2].filter_ms > 0
                for stream in (None, None, side):
                    st = G.denoise_nlm_demod_device(w, h, d_img, d_var, d_feat, d_fvar, 8, d_out, d_vout, guide=guide, stream=stream, **kw)
                    assert same_bits((hip_rt.to_host(G, d_out, img.shape), hip_rt.to_host(G, d_vout, img.shape), st), first)
                for p in (d_out, d_vout):
                    hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(img.nbytes)))
                assert G.denoise_nlm_demod_device(w, h, d_img, d_var, d_feat, d_fvar, 8, d_out, d_vout, guide=guide, stats=False, **kw) is None
                assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True)
                assert np.array_equal(hip_rt.to_host(G, d_vout, img.shape), first[1], equal_nan=True)
                hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(img.nbytes)))
                st = G.denoise_nlm_demod_device(w, h, d_img, d_var, d_feat, d_fvar, 8, d_out, guide=guide, **kw)       # var_out is optional
                assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True) and st.sum_var_out == first[2].sum_var_out
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    for p in (d_img, d_var, d_feat, d_fvar, d_out, d_vout):
        hip_rt.free(G, p)


def session_body(G, ses, scene, budget):
    """`ses` holds at least two passes: denoise_demod() is Scene.features with the window {budget, 0} fed to denoise_nlm_demod_device
    with the planes read() returns, bit for bit, in host and in device memory, with and without a guide."""
    h, w, _ = ses.shape
    fspp = 4
    kw = dict(window_radius=4, patch_radius=2, k=0.8)
    means, vars_, _ = ses.read()
    want_fm, want_fv = scene.features(fspp, window=(budget, 0))
    al = ND.effective_albedo(want_fm, 0, 7, 1e-3)
    assert len(np.unique(np.round(al.reshape(-1, 3), 3), axis=0)) > 4           # the divisor differs across the film
    d_out, d_vout = hip_rt.alloc(G, means["img"].nbytes), hip_rt.alloc(G, means["img"].nbytes)
    for guide in (None, G.nlm_guide(groups=[(3, 3, 1e-3)], k_f=0.7)):
        out, var_out, fm, fv, st = ses.denoise_demod(fspp, guide=guide, features=True, **kw)
        assert np.array_equal(fm, want_fm) and np.array_equal(fv, want_fv) and fv.any()
        d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (means["img"], vars_["img"], fm, fv))
        st2 = G.denoise_nlm_demod_device(w, h, d_img, d_var, d_feat, d_fvar, 8, d_out, d_vout, guide=guide, **kw)
        assert same_bits((hip_rt.to_host(G, d_out, out.shape), hip_rt.to_host(G, d_vout, out.shape), st2), (out, var_out, st))
        assert st.pixels_left_out == 0 and np.isfinite(out).all()
        plain = ses.denoise_guided(fspp, guide=guide, **kw) if guide is not None else ses.denoise(**kw)
        assert not np.array_equal(plain[0], out)                      # the division is at work
        # everything in device memory
        d_fm, d_fv = hip_rt.alloc(G, fm.nbytes), hip_rt.alloc(G, fm.nbytes)
        hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(out.nbytes)))
        st3 = ses.denoise_demod(fspp, guide=guide, out_ptr=d_out, var_out_ptr=d_vout, features_ptrs=(d_fm, d_fv), **kw)
        assert np.array_equal(hip_rt.to_host(G, d_out, out.shape), out) and st3.sum_var_out == st.sum_var_out
        assert np.array_equal(hip_rt.to_host(G, d_fm, fm.shape), fm) and np.array_equal(hip_rt.to_host(G, d_fv, fm.shape), fv)
        assert same_bits(ses.denoise_demod(fspp, guide=guide, **kw), (out, var_out, st))
        for p in (d_img, d_var, d_feat, d_fvar, d_fm, d_fv):
            hip_rt.free(G, p)
    # another floor, no coverage plane: the block reaches the kernel
    other = ses.denoise_demod(fspp, demod=G.nlm_demod(coverage_channel=-1, floor=0.5), **kw)
    assert not np.array_equal(other[0], ses.denoise_demod(fspp, **kw)[0])
    for bad in (1, budget + 1):
        with pytest.raises(G.GdptError, match="feature_spp"):
            ses.denoise_demod(bad)
    with pytest.raises(G.GdptError, match="floor"):
        ses.denoise_demod(fspp, demod=G.nlm_demod(floor=0.0))
    with pytest.raises(G.GdptError, match="num_channels"):
        ses.denoise_demod(fspp, guide=G.nlm_guide(num_channels=7, groups=[(3, 3, 1e-3)]))
    for p in (d_out, d_vout):
        hip_rt.free(G, p)


def room_desc(G):
    """The 4 x 4 x 4 room at 33 x 9 with a red, a green and a white wall, an image-textured floor and a block: many effective albedos."""
    b = room(G, "lambert_tex", 33, 9, -1, 5)
    return Built(b.finish(), 33, 9, b)


@pytest.mark.parametrize("path", [True, False], ids=["path", "gradpath"])
def test_session(G, path):
    """budget 16 in four passes of 4: refused before the second pass, then the demodulated filter on what read() returns."""
    sc = G.Scene(room_desc(G))
    ses = G.Progressive(sc, 16, path=path)
    ses.add_pass(4)
    with pytest.raises(G.GdptError, match="at least 2 passes"):
        ses.denoise_demod(4)
    ses.run(pass_spp=4)
    assert ses.status()["passes"] == 4
    session_body(G, ses, sc, 16)
    ses.close()
    sc.close()


def test_group_total(G):
    sd = room_desc(G)
    grp = G.ProgressiveGroup(sd, (0, 0), 16)
    grp.run(pass_spp=4)
    assert grp.total.status()["passes"] == 4
    sc = G.Scene(sd)
    session_body(G, grp.total, sc, 16)
    sc.close()
    grp.close()


EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")


def test_cli_demodulate(G, scene_tmp, tmp_path):
    xml = scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path")
    out, out2, den, dden, gden = (tmp_path / n for n in ("o.pfm", "o2.pfm", "d.pfm", "dd.pfm", "gd.pfm"))
    base = [EXE, "--spp", "16", "--pass-spp", "4"]
    nlm = ["--nlm-window", "4", "--nlm-patch", "2", "--nlm-k", "0.5"]
    r0 = subprocess.run([*base, "--denoised", str(den), *nlm, "-o", str(out), xml], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stderr
    r1 = subprocess.run([*base, "--denoised", str(dden), *nlm, "--nlm-demodulate", "--feature-spp", "4", "-o", str(out2), xml],
                        capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert open(out, "rb").read() == open(out2, "rb").read()                    # -o is what it is without the flag
    assert open(den, "rb").read() != open(dden, "rb").read()
    sc = G.Scene(G.parse_scene(xml))
    ses = G.Progressive(sc, 16, path=True)
    ses.run(pass_spp=4)
    want, _, st = ses.denoise_demod(4, window_radius=4, patch_radius=2, k=0.5)
    assert np.array_equal(read_pfm(dden, 24, 24), want.astype(np.float32))
    line = [l for l in r1.stdout.splitlines() if l.startswith("[gdpt] denoised:")]
    assert len(line) == 1 and "demodulated by the first-hit albedo" in line[0] and "guided by" not in line[0]
    # with a guide of normals and another floor; k = 1.0 when a guide is given without --nlm-k
    r2 = subprocess.run([*base, "--denoised", str(gden), "--nlm-window", "4", "--nlm-patch", "2", "--nlm-demodulate", "--nlm-albedo-floor", "0.05",
                         "--nlm-guide", "normal", "--nlm-kf", "0.7", "--feature-spp", "4", "-o", str(out2), xml], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr
    want, _, st = ses.denoise_demod(4, guide=G.nlm_guide(groups=[(3, 3, 1e-3)], k_f=0.7), demod=G.nlm_demod(floor=0.05), window_radius=4, patch_radius=2, k=1.0)
    assert np.array_equal(read_pfm(gden, 24, 24), want.astype(np.float32))
    assert open(out, "rb").read() == open(out2, "rb").read()
    ses.close()
    sc.close()
