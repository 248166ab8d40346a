"""The joint non-local-means filter on the GPU (include/gdpt.h: gdpt_denoise_nlm_joint*, gdpt_progressive_denoise_reconstruct): both
kernel forms against the numpy restatement (tests/nlm_joint_ref.py) and against each other, the three identities bit for bit, the
host and device entries, the session entry against the chain of public device entries, and the CLI."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import hip_rt
import nlm_joint_ref as J
from helpers import ROOT, scene_variant
from test_gpu_nlm import CBOX, FORMS, SUMS, masked_rel_l2, planted_film, rel_diff
from test_gpu_nlm_guided import planted_features
from test_gpu_progressive import read_pfm
from test_nlm_guided_ref import noisy_features
from test_nlm_ref import noisy_film

pytestmark = pytest.mark.gpu

# measured on an MI355X: the worst figure (masked relative L2 of out, var_out and of every companion's two outputs, relative difference
# of the four film sums and of the companions' variance sums) between either kernel form and the restatement, and between the two
# forms, over every case of the two tests below. The sides differ by FMA contraction, the order of the patch sums and the last place
# of exp; 100 x the measured value is the margin, never looser than 1e-9. Measured: 4.170e-16 for either form against the restatement
# over the 160 cases, 3.340e-16 between the forms, 6.859e-16 for either form on the 1025 x 345 film (its film sums run over 353 625
# pixels). While it is None the tests fail with what they measured.
NLM_JOINT_MEASURED = 6.9e-16
NLM_JOINT_BOUND = min(100 * NLM_JOINT_MEASURED, 1e-9) if NLM_JOINT_MEASURED else None

FILMS = [(1, 1), (16, 16), (17, 17), (33, 9), (40, 19)]      # a window of radius 10 reaches a third tile in the last
RADII = [(0, 0), (1, 0), (2, 1), (10, 3)]
COUNTS = [1, 2, 4]
GROUPS = [(0, 3, 1e-3), (3, 3, 2e-3), (6, 1, 5e-2)]
KW = dict(k=0.8)


def companions(w, h, seed, n, planted):
    """n films that share nothing with the guide film, and their variances; planted: a NaN in the last film, an infinity in the first,
    a negative and a non-finite variance, at pixels the guide film's own plants leave alone."""
    rng = np.random.default_rng(5000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    comps = [0.3 * np.cos(0.5 * x - 0.2 * y + j)[:, :, None] * np.array([1.0, -0.5, 0.25]) + 0.1 * rng.standard_normal((h, w, 3)) for j in range(n)]
    comp_vars = [0.01 * rng.uniform(0.5, 1.5, (h, w, 3)) for _ in range(n)]
    if planted:
        comps[n - 1][h // 3, w // 3, 2] = np.nan
        comps[0][h - 1, w // 4, 0] = -np.inf
        comp_vars[0][h // 4, w - 1, 1] = -1e-4
        comp_vars[n - 1][2 * h // 3, w // 5, 0] = np.inf
        if w > 16:
            comps[0][h // 2, 16, 1] = np.nan                   # one pixel beyond the first tile: in its halo
    return comps, comp_vars


def run_gpu(G, img, var, comps, comp_vars, feat, fvar, guided, r, f, **kw):
    return G.denoise_nlm_joint(img, var, comps, comp_vars, feat if guided else None, fvar if guided else None,
                               guide=G.nlm_guide(groups=GROUPS if guided else []), window_radius=r, patch_radius=f, **{**KW, **kw})


def run_ref(img, var, comps, comp_vars, feat, fvar, guided, r, f):
    return J.denoise(img, var, comps, comp_vars, feat if guided else None, fvar if guided else None, GROUPS if guided else (), r=r, f=f, **KW)


def as_dict(got):
    out, var_out, co, cvo, st = got
    d = dict(out=out, var_out=var_out, comp_out=co, comp_var_out=cvo, left_out=st.guide.pixels_left_out)
    d.update({k: getattr(st.guide, k) for k in SUMS})
    d["comp_sum_var_in"], d["comp_sum_var_out"] = list(st.sum_var_in)[:len(co)], list(st.sum_var_out)[:len(co)]
    return d


def figure(got, want):
    """The worst figure of one call against `want` (the restatement's dict, or another call's as_dict); the exact parts are asserted."""
    out, var_out, co, cvo, st = got
    n = len(co)
    figs = [masked_rel_l2(out, want["out"]), masked_rel_l2(var_out, want["var_out"])]
    figs += [rel_diff(getattr(st.guide, k), want[k]) for k in SUMS]
    for j in range(n):
        figs += [masked_rel_l2(co[j], want["comp_out"][j]), masked_rel_l2(cvo[j], want["comp_var_out"][j])]
        figs += [rel_diff(st.sum_var_in[j], want["comp_sum_var_in"][j]), rel_diff(st.sum_var_out[j], want["comp_sum_var_out"][j])]
    assert st.guide.pixels_left_out == want["left_out"]
    assert list(st.sum_var_in)[n:] == [0.0] * (4 - n) and list(st.sum_var_out)[n:] == [0.0] * (4 - n)
    for e, a, b in ((st.guide.error_in, st.guide.sum_var_in, st.guide.sum_sq_in), (st.guide.error_out, st.guide.sum_var_out, st.guide.sum_sq_out)):
        with np.errstate(all="ignore"):
            assert np.array_equal(e, np.sqrt(np.float64(a) / np.float64(b)), equal_nan=True)
    return max(figs)


@pytest.fixture(scope="module")
def cases(G):
    """Films x (r, f) x companion counts, guided and unguided, clean and planted: the restatement's result (computed once, left
    unchanged) and both forms'. Every count at (2, 1) and (10, 3), one in turn at the other radii."""
    out = []
    turn = 0
    for planted in (False, True):
        for (w, h) in FILMS:
            img, var = planted_film(w, h, 10 * w + h) if planted else noisy_film(w, h, 10 * w + h)
            feat, fvar = planted_features(w, h, w + h) if planted else noisy_features(w, h, w + h)
            for guided in (False, True):
                for (r, f) in RADII:
                    for n in (COUNTS if (r, f) in ((2, 1), (10, 3)) else (COUNTS[turn % 3],)):
                        comps, comp_vars = companions(w, h, w + 3 * h, n, planted)
                        want = run_ref(img, var, comps, comp_vars, feat, fvar, guided, r, f)
                        got = []
                        for direct in FORMS:
                            with G.debug_knobs(nlm_direct=direct):
                                got.append(run_gpu(G, img, var, comps, comp_vars, feat, fvar, guided, r, f))
                            st = got[-1][4].guide
                            assert (st.window_radius, st.patch_radius) == (r, f) and st.filter_ms > 0
                        out.append(((w, h, r, f, n, guided, planted), (img, var, comps, comp_vars, feat, fvar), want, got))
                    turn += 1
    return out


def test_both_forms_against_the_restatement(cases):
    worst = {0: 0.0, 1: 0.0}
    left = 0
    for key, (img, var, comps, comp_vars, feat, fvar), want, got in cases:
        w, h, r, f, n, guided, planted = key
        ok = J.valid_mask(img, var, comps, comp_vars, feat if guided else None, fvar if guided else None, GROUPS if guided else ())
        assert want["left_out"] == (~ok).sum() and (not planted or want["left_out"] >= 1), key      # pixels_left_out is exact (figure)
        left += want["left_out"]
        for direct in FORMS:
            o, vo, co, cvo, st = got[direct]
            pairs = [(o, img), (vo, var)] + list(zip(co, comps)) + list(zip(cvo, comp_vars))
            for a, b in pairs:                                    # invalid pixels keep their bits, in every film
                assert a[~ok].tobytes() == b[~ok].tobytes(), key
                if r == 0:
                    assert a.tobytes() == b.tobytes(), key
            worst[direct] = max(worst[direct], figure(got[direct], want))
    assert left > 100
    print(f"joint nlm against the restatement: worst figure tiled {worst[0]:.3e}, direct {worst[1]:.3e} (bound {NLM_JOINT_BOUND}), {len(cases)} cases")
    assert NLM_JOINT_BOUND is not None, f"NLM_JOINT_MEASURED has not been recorded; this run measured {max(worst.values()):.3e}"
    assert max(worst.values()) < NLM_JOINT_BOUND


def test_the_two_forms_agree(cases):
    worst = 0.0
    for key, films, want, got in cases:
        worst = max(worst, figure(got[0], as_dict(got[1])))
    print(f"joint nlm tiled against direct: worst figure {worst:.3e} (bound {NLM_JOINT_BOUND})")
    assert NLM_JOINT_BOUND is not None, f"NLM_JOINT_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < NLM_JOINT_BOUND


@pytest.mark.parametrize("direct", FORMS, ids=["tiled", "direct"])
def test_a_film_past_the_block_cap(G, direct):
    """1025 x 345: 65 x 22 = 1430 tiles on 1024 blocks, so 406 blocks walk a second tile."""
    w, h, r, f, n = 1025, 345, 2, 1, 2
    img, var = planted_film(w, h, 9)
    comps, comp_vars = companions(w, h, 9, n, True)
    want = run_ref(img, var, comps, comp_vars, None, None, False, r, f)
    with G.debug_knobs(nlm_direct=direct):
        got = run_gpu(G, img, var, comps, comp_vars, None, None, False, r, f)
    fig = figure(got, want)
    print(f"joint nlm past the block cap ({'direct' if direct else 'tiled'}): figure {fig:.3e} (bound {NLM_JOINT_BOUND})")
    assert NLM_JOINT_BOUND is not None, f"NLM_JOINT_MEASURED has not been recorded; this run measured {fig:.3e}"
    assert fig < NLM_JOINT_BOUND


def stats_tuple(st):
    return [getattr(st, k) for k in SUMS] + [st.pixels_left_out, st.error_in, st.error_out, st.window_radius, st.patch_radius]


def joint_bits(got):
    out, var_out, co, cvo, st = got
    return [a.tobytes() for a in [out, var_out, *co, *cvo]], stats_tuple(st.guide), list(st.sum_var_in), list(st.sum_var_out)


@pytest.mark.parametrize("direct", FORMS, ids=["tiled", "direct"])
def test_the_three_identities_bit_for_bit(G, direct):
    w, h = 40, 19
    img, var = planted_film(w, h, 3)                              # (invalid pixels in the guide film: the identities hold around them)
    feat, fvar = planted_features(w, h, 3)
    with G.debug_knobs(nlm_direct=direct):
        for (r, f) in ((3, 1), (10, 3)):
            kw = dict(window_radius=r, patch_radius=f, **KW)
            for guided in (False, True):
                guide = G.nlm_guide(groups=GROUPS if guided else [])
                ref = G.denoise_nlm_guided(img, var, feat if guided else None, fvar if guided else None, guide=guide, **kw)
                assert ref[2].pixels_left_out > 0
                # 1. valid companions change nothing in the guide film, whatever their number; n = 0 included
                for n in (0, 1, 2, 4):
                    comps, comp_vars = companions(w, h, 3, max(n, 1), False)
                    got = run_gpu(G, img, var, comps[:n], comp_vars[:n], feat, fvar, guided, r, f)
                    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes(), (r, f, guided, n)
                    assert stats_tuple(got[4].guide) == stats_tuple(ref[2]), (r, f, guided, n)
                if not guided:
                    plain = G.denoise_nlm(img, var, **kw)
                    got = run_gpu(G, img, var, comps[:2], comp_vars[:2], None, None, False, r, f)
                    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
                    assert stats_tuple(got[4].guide) == stats_tuple(plain[2])
                # 2. the guide film as its own companion comes back as out, var_out
                for slot in (0, 1):
                    cs, cv = [comps[0], comps[1]], [comp_vars[0], comp_vars[1]]
                    cs[slot], cv[slot] = img, var
                    got = run_gpu(G, img, var, cs, cv, feat, fvar, guided, r, f)
                    assert got[2][slot].tobytes() == got[0].tobytes() and got[3][slot].tobytes() == got[1].tobytes(), (r, f, guided, slot)
                    assert got[0].tobytes() == ref[0].tobytes()
                    assert got[4].sum_var_in[slot] == got[4].guide.sum_var_in and got[4].sum_var_out[slot] == got[4].guide.sum_var_out
        # 3. r = 0 returns every input
        comps, comp_vars = companions(w, h, 4, 4, True)
        for f in (0, 3):
            got = run_gpu(G, img, var, comps, comp_vars, feat, fvar, True, 0, f)
            for a, b in [(got[0], img), (got[1], var)] + list(zip(got[2], comps)) + list(zip(got[3], comp_vars)):
                assert a.tobytes() == b.tobytes()


def test_same_bits_twice_on_a_second_stream_from_the_host_and_enqueue_only(G):
    w, h, r, f, n = 40, 19, 3, 1, 2
    img, var = planted_film(w, h, 5)
    feat, fvar = planted_features(w, h, 5)
    comps, comp_vars = companions(w, h, 5, n, True)
    guide = G.nlm_guide(groups=GROUPS)
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (img, var, feat, fvar))
    d_comp, d_cvar = [hip_rt.upload(G, a) for a in comps], [hip_rt.upload(G, a) for a in comp_vars]
    d_out, d_vout = hip_rt.alloc(G, img.nbytes), hip_rt.alloc(G, img.nbytes)
    d_co, d_cvo = [hip_rt.alloc(G, img.nbytes) for _ in range(n)], [hip_rt.alloc(G, img.nbytes) for _ in range(n)]
    side = hip_rt.stream(G)
    kw = dict(window_radius=r, patch_radius=f, **KW)

    def device(**extra):
        st = G.denoise_nlm_joint_device(w, h, d_img, d_var, d_comp, d_cvar, d_out, d_co, var_out_ptr=d_vout, comp_var_out_ptrs=d_cvo, feat_ptr=d_feat,
                                        feat_var_ptr=d_fvar, guide=guide, **kw, **extra)
        films = [hip_rt.to_host(G, p, img.shape) for p in (d_out, d_vout)]
        return films[0], films[1], [hip_rt.to_host(G, p, img.shape) for p in d_co], [hip_rt.to_host(G, p, img.shape) for p in d_cvo], st

    for direct in FORMS:
        with G.debug_knobs(nlm_direct=direct):
            first = run_gpu(G, img, var, comps, comp_vars, feat, fvar, True, r, f)             # the host entry
            assert first[4].guide.pixels_left_out > 4 and first[4].sum_var_out[1] > 0 and first[4].guide.filter_ms > 0
            for stream in (None, None, side):
                assert joint_bits(device(stream=stream)) == joint_bits(first)
            for p in (d_out, d_vout, *d_co, *d_cvo):
                hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(img.nbytes)))
            got = device(stats=False)                                                           # enqueue-only
            assert got[4] is None and joint_bits((*got[:4], first[4]))[0] == joint_bits(first)[0]
            # the variance outputs are optional, one by one
            hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_co[1]), 0, hip_rt.C.c_size_t(img.nbytes)))
            st = G.denoise_nlm_joint_device(w, h, d_img, d_var, d_comp, d_cvar, d_out, d_co, comp_var_out_ptrs=[None, d_cvo[1]], feat_ptr=d_feat,
                                            feat_var_ptr=d_fvar, guide=guide, **kw)
            assert hip_rt.to_host(G, d_co[1], img.shape).tobytes() == first[2][1].tobytes() and list(st.sum_var_out) == list(first[4].sum_var_out)
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    for p in (d_img, d_var, d_feat, d_fvar, d_out, d_vout, *d_comp, *d_cvar, *d_co, *d_cvo):
        hip_rt.free(G, p)


BUDGET, PASS, FSPP = 32, 4, 4
NLM = dict(window_radius=4, patch_radius=2)


def chain(G, ses, scene, guide, radius, weighted, alpha):
    """gdpt_progressive_denoise_reconstruct composed from the public device entries, on the default stream: (out, filtered,
    filtered_var, joint stats, reconstruction stats)."""
    h, w, _ = ses.shape
    nb = h * w * 3 * 8
    raw, asm_var = [hip_rt.alloc(G, nb) for _ in range(5)], [hip_rt.alloc(G, nb) for _ in range(3)]
    asm, fil, fvar_ = [hip_rt.alloc(G, nb) for _ in range(3)], [hip_rt.alloc(G, nb) for _ in range(3)], [hip_rt.alloc(G, nb) for _ in range(3)]
    d_out, d_sm = hip_rt.alloc(G, nb), hip_rt.alloc(G, nb)
    nf = h * w * 8 * 8
    d_fm, d_fv = hip_rt.alloc(G, nf), hip_rt.alloc(G, nf)
    ses.read_device(mean_ptrs=raw, assembled_var_ptrs=asm_var)
    G.assemble_device(w, h, raw, asm)
    var_c = asm_var[0]
    if radius is not None:
        G.variance_smooth_device(w, h, asm[0], asm_var[0], d_sm, radius=radius)
        var_c = d_sm
    if guide is not None:
        scene.features_device(d_fm, d_fv, FSPP, window=(BUDGET, 0))
    st = G.denoise_nlm_joint_device(w, h, asm[0], var_c, asm[1:], asm_var[1:], fil[0], fil[1:], var_out_ptr=fvar_[0], comp_var_out_ptrs=fvar_[1:],
                                    feat_ptr=d_fm if guide is not None else None, feat_var_ptr=d_fv if guide is not None else None, guide=guide, **NLM)
    if weighted is None:
        rst = G.reconstruct_device(w, h, fil[0], fil[1], fil[2], d_out, dataCost=alpha, norm=G.RECON_L2)
    else:
        rst = G.reconstruct_weighted_device(w, h, fil[0], fil[1], fil[2], fvar_[0], fvar_[1], fvar_[2], d_out, dataCost=alpha, norm=weighted).recon
    res = (hip_rt.to_host(G, d_out, ses.shape), [hip_rt.to_host(G, p, ses.shape) for p in fil], [hip_rt.to_host(G, p, ses.shape) for p in fvar_], st, rst)
    for p in (*raw, *asm_var, *asm, *fil, *fvar_, d_out, d_sm, d_fm, d_fv):
        hip_rt.free(G, p)
    return res


def session_body(G, ses, scene):
    h, w, _ = ses.shape
    seen = set()
    for weighted in (None, G.RECON_L2):
        for guide in (None, G.nlm_guide(k_f=0.7)):
            for radius in (None, 2):
                kw = dict(alpha=0.2, guide=guide, feature_spp=FSPP, var_smooth_radius=radius, weighted=weighted, **NLM)
                out, fl, fv, st, rst = ses.denoise_reconstruct(filtered=True, **kw)
                want = chain(G, ses, scene, guide, radius, weighted, 0.2)
                assert out.tobytes() == want[0].tobytes(), (weighted, guide is not None, radius)
                for k in range(3):
                    assert fl[k].tobytes() == want[1][k].tobytes() and fv[k].tobytes() == want[2][k].tobytes(), (weighted, guide is not None, radius, k)
                assert stats_tuple(st.guide) == stats_tuple(want[3].guide) and list(st.sum_var_in) == list(want[3].sum_var_in)
                assert list(st.sum_var_out) == list(want[3].sum_var_out) and st.sum_var_out[1] > 0 and st.sum_var_out[2] == 0.0
                assert (rst.recon.norm, rst.recon.irls_rounds) == (want[4].norm, want[4].irls_rounds)
                assert np.isfinite(out).all() and st.guide.pixels_left_out == 0
                # the same bits without the planes asked for, and in device memory
                assert ses.denoise_reconstruct(**kw)[0].tobytes() == out.tobytes()
                seen.add(out.tobytes())
    assert len(seen) == 8                                         # every option is at work
    nb = out.nbytes
    d_out, d_f, d_v = hip_rt.alloc(G, nb), [hip_rt.alloc(G, nb) for _ in range(3)], [hip_rt.alloc(G, nb) for _ in range(3)]
    st2, _ = ses.denoise_reconstruct(out_ptr=d_out, filtered_ptrs=d_f, filtered_var_ptrs=[None, d_v[1], None], **kw)
    assert hip_rt.to_host(G, d_out, out.shape).tobytes() == out.tobytes() and hip_rt.to_host(G, d_f[2], out.shape).tobytes() == fl[2].tobytes()
    assert hip_rt.to_host(G, d_v[1], out.shape).tobytes() == fv[1].tobytes() and stats_tuple(st2.guide) == stats_tuple(st.guide)
    for p in (d_out, *d_f, *d_v):
        hip_rt.free(G, p)
    plain, _ = ses.reconstruct(alpha=0.2, norm=G.RECON_L2)
    assert plain.tobytes() != out.tobytes()


@pytest.mark.parametrize("shift", ["reference", "reconnect"])
def test_session_against_the_chain_of_device_entries(G, scene_tmp, shift):
    """cbox 40 x 24, 32 spp in passes of 4: a one-pass session is refused, then every option against the composed chain."""
    sd = G.parse_scene(scene_variant(scene_tmp, CBOX, width=40, height=24))
    sc = G.Scene(sd)
    ses = G.Progressive(sc, BUDGET, shift=G.SHIFT_RECONNECT if shift == "reconnect" else G.SHIFT_REFERENCE)
    ses.add_pass(PASS)
    with pytest.raises(G.GdptError, match="gdpt_progressive_denoise_reconstruct: variances need at least 2 passes"):
        ses.denoise_reconstruct()
    ses.run(pass_spp=PASS)
    assert ses.status()["passes"] == BUDGET // PASS
    session_body(G, ses, sc)
    for bad in (1, BUDGET + 1):
        with pytest.raises(G.GdptError, match="feature_spp"):
            ses.denoise_reconstruct(guide=G.nlm_guide(), feature_spp=bad)
    ses.close()
    sc.close()


@pytest.mark.parametrize("shift", ["reference", "reconnect"])
def test_group_total_against_the_chain_of_device_entries(G, scene_tmp, shift):
    sd = G.parse_scene(scene_variant(scene_tmp, CBOX, width=40, height=24))
    grp = G.ProgressiveGroup(sd, (0, 0), BUDGET, shift=G.SHIFT_RECONNECT if shift == "reconnect" else G.SHIFT_REFERENCE)
    grp.run(pass_spp=PASS)
    assert grp.total.status()["passes"] == BUDGET // PASS
    sc = G.Scene(sd)
    session_body(G, grp.total, sc)
    sc.close()
    grp.close()


def test_a_path_session_is_refused_by_name(G, scene_tmp):
    sd = G.parse_scene(scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path"))
    sc = G.Scene(sd)
    ses = G.Progressive(sc, 8, path=True)
    ses.run(pass_spp=4)
    with pytest.raises(G.GdptError, match="gdpt_progressive_denoise_reconstruct: an Integrator::Path session has no gradients"):
        ses.denoise_reconstruct()
    ses.close()
    sc.close()


EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")


def test_cli_nlm_joint(G, scene_tmp, tmp_path):
    xml = scene_variant(scene_tmp, CBOX, width=40, height=24)
    out, out0, den, den0 = tmp_path / "o.pfm", tmp_path / "o0.pfm", tmp_path / "d.pfm", tmp_path / "d0.pfm"
    base = [EXE, "--spp", str(BUDGET), "--pass-spp", str(PASS)]
    nlm = ["--nlm-window", "4", "--nlm-patch", "2"]
    r0 = subprocess.run([*base, "--denoised", str(den0), *nlm, "-o", str(out0), xml], capture_output=True, text=True, timeout=300)
    r1 = subprocess.run([*base, "--denoised", str(den), "--nlm-joint", *nlm, "--nlm-var-smooth", "2", "--reconstruct", "wl2", "-o", str(out), xml],
                        capture_output=True, text=True, timeout=300)
    r2 = subprocess.run([*base, "--reconstruct", "wl2", "-o", str(out0), xml], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and r1.returncode == 0 and r2.returncode == 0, r0.stderr + r1.stderr + r2.stderr
    sha = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()      # noqa: E731
    assert sha(out) == sha(out0)                                  # -o is the plain reconstruction, with or without --nlm-joint
    sc = G.Scene(G.parse_scene(xml))
    ses = G.Progressive(sc, BUDGET)
    ses.run(pass_spp=PASS)
    want, st, _ = ses.denoise_reconstruct(var_smooth_radius=2, weighted=G.RECON_L2, **NLM)
    assert np.array_equal(read_pfm(den, 40, 24), want.astype(np.float32))
    assert not np.array_equal(read_pfm(den, 40, 24), read_pfm(den0, 40, 24))
    line = [l for l in r1.stdout.splitlines() if l.startswith("[gdpt] joint:")]
    assert len(line) == 1 and not [l for l in r1.stdout.splitlines() if l.startswith("[gdpt] denoised:")]
    m = re.fullmatch(r"\[gdpt\] joint: (\d+) pixels left out; variance c ×(\S+), cx ×(\S+), cy ×(\S+)", line[0])
    assert m and int(m.group(1)) == st.guide.pixels_left_out == 0
    ratios = [st.guide.sum_var_out / st.guide.sum_var_in, st.sum_var_out[0] / st.sum_var_in[0], st.sum_var_out[1] / st.sum_var_in[1]]
    assert all(0 < x < 1 for x in ratios)
    assert [float(m.group(k)) for k in (2, 3, 4)] == pytest.approx(ratios, rel=1e-4)      # (printed with six digits)
    ses.close()
    sc.close()
    r = subprocess.run([*base, "--denoised", str(den), "--nlm-joint", "--reconstruct", "l1", "-o", str(out), xml], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--nlm-joint is not combined with --reconstruct l1" in r.stderr, r.stderr
