"""The non-local-means filter on the GPU (include/gdpt.h: gdpt_denoise_nlm*, gdpt_progressive_denoise): both kernel forms against
the numpy restatement (tests/nlm_ref.py) and against each other, the same bits twice and on a second stream, the host entry, the
enqueue-only form, the sessions (Path, GradPath, a group's total), the CLI."""
import os
import subprocess

import numpy as np
import pytest

import hip_rt
import nlm_ref as N
from helpers import ROOT, rel_l2, scene_variant
from test_gpu_progressive import read_pfm
from test_nlm_ref import noisy_film

pytestmark = pytest.mark.gpu
CBOX = "cbox/cbox_gdpt.xml"

# measured on an MI355X: the worst figure (masked relative L2 of out and of var_out, relative difference of the four film sums)
# between either kernel form and the restatement, and between the two forms, over every case of the two tests below (the planted
# ones included). The sides differ by FMA contraction, the order of the patch sums and the last place of exp; 100 x the measured
# value is the margin, never looser than 1e-9. Measured: 4.238e-16 for either form against the restatement, 2.951e-16 between the forms,
# over the 84 cases (7 films x 6 radii, clean and planted).
NLM_MEASURED = 4.3e-16
NLM_BOUND = min(100 * NLM_MEASURED, 1e-9) if NLM_MEASURED else None

FILMS = [(1, 1), (2, 2), (1, 7), (7, 1), (17, 17), (33, 9), (40, 19)]      # W x H: 17 x 17 is one pixel beyond a 16 x 16 tile in each direction
RADII = [(0, 0), (0, 3), (1, 0), (2, 1), (3, 3), (10, 3)]                  # (r, f): at (10, 3) the window exceeds every film
FORMS = (0, 1)                                                             # knob nlm_direct


def planted_film(w, h, seed):
    """NaN, +Inf, -Inf and a negative variance: at a corner, at an edge, in the middle and one pixel beyond the first tile (its halo)."""
    img, var = noisy_film(w, h, seed)
    spots = [(0, 0, "nan"), (0, w // 2, "neg"), (h // 2, w // 2, "-inf"), (h - 1, w - 1, "+inf")]
    if w > 16:
        spots += [(min(5, h - 1), 16, "neg"), (h // 2, 15, "nan")]
    if h > 16:
        spots += [(16, 3, "+inf")]
    for y, x, kind in spots:
        if kind == "nan":
            img[y, x, 1] = np.nan
        elif kind == "+inf":
            var[y, x, 0] = np.inf
        elif kind == "-inf":
            img[y, x, 2] = -np.inf
        else:
            var[y, x, 2] = -1e-4
    return img, var


def masked_rel_l2(got, want):
    """Relative L2 over the finite entries; the non-finite entries must be the same ones."""
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    return rel_l2(got[fin], want[fin]) if fin.any() else 0.0


def rel_diff(got, want):
    if want == 0.0:
        assert got == 0.0
        return 0.0
    return abs(got - want) / abs(want)


SUMS = ("sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out")


def figure(out, var_out, st, want):
    """The worst figure of one call against `want` (the restatement's dict, or another call's); the exact parts are asserted here."""
    figs = [masked_rel_l2(out, want["out"]), masked_rel_l2(var_out, want["var_out"])]
    figs += [rel_diff(getattr(st, k), want[k]) for k in SUMS]
    assert st.pixels_left_out == want["left_out"]
    for e, a, b in ((st.error_in, st.sum_var_in, st.sum_sq_in), (st.error_out, st.sum_var_out, st.sum_sq_out)):
        with np.errstate(all="ignore"):
            assert np.array_equal(e, np.sqrt(np.float64(a) / np.float64(b)), equal_nan=True)
    return max(figs)


def as_dict(out, var_out, st):
    d = dict(out=out, var_out=var_out, left_out=st.pixels_left_out)
    d.update({k: getattr(st, k) for k in SUMS})
    return d


@pytest.fixture(scope="module")
def cases(G):
    """Every film x (r, f), clean and planted: the inputs, the restatement's result (computed once, left unchanged) and both forms'."""
    out = []
    for planted in (False, True):
        for (w, h) in FILMS:
            img, var = planted_film(w, h, 10 * w + h) if planted else noisy_film(w, h, 10 * w + h)
            for (r, f) in RADII:
                want = N.denoise(img, var, r=r, f=f)
                got = []
                for direct in FORMS:
                    with G.debug_knobs(nlm_direct=direct):
                        got.append(G.denoise_nlm(img, var, window_radius=r, patch_radius=f))
                    assert (got[-1][2].window_radius, got[-1][2].patch_radius) == (r, f) and got[-1][2].filter_ms > 0
                out.append(((w, h, r, f, planted), img, var, want, got))
    return out


def test_both_forms_against_the_restatement(cases):
    worst = {0: 0.0, 1: 0.0}
    for key, img, var, want, got in cases:
        w, h, r, f, planted = key
        ok = N.valid_mask(img, var)
        assert want["left_out"] == (~ok).sum() and (not planted or want["left_out"] >= 1)
        for direct in FORMS:
            o, vo, st = got[direct]
            assert np.array_equal(o[~ok], img[~ok], equal_nan=True) and np.array_equal(vo[~ok], var[~ok], equal_nan=True), key
            if r == 0:
                assert np.array_equal(o, img, equal_nan=True) and np.array_equal(vo, var, equal_nan=True), key
            worst[direct] = max(worst[direct], figure(o, vo, st, want))
    print(f"nlm against the restatement: worst figure tiled {worst[0]:.3e}, direct {worst[1]:.3e} (bound {NLM_BOUND})")
    assert NLM_BOUND is not None, f"NLM_MEASURED has not been recorded; this run measured {max(worst.values()):.3e}"
    assert max(worst.values()) < NLM_BOUND


def test_the_two_forms_agree(cases):
    worst = 0.0
    for key, img, var, want, got in cases:
        worst = max(worst, figure(*got[0], as_dict(*got[1])))
    print(f"nlm tiled against direct: worst figure {worst:.3e} (bound {NLM_BOUND})")
    assert NLM_BOUND is not None, f"NLM_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < NLM_BOUND


def test_same_bits_twice_on_a_second_stream_from_the_host_and_enqueue_only(G):
    w, h, r, f = 40, 19, 3, 1
    img, var = planted_film(w, h, 5)
    d_img, d_var = hip_rt.upload(G, img), hip_rt.upload(G, var)
    d_out, d_vout = hip_rt.alloc(G, img.nbytes), hip_rt.alloc(G, img.nbytes)
    side = hip_rt.stream(G)
    for direct in FORMS:
        with G.debug_knobs(nlm_direct=direct):
            runs = []
            for stream in (None, None, side):
                st = G.denoise_nlm_device(w, h, d_img, d_var, d_out, d_vout, stream=stream, window_radius=r, patch_radius=f)
                runs.append((hip_rt.to_host(G, d_out, img.shape), hip_rt.to_host(G, d_vout, img.shape), st))
            runs.append(G.denoise_nlm(img, var, window_radius=r, patch_radius=f))           # the host entry
            first = runs[0]
            assert first[2].pixels_left_out > 0 and first[2].sum_var_out > 0
            for o, vo, st in runs[1:]:
                assert np.array_equal(o, first[0], equal_nan=True) and np.array_equal(vo, first[1], equal_nan=True)
                assert [getattr(st, k) for k in SUMS] == [getattr(first[2], k) for k in SUMS] and st.pixels_left_out == first[2].pixels_left_out
            # stats == NULL: enqueue-only, the same planes; var_out is optional
            for p in (d_out, d_vout):
                hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(img.nbytes)))
            assert G.denoise_nlm_device(w, h, d_img, d_var, d_out, d_vout, stats=False, window_radius=r, patch_radius=f) is None
            assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True)
            assert np.array_equal(hip_rt.to_host(G, d_vout, img.shape), first[1], equal_nan=True)
            hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(img.nbytes)))
            st = G.denoise_nlm_device(w, h, d_img, d_var, d_out, window_radius=r, patch_radius=f)
            assert np.array_equal(hip_rt.to_host(G, d_out, img.shape), first[0], equal_nan=True) and st.sum_var_out == first[2].sum_var_out
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    for p in (d_img, d_var, d_out, d_vout):
        hip_rt.free(G, p)


def session_body(G, ses):
    """`ses` holds at least two passes: denoise() is denoise_nlm_device on the planes read() returns, bit for bit, in host and in
    device memory."""
    h, w, _ = ses.shape
    kw = dict(window_radius=4, patch_radius=2)
    out, var_out, st = ses.denoise(**kw)
    means, vars_, _ = ses.read()
    d_img, d_var = hip_rt.upload(G, means["img"]), hip_rt.upload(G, vars_["img"])
    d_out, d_vout = hip_rt.alloc(G, out.nbytes), hip_rt.alloc(G, out.nbytes)
    st2 = G.denoise_nlm_device(w, h, d_img, d_var, d_out, d_vout, **kw)
    assert np.array_equal(hip_rt.to_host(G, d_out, out.shape), out) and np.array_equal(hip_rt.to_host(G, d_vout, out.shape), var_out)
    assert [getattr(st, k) for k in SUMS] == [getattr(st2, k) for k in SUMS] and st.pixels_left_out == st2.pixels_left_out == 0
    # the estimate of the valid pixels is the session's own, up to the order of its sum
    assert abs(st.error_in - ses.status()["error"]) <= 1e-12 * st.error_in and 0 < st.error_out < st.error_in
    assert np.isfinite(out).all() and not np.array_equal(out, means["img"])
    hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(d_out), 0, hip_rt.C.c_size_t(out.nbytes)))
    st3 = ses.denoise(out_ptr=d_out, var_out_ptr=d_vout, **kw)
    assert np.array_equal(hip_rt.to_host(G, d_out, out.shape), out) and st3.sum_var_out == st.sum_var_out
    with pytest.raises(G.GdptError, match="window_radius"):
        ses.denoise(window_radius=11)
    for p in (d_img, d_var, d_out, d_vout):
        hip_rt.free(G, p)


@pytest.mark.parametrize("path", [True, False], ids=["path", "gradpath"])
def test_session(G, scene_tmp, path):
    """cbox 24 x 24, budget 16 in four passes of 4: refused after one pass, then the filter on the planes read() returns."""
    sd = G.parse_scene(scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path" if path else None))
    sc = G.Scene(sd)
    ses = G.Progressive(sc, 16, path=path)
    ses.add_pass(4)
    with pytest.raises(G.GdptError, match="at least 2 passes"):
        ses.denoise()
    ses.run(pass_spp=4)
    assert ses.status()["passes"] == 4
    session_body(G, ses)
    ses.close()
    sc.close()


def test_group_total(G, scene_tmp):
    sd = G.parse_scene(scene_variant(scene_tmp, CBOX, width=24, height=24))
    grp = G.ProgressiveGroup(sd, (0, 0), 16)
    grp.run(pass_spp=4)
    assert grp.total.status()["passes"] == 4
    session_body(G, grp.total)
    grp.close()


def test_cli_denoised(G, scene_tmp, tmp_path):
    exe = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")
    xml = scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path")
    plain, out, den = tmp_path / "p.pfm", tmp_path / "o.pfm", tmp_path / "d.pfm"
    base = [exe, "--spp", "16", "--pass-spp", "4"]
    r0 = subprocess.run([*base, "-o", str(plain), xml], capture_output=True, text=True, timeout=300)
    r = subprocess.run([*base, "--denoised", str(den), "--nlm-window", "4", "--nlm-patch", "2", "--nlm-k", "0.5", "-o", str(out), xml],
                       capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and r.returncode == 0, r0.stderr + r.stderr
    assert open(plain, "rb").read() == open(out, "rb").read()
    sc = G.Scene(G.parse_scene(xml))
    ses = G.Progressive(sc, 16, path=True)
    ses.run(pass_spp=4)
    want, _, st = ses.denoise(window_radius=4, patch_radius=2, k=0.5)
    assert np.array_equal(read_pfm(den, 24, 24), want.astype(np.float32))
    assert np.array_equal(read_pfm(out, 24, 24), ses.read()[0]["img"].astype(np.float32))
    line = [l for l in r.stdout.splitlines() if l.startswith("[gdpt] denoised:")]
    assert len(line) == 1 and "filter_ms" in line[0] and not [l for l in r0.stdout.splitlines() if l.startswith("[gdpt] denoised:")], r.stdout
    for name, val in (("error_in", st.error_in), ("error_out", st.error_out)):
        printed = float(line[0].split(name + " ")[1].split()[0].rstrip(","))
        assert abs(printed - val) <= 1e-5 * val
    ses.close()
    sc.close()
    r = subprocess.run([exe, "--spp", "16", "--denoised", str(den), "-o", str(out), xml], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--denoised needs --pass-spp" in r.stderr and "no variance exists without passes" in r.stderr
