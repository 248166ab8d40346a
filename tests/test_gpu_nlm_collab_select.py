"""The collaborative regression as a candidate of the per-pixel filter selection (include/gdpt.h: GDPT_SELECT_NLM_COLLAB in
gdpt_progressive_group_denoise_select; `collab` in lajolla --select): the selection between the point regression and its collaborative
form is, bit for bit, the chain composed from Python with the device entries, the candidate's stats carry the NaN fields of
gdpt_denoise_nlm_collab, and what the selection refuses stays refused."""
import math
import os
import subprocess

import numpy as np
import pytest

import hip_rt
from helpers import ROOT, scene_variant
from test_gpu_filter_select import CBOX, read_i32, stats_bits
from test_gpu_progressive import read_pfm

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")
SUMS = ("pixels_left_out", "sum_var_in", "sum_sq_in", "sum_sq_out")


def chain(G, sessions, sc, candidates, B, fspp, s):
    """The chain of include/gdpt.h for regress and collab candidates, composed from Python with the device entries: for each of A, B
    and the total, read() of buffer 0 and the candidate's device filter on the features of Scene.features with the window {B, 0};
    then filter_select_device. Returns (out, sel, mse, stats, the candidates' stats on the total)."""
    h, w, _ = sessions[0].shape
    fm, fv = sc.features(fspp, window=(B, 0))
    d_feat, d_fvar = hip_rt.upload(G, fm), hip_rt.upload(G, fv)
    nbytes = 24 * w * h
    held, films, stats_t, halves = [d_feat, d_fvar], [[], [], []], [], []
    for k, ses in enumerate(sessions):
        means, vars_, _ = ses.read()
        d_img, d_var = hip_rt.upload(G, means["img"]), hip_rt.upload(G, vars_["img"])
        held += [d_img, d_var]
        if k < 2:
            halves += [d_img, d_var]
        for c in candidates:
            d_out = hip_rt.alloc(G, nbytes)
            held.append(d_out)
            entry = {"regress": G.denoise_nlm_regress_device, "collab": G.denoise_nlm_collab_device}[c["filter"]]
            st = entry(w, h, d_img, d_var, d_feat, d_fvar, d_out, guide=c.get("guide"), regress=c.get("regress"), **c.get("nlm", {}))
            films[k].append(d_out)
            if k == 2:
                stats_t.append(st)
    d_o, d_s, d_m = hip_rt.alloc(G, nbytes), hip_rt.alloc(G, 4 * w * h), hip_rt.alloc(G, 8 * w * h)
    st = G.filter_select_device(w, h, films[0], films[1], films[2], *halves, d_o, d_s, d_m, radius=s)
    res = (hip_rt.to_host(G, d_o, (h, w, 3)), read_i32(G, d_s, (h, w)), hip_rt.to_host(G, d_m, (h, w)), st, stats_t)
    for p in held + [d_o, d_s, d_m]:
        hip_rt.free(G, p)
    return res


@pytest.mark.parametrize("path", [True, False], ids=["path", "gradpath"])
def test_group_denoise_select_between_the_point_and_the_collaborative_regression(G, scene_tmp, path):
    """cbox at 40 x 24, budget 32 in passes of 4 on a group over (0, 0)."""
    B, P = 32, 4
    xml = scene_variant(scene_tmp, CBOX, width=40, height=24, integrator="path") if path else scene_variant(scene_tmp, CBOX, width=40, height=24)
    sd = G.parse_scene(xml)
    grp = G.ProgressiveGroup(sd, (0, 0), B, path=path)
    grp.run(pass_spp=P)
    blocks = dict(guide=G.nlm_guide(groups=[(0, 3, 1e-3)]), regress=G.nlm_regress(ridge=1e-3), nlm=dict(k=4.0, window_radius=4, patch_radius=2))
    cands = [dict(filter="regress", **blocks), dict(filter="collab", **blocks)]
    a, b = grp.halves()
    sc = G.Scene(sd)
    fspp, s = 4, 4
    want = chain(G, (a, b, grp.total), sc, cands, B, fspp, s)
    out, sel, mse, st, cst = grp.denoise_select(cands, radius=s, feature_spp=fspp, maps=True)
    assert np.array_equal(out, want[0]) and np.array_equal(sel, want[1]) and np.array_equal(mse, want[2])
    assert stats_bits(st, want[3], 2) and st.pixels_left_out == 0 and sum(st.chosen[:2]) == 40 * 24
    for got, ref in zip(cst, want[4]):
        assert [getattr(got, k) for k in SUMS] == [getattr(ref, k) for k in SUMS]
    assert math.isnan(cst[1].sum_var_out) and math.isnan(cst[1].error_out) and cst[0].sum_var_out > 0
    assert set(sel.ravel().tolist()) == {0, 1}                                   # each wins somewhere
    print(f"selected: regress {st.chosen[0]}, collab {st.chosen[1]} of {40 * 24} pixels")
    # n = 1: the session call on the total; by its GDPT_SELECT_* value as well
    one, st1, _ = grp.denoise_select([cands[1]], feature_spp=fspp)
    ref = grp.total.denoise_collab(fspp, guide=blocks["guide"], regress=blocks["regress"], **blocks["nlm"])[0]
    assert np.array_equal(one, ref) and st1.chosen[0] == 40 * 24
    assert G.SELECT_NLM_COLLAB == 6
    assert np.array_equal(grp.denoise_select([dict(cands[1], filter=6)], feature_spp=fspp)[0], ref)
    # refusals that name their field
    for bad, match in (([dict(filter=9)], "filter must be one of"), ([dict(filter=7)], "filter must be one of"),
                       ([dict(filter="collab", var_smooth=2)], "var_smooth_radius"), ([dict(filter="collab", demod=G.nlm_demod())], "demod must be null"),
                       ([dict(filter="collab", atrous=dict(levels=3))], "atrous must be null"),
                       ([dict(filter="guided", regress=G.nlm_regress())], "regress must be null"),
                       ([dict(filter="collab", regress=G.nlm_regress(ridge=0.0))], "ridge")):
        with pytest.raises(G.GdptError, match=match):
            grp.denoise_select(bad)
    sc.close()
    grp.close()


def test_cli_select_collab(G, scene_tmp, tmp_path):
    xml = scene_variant(scene_tmp, CBOX, width=40, height=24, integrator="path")
    out, den = tmp_path / "o.pfm", tmp_path / "d.pfm"
    r = subprocess.run([EXE, "--spp", "32", "--pass-spp", "4", "--sample-devices", "0,0", "--denoised", str(den), "--select", "regress,collab", "--select-radius", "3", "--feature-spp", "4",
                        "-o", str(out), xml], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    grp = G.ProgressiveGroup(G.parse_scene(xml), (0, 0), 32, path=True)
    grp.run(pass_spp=4)
    blocks = dict(guide=G.nlm_guide(groups=[(0, 3, 1e-3)]), nlm=dict(k=4.0))
    want, st, _ = grp.denoise_select([dict(filter="regress", **blocks), dict(filter="collab", **blocks)], radius=3, feature_spp=4)
    assert np.array_equal(read_pfm(den, 40, 24), want.astype(np.float32))
    line = [l for l in r.stdout.splitlines() if l.startswith("[gdpt] selected:")]
    assert len(line) == 1 and " regress " in line[0] and " collab " in line[0]
    grp.close()
    r = subprocess.run([EXE, "--pass-spp", "4", "--sample-devices", "0,0", "--denoised", str(den), "--select", "collab,collab", "-o", str(out), xml],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "each once" in r.stderr and "collab" in r.stderr
