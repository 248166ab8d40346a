"""The per-pixel filter selection on the GPU (include/gdpt.h: gdpt_filter_select*): the kernel's window means against the numpy
restatement (tests/filter_select_ref.py), the exact parts of the definition on the kernel's own window means, the choice against the
restatement's, the five identities bit for bit, and the same bits from two calls, a second stream, the host and device entries and
the enqueue-only form; and the two halves of a progressive group (gdpt_progressive_group_halves) against slices drawn and merged by
hand, the session entry (gdpt_progressive_group_denoise_select) against the composed chain, and the CLI."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import filter_select_ref as FS
import hip_rt
from test_filter_select_ref import identities
from test_gpu_nlm import masked_rel_l2, rel_diff

pytestmark = pytest.mark.gpu

# The worst figure (masked relative L2 of the n planes E_j, relative difference of sum_sq_out and, scaled by the film sum of |e_j|, of
# every sum_e[j]) between the kernel and the restatement over every case of the first two tests below. Both sides form e_j in the same
# correctly rounded operations and add the window in the same order; the film sums differ by the order of their reduction. 100 x the
# measured value is the margin, never looser than 1e-9, as in tests/test_gpu_nlm.py. Measured on an MI355X: 3.967e-16 over the 192 cases
# and 7.241e-16 on the film past the block cap (n = 8, radius 8), with no pixel's choice differing from the restatement's.
SELECT_MEASURED = 7.3e-16
SELECT_BOUND = min(100 * SELECT_MEASURED, 1e-9) if SELECT_MEASURED is not None else None

# W x H: 17 x 17 is one pixel beyond a 16 x 16 tile each way; at 70 x 37 a radius-8 window reaches into a third tile
FILMS = [(1, 1), (16, 16), (17, 17), (33, 9), (40, 19), (70, 37)]
LARGE = (1025, 345)                                        # 65 x 22 = 1430 tiles, beyond the cap of 1024 blocks
COUNTS = [1, 2, 3, 8]
RADII = [0, 1, 4, 8]


def inputs(w, h, n, seed, kind=None):
    """fields() of the restatement, clean or with values planted in one kind of input; a planted film beyond the block cap also gets
    values in tile 1024 (the second trip of block 0) and on the border of the tile before it."""
    f = FS.fields(w, h, n, seed)
    if kind is None:
        return f
    f = FS.plant(f, kind, seed + 1)
    tiles_x = (w + 15) // 16
    if tiles_x * ((h + 15) // 16) > 1024:
        y0, x0 = 16 * (1024 // tiles_x), 16 * (1024 % tiles_x)
        f[4][y0 + 1, x0, 1], f[3][y0 + 3, x0 - 1, 0], f[0][-1][y0, x0 + 15, 2], f[2][0][y0 + 15, x0 + 2, 0] = -1e-3, np.inf, np.nan, -np.inf
    return f


def gpu_select(G, FA, FB, T, uA, vA, uB, vB, radius):
    """G.filter_select with the restatement's signature and keys."""
    out, sel, mse, E, st = G.filter_select(FA, FB, T, uA, vA, uB, vB, radius=radius, E=True)
    n = len(T)
    assert st.radius == radius and st.num_candidates == n and st.select_ms > 0
    assert list(st.chosen[n:]) == [0] * (8 - n) and list(st.sum_e[n:]) == [0.0] * (8 - n)
    return dict(out=out, sel=sel, mse=mse, E=E, left_out=int(st.pixels_left_out), chosen=list(st.chosen[:n]), sum_e=list(st.sum_e[:n]),
                sum_mse=st.sum_mse, sum_sq_out=st.sum_sq_out)


def exact_parts(got, T, ok):
    """On the kernel's own E: sel is the lowest-index argmin, out is T[sel], mse is E_sel; the invalid pixels' bits and the counts."""
    E = np.where(ok[None], got["E"], np.inf)
    assert not np.isnan(got["E"][:, ok]).any() and np.isnan(got["E"][:, ~ok]).all()
    assert np.array_equal(got["sel"][ok], np.argmin(E, axis=0)[ok]) and (got["sel"][~ok] == -1).all()
    assert np.array_equal(got["mse"][ok], np.min(E, axis=0)[ok]) and np.isnan(got["mse"][~ok]).all()
    want = T[0].copy()
    for j in range(1, len(T)):
        want[got["sel"] == j] = T[j][got["sel"] == j]
    assert np.array_equal(got["out"], want, equal_nan=True)
    assert got["left_out"] == (~ok).sum() and got["chosen"] == [int((got["sel"] == j).sum()) for j in range(len(T))]


def against_the_restatement(got, want, ok, key):
    """(the figure, the number of excused pixels): E, the sums; sel where the restatement's choice is clear."""
    n = len(got["E"])
    fig = masked_rel_l2(got["E"], want["E"])
    if ok.any():
        fig = max(fig, rel_diff(got["sum_sq_out"], float((got["out"] * got["out"])[ok].sum())))
        for j in range(n):
            scale = float(np.abs(want["e"][j][ok]).sum())
            fig = max(fig, abs(got["sum_e"][j] - want["sum_e"][j]) / scale)
        fig = max(fig, abs(got["sum_mse"] - float(got["mse"][ok].sum())) / float(np.abs(got["mse"][ok]).sum()))
    differ = ok & (got["sel"] != want["sel"])
    if differ.any():
        assert SELECT_BOUND is not None, (key, "sel differs before a bound was recorded", int(differ.sum()))
        ys, xs = np.nonzero(differ)
        gap = np.abs(want["E"][got["sel"][ys, xs], ys, xs] - want["E"][want["sel"][ys, xs], ys, xs])
        assert (gap < SELECT_BOUND * np.abs(want["E"][:, ok]).max()).all(), key
        assert differ.sum() <= 0.01 * ok.sum(), key
    return fig, int(differ.sum())


def run_case(G, w, h, n, s, kind, seed):
    f = inputs(w, h, n, seed, kind)
    want = FS.select(*f, radius=s)
    got = gpu_select(G, *f, s)
    ok = FS.valid_mask(*f)
    key = (w, h, n, s, kind)
    assert want["left_out"] == (~ok).sum() and (kind is None) == (want["left_out"] == 0), key
    exact_parts(got, f[2], ok)
    if s == 0:
        assert np.array_equal(got["E"][:, ok], want["e"][:, ok]), key          # s = 0 gives E = e, and e is formed in the header's operations
    return against_the_restatement(got, want, ok, key)


def test_against_the_restatement(G):
    """Every film x n x radius, clean and planted (the kind of input planted in rotates over the cases)."""
    worst, cases, excused = 0.0, 0, 0
    for (w, h) in FILMS:
        for n in COUNTS:
            for s in RADII:
                for kind in (None, FS.KINDS[cases // 2 % len(FS.KINDS)]):
                    fig, ex = run_case(G, w, h, n, s, kind, 10 * w + h + n)
                    worst, cases, excused = max(worst, fig), cases + 1, excused + ex
    assert cases == 192
    print(f"filter selection against the restatement over {cases} cases: worst figure {worst:.3e}, {excused} pixels excused (bound {SELECT_BOUND})")
    assert SELECT_BOUND is not None, f"SELECT_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < SELECT_BOUND


@pytest.mark.parametrize("n,s,kind", [(3, 4, None), (8, 8, "vA")], ids=["3-4-clean", "8-8-planted"])
def test_a_film_past_the_block_cap(G, n, s, kind):
    fig, ex = run_case(G, *LARGE, n, s, kind, 77)
    print(f"{LARGE}, n = {n}, s = {s}: figure {fig:.3e}, {ex} pixels excused (bound {SELECT_BOUND})")
    assert SELECT_BOUND is not None and fig < SELECT_BOUND


@pytest.mark.parametrize("w,h", [(40, 19), (70, 37)])
@pytest.mark.parametrize("s", RADII)
def test_exact_identities_bit_for_bit(G, w, h, s):
    identities(lambda *a, radius: gpu_select(G, *a, radius), w, h, s, 5)


def read_i32(G, ptr, shape):
    out = np.empty(shape, dtype=np.int32)
    hip_rt.ck(hip_rt.rt(G).hipDeviceSynchronize())
    hip_rt.ck(hip_rt.rt(G).hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2))
    return out


STATS = ("pixels_left_out", "sum_mse", "sum_sq_out")


def stats_bits(a, b, n):
    return [getattr(a, k) for k in STATS] == [getattr(b, k) for k in STATS] and list(a.chosen[:n]) == list(b.chosen[:n]) and \
        list(a.sum_e[:n]) == list(b.sum_e[:n])


@pytest.mark.parametrize("w,h", [(40, 19), LARGE])
def test_host_and_device_entries_same_bits_second_stream_and_enqueue_only(G, w, h):
    n = 3
    f = inputs(w, h, n, 5, "FB")
    flat = list(f[0]) + list(f[1]) + list(f[2]) + list(f[3:])
    d_in = [hip_rt.upload(G, a) for a in flat]
    d_FA, d_FB, d_T, d_half = d_in[:n], d_in[n:2 * n], d_in[2 * n:3 * n], d_in[3 * n:]
    px = w * h
    d_out, d_sel, d_mse, d_E = hip_rt.alloc(G, 24 * px), hip_rt.alloc(G, 4 * px), hip_rt.alloc(G, 8 * px), hip_rt.alloc(G, 8 * n * px)
    sizes = ((d_out, 24 * px), (d_sel, 4 * px), (d_mse, 8 * px), (d_E, 8 * n * px))
    side = hip_rt.stream(G)

    def zero():
        for p, nbytes in sizes:
            hip_rt.ck(hip_rt.rt(G).hipMemset(C.c_void_p(p), 0, C.c_size_t(nbytes)))

    def device_bits():
        return (hip_rt.to_host(G, d_out, (h, w, 3)), read_i32(G, d_sel, (h, w)), hip_rt.to_host(G, d_mse, (h, w)), hip_rt.to_host(G, d_E, (n, h, w)))

    same = lambda a, b: all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))      # noqa: E731
    for s in (1, 8):
        *first, st0 = G.filter_select(*f, radius=s, E=True)                      # the host entry
        assert st0.pixels_left_out >= 1 and st0.select_ms > 0
        *again, st1 = G.filter_select(*f, radius=s, E=True)
        assert same(again, first) and stats_bits(st1, st0, n)
        out_only, st2 = G.filter_select(*f, radius=s, maps=False)                # the nullable outputs left out
        assert np.array_equal(out_only, first[0], equal_nan=True) and stats_bits(st2, st0, n)
        for stream in (None, None, side):
            zero()
            st = G.filter_select_device(w, h, d_FA, d_FB, d_T, *d_half, d_out, d_sel, d_mse, d_E, stream=stream, radius=s)
            assert same(device_bits(), first) and stats_bits(st, st0, n), (s, stream)
        zero()
        assert G.filter_select_device(w, h, d_FA, d_FB, d_T, *d_half, d_out, d_sel, d_mse, d_E, stats=False, radius=s) is None
        assert same(device_bits(), first)
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    for p in d_in + [d_out, d_sel, d_mse, d_E]:
        hip_rt.free(G, p)


CBOX = "cbox/cbox_gdpt.xml"


def session_planes(ses):
    """The means and variances of the session's buffers and, for GradPath, the assembled variances."""
    means, var, asm = ses.read()
    return [means[k] for k in ses.names] + [var[k] for k in ses.names] + ([] if ses.path else [asm[k] for k in ("c", "cx", "cy")])


@pytest.mark.parametrize("path", [True, False], ids=["path", "gradpath"])
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["two", "three"])
def test_group_halves(G, scene_tmp, devices, path):
    """cbox at 40 x 24, budget 32 in passes of 4: halves() is, bit for bit, the members' slices drawn by hand and merged alternately, in
    member order, into two accumulators; the halves are rebuilt after a round, read and denoise as sessions, and take no passes."""
    from helpers import scene_variant
    B, P, N = 32, 4, len(devices)
    xml = scene_variant(scene_tmp, CBOX, width=40, height=24, integrator="path") if path else scene_variant(scene_tmp, CBOX, width=40, height=24)
    sd = G.parse_scene(xml)
    grp = G.ProgressiveGroup(sd, devices, B, path=path)
    with pytest.raises(G.GdptError, match="at least two members that hold samples"):
        grp.halves()
    grp.run(pass_spp=P, max_rounds=1)
    early = [h.read()[0]["img"] for h in grp.halves()]          # (one pass a half: no variance yet)
    grp.run(pass_spp=P)
    a, b = grp.halves()
    sc = G.Scene(sd)
    acc = [G.Progressive(sc, B, path=path, slice=(0, 0)) for _ in range(2)]
    for i in range(N):
        first, end = i * B // N, (i + 1) * B // N
        s = G.Progressive(sc, B, path=path, slice=(first, end - first))
        assert s.run(pass_spp=P)["stop_reason"] == "budget"
        acc[i & 1].merge(s)
        s.close()
    for half, hand, before in zip((a, b), acc, early):
        planes = session_planes(half)
        assert all(np.array_equal(x, y) for x, y in zip(planes, session_planes(hand))) and len(planes) >= 2
        assert not np.array_equal(half.read()[0]["img"], before)          # the round marked them stale
        assert half.status()["passes"] == hand.status()["passes"] >= 2 and half.status()["spp"] == hand.status()["spp"]
        got, want = half.denoise(window_radius=4, patch_radius=2), hand.denoise(window_radius=4, patch_radius=2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        with pytest.raises(G.GdptError, match="half of a group"):
            half.add_pass(P)
        with pytest.raises(G.GdptError, match="half of a group"):
            half.merge(hand)
    assert a.status()["spp"] + b.status()["spp"] == grp.total.status()["spp"] == B
    # the halves feed the selection: the mean against a plain filter of each half, chosen per pixel
    (mA, vA, _), (mB, vB, _) = a.read(), b.read()
    kw = dict(window_radius=4, patch_radius=2)
    T = [grp.total.read()[0]["img"], grp.total.denoise(**kw)[0]]
    out, sel, mse, st = G.filter_select([mA["img"], a.denoise(**kw)[0]], [mB["img"], b.denoise(**kw)[0]], T, mA["img"], vA["img"], mB["img"], vB["img"])
    assert st.pixels_left_out == 0 and st.chosen[0] + st.chosen[1] == 40 * 24 and st.chosen[1] > 0
    assert np.array_equal(out, np.where((sel == 1)[..., None], T[1], T[0]))
    for s in acc:
        s.close()
    sc.close()
    grp.close()


def chain(G, sessions, sc, candidates, B, fspp, s):
    """The chain of include/gdpt.h composed from Python with the device entries: for every candidate and each of A, B and the total,
    read() of buffer 0, the optional variance_smooth_device, the candidate's device filter on the features of Scene.features with the
    window {B, 0}; then filter_select_device. Returns (out, sel, mse, stats, the candidates' stats on the total)."""
    h, w, _ = sessions[0].shape
    fm, fv = sc.features(fspp, window=(B, 0))
    d_feat, d_fvar = hip_rt.upload(G, fm), hip_rt.upload(G, fv)
    nbytes = 24 * w * h
    held, films, stats_t, halves = [d_feat, d_fvar], [[], [], []], [], []
    for k, ses in enumerate(sessions):
        means, vars_, _ = ses.read()
        d_img, d_var, d_sm = hip_rt.upload(G, means["img"]), hip_rt.upload(G, vars_["img"]), hip_rt.alloc(G, nbytes)
        held += [d_img, d_var, d_sm]
        if k < 2:
            halves += [d_img, d_var]
        for c in candidates:
            d_out = hip_rt.alloc(G, nbytes)
            held.append(d_out)
            f, st, kw = c["filter"], None, c.get("nlm", {})
            d_v = d_var
            if c.get("var_smooth") is not None:
                dm = dict(feat_ptr=d_feat, feat_var_ptr=d_fvar, num_channels=8, demod=c.get("demod") or G.nlm_demod()) if f == "demod" else {}
                G.variance_smooth_device(w, h, d_img, d_var, d_sm, radius=c["var_smooth"], **dm)
                d_v = d_sm
            if f == "mean":
                d_out = d_img
            elif f == "nlm":
                st = G.denoise_nlm_device(w, h, d_img, d_v, d_out, **kw)
            elif f == "guided":
                st = G.denoise_nlm_guided_device(w, h, d_img, d_v, d_feat, d_fvar, d_out, guide=c.get("guide"), **kw)
            elif f == "demod":
                st = G.denoise_nlm_demod_device(w, h, d_img, d_v, d_feat, d_fvar, 8, d_out, guide=c.get("guide"), demod=c.get("demod"), **kw)
            elif f == "regress":
                st = G.denoise_nlm_regress_device(w, h, d_img, d_v, d_feat, d_fvar, d_out, guide=c.get("guide"), regress=c.get("regress"), **kw)
            else:
                st = G.denoise_atrous_device(w, h, d_img, d_v, d_feat, d_fvar, 8, d_out, guide=c.get("guide"), demod=c.get("demod"), **c.get("atrous", {}))
            films[k].append(d_out)
            if k == 2:
                stats_t.append(st)
    d_o, d_s, d_m = hip_rt.alloc(G, nbytes), hip_rt.alloc(G, 4 * w * h), hip_rt.alloc(G, 8 * w * h)
    st = G.filter_select_device(w, h, films[0], films[1], films[2], *halves, d_o, d_s, d_m, radius=s)
    res = (hip_rt.to_host(G, d_o, (h, w, 3)), read_i32(G, d_s, (h, w)), hip_rt.to_host(G, d_m, (h, w)), st, stats_t, fm, fv)
    for p in held + [d_o, d_s, d_m]:
        hip_rt.free(G, p)
    return res


NLM_STATS = ("pixels_left_out", "sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out")


@pytest.mark.parametrize("path", [True, False], ids=["path", "gradpath"])
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["two", "three"])
def test_group_denoise_select(G, scene_tmp, devices, path):
    """cbox at 40 x 24, budget 32 in passes of 4: denoise_select is, bit for bit, the chain composed from Python with the device
    entries; n = 1 is the matching Progressive.denoise_* on the total; a half with one pass is refused by name."""
    from helpers import scene_variant
    B, P = 32, 4
    xml = scene_variant(scene_tmp, CBOX, width=40, height=24, integrator="path") if path else scene_variant(scene_tmp, CBOX, width=40, height=24)
    sd = G.parse_scene(xml)
    grp = G.ProgressiveGroup(sd, devices, B, path=path)
    small = dict(window_radius=4, patch_radius=2)
    cands = [dict(filter="mean"), dict(filter="atrous", guide=G.nlm_guide(), atrous=dict(levels=3)), dict(filter="nlm", var_smooth=2, nlm=dict(k=0.8, **small)),
             dict(filter="demod", nlm=small), dict(filter="guided", var_smooth=1, nlm=dict(k=1.0, **small)),
             dict(filter="regress", guide=G.nlm_guide(groups=[(0, 3, 1e-3)]), nlm=dict(k=4.0, **small))]
    grp.run(pass_spp=P, max_rounds=1)
    with pytest.raises(G.GdptError, match=r"half (A \(members 0\)|B \(members 1\)) holds 1 pass"):
        grp.denoise_select(cands[:2])
    grp.run(pass_spp=P)
    a, b = grp.halves()
    sc = G.Scene(sd)
    fspp, s = 4, 4
    want = chain(G, (a, b, grp.total), sc, cands, B, fspp, s)
    out, sel, mse, fm, fv, st, cst = grp.denoise_select(cands, radius=s, feature_spp=fspp, maps=True, features=True)
    assert np.array_equal(out, want[0]) and np.array_equal(sel, want[1]) and np.array_equal(mse, want[2])
    assert stats_bits(st, want[3], len(cands)) and st.pixels_left_out == 0 and sum(st.chosen[:len(cands)]) == 40 * 24
    assert np.array_equal(fm, want[5]) and np.array_equal(fv, want[6])
    for got, ref in zip(cst[1:], want[4][1:]):
        assert [getattr(got, k) for k in NLM_STATS] == [getattr(ref, k) for k in NLM_STATS]
    assert len(set(sel.ravel().tolist())) >= 2                                   # more than one candidate wins somewhere
    # the outputs left on the device, and without the maps
    d_o, d_s, d_m = hip_rt.alloc(G, out.nbytes), hip_rt.alloc(G, sel.nbytes), hip_rt.alloc(G, mse.nbytes)
    st2, _ = grp.denoise_select(cands, radius=s, feature_spp=fspp, out_ptrs=(d_o, d_s, d_m))
    assert np.array_equal(hip_rt.to_host(G, d_o, out.shape), out) and np.array_equal(read_i32(G, d_s, sel.shape), sel)
    assert np.array_equal(hip_rt.to_host(G, d_m, mse.shape), mse) and stats_bits(st2, st, len(cands))
    out3, st3, _ = grp.denoise_select(cands, radius=s, feature_spp=fspp)
    assert np.array_equal(out3, out) and stats_bits(st3, st, len(cands))
    for p in (d_o, d_s, d_m):
        hip_rt.free(G, p)
    # n = 1: the matching session call on the total
    t = grp.total
    for cand, ref in ((cands[0], t.read()[0]["img"]), (cands[1], t.denoise_atrous(fspp, guide=G.nlm_guide(), levels=3)[0]),
                      (cands[2], t.denoise_smoothed("plain", radius=2, k=0.8, **small)[0]), (cands[3], t.denoise_demod(fspp, **small)[0]),
                      (cands[5], t.denoise_regress(fspp, guide=G.nlm_guide(groups=[(0, 3, 1e-3)]), k=4.0, **small)[0])):
        one, st1, _ = grp.denoise_select([cand], feature_spp=fspp)
        assert np.array_equal(one, ref) and st1.chosen[0] == 40 * 24, cand["filter"]
    # refusals that name their field
    for bad, match in (([], "n must be in"), ([dict(filter=9)], "filter must be one of"), ([dict(filter="atrous", var_smooth=2)], "var_smooth_radius"),
                       ([dict(filter="nlm", var_smooth=5)], "var_smooth_radius"), ([dict(filter="mean", nlm=small)], "takes no parameter block"),
                       ([dict(filter="nlm", guide=G.nlm_guide())], "guide must be null"), ([dict(filter="guided", regress=G.nlm_regress())], "regress must be null")):
        with pytest.raises(G.GdptError, match=match):
            grp.denoise_select(bad)
    with pytest.raises(G.GdptError, match="radius"):
        grp.denoise_select(cands[:1], radius=9)
    sc.close()
    grp.close()


def test_cli_select(G, scene_tmp, tmp_path):
    """lajolla --select: the denoised file, the map and the estimate are what ProgressiveGroup.denoise_select gives for the names'
    configurations; without --select, -o and --denoised are byte for byte what the parent build wrote (the command and the hashes of
    tests/test_gpu_nlm_regress.py, which the parent commit passes)."""
    from helpers import ROOT, scene_variant
    from test_gpu_nlm_regress import PARENT_SHA256
    from test_gpu_progressive import read_pfm
    exe = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")
    xml = scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path")
    out, den, sden, smap, smse = (tmp_path / n for n in ("o.pfm", "d.pfm", "s.pfm", "m.pfm", "e.pfm"))
    base = [exe, "--spp", "16", "--pass-spp", "4"]
    r0 = subprocess.run([*base, "--denoised", str(den), "--nlm-window", "4", "--nlm-patch", "2", "--nlm-guide", "albedo,normal", "-o", str(out), xml],
                        capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stderr
    sha = tuple(hashlib.sha256(open(p, "rb").read()).hexdigest() for p in (out, den))
    print("lajolla without --select: sha256", sha)
    assert sha == PARENT_SHA256
    assert "[gdpt] selected:" not in r0.stdout
    r1 = subprocess.run([*base, "--sample-devices", "0,0", "--denoised", str(sden), "--select", "mean,atrous,nlm,atrous-demod", "--nlm-var-smooth", "2",
                         "--select-radius", "3", "--select-map", str(smap), "--select-mse", str(smse), "--feature-spp", "4", "--nlm-albedo-floor", "0.05",
                         "-o", str(out), xml], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    lines = [l for l in r1.stdout.splitlines() if l.startswith("[gdpt] selected:")]
    assert len(lines) == 1 and "radius 3" in lines[0] and all(f" {n} " in lines[0] for n in ("mean", "atrous", "nlm", "atrous-demod")), r1.stdout
    assert "[gdpt] denoised:" not in r1.stdout
    grp = G.ProgressiveGroup(G.parse_scene(xml), (0, 0), 16, path=True)
    grp.run(pass_spp=4)
    block = G.nlm_demod(floor=0.05)
    cands = [dict(filter="mean"), dict(filter="atrous", guide=G.nlm_guide()), dict(filter="nlm", var_smooth=2),
             dict(filter="atrous", guide=G.nlm_guide(groups=[(3, 3, 1e-3)]), demod=block)]
    want, sel, mse, st, _ = grp.denoise_select(cands, radius=3, feature_spp=4, maps=True)
    assert np.array_equal(read_pfm(out, 24, 24), grp.total.read()[0]["img"].astype(np.float32))
    assert np.array_equal(read_pfm(sden, 24, 24), want.astype(np.float32))
    assert np.array_equal(read_pfm(smap, 24, 24)[..., 0], sel.astype(np.float32)) and np.array_equal(read_pfm(smse, 24, 24)[..., 1], mse.astype(np.float32))
    share = 100.0 * st.chosen[1] / (24 * 24 - st.pixels_left_out)
    assert f" atrous {share:.6g} % (error " in lines[0], (share, lines[0])
    grp.close()
