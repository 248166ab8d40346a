"""The multi-scale non-local-means filters on the GPU (include/gdpt.h: gdpt_nlm_pyramid_down*, gdpt_nlm_pyramid_up*,
gdpt_denoise_nlm_multiscale*, gdpt_progressive_denoise_multiscale): the two operators alone against the numpy restatement
(tests/nlm_pyramid_ref.py), the multi-scale call against the restatement and, bit for bit, against the composed device calls, the exact
properties of the definition, the same bits from two calls, a second stream, the host and device entries and the enqueue-only form, the
sessions (Path, GradPath, a group's total) against the composed calls, and the CLI."""
import subprocess

import numpy as np
import pytest

import hip_rt
import nlm_pyramid_ref as P
from helpers import scene_variant
from test_gpu_nlm import CBOX, SUMS, masked_rel_l2
from test_gpu_nlm_demod import room_desc
from test_gpu_progressive import read_pfm
from test_gpu_var_smooth import EXE, filter_bits
from test_nlm_pyramid_ref import level

pytestmark = pytest.mark.gpu

# The two operators against the restatement: the worst masked relative L2 of any output array over every case of the first test. Both
# sides add the same terms in the same order, divide in single correctly rounded operations and keep the products and sums of the
# interpolation apart (the kernel is compiled without contraction there), so the figure is expected to be 0. The bound is 100 x the
# measured value, never looser than 1e-9, as in tests/test_gpu_nlm.py. Measured on an MI355X over the 80 cases: 0.0, every array the
# same bits, so the bound is 0 and the comparison is for equality.
PYRAMID_OPS_MEASURED = 0.0
PYRAMID_OPS_BOUND = min(100 * PYRAMID_OPS_MEASURED, 1e-9) if PYRAMID_OPS_MEASURED is not None else None
# The multi-scale call against the restatement: the worst masked relative L2 of out and of var_out over every case of the second test.
# The levels' filters differ from their restatements as tests/test_gpu_nlm*.py measure (FMA contraction, the order of the patch sums,
# the last place of exp), and a coarser level's difference enters the finer ones through the correction.
# Measured on an MI355X over the 72 cases: 2.269e-16 (plain), 2.128e-16 (guided), 1.404e-16 (demodulated, with a coverage plane and a guide).
MULTISCALE_MEASURED = 2.3e-16
MULTISCALE_BOUND = min(100 * MULTISCALE_MEASURED, 1e-9) if MULTISCALE_MEASURED is not None else None

# W x H: 17 x 17 is one pixel beyond a 16 x 16 tile each way (and its coarse level one beyond an 8 x 8 half tile); odd extents leave cells
# of one or two pixels; 530 x 500 has 34 x 32 = 1088 fine tiles, beyond the cap of 1024 blocks
OP_FILMS = [(1, 1), (2, 2), (3, 3), (1, 7), (7, 1), (17, 17), (33, 9), (40, 19), (35, 33), (530, 500)]
CALL_FILMS = [(17, 17), (33, 9), (40, 19)]
RADII = [(2, 1), (10, 3)]
KINDS = ["plain", "guided", "demod", "demod-cov-guide"]      # "demod" alone: no coverage plane, no guide


def blocks(G, kind):
    """(the restatement's kind_args, the keywords of the library's entries) of a kind of KINDS"""
    if kind == "plain":
        return P.kind_args("plain"), dict(kind="plain")
    if kind == "guided":
        return P.kind_args("guided"), dict(kind="guided")                     # NULL guide: the default guide
    if kind == "demod":
        return P.kind_args("demod", coverage_channel=-1), dict(kind="demod", demod=G.nlm_demod(coverage_channel=-1))
    return P.kind_args("demod", groups=[(3, 3, 1e-3)], coverage_channel=7), dict(kind="demod", guide=G.nlm_guide(groups=[(3, 3, 1e-3)]))


def planes_of(lv):
    return {} if lv[2] is None else dict(feat=lv[2], feat_var=lv[3])


def op_level(ka, w, h, seed, dirty):
    """level() of tests/test_nlm_pyramid_ref.py; a planted film beyond the block cap also gets values in tile 1024 (the second trip of
    block 0) and on the border of the tile before it."""
    lv = level(ka, w, h, seed, dirty)
    tiles_x = (w + 15) // 16
    if dirty and tiles_x * ((h + 15) // 16) > 1024:
        y0, x0 = 16 * (1024 // tiles_x), 16 * (1024 % tiles_x)
        lv[1][y0 + 1, x0, 1], lv[0][y0 + 3, x0 - 1, 0] = np.nan, np.inf
        if lv[2] is not None:
            lv[2][1, y0, x0 + 15], lv[3][7, y0 + 15, x0 + 2] = -np.inf, -1e-3
    return lv


def fig(got, want):
    return 0.0 if want is None and got is None else masked_rel_l2(got, want)


def test_down_and_up_alone_against_the_restatement(G):
    worst, cases, empty = 0.0, 0, 0
    for dirty in (False, True):
        for (w, h) in OP_FILMS:
            for kind in KINDS:
                ka, kw = blocks(G, kind)
                key = (w, h, kind, dirty)
                lv = op_level(ka, w, h, 10 * w + h, dirty)
                ok = P.valid_mask(ka, *lv)
                want = P.down(ka, *lv)
                got = G.nlm_pyramid_down(lv[0], lv[1], **planes_of(lv), **kw)
                st = got[4]
                assert (st.pixels_left_out, st.cells_empty) == ((~ok).sum(), (want[4] == 0).sum()) and st.op_ms > 0, key
                assert (st.coarse_height, st.coarse_width) == want[0].shape[:2] == got[0].shape[:2], key
                assert (not dirty) or st.pixels_left_out >= 1, key
                worst = max([worst] + [fig(g, b) for g, b in zip(got[:4], want[:4])])
                rng = np.random.default_rng(w + 100 * h)
                F = np.where(ok[:, :, None], lv[0] + 0.01 * rng.standard_normal(lv[0].shape), lv[0])
                coarse = np.where((want[4] > 0)[:, :, None], want[0] + 0.01 * rng.standard_normal(want[0].shape), np.nan)
                want_up = P.up(ka, *lv, F, coarse)
                out, st = G.nlm_pyramid_up(lv[0], lv[1], F, coarse, **planes_of(lv), **kw)
                assert np.array_equal(out[~ok], lv[0][~ok], equal_nan=True) and np.isfinite(out[ok]).all(), key      # the kept pixels are exactly ~ok
                assert (st.pixels_left_out, st.cells_empty) == ((~ok).sum(), 0) and st.op_ms > 0, key
                assert (st.coarse_height, st.coarse_width) == want[0].shape[:2], key
                worst = max(worst, fig(out, want_up))
                cases, empty = cases + 1, empty + int((want[4] == 0).sum())
    assert cases == 80 and empty >= 24
    print(f"pyramid down and up against the restatement over {cases} cases: worst figure {worst:.3e} (bound {PYRAMID_OPS_BOUND})")
    assert PYRAMID_OPS_BOUND is not None, f"PYRAMID_OPS_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst <= PYRAMID_OPS_BOUND


class Device:
    """A level's host arrays on the device, and scratch of its size; everything is freed by close()."""

    def __init__(self, G, lv):
        self.G, self.lv, self.ptrs = G, lv, []
        self.h, self.w = lv[0].shape[:2]
        self.img, self.var = self.up(lv[0]), self.up(lv[1])
        self.feat, self.fvar = (self.up(lv[2]), self.up(lv[3])) if lv[2] is not None else (None, None)
        self.nc = 0 if lv[2] is None else lv[2].shape[0]

    def up(self, a):
        self.ptrs.append(hip_rt.upload(self.G, a))
        return self.ptrs[-1]

    def alloc(self, doubles):
        self.ptrs.append(hip_rt.alloc(self.G, 8 * max(doubles, 1)))
        return self.ptrs[-1]

    def planes(self):
        return {} if self.feat is None else dict(feat_ptr=self.feat, feat_var_ptr=self.fvar, num_channels=self.nc)

    def close(self):
        for p in self.ptrs:
            hip_rt.free(self.G, p)


def device_filter(G, w, h, img, var, feat, fvar, nc, kw, out, var_out, nlm, stream=None):
    """The kind's existing device filter on one level."""
    if kw["kind"] == "plain":
        return G.denoise_nlm_device(w, h, img, var, out, var_out, stream=stream, **nlm)
    if kw["kind"] == "guided":
        return G.denoise_nlm_guided_device(w, h, img, var, feat, fvar, out, var_out, guide=kw.get("guide"), stream=stream, **nlm)
    return G.denoise_nlm_demod_device(w, h, img, var, feat, fvar, nc, out, var_out, guide=kw.get("guide"), demod=kw.get("demod"), stream=stream, **nlm)


def composed(G, dev, kw, levels, nlm, stream=None):
    """The multi-scale call spelt out: down, the kind's filter on every level, up. Returns (out, var_out, [GdptNlmStats], extents)."""
    ext = P.extents(dev.h, dev.w, levels)
    lv = [(dev.img, dev.var, dev.feat, dev.fvar)]
    for (hc, wc) in ext[1:]:
        nxt = (dev.alloc(3 * hc * wc), dev.alloc(3 * hc * wc)) + ((dev.alloc(dev.nc * hc * wc), dev.alloc(dev.nc * hc * wc)) if dev.nc else (None, None))
        hf, wf = ext[len(lv) - 1]
        extra = dict(feat_ptr=lv[-1][2], feat_var_ptr=lv[-1][3], feat_out_ptr=nxt[2], feat_var_out_ptr=nxt[3], num_channels=dev.nc) if dev.nc else {}
        G.nlm_pyramid_down_device(wf, hf, lv[-1][0], lv[-1][1], nxt[0], nxt[1], stream=stream, stats=False, **extra, **kw)
        lv.append(nxt)
    F, stats = [], []
    d_vout = dev.alloc(3 * dev.h * dev.w)
    for l, (hl, wl) in enumerate(ext):
        F.append(dev.alloc(3 * hl * wl))
        stats.append(device_filter(G, wl, hl, *lv[l], dev.nc, kw, F[l], d_vout if l == 0 else None, nlm, stream))
    out = F[-1]
    for l in range(len(ext) - 2, -1, -1):
        hl, wl = ext[l]
        nxt = dev.alloc(3 * hl * wl)
        extra = dict(feat_ptr=lv[l][2], feat_var_ptr=lv[l][3], num_channels=dev.nc) if dev.nc else {}
        G.nlm_pyramid_up_device(wl, hl, lv[l][0], lv[l][1], F[l], out, nxt, stream=stream, stats=False, **extra, **kw)
        out = nxt
    shape = (dev.h, dev.w, 3)
    return hip_rt.to_host(G, out, shape), hip_rt.to_host(G, d_vout, shape), stats, ext


def restated_at_every_level_count(ka, lv, nlm):
    """[the restatement's (out, var_out, left_out, extents) at levels = 1 .. 4]; a level's filter does not depend on the count, so each runs once."""
    ext = P.extents(lv[0].shape[0], lv[0].shape[1], P.MAX_LEVELS)
    pyr = [lv]
    for _ in ext[1:]:
        pyr.append(P.down(ka, *pyr[-1])[:4])
    res = [P.filter_level(ka, *p, **nlm) for p in pyr]
    outs = []
    for levels in range(1, P.MAX_LEVELS + 1):
        made = min(levels, len(ext))
        out = res[made - 1]["out"]
        for l in range(made - 2, -1, -1):
            out = P.up(ka, *pyr[l], res[l]["out"], out)
        outs.append((out, res[0]["var_out"], res[0]["left_out"], ext[:made]))
    return outs


def stats_bits(a, b):
    return [getattr(a, k) for k in SUMS] == [getattr(b, k) for k in SUMS] and a.pixels_left_out == b.pixels_left_out


@pytest.mark.parametrize("kind", ["plain", "guided", "demod-cov-guide"])
def test_the_multiscale_call_against_the_restatement_and_the_composed_calls(G, kind):
    ka, kw = blocks(G, kind)
    worst, cases = 0.0, 0
    for (w, h) in CALL_FILMS:
        lv = level(ka, w, h, 10 * w + h, True)
        ok = P.valid_mask(ka, *lv)
        dev = Device(G, lv)
        d_out, d_vout = dev.alloc(3 * w * h), dev.alloc(3 * w * h)
        for (r, f) in RADII:
            nlm = dict(window_radius=r, patch_radius=f)
            want = restated_at_every_level_count(ka, lv, dict(r=r, f=f))
            single = device_filter(G, w, h, dev.img, dev.var, dev.feat, dev.fvar, dev.nc, kw, d_out, d_vout, nlm)
            single = (hip_rt.to_host(G, d_out, lv[0].shape), hip_rt.to_host(G, d_vout, lv[0].shape), single)
            for levels in range(1, P.MAX_LEVELS + 1):
                key = (w, h, r, f, levels)
                st = G.denoise_nlm_multiscale_device(w, h, dev.img, dev.var, d_out, d_vout, levels=levels, **dev.planes(), **kw, **nlm)
                out, vout = hip_rt.to_host(G, d_out, lv[0].shape), hip_rt.to_host(G, d_vout, lv[0].shape)
                w_out, w_vout, w_left, w_ext = want[levels - 1]
                # the exact parts: the levels made, the kept pixels, the finest level's variance and stats
                assert st.levels == len(w_ext) and [(st.height[l], st.width[l]) for l in range(st.levels)] == w_ext and st.total_ms > 0, key
                assert st.level[0].pixels_left_out == w_left == (~ok).sum() > 0, key
                assert np.array_equal(out[~ok], lv[0][~ok], equal_nan=True) and np.isfinite(out[ok]).all(), key
                assert np.array_equal(vout, single[1], equal_nan=True) and stats_bits(st.level[0], single[2]), key
                assert all(st.level[l].filter_ms > 0 and st.level[l].window_radius == r for l in range(st.levels)), key
                if levels == 1:                                     # the existing entry, bit for bit
                    assert np.array_equal(out, single[0], equal_nan=True), key
                else:
                    assert not np.array_equal(out, single[0], equal_nan=True), key
                # the composition of the two operators and the existing device filters, bit for bit
                c_out, c_vout, c_stats, c_ext = composed(G, dev, kw, levels, nlm)
                assert np.array_equal(out, c_out, equal_nan=True) and np.array_equal(vout, c_vout, equal_nan=True) and c_ext == w_ext, key
                assert all(stats_bits(st.level[l], c_stats[l]) for l in range(st.levels)), key
                worst, cases = max(worst, masked_rel_l2(out, w_out), masked_rel_l2(vout, w_vout)), cases + 1
        dev.close()
    assert cases == 24
    print(f"multi-scale nlm ({kind}) against the restatement over {cases} cases: worst figure {worst:.3e} (bound {MULTISCALE_BOUND})")
    assert MULTISCALE_BOUND is not None, f"MULTISCALE_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < MULTISCALE_BOUND


@pytest.mark.parametrize("kind", KINDS)
def test_a_dyadic_constant_film_comes_back_unchanged(G, kind):
    ka, kw = blocks(G, kind)
    for (w, h) in ((40, 19), (17, 17), (1, 1)):
        _, _, feat, fvar = level(ka, w, h, 1, False)
        if feat is not None:                # dyadic constant planes without variance: every weight is 1, the albedo divides exactly
            feat[:], fvar[:], feat[7] = 0.5, 0.0, 1.0
        for value, variance in ((0.375, 2.0 ** -10), (-3.0, 0.0)):
            img, var = np.full((h, w, 3), value), np.full((h, w, 3), variance)
            for levels in range(1, P.MAX_LEVELS + 1):
                out, vout, st = G.denoise_nlm_multiscale(img, var, **planes_of((img, var, feat, fvar)), levels=levels, window_radius=3, patch_radius=1, **kw)
                assert np.array_equal(out, img) and st.levels == len(P.extents(h, w, levels)) and st.level[0].pixels_left_out == 0, (w, h, levels)


@pytest.mark.parametrize("kind", ["plain", "demod-cov-guide"])
def test_same_bits_twice_on_a_second_stream_from_the_host_and_enqueue_only(G, kind):
    ka, kw = blocks(G, kind)
    w, h, levels = 40, 19, 3
    nlm = dict(window_radius=3, patch_radius=1)
    lv = level(ka, w, h, 5, True)
    dev = Device(G, lv)
    d_out, d_vout = dev.alloc(3 * w * h), dev.alloc(3 * w * h)
    side = hip_rt.stream(G)
    zero = lambda: [hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(lv[0].nbytes))) for p in (d_out, d_vout)]      # noqa: E731
    first = G.denoise_nlm_multiscale(lv[0], lv[1], **planes_of(lv), levels=levels, **kw, **nlm)              # the host entry
    assert first[2].levels == 3 and first[2].level[0].pixels_left_out > 4 and first[2].level[2].sum_var_out > 0
    again = G.denoise_nlm_multiscale(lv[0], lv[1], **planes_of(lv), levels=levels, **kw, **nlm)
    assert filter_bits((first[0], first[1], first[2].level[0]), (again[0], again[1], again[2].level[0]))
    for stream in (None, None, side):
        zero()
        st = G.denoise_nlm_multiscale_device(w, h, dev.img, dev.var, d_out, d_vout, levels=levels, stream=stream, **dev.planes(), **kw, **nlm)
        got = (hip_rt.to_host(G, d_out, lv[0].shape), hip_rt.to_host(G, d_vout, lv[0].shape), st.level[0])
        assert filter_bits(got, (first[0], first[1], first[2].level[0])), stream
        assert all(stats_bits(st.level[l], first[2].level[l]) for l in range(3)), stream
    # the composition on the second stream
    c_out, c_vout, _, _ = composed(G, dev, kw, levels, nlm, stream=side)
    assert np.array_equal(c_out, first[0], equal_nan=True) and np.array_equal(c_vout, first[1], equal_nan=True)
    # stats == NULL: enqueue-only, the same planes; var_out is optional
    zero()
    assert G.denoise_nlm_multiscale_device(w, h, dev.img, dev.var, d_out, d_vout, levels=levels, stats=False, **dev.planes(), **kw, **nlm) is None
    assert np.array_equal(hip_rt.to_host(G, d_out, lv[0].shape), first[0], equal_nan=True)
    assert np.array_equal(hip_rt.to_host(G, d_vout, lv[0].shape), first[1], equal_nan=True)
    zero()
    st = G.denoise_nlm_multiscale_device(w, h, dev.img, dev.var, d_out, levels=levels, stream=side, **dev.planes(), **kw, **nlm)
    assert np.array_equal(hip_rt.to_host(G, d_out, lv[0].shape), first[0], equal_nan=True) and st.levels == 3
    assert not hip_rt.to_host(G, d_vout, lv[0].shape).any()
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    dev.close()


def session_body(G, ses, scene, budget):
    """`ses` holds two passes: denoise_multiscale() is, bit for bit, read(), Scene.features with the window {budget, 0} where the kind
    needs it, variance_smooth_device where a radius is given, and denoise_nlm_multiscale_device; in host and in device memory."""
    h, w, _ = ses.shape
    assert ses.status()["passes"] == 2
    fspp = 4
    nlm = dict(window_radius=4, patch_radius=2, k=0.8)
    means, vars_, _ = ses.read()
    img, var = means["img"], vars_["img"]
    fm, fv = scene.features(fspp, window=(budget, 0))
    d_img, d_var, d_feat, d_fvar = (hip_rt.upload(G, a) for a in (img, var, fm, fv))
    d_sm, d_out, d_vout = (hip_rt.alloc(G, img.nbytes) for _ in range(3))
    d_fm, d_fv = hip_rt.alloc(G, fm.nbytes), hip_rt.alloc(G, fm.nbytes)
    guide = G.nlm_guide(groups=[(3, 3, 1e-3)], k_f=0.7)
    block = G.nlm_demod(floor=0.05)
    planes = dict(feat_ptr=d_feat, feat_var_ptr=d_fvar, num_channels=8)
    for kind, levels, radius, opts in (("plain", 2, None, {}), ("plain", 3, 2, {}), ("plain", 1, None, {}), ("guided", 2, None, {}),
                                       ("guided", 2, 1, dict(guide=guide)), ("demod", 2, None, {}), ("demod", 3, 2, dict(guide=guide, demod=block))):
        key = (kind, levels, radius)
        # the chain
        d_v = d_var
        if radius is not None:
            extra = dict(demod=opts.get("demod", G.nlm_demod()), **planes) if kind == "demod" else {}
            G.variance_smooth_device(w, h, d_img, d_var, d_sm, radius=radius, **extra)
            d_v = d_sm
        st2 = G.denoise_nlm_multiscale_device(w, h, d_img, d_v, d_out, d_vout, kind=kind, levels=levels, **({} if kind == "plain" else planes), **opts, **nlm)
        want = (hip_rt.to_host(G, d_out, img.shape), hip_rt.to_host(G, d_vout, img.shape), st2.level[0])
        # the session, into host memory
        if kind == "plain":
            out, var_out, st = ses.denoise_multiscale(kind, levels=levels, radius=radius, **nlm)
        else:
            out, var_out, gfm, gfv, st = ses.denoise_multiscale(kind, levels=levels, radius=radius, feature_spp=fspp, features=True, **opts, **nlm)
            assert np.array_equal(gfm, fm) and np.array_equal(gfv, fv), key
        assert filter_bits((out, var_out, st.level[0]), want), key
        assert st.levels == st2.levels == levels and all(stats_bits(st.level[l], st2.level[l]) for l in range(levels)), key
        assert [(st.height[l], st.width[l]) for l in range(levels)] == P.extents(h, w, levels) and np.isfinite(out).all(), key
        single = ses.denoise(**nlm) if kind == "plain" else ses.denoise_guided(fspp, guide=opts.get("guide"), **nlm) if kind == "guided" else \
            ses.denoise_demod(fspp, guide=opts.get("guide"), demod=opts.get("demod"), **nlm)
        if levels == 1:
            assert filter_bits(single, (out, var_out, st.level[0])), key
        else:
            assert not np.array_equal(single[0], out), key                      # the coarser levels are at work
        # ... and into device memory
        for p in (d_out, d_vout):
            hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(img.nbytes)))
        extra = {} if kind == "plain" else dict(feature_spp=fspp, features_ptrs=(d_fm, d_fv), **opts)
        st3 = ses.denoise_multiscale(kind, levels=levels, radius=radius, out_ptr=d_out, var_out_ptr=d_vout, **extra, **nlm)
        assert filter_bits((hip_rt.to_host(G, d_out, img.shape), hip_rt.to_host(G, d_vout, img.shape), st3.level[0]), want), key
        if kind != "plain":
            assert np.array_equal(hip_rt.to_host(G, d_fm, fm.shape), fm) and np.array_equal(hip_rt.to_host(G, d_fv, fm.shape), fv), key
    for bad in (1, budget + 1):
        with pytest.raises(G.GdptError, match="feature_spp"):
            ses.denoise_multiscale("guided", feature_spp=bad)
    with pytest.raises(G.GdptError, match="levels"):
        ses.denoise_multiscale("plain", levels=5)
    with pytest.raises(G.GdptError, match="guide must be null"):
        ses.denoise_multiscale("plain", guide=guide)
    with pytest.raises(G.GdptError, match="kind"):
        ses.denoise_multiscale("median")
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
            ses.denoise_multiscale(kind, feature_spp=4)
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


def test_cli_nlm_levels(G, scene_tmp, tmp_path):
    xml = scene_variant(scene_tmp, CBOX, width=24, height=24, integrator="path")
    out, out2, den, den1, den2, dden = (tmp_path / n for n in ("o.pfm", "o2.pfm", "d.pfm", "d1.pfm", "d2.pfm", "dd.pfm"))
    base = [EXE, "--spp", "8", "--pass-spp", "4"]
    nlm = ["--nlm-window", "4", "--nlm-patch", "2"]
    runs = [[*base, "--denoised", str(den), *nlm, "-o", str(out), xml], [*base, "--denoised", str(den1), *nlm, "--nlm-levels", "1", "-o", str(out2), xml],
            [*base, "--denoised", str(den2), *nlm, "--nlm-levels", "2", "-o", str(out2), xml],
            [*base, "--denoised", str(dden), *nlm, "--nlm-levels", "3", "--nlm-var-smooth", "1", "--nlm-demodulate", "--nlm-guide", "normal", "--feature-spp", "4",
             "-o", str(out2), xml]]
    done = []
    for cmd in runs:
        done.append(subprocess.run(cmd, capture_output=True, text=True, timeout=300))
        assert done[-1].returncode == 0, done[-1].stderr
        if len(done) > 1:
            assert open(out, "rb").read() == open(out2, "rb").read()            # -o is what it is without the flag
    data = lambda p: open(p, "rb").read()      # noqa: E731
    assert data(den1) == data(den)                                              # one level: the single-scale filter
    assert data(den2) != data(den) and data(dden) != data(den) and data(dden) != data(den2)
    lines = [[l for l in r.stdout.splitlines() if l.startswith("[gdpt] denoised:")] for r in done]
    assert all(len(l) == 1 for l in lines)
    assert " levels in " not in lines[0][0] and ", 1 levels in " in lines[1][0] and ", 2 levels in " in lines[2][0] and ", 3 levels in " in lines[3][0]
    assert "variance smoothed over radius 1" in lines[3][0]
    sc = G.Scene(G.parse_scene(xml))
    ses = G.Progressive(sc, 8, path=True)
    ses.run(pass_spp=4)
    want = ses.denoise_multiscale("plain", levels=2, window_radius=4, patch_radius=2)[0]
    assert np.array_equal(read_pfm(den2, 24, 24), want.astype(np.float32))
    want = ses.denoise_multiscale("demod", levels=3, radius=1, feature_spp=4, guide=G.nlm_guide(groups=[(3, 3, 1e-3)]), window_radius=4, patch_radius=2, k=1.0)[0]
    assert np.array_equal(read_pfm(dden, 24, 24), want.astype(np.float32))
    ses.close()
    sc.close()
