"""The image-space kernels on the smallest films past their block caps. Every kernel that runs after a render strides over its
tiles or pixels with at most 1024 blocks of 256 threads (4096 for the variance read-out) and reduces its per-block partials with
256 threads, so up to 512 x 512 pixels no thread takes a second trip of either loop. Here: WIDE = 1025 x 345 and TALL = 33 x 8201
(513 x 171 for the Poisson CG), on which some block takes a second trip of the work loop and the reduction a second trip over the
partials; every test asserts that first, through gdpt_debug_image_grid (include/gdpt_debug.h), so that a raised cap fails the
test in place of quietly uncovering the loops. Each kernel is held to the assertions and bounds its own test module states for small
films: inputs, comparisons and bounds are imported from there."""
import functools

import numpy as np
import pytest

import hip_rt
import nlm_ref as N
import progressive_merge_ref as M
import progressive_ref as P
import recon_l1_ref as R
import recon_weighted_ref as RW
from helpers import rel_l2, scene_variant
from test_gpu_nlm import NLM_BOUND, as_dict, figure, planted_film
from test_gpu_progressive import BUFS, M2_BOUND, render_window, session_planes
from test_gpu_progressive_merge import check_against, state_of
from test_gpu_recon_l1 import ALPHA, TIGHT
from test_gpu_recon_spread import SPREAD_BOUND, compare, synthetic
from test_gpu_poisson_and_pipeline import weights
from test_nlm_ref import noisy_film
from test_poisson_oracle import lcg_fields

pytestmark = pytest.mark.gpu

WIDE = (1025, 345)      # 353 625 px; 33 x 44 = 1452 tiles of 32 x 8, 65 x 22 = 1430 of 16 x 16: ragged by one pixel both ways, both sizes
TALL = (33, 8201)       # 270 633 px; 2 x 1026 = 2052 tiles of 32 x 8 (every second one a single column), 3 x 513 = 1539 of 16 x 16
CG_FILM = (513, 171)    # 3 W H = 263 169: one block-stride past 1024 x 256 elements
FILMS = [WIDE, TALL]
REDUCTION = 256         # threads of finish_kernel / reduce_partials: more partials than this, and the reduction takes a second trip


def past_both_thresholds(G, kernel, w, h):
    """Asserts that on a w x h film some block of `kernel` takes a second trip of its work loop and the reduction of the block
    partials a second trip over them; returns (blocks, units)."""
    blocks, units = G.debug_knobs.image_grid(kernel, w, h)
    assert units > blocks, f"{kernel} at {w}x{h}: {units} units on {blocks} blocks: no block takes a second trip"
    assert blocks > REDUCTION, f"{kernel} at {w}x{h}: {blocks} partials: the reduction takes one trip"
    return blocks, units


def second_trip_spots(G, w, h):
    """((x, y) inside, [(x, y) of two pixels in its halo]): a pixel which spread_kernel reaches on a second trip (pixel group >=
    blocks) and whose 32 x 8 tile (box_kernel) and 16 x 16 tile (the NLM kernels) both have an index >= the blocks launched, and two
    pixels next to that tile, above it and right of it, in tiles of a second trip as well."""
    x0, y0 = (96 if w >= 160 else 0), (h // 16 - 1) * 16          # a corner of both tile grids
    inside, halo = (x0 + 5, y0 + 3), [(x0 + 5, y0 - 1), (x0 + 32, y0 + 4)]
    for x, y in [inside] + halo:
        assert 0 <= x < w and 0 <= y < h
        assert (y * w + x) // 256 >= G.debug_knobs.image_grid("spread", w, h)[0]
        for kernel, tw, th in (("box", 32, 8), ("nlm", 16, 16), ("recon_tiles", 32, 8)):
            assert (y // th) * -(-w // tw) + x // tw >= G.debug_knobs.image_grid(kernel, w, h)[0], (kernel, x, y)
    assert halo[0][1] // 16 != inside[1] // 16 and halo[1][0] // 32 != inside[0] // 32      # other tiles, in both grids
    return inside, halo


# ---- recon_l1 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", FILMS)
def test_recon_l1(G, w, h):
    """K = 2 rounds against the restatement's direct solves: the assertions of test_gpu_recon_l1.test_gpu_equals_the_restatement; the
    call twice for the same bits and stats."""
    past_both_thresholds(G, "recon_tiles", w, h)
    past_both_thresholds(G, "recon_pixels", w, h)
    K = 2
    _, u, gx, gy = R.synthetic(w, h, seed=1)
    ref, e, _ = R.irls(u, gx, gy, ALPHA, K, TIGHT["eps_init"], TIGHT["eps_decay"], TIGHT["eps_floor"])
    out, st = G.reconstruct(w, h, u, gx, gy, ALPHA, irls_iters=K, **TIGHT)
    err = rel_l2(out, ref)
    print(f"l1 {w}x{h}: rel L2 {err:.3e}, CG iterations {st.cg_iters_total} (last round {st.cg_iters_last}), residual {st.rel_residual_last:.2e}, "
          f"energy {st.energy_first:.6f} -> {st.energy_last:.6f} (restatement {e[0]:.6f} -> {e[-1]:.6f}; relative differences "
          f"{abs(st.energy_first - e[0]) / e[0]:.2e}, {abs(st.energy_last - e[-1]) / e[-1]:.2e})")
    assert err < 1e-7
    assert st.norm == G.RECON_L1 and st.irls_rounds == K + 1
    assert st.energy_last <= st.energy_first
    assert abs(st.energy_first - e[0]) <= 1e-8 * e[0] and abs(st.energy_last - e[-1]) <= 1e-8 * e[-1]
    assert st.rel_residual_last <= TIGHT["cg_tol"]
    assert st.cg_iters_total >= st.cg_iters_last > 0 and st.solve_ms > 0
    again, sb = G.reconstruct(w, h, u, gx, gy, ALPHA, irls_iters=K, **TIGHT)
    assert np.array_equal(again, out)
    assert (st.cg_iters_total, st.energy_first, st.energy_last, st.rel_residual_last) == (sb.cg_iters_total, sb.energy_first, sb.energy_last, sb.rel_residual_last)


# ---- recon_weighted -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def weighted_case(w, h):
    """The heteroscedastic input with recon_weighted_ref.spoil's rows planted at the film's origin and once more in a tile of the
    second trip, and the restatement's confidences and iterates 0, 1 on it: computed once, shared, read only."""
    _, *planes = RW.heteroscedastic(w, h, 1)
    planes = list(RW.spoil(*planes))
    x0, y0 = (96 if w >= 160 else 16), (h // 16 - 1) * 16
    for a, b in zip(planes, RW.spoil(*[p[y0:, x0:] for p in planes])):
        a[y0:, x0:] = b
    _, energies, iterates, conf = RW.weighted(*planes, ALPHA, 1, 0.05, TIGHT["eps_init"], TIGHT["eps_decay"], TIGHT["eps_floor"])
    return planes, energies, iterates, conf, (x0, y0)


@pytest.mark.parametrize("norm", ["wl2", "wl1"])
@pytest.mark.parametrize("w,h", FILMS)
def test_recon_weighted(G, w, h, norm):
    """Weighted L2 and weighted L1 (K = 1): the assertions of test_gpu_recon_weighted.test_gpu_equals_the_restatement and
    test_confidence_planes_scales_and_counts; the dropped rows and the isolated pixels lie at the origin and in a tile of the second
    trip, and their counts are the restatement's."""
    blocks, _ = past_both_thresholds(G, "recon_tiles", w, h)
    past_both_thresholds(G, "recon_pixels", w, h)
    planes, energies, iterates, want, (x0, y0) = weighted_case(w, h)
    assert ((y0 + 1) // 8) * -(-w // 32) + (x0 + 2) // 32 >= blocks                # spoil's first row, of the second copy
    assert want["rows_dropped"] == 18 and want["pixels_isolated"] == 2           # spoil: 9 rows and 1 pixel, twice
    K = 0 if norm == "wl2" else 1
    kw = dict(norm=G.RECON_L2) if norm == "wl2" else dict(norm=G.RECON_L1, irls_iters=1)
    out, conf, st = G.reconstruct_weighted(w, h, *planes, ALPHA, conf_floor=0.05, confidence=True, **kw, **TIGHT)
    err = rel_l2(out, iterates[K])
    figs = [abs(st.scale_data - want["scale_data"]) / want["scale_data"], abs(st.scale_grad - want["scale_grad"]) / want["scale_grad"]]
    figs += [rel_l2(conf[..., k], want[name]) for k, name in enumerate(("kd", "kx", "ky"))]
    print(f"{norm} {w}x{h}: rel L2 {err:.3e}, CG iterations {st.recon.cg_iters_total}, residual {st.recon.rel_residual_last:.2e}, "
          f"energy {st.recon.energy_last:.6f} (restatement {energies[K]:.6f}, relative difference {abs(st.recon.energy_last - energies[K]) / energies[K]:.2e}); "
          f"scales and confidence planes: worst figure {max(figs):.2e}; {st.rows_dropped} rows dropped, {st.pixels_isolated} pixels isolated")
    assert err < 1e-7
    assert st.recon.irls_rounds == K + 1 and st.recon.norm == (G.RECON_L2 if norm == "wl2" else G.RECON_L1)
    assert abs(st.recon.energy_last - energies[K]) <= 1e-8 * energies[K]
    assert st.recon.rel_residual_last <= TIGHT["cg_tol"] and st.recon.cg_iters_total > 0 and st.recon.solve_ms > 0
    assert abs(st.scale_data - want["scale_data"]) <= 1e-12 * want["scale_data"]
    assert abs(st.scale_grad - want["scale_grad"]) <= 1e-12 * want["scale_grad"]
    assert (st.rows_dropped, st.pixels_isolated) == (want["rows_dropped"], want["pixels_isolated"])
    for k, name in enumerate(("kd", "kx", "ky")):
        assert np.array_equal(conf[..., k] == 0, want[name] == 0), name
        assert rel_l2(conf[..., k], want[name]) <= 1e-12, name
        assert np.abs(conf[..., k] - want[name]).max() <= 1e-12 * np.abs(want[name]).max(), name
    assert np.isfinite(out).all() and (out[6, 9] == 0).all() and (out[y0 + 6, x0 + 9] == 0).all()


# ---- spread / box ---------------------------------------------------------------------------------------------------------------

def spread_inputs(G, w, h, n, planted):
    images, ws, total = synthetic(w, h, n, 100 * w + n, planted)
    if planted:
        (x, y), halo = second_trip_spots(G, w, h)
        images[1][y, x, 0] = np.nan
        total[y, x + 1, 2] = np.inf
        images[0][halo[0][1], halo[0][0], 1] = -np.inf
        total[halo[1][1], halo[1][0], 0] = np.nan
    return images, ws, total


@pytest.mark.parametrize("planted", [False, True], ids=["clean", "planted"])
@pytest.mark.parametrize("w,h", FILMS)
def test_spread_and_box(G, w, h, planted):
    """N in {2, 16} x radius in {0, 1, 8}: var, the map and the two sums under SPREAD_BOUND, the left-out count exact
    (test_gpu_recon_spread.compare); planted: that module's NaN / Inf and four more, in a tile of the second trip and in its halo."""
    past_both_thresholds(G, "spread", w, h)
    past_both_thresholds(G, "box", w, h)
    worst = 0.0
    for n in (2, 16):
        images, ws, total = spread_inputs(G, w, h, n, planted)
        for r in (0, 1, 8):
            var, emap, st = G.recon_spread(images, ws, total=total, radius=r)
            fig, e = compare(var, emap, st, images, ws, total, r)
            worst = max(worst, fig)
            assert st.pixels_left_out == (9 if planted else 0)       # synthetic's five pixels and the four of the second trip
    print(f"spread {w}x{h} {'planted' if planted else 'clean'}: worst figure {worst:.3e} (bound {SPREAD_BOUND})")
    assert worst < SPREAD_BOUND


@pytest.mark.parametrize("w,h", FILMS)
def test_spread_same_bits_twice_and_on_a_second_stream(G, w, h):
    past_both_thresholds(G, "spread", w, h)
    past_both_thresholds(G, "box", w, h)
    n, r = 3, 8
    images, ws, total = spread_inputs(G, w, h, n, True)
    ptrs = [hip_rt.upload(G, x) for x in images] + [hip_rt.upload(G, total)]
    d_var, d_map = hip_rt.alloc(G, 8 * w * h * 3), hip_rt.alloc(G, 8 * w * h)
    side = hip_rt.stream(G)
    runs = []
    for stream in (None, None, side):
        for p, nbytes in ((d_var, 8 * w * h * 3), (d_map, 8 * w * h)):
            hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(nbytes)))
        st = G.recon_spread_device(w, h, ptrs[:n], ws, total_ptr=ptrs[n], radius=r, var_ptr=d_var, map_ptr=d_map, stream=stream)
        runs.append((hip_rt.to_host(G, d_var, (h, w, 3)), hip_rt.to_host(G, d_map, (h, w)), st.sum_var, st.sum_sq, st.pixels_left_out))
    first = runs[0]
    assert first[4] == 9 and first[2] > 0
    for var, emap, sv, sq, out in runs[1:]:
        assert np.array_equal(var, first[0], equal_nan=True) and np.array_equal(emap, first[1], equal_nan=True)
        assert (sv, sq, out) == first[2:]
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    for p in ptrs + [d_var, d_map]:
        hip_rt.free(G, p)


# ---- NLM ------------------------------------------------------------------------------------------------------------------------

def nlm_inputs(G, w, h, planted):
    if not planted:
        return noisy_film(w, h, 10 * w + h)
    img, var = planted_film(w, h, 10 * w + h)
    (x, y), halo = second_trip_spots(G, w, h)
    img[y, x, 1] = np.nan
    var[halo[0][1], halo[0][0], 0] = np.inf
    var[halo[1][1], halo[1][0], 2] = -1e-4
    return img, var


def both_forms(G, img, var, r, f):
    got = []
    for direct in (0, 1):
        with G.debug_knobs(nlm_direct=direct):
            got.append(G.denoise_nlm(img, var, window_radius=r, patch_radius=f))
        assert (got[-1][2].window_radius, got[-1][2].patch_radius) == (r, f) and got[-1][2].filter_ms > 0
    return got


@pytest.mark.parametrize("planted", [False, True], ids=["clean", "planted"])
@pytest.mark.parametrize("w,h", FILMS)
def test_nlm_both_forms(G, w, h, planted):
    """(r, f) = (2, 1) and (3, 3): both forms against the restatement and against each other under NLM_BOUND with test_gpu_nlm.figure
    (the left-out count exact); (10, 3), the largest stage in LDS: the tiled form against the direct one (the restatement takes 20 s
    there); the tiled form twice for the same bits. planted: that module's spots and three more, in a tile of the second trip and in
    its halo."""
    past_both_thresholds(G, "nlm", w, h)
    img, var = nlm_inputs(G, w, h, planted)
    ok = N.valid_mask(img, var)
    assert (~ok).sum() == (10 if planted else 0)                      # planted_film's seven pixels and the three of the second trip
    worst = {"tiled": 0.0, "direct": 0.0, "forms": 0.0}
    for (r, f) in ((2, 1), (3, 3), (10, 3)):
        got = both_forms(G, img, var, r, f)
        if r < 10:
            want = N.denoise(img, var, r=r, f=f)
            assert want["left_out"] == (~ok).sum()
            for name, (o, vo, st) in zip(("tiled", "direct"), got):
                assert np.array_equal(o[~ok], img[~ok], equal_nan=True) and np.array_equal(vo[~ok], var[~ok], equal_nan=True), (name, r, f)
                worst[name] = max(worst[name], figure(o, vo, st, want))
        worst["forms"] = max(worst["forms"], figure(*got[0], as_dict(*got[1])))
        assert got[0][2].pixels_left_out == (~ok).sum()
        with G.debug_knobs(nlm_direct=0):
            o, vo, st = G.denoise_nlm(img, var, window_radius=r, patch_radius=f)
        assert np.array_equal(o, got[0][0], equal_nan=True) and np.array_equal(vo, got[0][1], equal_nan=True)
        assert all(getattr(st, k) == getattr(got[0][2], k) for k in ("sum_var_in", "sum_sq_in", "sum_var_out", "sum_sq_out", "pixels_left_out"))
    print(f"nlm {w}x{h} {'planted' if planted else 'clean'}: worst figure tiled {worst['tiled']:.3e}, direct {worst['direct']:.3e} against the restatement, "
          f"tiled against direct {worst['forms']:.3e} (bound {NLM_BOUND})")
    assert max(worst.values()) < NLM_BOUND


# ---- the progressive session ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide_cbox(G, scene_tmp):
    sd = G.parse_scene(scene_variant(scene_tmp, "cbox/cbox_gdpt.xml", width=WIDE[0], height=WIDE[1]))
    return G.Scene(sd), G.Scene(sd)


def test_progressive_fold_and_read_out(G, wide_cbox):
    """cbox at WIDE, passes 1, 1, 2: the body of test_gpu_progressive.test_fold_against_the_restatement (fold_kernel, finish_kernel;
    read() runs variance_kernel past its 4096 blocks), and the same session once more for the same bits."""
    w, h = WIDE
    past_both_thresholds(G, "fold", w, h)
    past_both_thresholds(G, "variance", w, h)
    sc, _ = wide_cbox
    sizes = [1, 1, 2]
    budget = sum(sizes)
    ses = G.Progressive(sc, budget)
    ref = P.Fold()
    done = 0
    for k, n in enumerate(sizes):
        ses.add_pass(n)
        bufs, _ = render_window(G, sc, n, (budget, done))
        ref.add(bufs, n)
        done += n
        st = ses.status()
        if k == 0:
            assert np.isnan(st["error"])
            means, v, a = ses.read()
            assert v is None and a is None
            for name in BUFS:
                assert np.array_equal(means[name], bufs[name])      # one pass: the mean is the pass
            continue
        means, var, asm = ses.read()
        want_var, want_asm = ref.var_mean(), ref.assembled_var()
        worst = worst_mean = 0.0
        for name in BUFS:
            e_mean = rel_l2(means[name], ref.mean[name])
            e_m2 = rel_l2(var[name] * ref.norm(), ref.M2[name])
            worst, worst_mean = max(worst, e_m2), max(worst_mean, e_mean)
            assert e_mean < 1e-13, (k, name, e_mean)
            assert rel_l2(var[name], want_var[name]) < M2_BOUND, (k, name)
        for name in ("c", "cx", "cy"):
            assert rel_l2(asm[name], want_asm[name]) < M2_BOUND, (k, name)
        assert np.array_equal(asm["c"], var["img"])
        e_ref, out_ref = ref.error_estimate()
        print(f"{w}x{h} pass {k + 1}: means rel L2 (worst buffer) {worst_mean:.2e}, M2 {worst:.2e}; error estimate {st['error']:.6e} against {e_ref:.6e} "
              f"(relative difference {abs(st['error'] - e_ref) / e_ref:.2e})")
        assert worst < M2_BOUND
        assert st["pixels_left_out"] == out_ref == 0
        assert abs(st["error"] - e_ref) <= (M2_BOUND + 1e-12) * e_ref
    again = G.Progressive(sc, budget)
    for n in sizes:
        again.add_pass(n)
    sa, sb = ses.status(), again.status()
    assert (sa["passes"], sa["spp"], sa["error"], sa["pixels_left_out"]) == (sb["passes"], sb["spp"], sb["error"], sb["pixels_left_out"])
    assert np.isfinite(sa["error"]) and sa["error"] > 0
    for x, y in zip(session_planes(ses), session_planes(again)):
        assert np.array_equal(x, y)
    ses.close(), again.close()


def test_progressive_merge(G, wide_cbox):
    """cbox at WIDE: the slices [0, 2) and [2, 4) of a block of 4, two passes of 1 each, read back and merged: merge_kernel and
    finish_kernel against progressive_merge_ref as test_gpu_progressive_merge.test_merge_against_the_restatement does."""
    w, h = WIDE
    past_both_thresholds(G, "fold", w, h)
    past_both_thresholds(G, "variance", w, h)
    sc1, sc2 = wide_cbox
    a, b = G.Progressive(sc1, 4, slice=(0, 2)), G.Progressive(sc2, 4, slice=(2, 2))
    for s in (a, b):
        s.add_pass(1), s.add_pass(1)
    fa, fb = state_of(a), state_of(b)
    b_before = session_planes(b)
    st = a.merge(b)
    check_against(a, M.merge(fa, fb), f"{w}x{h} merge")
    assert (st["passes"], st["spp"], st["budget_spp"]) == (4, 4, 4) and st["totals"].samples == w * h * 4 and st["fold_ms"] > 0
    for x, y in zip(session_planes(b), b_before):
        assert np.array_equal(x, y)                  # src is unchanged
    a.close(), b.close()


# ---- the Poisson CG -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [CG_FILM, WIDE])
def test_poisson_cg(G, O, w, h):
    """The comparison and the bounds of test_gpu_poisson_and_pipeline.test_poisson_cg_matches_dct_oracle; the solve must have stopped
    on its tolerance, not on max_iters."""
    past_both_thresholds(G, "cg", w, h)
    max_iters = 4000
    c, gx, gy = lcg_fields(w, h, seed=w * 1000 + h)
    ref = O.fourier_solve(c, gx, gy, 0.04)
    out, st = G.fourierSolve(w, h, c, gx, gy, 0.04, solver=G.SOLVER_CG, max_iters=max_iters, return_stats=True)
    err = rel_l2(out, ref)
    print(f"cg {w}x{h}: rel L2 {err:.3e}, {st.iterations} iterations, residual {st.rel_residual:.2e}")
    assert st.solver == G.SOLVER_CG and 0 < st.iterations < max_iters, "the solve was cut off at max_iters"
    assert st.rel_residual < 2e-10
    assert err < 1e-6          # includes the reference's fp32-lambda quirk (3-4e-9) and the CG tolerance
    np.testing.assert_allclose((weights(w, h) * out).sum(axis=(0, 1)), (weights(w, h) * c).sum(axis=(0, 1)), rtol=1e-7)
