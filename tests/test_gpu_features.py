"""The feature render on the GPU (include/gdpt.h: gdpt_features_render*): both kernel forms (the scene in LDS, the walk from HBM)
against the sample-by-sample restatement (tests/features_ref.py) and against each other, what is exact (coverage, zero variances,
the clearcoat albedo), windows, bands, a film past the block cap, the same bits twice / on a second stream / enqueue-only, and
that a render of the same handle is not disturbed."""
import numpy as np
import pytest

import features_ref as FR
import hip_rt
from helpers import Built, DescBuilder, _camera, _quad, rel_l2, room

pytestmark = pytest.mark.gpu

# measured on an MI355X: the worst relative L2 of a mean or variance plane of either kernel form against the restatement, over every
# case of test_both_forms_against_the_restatement (7 scenes x 2 films x 3 sample counts x 2 forms) and the windows of
# test_a_window_is_those_samples_of_the_block. The sides differ by FMA contraction in the camera, vertex and texture code;
# the fold itself is written without contraction. 100 x the measured value is the margin (the rule of tests/test_gpu_nlm.py), never
# looser than 1e-9. Measured: 2.136e-14.
FEATURES_MEASURED = 2.2e-14
FEATURES_BOUND = min(100 * FEATURES_MEASURED, 1e-9) if FEATURES_MEASURED else None

KINDS = ["lambert", "lambert_tex", "lambert_sphere", "disney_clearcoat", "glass", "rough", "open"]
FILMS = [(17, 17), (33, 9)]          # one pixel beyond a 16 x 16 tile in each direction; three tiles in a row, a ragged one
SPPS = [1, 2, 5]


def open_scene(G, w, h):
    """One sphere and one emitter quad in empty space: most border pixels of the film miss."""
    b = DescBuilder(G)
    ct = lambda v: DescBuilder.const_tex(G, v)      # noqa: E731
    b.sphere((0.1, -0.1, -1.0), 0.8, b.material(G.MAT_LAMBERTIAN, [ct((0.3, 0.5, 0.7))]))
    _quad(b, [[-0.6, 0.9, -1.6], [0.6, 0.9, -1.6], [0.6, 1.1, -0.4], [-0.6, 1.1, -0.4]], b.material(G.MAT_LAMBERTIAN, [ct(0.0)]), (0, 0, 0),
          light=(5.0, 5.0, 5.0))
    _camera(G, b.desc.camera, w, h)
    b.desc.max_depth, b.desc.rr_depth = 4, 3
    return b


def build(G, kind, w, h):
    b = open_scene(G, w, h) if kind == "open" else room(G, kind, w, h, 4, 3)
    return Built(b.finish(), w, h, b)


@pytest.fixture(scope="module")
def scenes(G, O):
    """Every scene x film: the description, the device scene and the oracle scene (made once)."""
    out = {}
    for kind in KINDS:
        for film in FILMS:
            s = build(G, kind, *film)
            out[kind, film] = (s, G.Scene(s), O.OracleScene(s.ptr, use_bvh=True))
    yield out
    for _, sc, osc in out.values():
        sc.close()
        osc.close()


@pytest.fixture(scope="module")
def cases(G, scenes):
    """Every scene x film x spp: the restatement's samples (computed once, left unchanged) and both forms' planes."""
    out = []
    for (kind, film), (s, sc, osc) in scenes.items():
        for spp in SPPS:
            vals, shapes = FR.samples(osc, s.ptr.contents, spp)
            got = []
            for no_lds in (0, 1):
                with G.debug_knobs(no_lds_scene=no_lds):
                    got.append(sc.features(spp, want_stats=True))
            out.append(((kind, film, spp), s, vals, shapes, got))
    return out


def plane_figures(got_mean, got_var, want_mean, want_var):
    figs = []
    for c in range(8):
        for got, want in ((got_mean[c], want_mean[c]), (got_var[c], want_var[c])):
            assert np.isfinite(got).all()
            figs.append(rel_l2(got, want) if np.any(want) else float(np.abs(got).max()))
    return figs


def test_both_forms_against_the_restatement(G, cases):
    worst, seen_clearcoat, seen_flat, seen_miss, seen_mixed = 0.0, 0, 0, 0, 0
    for key, s, vals, shapes, got in cases:
        kind, (w, h), spp = key
        desc = s.ptr.contents
        want_mean, want_var = FR.fold(vals)
        for mean, var, st in got:
            assert mean.shape == var.shape == (8, h, w)
            figs = plane_figures(mean, var, want_mean, want_var)
            worst = max(worst, max(figs))
            # what is exact: the pixels of hits only and of misses only, the variance of one sample, the counters
            assert np.array_equal(mean[7] == 1.0, want_mean[7] == 1.0) and np.array_equal(mean[7] == 0.0, want_mean[7] == 0.0), key
            miss = want_mean[7] == 0.0
            assert not mean[:, miss].any() and not var[:, miss].any(), key
            if spp == 1:
                assert not var.any(), key
            assert (var >= 0).all() and not var[7][(want_mean[7] == 1.0) | miss].any(), key
            assert st.samples == w * h * spp and st.rays == w * h * spp and st.render_ms > 0
            assert (st.bounces, st.nodes_visited, st.tris_tested, st.nonfinite_samples, st.node_bytes, st.wave_steps) == (0,) * 6
            # pixels whose samples all hit one flat mesh with a constant slot-0 texture: albedo and normal have variance exactly 0
            one = (shapes == shapes[0]).all(axis=0) & (shapes[0] >= 0)
            for sid in np.unique(shapes[0][one]):
                shp = desc.shapes[int(sid)]
                mat = desc.materials[shp.material_id]
                if shp.type != G.SHAPE_TRIMESH or bool(shp.normals) or (mat.type != G.MAT_DISNEY_CLEARCOAT and mat.tex[0].type != G.TEX_CONSTANT):
                    continue
                px = one & (shapes[0] == sid)
                assert not var[0:6][:, px].any(), (key, int(sid))
                seen_flat += int(px.sum())
                if mat.type == G.MAT_DISNEY_CLEARCOAT:
                    assert (mean[0:3][:, px] == 1.0).all(), key
                    seen_clearcoat += int(px.sum())
            seen_miss += int(miss.sum())
            seen_mixed += int(((want_mean[7] > 0) & (want_mean[7] < 1)).sum())
        # the two forms, bit for bit
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), key
    assert seen_clearcoat > 0 and seen_flat > 1000 and seen_miss > 100 and seen_mixed > 0
    print(f"features against the restatement: worst plane figure {worst:.3e} (bound {FEATURES_BOUND})")
    assert FEATURES_BOUND is not None, f"FEATURES_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < FEATURES_BOUND


def test_most_border_pixels_of_the_open_scene_miss(cases):
    for key, s, vals, shapes, got in cases:
        kind, (w, h), spp = key
        if kind != "open":
            continue
        cov = got[0][0][7]
        border = np.ones((h, w), dtype=bool)
        border[1:-1, 1:-1] = False
        assert (cov[border] == 0.0).mean() > 0.5 and (cov == 1.0).any(), key


def test_a_window_is_those_samples_of_the_block(G, scenes):
    """A window {B, a} of n samples is the fold of samples a .. a + n - 1 of the restatement's block of B streams."""
    worst = 0.0
    for kind, film in (("lambert_tex", (17, 17)), ("open", (33, 9))):
        s, sc, osc = scenes[kind, film]
        block = 7
        vals, _ = FR.samples(osc, s.ptr.contents, block)            # stream_spp = 7, first_sample = 0: the whole block
        for (a, n) in ((0, 7), (0, 3), (2, 4), (6, 1)):
            want_mean, want_var = FR.fold(vals[a:a + n])
            for no_lds in (0, 1):
                with G.debug_knobs(no_lds_scene=no_lds):
                    mean, var = sc.features(n, window=(block, a))
                worst = max(worst, max(plane_figures(mean, var, want_mean, want_var)))
                assert np.array_equal(mean[7] == 1.0, want_mean[7] == 1.0) and np.array_equal(mean[7] == 0.0, want_mean[7] == 0.0)
        # and the plain call is the window {spp, 0}
        assert all(np.array_equal(p, q) for p, q in zip(sc.features(3), sc.features(3, window=(3, 0))))
        with pytest.raises(G.GdptError, match="must lie inside"):
            sc.features(4, window=(7, 4))
    print(f"feature windows against the restatement: worst plane figure {worst:.3e} (bound {FEATURES_BOUND})")
    assert FEATURES_BOUND is not None, f"FEATURES_MEASURED has not been recorded; this run measured {worst:.3e}"
    assert worst < FEATURES_BOUND


def test_bands_tile_the_film_and_leave_the_other_rows_alone(G, scenes):
    for kind, film in (("lambert_sphere", (17, 17)), ("glass", (33, 9))):
        s, sc, osc = scenes[kind, film]
        w, h = film
        for no_lds in (0, 1):
            with G.debug_knobs(no_lds_scene=no_lds):
                whole = sc.features(3)
                cut = h // 2 + 1
                mean, var = np.full((8, h, w), -7.0), np.full((8, h, w), -9.0)
                sc.features(3, rows=(cut, h), out=(mean, var))
                assert (mean[:, :cut] == -7.0).all() and (var[:, :cut] == -9.0).all()          # rows outside the band are untouched
                assert np.array_equal(mean[:, cut:], whole[0][:, cut:]) and np.array_equal(var[:, cut:], whole[1][:, cut:])
                sc.features(3, rows=(0, cut), out=(mean, var))
                assert np.array_equal(mean, whole[0]) and np.array_equal(var, whole[1])
        with pytest.raises(G.GdptError, match="row_end"):
            sc.features(3, rows=(0, h + 1))


def test_a_film_past_the_block_cap_equals_itself_in_four_bands(G):
    """1025 x 345: 65 x 22 = 1430 tiles for 1024 blocks, so some blocks take a second trip; four bands of 87, 86, 86 and 86 rows (none
    a multiple of the tile) are launches below the cap. 1 spp."""
    w, h = 1025, 345
    s = build(G, "lambert_sphere", w, h)
    sc = G.Scene(s)
    assert G.debug_knobs.image_grid("nlm", w, h) == (1024, 65 * 22)          # the same 16 x 16 tile grid
    mean, var = sc.features(1)
    assert (mean[7] == 1.0).all() and not var.any() and (mean[6] > 0.3).all()        # a closed room: every pixel of every trip was written
    bm, bv = np.full((8, h, w), -1.0), np.full((8, h, w), -1.0)
    cuts = [0, 87, 173, 259, 345]
    for y0, y1 in zip(cuts, cuts[1:]):
        sc.features(1, rows=(y0, y1), out=(bm, bv))
    assert np.array_equal(bm, mean) and np.array_equal(bv, var)
    with G.debug_knobs(no_lds_scene=1):
        hm, hv = sc.features(1)
    assert np.array_equal(hm, mean) and np.array_equal(hv, var)
    sc.close()


def test_same_bits_twice_on_a_second_stream_and_enqueue_only(G, scenes):
    s, sc, osc = scenes["rough", (33, 9)]
    w, h = 33, 9
    nbytes = 8 * w * h * 8
    d_mean, d_var = hip_rt.alloc(G, nbytes), hip_rt.alloc(G, nbytes)
    side = hip_rt.stream(G)
    first = sc.features(5)
    assert first[1].any()
    for stream, want_stats in ((None, True), (None, True), (side, True), (None, False), (side, False)):
        for p in (d_mean, d_var):
            hip_rt.ck(hip_rt.rt(G).hipMemset(hip_rt.C.c_void_p(p), 0, hip_rt.C.c_size_t(nbytes)))
        hip_rt.ck(hip_rt.rt(G).hipDeviceSynchronize())
        st = sc.features_device(d_mean, d_var, 5, stream=stream, want_stats=want_stats)
        assert (st is None) == (not want_stats) and (st is None or st.rays == w * h * 5)
        assert np.array_equal(hip_rt.to_host(G, d_mean, (8, h, w)), first[0]) and np.array_equal(hip_rt.to_host(G, d_var, (8, h, w)), first[1])
    G.poisson_forget_stream(side)
    hip_rt.stream_destroy(G, side)
    for p in (d_mean, d_var):
        hip_rt.free(G, p)


def test_a_render_of_the_same_handle_is_not_disturbed(G, scenes):
    """It is no render route and takes none of the handle's launch scratch: a GradPath render before and after gives the same bits,
    and the last route is still that render's."""
    for kind in ("lambert", "glass"):
        s, sc, osc = scenes[kind, (17, 17)]
        before, st0 = sc.render(spp=4)
        route = G.debug_knobs.last_route()
        sc.features(3)
        assert G.debug_knobs.last_route() == route and "feature" not in " ".join(G.debug_knobs.route_names())
        after, st1 = sc.render(spp=4)
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=True), (kind, k)
        assert st0.rays == st1.rays
