"""The one-sided lane machine on an LDS-resident scene takes the LDS its scene needs (csrc/lds_layout.h: the scene copy and the stack
are sized per launch) instead of the caps every scene was given before (20 KB of copy, 12 stack levels). The knob lds_fixed_layout
asks the same kernel for the caps. Where the tables lie in LDS and how long a lane's stack column is must not show anywhere: buffers,
traversal counters and the route name are compared bit for bit between the two layouts, and the buffers with the walk of the HBM
tables (knob no_lds_scene) — for every LDS route, the deepest and the shallowest tree that take one, a band of an odd film, and two
scenes of different size rendered alternately on one device. Film 48x32, 6 spp, the counting build."""
import numpy as np
import pytest

from helpers import Built, DescBuilder, _camera, _quad
from test_gpu_leaf_cursor import BUFS, FILM, assert_same, cbox, lds_scene, odd_room, render_counting

pytestmark = pytest.mark.gpu


def assert_fits(G, sc, what, route=None, rows=(0, 0)):
    """Fitted layout == fixed layout (buffers, counters, route); buffers == the walk from HBM. Returns the fitted render."""
    fitted = render_counting(G, sc, rows=rows)
    fixed = render_counting(G, sc, rows=rows, lds_fixed_layout=1)
    hbm = render_counting(G, sc, rows=rows, no_lds_scene=1)
    if route is not None:
        assert fitted[2] == route, (what, fitted[2])
    assert "lds" in fitted[2] and "hbm" in hbm[2], (what, fitted[2], hbm[2])
    assert_same(fitted, fixed, what)
    for k in BUFS:
        assert np.array_equal(fitted[0][k], hbm[0][k]), f"{what}: buffer {k} differs from the walk from HBM ({np.count_nonzero(fitted[0][k] != hbm[0][k])} values)"
    return fitted


@pytest.mark.parametrize("kind,route", [("cbox", "lambert_plain/lds_const"), ("lambert_tex", "lambert_plain/lds_tex"),
                                        ("sphere_emitter", "lambert/lds_wide"), ("general_mix", "general/lds_wide")])
def test_every_bvh4_route(G, scene_tmp, kind, route):
    sc = G.Scene(lds_scene(G, scene_tmp, kind))
    try:
        assert_fits(G, sc, kind, route)
    finally:
        sc.close()


def test_deepest_tree_bvh2_route(G):
    """odd_room with one record per leaf: its BVH4 needs more stack than the LDS column has, so it is walked in its BVH2 form — the
    deepest tree that still takes an LDS route (8 levels of the cap's 12)."""
    sd = odd_room(G)
    with G.debug_knobs(bvh_leaf_max=1, bvh_leaf_factor=0.8):
        sc = G.Scene(sd)
    try:
        depth = sc.info()["bvh_depth"]
        print("odd_room, one record per leaf: bvh_depth", depth)
        assert 1 < depth <= 12, depth                  # (kLdsSceneLevels = 12)
        assert_fits(G, sc, "odd_room bvh_leaf_max=1", "lambert/lds_bvh2")
    finally:
        sc.close()


def one_quad_room(G, film):
    """One emitting quad in front of the camera: two triangles, one leaf under the root, a stack bound of zero."""
    b = DescBuilder(G)
    m = b.material(G.MAT_LAMBERTIAN, [DescBuilder.const_tex(G, 0.6)])
    _quad(b, [[-1.5, -1.0, -1.0], [1.5, -1.0, -1.0], [1.5, 1.0, -1.0], [-1.5, 1.0, -1.0]], m, (0, 0, 1.6), light=(2.0, 1.5, 1.0))
    _camera(G, b.desc.camera, *film)
    return Built(b.finish(), *film, b)


def test_shallowest_tree(G):
    sc = G.Scene(one_quad_room(G, FILM))
    try:
        info = sc.info()
        print("one quad:", info)
        assert info["num_tris"] == 2 and info["num_nodes"] == 1 and info["bvh_depth"] <= 1, info
        assert_fits(G, sc, "one quad", "lambert_plain/lds_const")
    finally:
        sc.close()


def test_band_of_an_odd_film(G, scene_tmp):
    sc = G.Scene(cbox(G, scene_tmp, film=(47, 31)))
    try:
        got = assert_fits(G, sc, "rows 5..23 of 47x31", rows=(5, 23))
        for k in BUFS:
            assert not np.any(got[0][k][:5]) and not np.any(got[0][k][23:]), k
    finally:
        sc.close()


def test_two_scenes_alternating_on_one_device(G, scene_tmp):
    """cbox (16 KB of tables) and the one-quad room (a few hundred bytes), A B A B on one device: the dynamic size changes with every
    launch. Every render equals the scene's first, and the first equals the fixed layout."""
    a, b = G.Scene(cbox(G, scene_tmp)), G.Scene(one_quad_room(G, FILM))
    try:
        first = {0: assert_fits(G, a, "cbox"), 1: assert_fits(G, b, "one quad")}
        for i in range(4):
            got = render_counting(G, (a, b)[i % 2])
            assert_same(got, first[i % 2], f"launch {i}")
    finally:
        a.close()
        b.close()
