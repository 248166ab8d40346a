"""The leaf cursor of the LDS-resident one-sided lane machines (csrc/leaf_cursor.h, render_device.h: leaf_step) against the same
kernels with whole-leaf trips (knob whole_leaf_trips, include/gdpt_debug.h): the records of a leaf are tested in the same order with
no node visit in between, so images and traversal counters must agree bit for bit — for every LDS route, every leaf size, rays that
re-enter the walk holding a shortened leaf, and a band of an odd film."""
import ctypes as C

import numpy as np
import pytest

from helpers import Built, DescBuilder, odd_room_builder, room, scene_variant

BUFS = ("img", "cx0", "cy0", "cx1", "cy1")
FILM, SPP = (48, 32), 6
COUNTERS = ("rays", "bounces", "nodes_visited", "tris_tested", "nonfinite_samples")


def render_counting(G, sc, spp=SPP, rows=(0, 0), **knobs):
    """Five buffers + stats of the counting build (request flag: nodes_visited preset to UINT64_MAX), and the route."""
    bufs = {k: np.zeros((sc.height, sc.width, 3)) for k in BUFS}
    st = G.GdptRenderStats()
    st.nodes_visited = 2 ** 64 - 1
    p = G._params(spp, G.RNG_SAMPLE, rows)
    with G.debug_knobs(**knobs):
        G._check(G.lib().gdpt_render(sc.handle, C.byref(p), *[bufs[k].ctypes.data_as(C.POINTER(C.c_double)) for k in BUFS], C.byref(st)))
        route = G.debug_knobs.last_route()
    return bufs, st, route


def assert_same(a, b, what):
    (ba, sa, ra), (bb, sb, rb) = a, b
    assert ra == rb, (what, ra, rb)
    for k in BUFS:
        assert np.array_equal(ba[k], bb[k]), f"{what}: buffer {k} differs ({np.count_nonzero(ba[k] != bb[k])} values)"
    for c in COUNTERS:
        assert getattr(sa, c) == getattr(sb, c), (what, c, getattr(sa, c), getattr(sb, c))
    assert sa.wave_leaf_trips > 0 and sb.wave_leaf_trips > 0
    assert np.any(ba["img"]) and np.any(ba["cx0"]), f"{what}: empty image, the case would be vacuous"


def cbox(G, tmp, film=FILM):
    return G.parse_scene(scene_variant(tmp, "cbox/cbox_gdpt.xml", width=film[0], height=film[1]))


def lds_scene(G, tmp, kind):
    if kind == "cbox":
        return cbox(G, tmp)
    b = room(G, "lambert" if kind == "sphere_emitter" else kind, *FILM, -1, 5)
    if kind == "sphere_emitter":
        dark = b.material(G.MAT_LAMBERTIAN, [DescBuilder.const_tex(G, 0.0)])
        b.sphere((1.0, -1.2, -0.8), 0.5, dark, light=(5.0, 4.0, 3.0))
    return Built(b.finish(), *FILM, b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,route", [("cbox", "lambert_plain/lds_const"), ("sphere_emitter", "lambert/lds_wide"),
                                        ("lambert_tex", "lambert_plain/lds_tex"), ("general_mix", "general/lds_wide")])
def test_bit_identical_to_whole_leaf_trips(G, scene_tmp, kind, route):
    sc = G.Scene(lds_scene(G, scene_tmp, kind))
    try:
        spheres = sc.info()["num_spheres"]
        cursor = render_counting(G, sc)
        whole = render_counting(G, sc, whole_leaf_trips=1)
    finally:
        sc.close()
    assert cursor[2] == route and spheres == (1 if kind == "sphere_emitter" else 0)
    assert_same(cursor, whole, kind)


def odd_room(G):
    b = odd_room_builder(G, FILM)
    return Built(b.finish(), *FILM, b)


# scene -> bvh_leaf_max -> bvh_leaf_factor. cbox: the factors at which the builder mixes the sizes it can make of 19 quads (1, 2 and 4).
LEAF_FACTORS = {"cbox": {1: 0.8, 2: 1.4, 3: 1.5, 4: 0.01}, "odd_room": {1: 0.8, 2: 0.8, 3: 0.8, 4: 0.8}}


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cbox", "odd_room"])
def test_every_leaf_size(G, scene_tmp, scene):
    """bvh_leaf_max 1, 2, 3, 4: each render equals its whole-leaf twin, and all four equal one another — the closest hit does not depend
    on the tree. In odd_room leaves of every size 1 .. bvh_leaf_max occur (a three-record leaf is the case where a two-record step is
    followed by a short one: clamped second read, masked test). Where leaves of three or four records exist the cursor form must
    make more leaf trips than the knob's kernel for the same records tested: the knob really selects another kernel."""
    sd = cbox(G, scene_tmp) if scene == "cbox" else odd_room(G)
    renders = []
    for leaf_max, factor in LEAF_FACTORS[scene].items():
        with G.debug_knobs(bvh_leaf_max=leaf_max, bvh_leaf_factor=factor):
            sc = G.Scene(sd)
        try:
            hist = sc.leaf_histogram()
            print(scene, "bvh_leaf_max", leaf_max, "factor", factor, "leaf histogram", hist)
            assert not any(hist[leaf_max:]) and sum(hist) > 0, (leaf_max, hist)
            if scene == "odd_room":
                assert all(h > 0 for h in hist[:leaf_max]), (leaf_max, hist)
            cursor = render_counting(G, sc)
            whole = render_counting(G, sc, whole_leaf_trips=1)
        finally:
            sc.close()
        # (odd_room with one record per leaf is too deep for the BVH4 stack in LDS and is walked in its BVH2 form: also an LDS route)
        assert cursor[2] in ("lambert_plain/lds_const", "lambert/lds_bvh2"), cursor[2]
        assert_same(cursor, whole, f"{scene} bvh_leaf_max={leaf_max}")
        print("   wave_leaf_trips: cursor", cursor[1].wave_leaf_trips, "whole-leaf", whole[1].wave_leaf_trips)
        if hist[2] + hist[3] > 0:
            assert cursor[1].wave_leaf_trips > whole[1].wave_leaf_trips, (cursor[1].wave_leaf_trips, whole[1].wave_leaf_trips)
        renders.append(cursor[0])
    for r in renders[1:]:
        for k in BUFS:
            assert np.array_equal(r[k], renders[0][k]), k


@pytest.mark.gpu
def test_resumed_leaves(G, scene_tmp):
    """keep_frac 224: the trace phase is left while 7/8 of its rays are unfinished, so most lanes come back into the walk holding
    a node or a shortened leaf."""
    sc = G.Scene(cbox(G, scene_tmp))
    try:
        default = render_counting(G, sc)
        early = render_counting(G, sc, keep_frac=224)
        early_whole = render_counting(G, sc, keep_frac=224, whole_leaf_trips=1)
    finally:
        sc.close()
    assert_same(early, default, "keep_frac=224 against the default")
    assert_same(early, early_whole, "keep_frac=224 against whole-leaf trips")
    assert early[1].wave_steps > default[1].wave_steps        # the phase really was left earlier: more, emptier wave steps


@pytest.mark.gpu
def test_band_of_an_odd_film(G, scene_tmp):
    """Rows 5..27 of a 50x37 film (plan_rows left at its default): ragged edge tiles, items that end mid-leaf."""
    sc = G.Scene(cbox(G, scene_tmp, film=(50, 37)))
    try:
        cursor = render_counting(G, sc, rows=(5, 27))
        whole = render_counting(G, sc, rows=(5, 27), whole_leaf_trips=1)
    finally:
        sc.close()
    assert_same(cursor, whole, "rows 5..27 of 50x37")
    for k in BUFS:
        assert not np.any(cursor[0][k][:5]) and not np.any(cursor[0][k][27:]), k
