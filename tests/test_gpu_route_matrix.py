"""Route matrix: every kernel the render dispatch can pick (include/gdpt_debug.h: route names), driven to its route and
compared with the CPU oracle where kernels go wrong: depth and roulette limits, films smaller than one 16x16 tile, sample
counts for which the work-item plan lays every chunk size down 8 times and takes samples back, row bands cut at odd rows.

Every case first asserts that the library reports the route its table row names, so a row that stops reaching its
kernel fails instead of passing on another one. The axes are combined pairwise, not as a full product: case i of a
route takes DEPTHS[i] and cycles films and sample counts with an offset per table row.

Tolerances (relative L2 per buffer): 1e-9 where only Lambertian lobes and box filters enter (fp64 on both sides, FMA
contraction apart), 1e-7 where transcendentals or textures do, 1e-6 for environment maps (as test_path_integrator.py)."""
import math
import os
import re

import numpy as np
import pytest

from helpers import Built, DescBuilder, _box, _camera, _quad, rel_l2, room, scene_variant  # noqa: F401 (other modules import them from here)

BUFS = ("img", "cx0", "cy0", "cx1", "cy1")
THREADS = min(16, os.cpu_count() or 1)
DEPTHS = [(0, 5), (1, 5), (2, 5), (3, 5), (-1, 0), (-1, 1), (-1, 2), (-1, 3), (4, 2)]    # (maxDepth, rrDepth)
FILMS = [(1, 1), (7, 5), (17, 3), (1, 33), (40, 24)]
SPPS = [1, 3, 13, 37]
SMALL_FILM_LANES = 256 * 2 * 256        # resident lanes of one MI355X (256 CUs, 2 blocks of 256 each)


def way(kind, integ="grad", rng="sample", shift="reference", tol=1e-9, **knobs):
    return dict(kind=kind, integ=integ, rng=rng, shift=shift, tol=tol, knobs=knobs)


T7, T6 = 1e-7, 1e-6
ROUTES = {
    # GradPath, sample stream, one-sided lobes: the lane machine with lazy offsets
    "lambert_plain/lds_const": [way("lambert")],
    "lambert_plain/lds_tex": [way("lambert_tex", tol=T7)],
    "lambert_plain/hbm_const": [way("lambert", no_lds_scene=1)],
    "lambert_plain/hbm_tex": [way("lambert_tex", tol=T7, no_lds_scene=1)],
    "lambert/lds_wide": [way("lambert_sphere")],
    "lambert/lds_bvh2": [way("lambert", lds_wide=0), way("lambert_sphere", lds_wide=0)],
    "lambert/hbm": [way("lambert_sphere", no_lds_scene=1)],
    "lambert_stamped/lds_plain": [way("lambert", stamps=1)],
    "lambert_stamped/lds": [way("lambert_sphere", stamps=1)],
    "lambert_stamped/hbm": [way("lambert", stamps=1, no_lds_scene=1)],
    "general_set_a/disney_diffuse": [way("disney_diffuse", tol=T7, no_lds_scene=1)],
    "general_set_a/disney_metal": [way("disney_metal", tol=T7, no_lds_scene=1)],
    "general_set_b/disney_clearcoat": [way("disney_clearcoat", tol=T7, no_lds_scene=1)],
    "general_set_b/disney_sheen": [way("disney_sheen", tol=T7, no_lds_scene=1)],
    "general/lds_wide": [way("general_mix", tol=T7)],
    "general/lds_bvh2": [way("general_mix", tol=T7, lds_wide=0)],
    "general/hbm": [way("general_mix", tol=T7, no_lds_scene=1),
                    way("disney_metal", tol=T7, no_lds_scene=1, full_material_switch=1)],
    "wavefront/lambert": [way("lambert_sphere", wavefront=1, no_lds_scene=1)],
    "wavefront/general": [way("general_mix", tol=T7, wavefront=1, no_lds_scene=1)],
    # GradPath, two-sided lobes: offsets replayed from the bounce log (an LDS scene in BVH2 form is walked from HBM)
    "twosided/lds": [way("bsdf", tol=T7)],
    "twosided/hbm": [way("bsdf", tol=T7, no_lds_scene=1), way("bsdf", tol=T7, lds_wide=0)],
    "twosided/hbm_glass": [way("glass", tol=T7, no_lds_scene=1)],
    # GradPath, straight loops: rough lobes go to the eager evaluator (not to the lane machine)
    "eager": [way("rough", tol=T7), way("lambert", force_eager=1), way("bsdf", tol=T7, no_twosided_machine=1)],
    "tile_eager": [way("bsdf", rng="tile", tol=T7), way("rough", rng="tile", tol=T7)],
    "tile_phases_lambert": [way("lambert", rng="tile")],
    "tile_phases_general": [way("general_mix", rng="tile", tol=T7)],
    # GradPath, reconnection shift (the general kernel walks every scene from HBM)
    "reconnect/lds_lambert": [way("lambert", shift="reconnect")],
    "reconnect/hbm_lambert": [way("lambert", shift="reconnect", no_lds_scene=1)],
    "reconnect/general": [way("general_mix", shift="reconnect", tol=T7),
                          way("general_mix", shift="reconnect", tol=T7, no_lds_scene=1)],
    # Integrator::Path
    "path/tile": [way("lambert", integ="path", rng="tile")],
    "path/eager": [way("lambert", integ="path", force_eager=1)],
    "path_persistent/lds_lambert_plain": [way("lambert", integ="path")],
    "path_persistent/lds_lambert": [way("lambert_sphere", integ="path")],
    "path_persistent/lds_lambert_env": [way("env_lambert", integ="path", tol=T6)],
    "path_persistent/hbm_lambert": [way("lambert", integ="path", no_lds_scene=1)],
    "path_persistent/hbm_lambert_env": [way("env_lambert", integ="path", tol=T6, no_lds_scene=1)],
    "path_persistent/lds_general": [way("general_mix", integ="path", tol=T7)],
    "path_persistent/lds_general_env": [way("env_general", integ="path", tol=T6)],
    "path_persistent/hbm_general": [way("general_mix", integ="path", tol=T7, no_lds_scene=1)],
    "path_persistent/hbm_general_env": [way("env_general", integ="path", tol=T6, no_lds_scene=1)],
}


def _cases():
    """(route, way index, depth, film, spp, rows): the first way of a route meets every depth, further ways three."""
    out, g = [], 0
    for route, ways in ROUTES.items():
        for wi, w in enumerate(ways):
            picks = range(len(DEPTHS)) if wi == 0 else (g % 3, 3 + g % 3, 6 + g % 3)
            for i in picks:
                W, H = FILMS[(i + g) % len(FILMS)]
                spp = SPPS[(i + 2 * g) % len(SPPS)]
                rows = (0, 0)
                if H >= 24 and (i + g) % 2 == 0:
                    # the tile stream cuts whole 16-row tile rows only
                    rows = (16, H) if w["rng"] == "tile" and H > 16 else (0, 16) if w["rng"] == "tile" else (5, 19)
                out.append(pytest.param(route, wi, DEPTHS[i], (W, H), spp, rows,
                                        id=f"{route}-{wi}-d{DEPTHS[i][0]}r{DEPTHS[i][1]}-{W}x{H}-s{spp}-b{rows[0]}_{rows[1]}"))
            g += 1
    return out


CASES = _cases()


# ---- scenes ---------------------------------------------------------------------------------------------------------
# (the room and its parts: tests/helpers.py)


def make_scene(G, tmp, kind, film, depth):
    W, H = film
    if kind in ("env_general", "env_lambert"):
        xml = scene_variant(tmp, "disney_bsdf_test/disney_diffuse.xml")
        text = open(xml).read()
        # the three matpreview meshes replaced by two spheres and a rectangle (an LDS copy needs triangles): a scene small
        # enough for LDS (knob no_lds_scene: HBM)
        meshes = list(re.finditer(r'<shape type="serialized"[^>]*>.*?</transform>', text, re.S))
        assert len(meshes) == 3
        for n, m in enumerate(meshes[::-1]):
            shape = ('<shape type="rectangle"><transform name="toWorld"><scale x="3" y="3"/></transform>' if n == 0 else
                     f'<shape type="sphere"><point name="center" x="{n * 0.9:.1f}" y="0" z="1"/><float name="radius" value="0.8"/>')
            text = text[:m.start()] + shape + text[m.end():]
        if kind == "env_lambert":
            start = text.index('<bsdf type="disneydiffuse">')
            end = text.index("</bsdf>", start) + len("</bsdf>")
            text = text[:start] + '<bsdf type="diffuse"><rgb name="reflectance" value="0.82 0.67 0.16"/></bsdf>' + text[end:]
        out = xml.replace("_variant.xml", f"_{kind}.xml")
        open(out, "w").write(text)
        sd = G.parse_scene(out, film=film)
        sd.ptr.contents.max_depth, sd.ptr.contents.rr_depth = depth
        assert (sd.width, sd.height) == film
        return Built(sd.ptr, W, H, sd)
    b = room(G, kind, W, H, *depth)
    return Built(b.finish(), W, H, b)


def scene_types(s):
    d = s.ptr.contents
    return {d.materials[i].type for i in range(d.num_materials)}


def lambert_only(G, s):
    return scene_types(s) == {G.MAT_LAMBERTIAN}


# ---- the matrix -----------------------------------------------------------------------------------------------------
def render_both(G, O, s, w, spp, rows):
    rng = G.RNG_TILE if w["rng"] == "tile" else G.RNG_SAMPLE
    sc = G.Scene(s)
    try:
        with G.debug_knobs(**w["knobs"]):
            if w["integ"] == "path":
                got, st = sc.path_render(spp, rng, rows=rows)
            else:
                shift = G.SHIFT_RECONNECT if w["shift"] == "reconnect" else G.SHIFT_REFERENCE
                got, st = sc.render(spp, rng, rows=rows, shift=shift)
            route = G.debug_knobs.last_route()
    finally:
        sc.close()
    osc = O.OracleScene(s.ptr, use_bvh=True)
    if w["integ"] == "path":
        want, ost = osc.path_render(spp, rng, rows=rows, threads=THREADS)
    elif w["shift"] == "reconnect":
        want, ost = osc.reconnect_render(spp, rows=rows, threads=THREADS)
    else:
        want, ost = osc.render(spp, rng, rows=rows, threads=THREADS)
    osc.close()
    if w["integ"] == "path":
        got, want = {"img": got}, {"img": want}
    return route, got, st, want, ost


# Routes whose ray count equals the oracle's. The other kernels skip rays whose result cannot change the sample (lazy
# one-sided offsets, render_device.h; no replayed offset for a failed BSDF sample, render_twosided.h; and a few skipped
# offset or shadow rays in the straight-loop GradPath and the Path lane machine), so there the GPU traces at most as
# many rays as the oracle.
EXACT_RAYS = ("reconnect/", "path/tile", "path/eager")


def check_against_oracle(got, st, want, ost, tol, band, route, may_be_zero=False):
    r0, r1 = band
    for k in got:
        g, o = got[k][r0:r1], want[k][r0:r1]
        assert np.array_equal(np.isfinite(g), np.isfinite(o)), f"{k}: non-finite pixels differ"
        fin = np.isfinite(o)
        err = rel_l2(np.where(fin, g, 0.0), np.where(fin, o, 0.0))
        assert err < tol, f"{k}: rel L2 {err:.3e} (tolerance {tol:.0e})"
        # outside the band both sides leave the buffers untouched
        assert not np.any(got[k][:r0]) and not np.any(got[k][r1:]), f"{k}: written outside rows {band}"
        assert np.any(g) == np.any(o), f"{k}: zero on one side only"
    if not may_be_zero:     # the case renders light on both sides (a row whose film stays dark would test nothing)
        assert np.any(want["img"][r0:r1]) and np.any(got["img"][r0:r1]), "all-zero image: the case would be vacuous"
    assert st.bounces == ost.bounces, (st.bounces, ost.bounces)
    assert st.nonfinite_samples == ost.nonfinite_samples, (st.nonfinite_samples, ost.nonfinite_samples)
    if route.startswith(EXACT_RAYS):
        assert st.rays == ost.rays, ("rays", st.rays, ost.rays)
    else:
        assert 0 < st.rays <= ost.rays, ("rays", st.rays, ost.rays)


@pytest.mark.gpu
@pytest.mark.parametrize("route,wi,depth,film,spp,rows", CASES)
def test_route_against_oracle(G, O, scene_tmp, route, wi, depth, film, spp, rows):
    w = ROUTES[route][wi]
    s = make_scene(G, scene_tmp, w["kind"], film, depth)
    if w["kind"].startswith("lambert"):
        assert lambert_only(G, s)
    persistent = route.split("/")[0] not in ("eager", "tile_eager", "tile_phases_lambert", "tile_phases_general", "reconnect", "path")
    if persistent and spp in (13, 37):
        # work-item plan of a small film: every chunk size laid down q = 8 times, q * v - spp samples taken back
        begin = G.debug_knobs.chunk_plan(spp, film[0] * film[1], SMALL_FILM_LANES)
        sizes = np.diff(begin)
        assert sizes.sum() == spp and len(sizes) >= 8 and len(set(sizes[:8])) == 1 and spp % 8 != 0, sizes
    got_route, got, st, want, ost = render_both(G, O, s, w, spp, rows)
    assert got_route == route, f"table row reaches {got_route!r}, not {route!r}"
    band = (rows[0], rows[1]) if rows[1] > rows[0] else (0, film[1])
    # Environment-lit scenes at maxDepth 0 / 1 light only the pixels whose rays miss the objects (every room wall emits)
    may_be_zero = w["kind"].startswith("env") and depth[0] in (0, 1)
    check_against_oracle(got, st, want, ost, w["tol"], band, route, may_be_zero)
    assert st.samples == film[0] * (band[1] - band[0]) * spp


def test_route_table_names_every_route_the_library_reports(G):
    """A kernel arm added to the dispatch without a row here fails this (no GPU needed: the names are host data)."""
    names = G.debug_knobs.route_names()
    assert len(names) == len(set(names))
    assert set(ROUTES) == set(names)
    import threading
    seen = []
    t = threading.Thread(target=lambda: seen.append(G.debug_knobs.last_route()))     # a thread that has rendered nothing
    t.start()
    t.join()
    assert seen == [""]
    assert {c.values[0] for c in CASES} == set(ROUTES)


def test_small_film_plans_copy_their_chunks_and_take_samples_back(G):
    """The sample counts of the matrix make the persistent kernels' plan for a small film lay every chunk size down
    q = 8 times and give q * ceil(spp / q) - spp samples back (render_kernels.hip: make_chunk_plan)."""
    for W, H in FILMS:
        for spp in (13, 37):
            begin = G.debug_knobs.chunk_plan(spp, W * H, SMALL_FILM_LANES)
            sizes = list(np.diff(begin))
            assert sum(sizes) == spp and all(x >= 1 for x in sizes)
            assert sizes == sorted(sizes, reverse=True)
            # the first chunk size is laid down 8 times; 8 * ceil(spp / 8) - spp samples are taken back from the copies
            # (or, where every chunk holds a single sample, as many chunks dropped)
            assert len(sizes) >= 8 and len(set(sizes[:8])) == 1 and spp % 8 != 0, sizes


# ---- the two-sided replay machine's bounce log ----------------------------------------------------------------------
LOG_FILM, LOG_RR = (4, 3), 5000


def test_log_overflow_scene_runs_past_the_log(G, O):
    """Oracle only (no GPU): in the metal box most paths run to maxDepth, and the image at maxDepth 1100 differs from the
    one at 1025, so the GPU cases below render bounces past the replay's log."""
    bufs = {}
    for md in (1025, 1100):
        b = room(G, "metal_box", *LOG_FILM, md, LOG_RR)
        s = Built(b.finish(), *LOG_FILM, b)
        osc = O.OracleScene(s.ptr, use_bvh=True)
        bufs[md], st = osc.render(1, G.RNG_SAMPLE, threads=THREADS)
        osc.close()
        assert st.bounces >= LOG_FILM[0] * LOG_FILM[1] * (md - 1) * 0.75     # most paths run to maxDepth
    assert rel_l2(bufs[1100]["img"], bufs[1025]["img"]) > 1e-6



@pytest.mark.gpu
@pytest.mark.parametrize("max_depth,rr_depth,route", [(1025, LOG_RR, "twosided/lds"), (1026, LOG_RR, "eager"), (1100, LOG_RR, "eager"),
                                                     (-1, 224, "twosided/lds"), (-1, 225, "eager"), (-1, 1000, "eager")])
def test_two_sided_paths_longer_than_the_bounce_log(G, O, max_depth, rr_depth, route):
    """Two-sided lobes with a depth bound past the replay's log (render_twosided.h: kLogCap = 1024 iterations): the
    dispatch sends them to the straight-loop evaluator, which follows the reference to the end; at maxDepth 1025 the
    log holds every iteration and the replay machine stays exact. Without maxDepth the machine is kept while at least 800
    roulette draws separate rrDepth from the end of the log (rrDepth <= 224)."""
    b = room(G, "metal_box", *LOG_FILM, max_depth, rr_depth)
    s = Built(b.finish(), *LOG_FILM, b)
    got_route, got, st, want, ost = render_both(G, O, s, way("metal_box"), 1, (0, 0))
    assert got_route == route
    check_against_oracle(got, st, want, ost, 1e-7, (0, LOG_FILM[1]), route)
    assert np.nanmax(np.abs(want["cx0"])) > 0 and np.abs(want["img"]).max() > 0
