"""The one-sided lane machine after its instruction diet (render_device.h: camera_here, SliceQueue, lane_arm; csrc/item_slice.h) and the
resets of an overlapped launch enqueued when its scratch set is claimed (capi_device.hip: claim_scratch). Both must be invisible in
every result: the five buffers and the ray / bounce counters are compared bit for bit between the knobs that select another kernel or
another launch path (no_render_overlap, whole_leaf_trips, no_plain_kernel, no_lds_scene; include/gdpt_debug.h), and the buffers against
the oracle at the tolerance of tests/test_gpu_render_parity.py (1e-9 relative L2; the kernels may contract a*b+c, the oracle never does).

Shapes, the smallest at which the changed code takes each of its paths:
  50x35      ragged 16x16 edge tiles in both directions (tiles_x = 4: slices step over tile and tile-row boundaries; empty slots) and a
             film that is no power of two (the camera block's division path)
  16x16      a power-of-two film (the camera block's exact path), rows 7..16: one tile whose first seven pixel rows lie above the band
  96x80      1, 3 and 16 spp: 1, 3 and 6 chunks per pixel, so slices straddle 0, 2 and 5 chunk boundaries
  48x40x3    each pixel filter (box, tent, gaussian): the filter constants are read through camera_here too
"""
import os

import numpy as np
import pytest

from helpers import SCENES, rel_l2

pytestmark = pytest.mark.gpu

BUFS = ("img", "cx0", "cy0", "cx1", "cy1")
CBOX = os.path.join(SCENES, "cbox/cbox_gdpt.xml")
TOL = 1e-9                                        # tests/test_gpu_render_parity.py: TOL
COUNTERS = ("rays", "bounces", "samples", "nonfinite_samples")


def describe(G, film, filt=None):
    # torch before the first call into libgdpt.so: it brings a HIP runtime of its own, and imported after the library's it finds no device
    # (the tests of test_gpu_render_overlap.py import it first thing for the same reason)
    import torch  # noqa: F401
    sd = G.parse_scene(CBOX, film=film)
    if filt is not None:
        sd.desc.camera.filter_type, sd.desc.camera.filter_param = filt
    return sd


def new_bufs(film):
    import torch
    w, h = film
    return {k: torch.zeros((h, w, 3), dtype=torch.float64, device="cuda") for k in BUFS}


def enqueue(G, sc, bufs, spp, rows=(0, 0), want_stats=False):
    return sc.render_device([bufs[k].data_ptr() for k in BUFS], spp=spp, rng_scheme=G.RNG_SAMPLE, rows=rows, want_stats=want_stats)


def host(bufs):
    return {k: bufs[k].cpu().numpy() for k in BUFS}


def enqueue_only(G, sd, film, spp, rows, **knobs):
    """One enqueue-only render on a fresh handle: (host buffers, route, overlapped launches)."""
    import torch
    with G.debug_knobs(**knobs):
        sc = G.Scene(sd)
        bufs = new_bufs(film)
        enqueue(G, sc, bufs, spp, rows)
        torch.cuda.synchronize()
        route, overlapped = G.debug_knobs.last_route(), sc.overlapped_launches()
        sc.close()
    return host(bufs), route, overlapped


def with_stats(G, sc, spp, rows, **knobs):
    with G.debug_knobs(**knobs):
        bufs, st = sc.render(spp, G.RNG_SAMPLE, rows=rows)
        route = G.debug_knobs.last_route()
    return bufs, st, route


def assert_bits(got, ref, what):
    for k in BUFS:
        assert np.array_equal(got[k], ref[k]), f"{what}: buffer {k} differs in {np.count_nonzero(got[k] != ref[k])} values"


def check_case(G, film, spp, rows=(0, 0), filt=None):
    sd = describe(G, film, filt)
    lo, hi = rows if rows != (0, 0) else (0, film[1])
    # the product path: enqueue only, the kernel on a render stream, resets enqueued with the claim
    shipped, route, overlapped = enqueue_only(G, sd, film, spp, rows)
    assert route == "lambert_plain/lds_const" and overlapped == 1, (route, overlapped)
    assert np.abs(shipped["img"]).max() > 0 and np.abs(shipped["cx0"]).max() > 0 and np.abs(shipped["cy1"]).max() > 0
    for k in BUFS:
        assert not shipped[k][:lo].any() and not shipped[k][hi:].any(), k            # rows outside the band untouched
    in_stream, route, overlapped = enqueue_only(G, sd, film, spp, rows, no_render_overlap=1)
    assert route == "lambert_plain/lds_const" and overlapped == 0, (route, overlapped)
    assert_bits(in_stream, shipped, "no_render_overlap")
    # the knobs that select another kernel, each with its counters (a launch with stats: the caller's stream)
    sc = G.Scene(sd)
    try:
        base = with_stats(G, sc, spp, rows)
        assert base[2] == "lambert_plain/lds_const", base[2]
        assert_bits(base[0], shipped, "launch with stats")
        routes = set()
        for knobs in ({"whole_leaf_trips": 1}, {"no_plain_kernel": 1}, {"no_lds_scene": 1}, {"no_lds_scene": 1, "no_plain_kernel": 1}):
            other = with_stats(G, sc, spp, rows, **knobs)
            routes.add(other[2])
            assert_bits(other[0], shipped, knobs)
            for c in COUNTERS:
                assert getattr(other[1], c) == getattr(base[1], c), (knobs, c, getattr(other[1], c), getattr(base[1], c))
        assert len(routes) >= 3, routes               # the knobs really chose other kernels (whole_leaf_trips keeps the route's name)
    finally:
        sc.close()
    assert base[1].samples == film[0] * (hi - lo) * spp and base[1].rays > 0 and base[1].bounces > 0
    # the oracle renders the whole film; a band equals those rows of it (the work items are cut for the whole film either way)
    import oracle_py as O
    want, ost = O.OracleScene(sd.ptr).render(spp, G.RNG_SAMPLE, threads=8)
    for k in BUFS:
        err = rel_l2(shipped[k][lo:hi], want[k][lo:hi])
        print(film, spp, rows, filt, k, "rel L2 against the oracle", err)
        assert np.isfinite(shipped[k]).all() and err < TOL, f"{k}: rel L2 {err}"
    if rows == (0, 0):
        assert base[1].bounces == ost.bounces and base[1].nonfinite_samples == 0


def test_ragged_film_that_is_no_power_of_two(G):
    check_case(G, (50, 35), 3)


def test_band_inside_one_tile_of_a_power_of_two_film(G):
    check_case(G, (16, 16), 3, rows=(7, 16))


@pytest.mark.parametrize("spp", [1, 3, 16])
def test_slices_across_chunk_boundaries(G, spp):
    check_case(G, (96, 80), spp)


@pytest.mark.parametrize("name,param", [("FILTER_BOX", 1.0), ("FILTER_TENT", 2.0), ("FILTER_GAUSSIAN", 0.5)])
def test_each_pixel_filter(G, name, param):
    check_case(G, (48, 40), 3, filt=(getattr(G, name), param))


def test_resets_enqueued_with_the_claim(G):
    """One handle: three enqueue-only renders of different bands and spp with a launch with stats between the second and the third.
    Each equals the same call on a fresh handle with everything on the caller's stream; the launch with stats reports the counters a
    fresh handle reports (a reset enqueued early must not reach a set whose counters are still to be read, nor be missed)."""
    import torch
    film = (96, 80)
    sd = describe(G, film)
    calls = [(3, (0, 40)), (6, (8, 72)), (1, (0, 80))]
    refs = [enqueue_only(G, sd, film, spp, rows, no_render_overlap=1)[0] for spp, rows in calls]
    fresh = G.Scene(sd)
    want = enqueue(G, fresh, new_bufs(film), 5, (16, 64), want_stats=True)
    fresh.close()
    sc = G.Scene(sd)
    sets = [new_bufs(film) for _ in calls]
    stats_bufs = new_bufs(film)
    enqueue(G, sc, sets[0], *calls[0])
    enqueue(G, sc, sets[1], *calls[1])
    got = enqueue(G, sc, stats_bufs, 5, (16, 64), want_stats=True)
    enqueue(G, sc, sets[2], *calls[2])
    torch.cuda.synchronize()
    assert sc.overlapped_launches() == 3              # (the launch with stats stays on the caller's stream)
    for name in COUNTERS:
        assert getattr(got, name) == getattr(want, name), name
    assert got.rays > 0 and got.bounces > 0 and got.samples == film[0] * 48 * 5
    for bufs, ref, call in zip(sets, refs, calls):
        assert_bits(host(bufs), ref, call)
    sc.close()
