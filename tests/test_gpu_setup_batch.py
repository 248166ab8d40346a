"""The batched sample set-up of the plain Lambertian lane machine (render_device.h: lane_camera_batched and the per-wave table of
gdpt_render_phases<..., SETUP>; device_trace.h: sample_setup / primary_from_setup; csrc/pcg_jump.h). On a power-of-two film a sample's
set-up (stream seeding, two draws, pixel filter) is made ahead of use and at full wave width: for an item's first sample when the wave
fetches its queue slice, for the following samples by whichever lane of the wave next needs one. (pixel, stream index) decide a set-up,
so none of that may show in a result: the five buffers and the counters of the product path (enqueue-only, route
lambert_plain/lds_const) are compared bit for bit with the knobs that select a kernel without it (no_setup_batch: the same kernel with
the old camera block; no_plain_kernel, no_lds_scene: other kernels, which never had it), and the buffers with the oracle at the tolerance
of tests/test_gpu_render_parity.py (1e-9 relative L2; the kernels may contract a*b+c, the oracle never does).

Shapes, the smallest at which each new path can go wrong:
  16x16, 1 spp                 every sample is an item's first: the table alone; one tile, four slices
  16x16, 3 spp, rows 7..16     the empty slots of a band inside one tile have entries in the table that are never written nor read
  32x16, 16 spp                items of 5, 5, 2, 2, 1, 1 samples: set-ups made ahead within an item and moved to the current slot,
                               slices across five chunk boundaries, short refills in the queue's tail
  32x32, 3 spp, each filter    box, tent and gaussian through sample_setup
  50x35, 3 spp                 no power of two: lane_camera runs as before, with and without the knob
  16x16, 3 spp, max depth 1    a sample is its base ray and four offset rays: a lane uses set-ups up as fast as it can
  16x16, two windows of 3      first_sample != 0 and stream_spp != spp: the stream index as the table pass forms it; then the same as a
                               progressive session of two passes
"""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import SCENES, rel_l2

pytestmark = pytest.mark.gpu

BUFS = ("img", "cx0", "cy0", "cx1", "cy1")
CBOX = os.path.join(SCENES, "cbox/cbox_gdpt.xml")
TOL = 1e-9                                        # tests/test_gpu_render_parity.py: TOL
COUNTERS = ("rays", "bounces", "samples", "nonfinite_samples")
ROUTE = "lambert_plain/lds_const"
KNOBS = ({"no_setup_batch": 1}, {"no_plain_kernel": 1}, {"no_lds_scene": 1})


def describe(G, film, filt=None, max_depth=None):
    import torch  # noqa: F401  (before the first call into libgdpt.so, as in tests/test_gpu_step_diet.py)
    sd = G.parse_scene(CBOX, film=film)
    if filt is not None:
        sd.desc.camera.filter_type, sd.desc.camera.filter_param = filt
    if max_depth is not None:
        sd.desc.max_depth = max_depth
    return sd


def new_bufs(film):
    import torch
    w, h = film
    return {k: torch.zeros((h, w, 3), dtype=torch.float64, device="cuda") for k in BUFS}


def launch(G, sc, bufs, spp, rows=(0, 0), max_depth_override=0, window=None, want_stats=False):
    """gdpt_render_device / gdpt_render_window_device with every parameter the cases need; enqueue-only unless want_stats."""
    p = G._params(spp, G.RNG_SAMPLE, rows, max_depth_override=max_depth_override)
    st = G.GdptRenderStats() if want_stats else None
    tail = [C.c_void_p(bufs[k].data_ptr()) for k in BUFS] + [C.c_void_p(0), C.byref(st) if st is not None else None]
    if window is None:
        G._check(G.lib().gdpt_render_device(sc.handle, C.byref(p), *tail))
    else:
        win = G.GdptSampleWindow(int(window[0]), int(window[1]))
        G._check(G.lib().gdpt_render_window_device(sc.handle, C.byref(p), C.byref(win), *tail))
    return st


def host(bufs):
    return {k: bufs[k].cpu().numpy() for k in BUFS}


def assert_bits(got, ref, what):
    for k in BUFS:
        assert np.array_equal(got[k], ref[k]), f"{what}: buffer {k} differs in {np.count_nonzero(got[k] != ref[k])} values"


def against_knobs(G, sd, film, spp, expect_route=ROUTE, **kw):
    """The product path's buffers (one enqueue-only render on a fresh handle), after comparing them and the counters with every knob."""
    import torch
    sc = G.Scene(sd)
    bufs = new_bufs(film)
    launch(G, sc, bufs, spp, **kw)
    torch.cuda.synchronize()
    assert G.debug_knobs.last_route() == expect_route and sc.overlapped_launches() == 1, (G.debug_knobs.last_route(), sc.overlapped_launches())
    shipped = host(bufs)
    sc.close()
    assert np.abs(shipped["img"]).max() > 0 and np.abs(shipped["cx0"]).max() > 0 and np.abs(shipped["cy1"]).max() > 0
    sc = G.Scene(sd)
    try:
        bufs = new_bufs(film)
        base = launch(G, sc, bufs, spp, want_stats=True, **kw)
        assert G.debug_knobs.last_route() == expect_route
        assert_bits(host(bufs), shipped, "launch with stats")
        routes = set()
        for knobs in KNOBS:
            with G.debug_knobs(**knobs):
                bufs = new_bufs(film)
                other = launch(G, sc, bufs, spp, want_stats=True, **kw)
                routes.add(G.debug_knobs.last_route())
            assert_bits(host(bufs), shipped, knobs)
            for c in COUNTERS:
                assert getattr(other, c) == getattr(base, c), (knobs, c, getattr(other, c), getattr(base, c))
        assert len(routes) == 3 and expect_route in routes, routes       # (no_setup_batch keeps the route's name)
    finally:
        sc.close()
    assert base.rays > 0 and base.nonfinite_samples == 0
    return shipped, base


def against_oracle(G, shipped, sd_oracle, spp, rows, what):
    import oracle_py as O
    want, ost = O.OracleScene(sd_oracle.ptr).render(spp, G.RNG_SAMPLE, threads=8)
    lo, hi = rows
    for k in BUFS:
        err = rel_l2(shipped[k][lo:hi], want[k][lo:hi])
        print(what, k, "rel L2 against the oracle", err)
        assert np.isfinite(shipped[k]).all() and err < TOL, f"{what}, {k}: rel L2 {err}"
    return ost


def check_case(G, film, spp, rows=(0, 0), filt=None):
    sd = describe(G, film, filt)
    lo, hi = rows if rows != (0, 0) else (0, film[1])
    shipped, base = against_knobs(G, sd, film, spp, rows=rows)
    for k in BUFS:
        assert not shipped[k][:lo].any() and not shipped[k][hi:].any(), k            # rows outside the band untouched
    assert base.samples == film[0] * (hi - lo) * spp and base.bounces > 0
    ost = against_oracle(G, shipped, sd, spp, (lo, hi), (film, spp, rows, filt))
    if rows == (0, 0):
        assert base.bounces == ost.bounces


def test_one_sample_per_pixel_table_only(G):
    check_case(G, (16, 16), 1)


def test_band_inside_one_tile_leaves_empty_table_entries(G):
    check_case(G, (16, 16), 3, rows=(7, 16))


def test_items_of_several_samples_and_short_refills(G):
    check_case(G, (32, 16), 16)


@pytest.mark.parametrize("name,param", [("FILTER_BOX", 1.0), ("FILTER_TENT", 2.0), ("FILTER_GAUSSIAN", 0.5)])
def test_each_pixel_filter(G, name, param):
    check_case(G, (32, 32), 3, filt=(getattr(G, name), param))


def test_film_that_is_no_power_of_two_keeps_the_old_block(G):
    check_case(G, (50, 35), 3)


def test_base_ray_and_offsets_only(G):
    film, spp = (16, 16), 3
    shipped, base = against_knobs(G, describe(G, film), film, spp, max_depth_override=1)
    assert base.samples == film[0] * film[1] * spp and base.bounces == 0
    assert base.rays <= 5 * base.samples                                            # a base ray and at most four offset rays
    against_oracle(G, shipped, describe(G, film, max_depth=1), spp, (0, film[1]), "max depth 1")


def test_sample_windows_and_a_progressive_session(G):
    """Two windows of 3 samples of a block of 6 streams per pixel, each against the knobs; their mean against the oracle's 6 spp (the
    same 6 streams). Then a progressive session of two passes of 3, which renders those windows: its means under each knob, bit for bit."""
    film, spp, block = (16, 16), 3, 6
    sd = describe(G, film)
    halves = [against_knobs(G, sd, film, spp, window=(block, first))[0] for first in (0, spp)]
    assert not np.array_equal(halves[0]["img"], halves[1]["img"])
    mean = {k: 0.5 * (halves[0][k] + halves[1][k]) for k in BUFS}
    against_oracle(G, mean, sd, block, (0, film[1]), "two windows")

    def session(**knobs):
        with G.debug_knobs(**knobs):
            sc = G.Scene(sd)
            p = G.Progressive(sc, block)
            stats = [p.add_pass(spp), p.add_pass(spp)]
            means, _, _ = p.read(variances=False)
            p.close()
            sc.close()
        return means, stats
    means, stats = session()
    for k in BUFS:
        assert rel_l2(means[k], mean[k]) < TOL, k
    for knobs in KNOBS:
        other, ostats = session(**knobs)
        assert_bits(other, means, ("session", knobs))
        for a, b in zip(stats, ostats):
            for c in COUNTERS:
                assert getattr(a, c) == getattr(b, c), (knobs, c)


def test_small_solve_shape_beside_a_cbox_render_at_512(G):
    """What two resident blocks of the product kernel leave of a CU's LDS does not depend on the film: behind an enqueue-only cbox render
    (16x16) the launcher's hint must still make a 512x512 solve take the small-footprint GEMM shape (tests/test_gpu_solve_beside_render.py),
    with the set-up table in the kernel's static LDS and without it."""
    import torch
    film = (16, 16)
    sd = describe(G, film)
    t = {k: torch.zeros((512, 512, 3), dtype=torch.float64, device="cuda") for k in BUFS + ("c", "gx", "gy", "out")}

    def solve():
        G.assemble_solve_device(512, 512, [t[k].data_ptr() for k in BUFS], [t[k].data_ptr() for k in ("c", "gx", "gy")], t["out"].data_ptr(),
                                alpha=0.04, solver=G.SOLVER_DCT_MFMA)
        return G.debug_knobs.last_dct_shape()
    for knobs in ({}, {"no_setup_batch": 1}):
        with G.debug_knobs(**knobs):
            sc = G.Scene(sd)
            launch(G, sc, new_bufs(film), 1)
            beside = solve()
            torch.cuda.synchronize()
            assert sc.overlapped_launches() == 1 and G.debug_knobs.last_route() == ROUTE
            sc.close()
            alone = solve()
            torch.cuda.synchronize()
        assert beside == "32x32x16" and alone != beside, (knobs, beside, alone)
