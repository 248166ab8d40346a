"""Overlapped render launches (csrc/hip/capi_device.hip: begin_launch / claim_scratch): an enqueue-only launch of the one-sided lane
machine runs its kernel on one of the handle's two render streams with one of its two scratch sets; only gdpt_reduce_partials stays on
the caller's stream. Nothing of that may show in a result: every comparison here is bitwise against the same call made with the knob
no_render_overlap (everything on the caller's stream, one scratch set), on a fresh handle.

The shapes are the smallest that can still go wrong: a 48x40 film has ragged 16x16 edge tiles in both directions and fewer pixels
than the persistent grid has lanes; 6 spp are cut into several work items per pixel, 3 spp into another plan.

A handle's film is fixed at upload, so the scratch-growth case cannot change the film on one handle: it renders a 40-row band of a
96x80 film at 3 spp, then the whole 96x80 film at 6 spp (more pixel slots and more work items per pixel: the partials grow while
the first launch's reduction may still be in flight), then the band again."""
import os

import numpy as np
import pytest

from helpers import SCENES

pytestmark = pytest.mark.gpu

BUFS = ("img", "cx0", "cy0", "cx1", "cy1")
CBOX = os.path.join(SCENES, "cbox/cbox_gdpt.xml")
SMALL, LARGE = (48, 40), (96, 80)

_descs, _refs = {}, {}


def desc(G, film):
    if film not in _descs:
        _descs[film] = G.parse_scene(CBOX, film=film)
    return _descs[film]


def new_bufs(film):
    import torch
    w, h = film
    return {k: torch.zeros((h, w, 3), dtype=torch.float64, device="cuda") for k in BUFS}


def enqueue(sc, bufs, spp, rows=(0, 0), stream=None, want_stats=False):
    import gdpt_amd as G
    return sc.render_device([bufs[k].data_ptr() for k in BUFS], spp=spp, rng_scheme=G.RNG_SAMPLE, rows=rows, stream=stream, want_stats=want_stats)


def host(bufs):
    return {k: bufs[k].cpu().numpy() for k in BUFS}


def reference(G, film, spp, rows=(0, 0)):
    """The in-stream result of one call into zeroed buffers on a fresh handle; computed once per (film, spp, rows), never modified."""
    import torch
    key = (film, spp, rows)
    if key not in _refs:
        with G.debug_knobs(no_render_overlap=1):
            sc = G.Scene(desc(G, film))
            bufs = new_bufs(film)
            enqueue(sc, bufs, spp, rows)
            torch.cuda.synchronize()
            assert G.debug_knobs.last_route().startswith("lambert"), G.debug_knobs.last_route()
            assert sc.overlapped_launches() == 0
            _refs[key] = host(bufs)
            sc.close()
        for k in BUFS:
            _refs[key][k].setflags(write=False)
        assert np.abs(_refs[key]["img"]).max() > 0 and np.abs(_refs[key]["cx0"]).max() > 0
    return _refs[key]


def assert_same(got, ref, what):
    for k in BUFS:
        assert np.array_equal(got[k], ref[k]), (what, k)


def test_consecutive_frames_without_sync(G):
    import torch
    ref = reference(G, SMALL, 6)
    sc = G.Scene(desc(G, SMALL))
    bufs = new_bufs(SMALL)
    for _ in range(8):
        enqueue(sc, bufs, 6)
    torch.cuda.synchronize()
    assert G.debug_knobs.last_route().startswith("lambert"), G.debug_knobs.last_route()
    assert sc.overlapped_launches() == 8              # every one of them took the render streams
    assert_same(host(bufs), ref, "eight frames")
    sc.close()


def test_alternating_parameters(G):
    """Three calls with nothing between them but the enqueues: 6, 3, 6 spp and rows (0,40), (8,24), (0,40) into two buffer
    sets; the third call overwrites the first one's result with equal bits, the second set holds the band."""
    import torch
    calls = [(6, (0, 40)), (3, (8, 24)), (6, (0, 40))]
    refs = [reference(G, SMALL, spp, rows) for spp, rows in calls]
    sc = G.Scene(desc(G, SMALL))
    sets = [new_bufs(SMALL), new_bufs(SMALL)]
    for (spp, rows), bufs in zip(calls, (sets[0], sets[1], sets[0])):
        enqueue(sc, bufs, spp, rows)
    torch.cuda.synchronize()
    assert_same(host(sets[0]), refs[2], "spp 6, whole film")
    assert_same(host(sets[1]), refs[1], "spp 3, rows 8..24")
    assert sc.overlapped_launches() == 3
    sc.close()


def test_scratch_growth_between_frames_in_flight(G):
    import torch
    calls = [(3, (0, 40)), (6, (0, 80)), (3, (0, 40))]
    refs = [reference(G, LARGE, spp, rows) for spp, rows in calls]
    sc = G.Scene(desc(G, LARGE))
    # two frames first, so that both scratch sets exist at the small size and the large frame has to grow one that has been in use
    sets = [new_bufs(LARGE) for _ in range(4)]
    enqueue(sc, sets[3], *calls[0])
    for (spp, rows), bufs in zip(calls, sets):
        enqueue(sc, bufs, spp, rows)
    torch.cuda.synchronize()
    for bufs, ref, call in zip(sets, refs, calls):
        assert_same(host(bufs), ref, call)
    assert_same(host(sets[3]), refs[0], "first frame")
    assert sc.overlapped_launches() == 4
    sc.close()


def test_counters_after_enqueue_only_calls(G):
    import torch
    fresh = G.Scene(desc(G, SMALL))
    want = enqueue(fresh, new_bufs(SMALL), 6, want_stats=True)
    fresh.close()
    assert want.rays > 0 and want.bounces > 0 and want.samples == SMALL[0] * SMALL[1] * 6
    sc = G.Scene(desc(G, SMALL))
    bufs = new_bufs(SMALL)
    enqueue(sc, bufs, 6)
    enqueue(sc, bufs, 3)
    got = enqueue(sc, bufs, 6, want_stats=True)
    for name in ("rays", "bounces", "samples", "nonfinite_samples"):
        assert getattr(got, name) == getattr(want, name), name
    assert sc.overlapped_launches() == 2              # (the launch with stats stays on the caller's stream)
    torch.cuda.synchronize()
    assert_same(host(bufs), reference(G, SMALL, 6), "frame with stats")
    sc.close()


def test_two_caller_streams(G):
    import torch
    refs = {6: reference(G, SMALL, 6), 3: reference(G, SMALL, 3)}
    sc = G.Scene(desc(G, SMALL))
    lanes = [(torch.cuda.Stream(), new_bufs(SMALL), 6), (torch.cuda.Stream(), new_bufs(SMALL), 3)]
    torch.cuda.synchronize()                        # (the buffers were zeroed on the default stream)
    for i in range(6):
        st, bufs, spp = lanes[i % 2]
        enqueue(sc, bufs, spp, stream=st.cuda_stream)
    torch.cuda.synchronize()
    for st, bufs, spp in lanes:
        assert_same(host(bufs), refs[spp], ("stream", spp))
    assert sc.overlapped_launches() == 6
    sc.close()


def test_destroy_in_flight(G):
    import torch
    ref = reference(G, SMALL, 6)
    sc = G.Scene(desc(G, SMALL))
    doomed = new_bufs(SMALL)
    enqueue(sc, doomed, 6)
    enqueue(sc, doomed, 6)
    sc.close()                                      # no sync before it: the handle joins what it has in flight
    torch.cuda.synchronize()
    assert_same(host(doomed), ref, "frame enqueued before the handle went")
    sc = G.Scene(desc(G, SMALL))
    bufs = new_bufs(SMALL)
    enqueue(sc, bufs, 6)
    torch.cuda.synchronize()
    assert_same(host(bufs), ref, "fresh handle")
    sc.close()
