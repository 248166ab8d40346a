"""A frame's solve beside the next frame's render kernel: while a lane machine on an LDS-resident scene is enqueued on one of a handle's
render streams, the render launcher's per-device hint (csrc/hip/render_kernels.h: render_beside_hint) makes GDPT_SOLVER_DCT_MFMA take
its small-footprint shape, which fits into the LDS two resident render blocks leave. The choice follows the call sequence — set by an
enqueue-only launch, cleared by an in-stream launch (which joins the render streams), and by the handle's destruction — and must not
show in a result: steps of enqueue-only render -> assemble_solve with no synchronisation in between are compared bit for bit with the
same steps under no_render_overlap (everything on the caller's stream, the solver's default shape). cbox at 48x32 and 64x48, 4 spp.
No timing assertions."""
import os

import numpy as np
import pytest

from helpers import SCENES

pytestmark = pytest.mark.gpu

BUFS = ("img", "cx0", "cy0", "cx1", "cy1")
CBOX = os.path.join(SCENES, "cbox/cbox_gdpt.xml")
FILMS, SPP, ALPHA = ((48, 32), (64, 48)), 4, 0.04
SMALL_SHAPE, DEFAULT_SHAPE = "32x32x16", "32x64x32"       # (both films: fewer 64-row tiles than CUs -> 32-row tiles, deep prefetch)

_descs = {}


def desc(G, film):
    if film not in _descs:
        _descs[film] = G.parse_scene(CBOX, film=film)
    return _descs[film]


class Frame:
    """Device buffers of one step: the five rendered buffers, c / cx / cy and the reconstructed image."""

    def __init__(self, film):
        import torch
        w, h = film
        self.film = film
        self.t = {k: torch.zeros((h, w, 3), dtype=torch.float64, device="cuda") for k in BUFS + ("c", "gx", "gy", "out")}

    def step(self, G, sc, want_stats=False):
        """Enqueue-only render -> assemble_solve on the default stream; returns the solver's shape."""
        sc.render_device([self.t[k].data_ptr() for k in BUFS], spp=SPP, rng_scheme=G.RNG_SAMPLE, want_stats=want_stats)
        self.solve(G)
        return G.debug_knobs.last_dct_shape()

    def solve(self, G):
        w, h = self.film
        G.assemble_solve_device(w, h, [self.t[k].data_ptr() for k in BUFS], [self.t[k].data_ptr() for k in ("c", "gx", "gy")], self.t["out"].data_ptr(),
                                alpha=ALPHA, solver=G.SOLVER_DCT_MFMA)

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}


_refs = {}


def reference(G, film):
    """One step under no_render_overlap on a fresh handle: computed once per film, never modified."""
    import torch
    if film not in _refs:
        with G.debug_knobs(no_render_overlap=1):
            sc = G.Scene(desc(G, film))
            f = Frame(film)
            shape = f.step(G, sc)
            torch.cuda.synchronize()
            assert sc.overlapped_launches() == 0 and shape == DEFAULT_SHAPE, (sc.overlapped_launches(), shape)
            _refs[film] = f.host()
            sc.close()
        for v in _refs[film].values():
            v.setflags(write=False)
        assert np.any(_refs[film]["img"]) and np.any(_refs[film]["cx0"]) and np.any(_refs[film]["out"])
    return _refs[film]


def assert_same(got, ref, what):
    for k in ref:
        assert np.array_equal(got[k], ref[k]), f"{what}: {k} differs in {np.count_nonzero(got[k] != ref[k])} values"


@pytest.mark.parametrize("film", FILMS)
def test_four_steps_without_sync(G, film):
    import torch
    ref = reference(G, film)
    sc = G.Scene(desc(G, film))
    frames = [Frame(film), Frame(film)]
    shapes = [frames[i % 2].step(G, sc) for i in range(4)]
    torch.cuda.synchronize()
    assert sc.overlapped_launches() == 4
    assert shapes == [SMALL_SHAPE] * 4, shapes            # every solve was enqueued behind an overlapped launch
    for f in frames:
        assert_same(f.host(), ref, f"{film}, four steps")
    sc.close()


def test_alternating_film_sizes(G):
    """Two handles on one device, their steps interleaved: the hint passes from one to the other with every launch."""
    import torch
    refs = [reference(G, film) for film in FILMS]
    scs = [G.Scene(desc(G, film)) for film in FILMS]
    frames = [Frame(film) for film in FILMS]
    shapes = [frames[i % 2].step(G, scs[i % 2]) for i in range(4)]
    torch.cuda.synchronize()
    assert shapes == [SMALL_SHAPE] * 4, shapes
    for f, ref in zip(frames, refs):
        assert_same(f.host(), ref, f"{f.film}, alternating")
    for sc in scs:
        sc.close()


def test_default_shape_after_join_and_after_close(G):
    import torch
    film = FILMS[0]
    ref = reference(G, film)
    sc = G.Scene(desc(G, film))
    f = Frame(film)
    assert f.step(G, sc) == SMALL_SHAPE
    # a launch with stats stays on the caller's stream: it joins the handle's render streams, and nothing of the handle's is resident behind it
    assert f.step(G, sc, want_stats=True) == DEFAULT_SHAPE
    torch.cuda.synchronize()
    assert_same(f.host(), ref, "solve after the join")
    assert f.step(G, sc) == SMALL_SHAPE
    sc.close()                                             # no sync before it: the handle joins what it has in flight and takes its hint along
    f.solve(G)
    assert G.debug_knobs.last_dct_shape() == DEFAULT_SHAPE
    torch.cuda.synchronize()
    assert_same(f.host(), ref, "solve after the handle went")
