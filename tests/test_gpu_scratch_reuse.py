"""Scratch that grows on demand and is then reused (csrc/hip/device_mem.h: Buffer::grow, PerStream) must not change a result: these
paths are documented as same inputs -> same bits, so every comparison here is bitwise. A handle that has grown its buffers, or has
been forgotten and made again, must give what a fresh one gives."""
import os

import numpy as np
import pytest

import hip_rt as H
from helpers import SCENES

pytestmark = pytest.mark.gpu

ALPHA = 0.04
SIZES = [(17, 9), (40, 24), (17, 9)]     # 40x24: two tile columns and three tile rows of the reconstruction's 32x8 tile; then back


def fields(w, h):
    rng = np.random.default_rng(1000 * w + h)
    c, gx, gy = rng.standard_normal((3, h, w, 3))
    return [c, gx, gy] + list(rng.uniform(0.01, 1.0, (3, h, w, 3)))      # primal, gradients, their variances


SOLVES = {
    "cg": lambda G, w, h, p, out, s: G.poisson_solve_device(w, h, p[0], p[1], p[2], out, ALPHA, solver=G.SOLVER_CG, stream=s),
    "dct": lambda G, w, h, p, out, s: G.poisson_solve_device(w, h, p[0], p[1], p[2], out, ALPHA, solver=G.SOLVER_DCT, stream=s),
    "dct_mfma": lambda G, w, h, p, out, s: G.poisson_solve_device(w, h, p[0], p[1], p[2], out, ALPHA, solver=G.SOLVER_DCT_MFMA, stream=s),
    "l1": lambda G, w, h, p, out, s: G.reconstruct_device(w, h, p[0], p[1], p[2], out, ALPHA, norm=G.RECON_L1, irls_iters=2, stream=s),
    "weighted_l2": lambda G, w, h, p, out, s: G.reconstruct_weighted_device(w, h, *p, out, ALPHA, norm=G.RECON_L2, stream=s),
}


def solve(G, name, w, h, stream):
    ins = [H.upload(G, a) for a in fields(w, h)]
    out = H.upload(G, np.full((h, w, 3), 7.0))
    try:
        SOLVES[name](G, w, h, ins, out, stream)
        return H.to_host(G, out, (h, w, 3))      # (waits for the device: the DCT solvers only enqueue)
    finally:
        for p in ins + [out]:
            H.free(G, p)


@pytest.mark.parametrize("name", list(SOLVES))
def test_solver_scratch_grows_and_is_reused(G, name):
    fresh = {}
    for w, h in set(SIZES):                  # each on a stream of its own that has done nothing else
        s = H.stream(G)
        fresh[w, h] = solve(G, name, w, h, s)
        G.poisson_forget_stream(s)
        H.stream_destroy(G, s)
        assert np.isfinite(fresh[w, h]).all() and not (fresh[w, h] == 7.0).any()
    side = H.stream(G)
    for w, h in SIZES:                       # allocate, grow, reuse the larger buffers
        assert np.array_equal(solve(G, name, w, h, side), fresh[w, h]), (name, w, h)
    G.poisson_forget_stream(side)            # the registry's entry goes; the next call makes a new one
    w, h = SIZES[0]
    assert np.array_equal(solve(G, name, w, h, side), fresh[w, h]), (name, "after forget")
    G.poisson_forget_stream(side)
    H.stream_destroy(G, side)


BUFS = ("img", "cx0", "cy0", "cx1", "cy1")


@pytest.mark.parametrize("rel, knobs, route", [
    ("cbox/cbox_gdpt.xml", {}, "lambert"),                                        # persistent LDS route: the work-item partials
    ("disney_bsdf_test/disney_glass.xml", {}, "twosided/"),                       # two-sided machine: partials + bounce log
    ("cbox/cbox_gdpt.xml", dict(wavefront=1, no_lds_scene=1), "wavefront/"),      # the wavefront buffers
])
def test_render_scratch_grows_and_is_reused(G, rel, knobs, route):
    """One scene handle renders 4, then 64, then 4 samples per pixel: its scratch is sized by the work items, grows for the second
    render and is larger than needed for the third. (The wavefront pipeline is for scenes walked from HBM: beside wavefront=1 the
    cbox needs no_lds_scene=1 to take it, and the route is asserted.)"""
    sd = G.parse_scene(os.path.join(SCENES, rel), film=(32, 32))
    with G.debug_knobs(**knobs):
        alone = {}
        for spp in (4, 64):
            sc = G.Scene(sd)
            alone[spp], _ = sc.render(spp)
            assert G.debug_knobs.last_route().startswith(route), G.debug_knobs.last_route()
            sc.close()
        assert np.abs(alone[4]["cx0"]).max() > 0 and not np.array_equal(alone[4]["cx0"], alone[64]["cx0"])      # (the glass scene's img is 0)
        sc = G.Scene(sd)
        for spp in (4, 64, 4):
            got, _ = sc.render(spp)
            assert G.debug_knobs.last_route().startswith(route), G.debug_knobs.last_route()
            for k in BUFS:
                assert np.array_equal(got[k], alone[spp][k]), (rel, spp, k)
        sc.close()


def test_progressive_scratch_is_allocated_lazily_and_reused(G):
    """read with variances, reconstruct and reconstruct_weighted allocate a session's variance and assembly planes on first use; the
    second round runs on the planes the first one made."""
    sc = G.Scene(G.parse_scene(os.path.join(SCENES, "cbox/cbox_gdpt.xml"), film=(32, 32)))
    pr = G.Progressive(sc, 4)
    pr.add_pass(2)
    pr.add_pass(2)

    def everything():
        means, vars_, asm = pr.read()
        planes = [means[k] for k in BUFS] + [vars_[k] for k in BUFS] + [asm[k] for k in ("c", "cx", "cy")]
        return planes + [pr.reconstruct(ALPHA)[0], pr.reconstruct_weighted(ALPHA)[0]]

    first, second = everything(), everything()
    assert len(first) == 15 and all(np.isfinite(a).all() for a in first)
    assert first[5].max() > 0 and np.abs(first[13] - first[14]).max() > 0      # variances were measured; the two reconstructions differ
    for i, (a, b) in enumerate(zip(first, second)):
        assert np.array_equal(a, b), i
    pr.close()
    sc.close()
