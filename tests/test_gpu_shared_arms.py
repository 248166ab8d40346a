"""What the arms of the lane machine's step share (render_device.h: lane_consume — one set of bounce-1 draws for the bouncing and the
offset lanes, one emission per step, one sums block, acc_step, behind the arms). None of it may move a bit. Every case asserts
  (a) the five buffers are bit-equal, and the ray / bounce / sample / non-finite counters equal, across the knobs that select another
      launch path or another kernel (no_render_overlap, whole_leaf_trips, no_plain_kernel, no_lds_scene; include/gdpt_debug.h);
  (b) the relative L2 error of each buffer against the oracle is below 1e-9 (TOL of tests/test_gpu_render_parity.py);
  (c) the sha1 of each buffer and the four counters equal tests/golden/shared_arms_parent.json, recorded on the same shapes with the
      library of the commit BEFORE the change, built in a worktree of its own:
          python tests/test_gpu_shared_arms.py --record <that libgdpt.so> <out.json>
      (the record is data; it is never made with the code under test).

Cases, cbox unless said, the smallest that reach each changed path:
  50x35x3, 16x16x3 rows 7..16    ragged tiles and a film that is no power of two (lane_camera), a band inside one tile of a power-of-two
                                 film (lane_camera_batched): both camera blocks in front of the shared draws
  96x80 at 1, 3, 16 spp          items of 1 .. 5 samples: the sums block sees every add pattern an item can have
  32x32x4, max depth 1, 2, 3, 6  with rr_depth 3: C_NO_LOOP (offsets of a path that never bounces), offsets behind bounce 1, samples that
                                 end without offsets, and the Russian-roulette draw in front of the shared draws (depth 6)
  32x32x2, TILE scheme           the serial kernel: SERIAL_RNG, the lane's kept numbers instead of the jump, sums in registers (AccReg)
  disney_metal 32x32x2           a one-sided Disney lobe on smooth normals: the material switch, where pdf <= 0 and below() do occur.
                                 Checked on the CPU first, with the oracle's per-sample records: at least one sample of this film has
                                 sampled bounce 1 and still has prob == 1 and contrib == 1, the state of a path that left the loop at
                                 p2 <= 0 before any update (src/path_tracing.h:760): C_BROKE_BOUNCE1 is taken.
  disney_metal 128x96x4          the same scene on the largest film that still runs in a second or two. A path that leaves the loop at
                                 p2 <= 0 in a LATER bounce (C_BROKE_BOUNCE2, and the second "no offsets" site from bounce 3 on) leaves a
                                 record that a path ended by a miss in that bounce leaves too, so the oracle's records cannot show that one
                                 occurs on a given film. Those branches are covered here by (a) and (c) only, on 49 152 samples.
The kernels with the full material switch, which the Disney cases run, keep every arm's own copy (each shared item costs them spilled
registers: DESIGN.md 4.1); the two cases hold them to the parent's bits beside the Lambertian machines, which have the shared arms.
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import pytest

from helpers import ROOT, rel_l2, scene_variant

pytestmark = pytest.mark.gpu

BUFS = ("img", "cx0", "cy0", "cx1", "cy1")
TOL = 1e-9                                        # tests/test_gpu_render_parity.py: TOL
COUNTERS = ("rays", "bounces", "samples", "nonfinite_samples")
GOLDEN = os.path.join(ROOT, "tests", "golden", "shared_arms_parent.json")
KNOBS = ({"whole_leaf_trips": 1}, {"no_plain_kernel": 1}, {"no_lds_scene": 1})
CBOX, DISNEY = "cbox/cbox_gdpt.xml", "disney_bsdf_test/disney_metal.xml"

CASES = (
    dict(id="cbox_50x35_3spp", scene=CBOX, film=(50, 35), spp=3),
    dict(id="cbox_16x16_3spp_rows7to16", scene=CBOX, film=(16, 16), spp=3, rows=(7, 16)),
    dict(id="cbox_96x80_1spp", scene=CBOX, film=(96, 80), spp=1),
    dict(id="cbox_96x80_3spp", scene=CBOX, film=(96, 80), spp=3),
    dict(id="cbox_96x80_16spp", scene=CBOX, film=(96, 80), spp=16),
    dict(id="cbox_32x32_4spp_depth1_rr3", scene=CBOX, film=(32, 32), spp=4, max_depth=1, rr_depth=3),
    dict(id="cbox_32x32_4spp_depth2_rr3", scene=CBOX, film=(32, 32), spp=4, max_depth=2, rr_depth=3),
    dict(id="cbox_32x32_4spp_depth3_rr3", scene=CBOX, film=(32, 32), spp=4, max_depth=3, rr_depth=3),
    dict(id="cbox_32x32_4spp_depth6_rr3", scene=CBOX, film=(32, 32), spp=4, max_depth=6, rr_depth=3),
    dict(id="cbox_32x32_2spp_tile_scheme", scene=CBOX, film=(32, 32), spp=2, tile=True),
    dict(id="disney_metal_32x32_2spp", scene=DISNEY, film=(32, 32), spp=2, integrator="gradpath", count_breaks=True),
    dict(id="disney_metal_128x96_4spp", scene=DISNEY, film=(128, 96), spp=4, integrator="gradpath"),
)


def describe(G, tmp, case):
    import torch  # noqa: F401  (before the first call into libgdpt.so, as in tests/test_gpu_step_diet.py)
    w, h = case["film"]
    xml = scene_variant(tmp, case["scene"], width=w, height=h, integrator=case.get("integrator"), max_depth=case.get("max_depth"),
                        rr_depth=case.get("rr_depth"), tag=case["id"])
    return G.parse_scene(xml)


def scheme(G, case):
    return G.RNG_TILE if case.get("tile") else G.RNG_SAMPLE


def digest(bufs, st):
    """What the record holds of one render: sha1 of each buffer's bytes, the four counters."""
    out = {k: hashlib.sha1(np.ascontiguousarray(bufs[k], dtype=np.float64).tobytes()).hexdigest() for k in BUFS}
    out.update({c: int(getattr(st, c)) for c in COUNTERS})
    return out


def render_with_stats(G, sc, case, **knobs):
    with G.debug_knobs(**knobs):
        bufs, st = sc.render(case["spp"], scheme(G, case), rows=case.get("rows", (0, 0)))
        route = G.debug_knobs.last_route()
    return bufs, st, route


def enqueue_only(G, sd, case, **knobs):
    """The product path: one enqueue-only render into device memory on a fresh handle. Host copies of the five buffers."""
    import torch
    w, h = case["film"]
    with G.debug_knobs(**knobs):
        sc = G.Scene(sd)
        bufs = {k: torch.zeros((h, w, 3), dtype=torch.float64, device="cuda") for k in BUFS}
        sc.render_device([bufs[k].data_ptr() for k in BUFS], spp=case["spp"], rng_scheme=scheme(G, case), rows=case.get("rows", (0, 0)))
        torch.cuda.synchronize()
        sc.close()
    return {k: bufs[k].cpu().numpy() for k in BUFS}


def assert_bits(got, ref, what):
    for k in BUFS:
        assert np.array_equal(got[k], ref[k], equal_nan=True), f"{what}: buffer {k} differs in {np.count_nonzero(got[k] != ref[k])} values"


def samples_that_broke_at_bounce_1(G, O, sd, case):
    """CPU only: the samples whose oracle record shows a path that sampled bounce 1 and left the loop at p2 <= 0 before any update
    (prob still exactly 1, contrib still 1; a failed sampling returns the zero record instead, contrib 0)."""
    osc = O.OracleScene(sd.ptr, use_bvh=True)
    w, h = case["film"]
    n = 0
    for y in range(h):
        for x in range(w):
            for s in range(case["spp"]):
                state, inc = O.pcg_init((y * w + x) * case["spp"] + s)
                rec, _ = osc.grad_sample(x, y, state, inc)
                if not rec.primary_miss and rec.bounces >= 1 and rec.prob == 1.0 and tuple(rec.contrib) == (1.0, 1.0, 1.0):
                    n += 1
    return n


@pytest.fixture(scope="module")
def record():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_shared_arms_move_no_bit(G, O, scene_tmp, record, case):
    sd = describe(G, scene_tmp, case)
    lo, hi = case.get("rows", (0, case["film"][1]))
    sc = G.Scene(sd)
    try:
        base, st, route = render_with_stats(G, sc, case)
        # (a) the knobs that select another kernel, each with its counters; then the launch paths of the product (enqueue-only, with the
        # kernel on a render stream and with everything on the caller's stream)
        routes = {route}
        for knobs in KNOBS:
            other, ost, oroute = render_with_stats(G, sc, case, **knobs)
            routes.add(oroute)
            assert_bits(other, base, knobs)
            for c in COUNTERS:
                assert getattr(ost, c) == getattr(st, c), (knobs, c, getattr(ost, c), getattr(st, c))
        if case["scene"] == CBOX and not case.get("tile"):
            assert route == "lambert_plain/lds_const" and len(routes) >= 3, routes          # the knobs really chose other kernels
    finally:
        sc.close()
    assert_bits(enqueue_only(G, sd, case), base, "enqueue-only")
    assert_bits(enqueue_only(G, sd, case, no_render_overlap=1), base, "no_render_overlap")
    assert st.samples == case["film"][0] * (hi - lo) * case["spp"] and st.rays > 0
    # (b) the oracle renders the whole film; a band equals those rows of it
    want, wst = O.OracleScene(sd.ptr, use_bvh=case["scene"] != CBOX).render(case["spp"], scheme(G, case), threads=8)
    for k in BUFS:
        err = rel_l2(base[k][lo:hi], want[k][lo:hi])
        print(case["id"], k, "rel L2 against the oracle", err)
        assert np.isfinite(base[k]).all() and err < TOL, f"{k}: rel L2 {err}"
    if "rows" not in case:
        assert st.bounces == wst.bounces and st.nonfinite_samples == wst.nonfinite_samples
    if case["scene"] == DISNEY:
        if case.get("count_breaks"):
            broke = samples_that_broke_at_bounce_1(G, O, sd, case)
            print(case["id"], "samples that left the loop at p2 <= 0 in bounce 1:", broke)
            assert broke >= 1
        assert any(np.abs(base[k]).max() > 0 for k in BUFS[1:])
    else:
        assert np.abs(base["img"]).max() > 0 and np.abs(base["cx0"]).max() > 0 and np.abs(base["cy1"]).max() > 0
    # (c) the commit before the change, on the same shapes
    got = digest(base, st)
    assert got == record["cases"][case["id"]], (got, record["cases"][case["id"]])


def main(argv):
    """--record <libgdpt.so> <out.json>: the record of (c), made with another build of the library (the commit before the change)."""
    if len(argv) != 4 or argv[1] != "--record":
        sys.exit(main.__doc__)
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import gdpt_amd as G
    G.LIB_PATH = os.path.abspath(argv[2])
    out = {"what": "sha1 of the five buffers and the counters of tests/test_gpu_shared_arms.py's cases, rendered by the library of the parent commit",
           "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            sc = G.Scene(describe(G, tmp, case))
            bufs, st, route = render_with_stats(G, sc, case)
            sc.close()
            out["cases"][case["id"]] = digest(bufs, st)
            print(case["id"], route, out["cases"][case["id"]], flush=True)
    with open(argv[3], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv)
