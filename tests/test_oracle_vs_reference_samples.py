"""The CPU oracle against the reference's own integrators, sample by sample (no GPU).

tests/golden/ref_samples_<case>.npz hold what the reference's unmodified grad_path_tracing and path_tracing returned, linked against a
brute-force stand-in for the Embree library that shares oracle/brute_hit.h with the oracle (oracle/ref_samples.cpp, rtc_standin.cpp;
the cases are oracle/ref_cases.py): (a) scattered samples, sample i on pixel (37 i mod W, 91 i mod H) of the scene's own film with
init_pcg32(offset + i): every field of the record, the PCG state after the call, and `margin`; (b) a 40x24 film in render.cpp's
tile order, one init_pcg32(tile) stream per tile. tests/golden/ref_fourier.npz holds the reference's fourierSolve on top of a
long-double DCT-I (oracle/dct_standin.cpp). This module runs the oracle on the same inputs. Regenerate with
`make -C oracle ref_samples && python oracle/gen_golden.py samples` (needs the reference tree; byte for byte reproducible).

Conditioning, from the reference's record alone: a sample whose margin (the smallest distance of any of its rays' answers from
changing: barycentric distance from an edge, relative gap in t to the runner-up or to an end of the ray's interval, angular distance
from a sphere's silhouette) is below MARGIN_THRESHOLD = 1e-6 keeps only the finiteness check; at most 2 % of a scene's samples, or of
a film's pixels, may be such. Recorded: no sample on 15 cases, 3 of 1024 on path_veach_mi, 3 of 256 on path_sponza; film pixels
3 (grad_cbox), 1 (grad_cbox_d1_rr5, grad_cbox_dinf_rr1, path_veach_mi, grad_sponza_d2), 3 (path_sponza), of 960. One more kind of sample is kept out
the same way and counts towards the same cap: `undefined`, where the reference reads memory out of range (make_mipmap on a
one-texel-high level, src/mipmap.h:33-43) and the generator, run twice with different padding behind every allocation,
got two answers: 1 pixel each of the path_sponza and grad_sponza_d2 films.

On every kept sample: the PCG state after the sample is equal (the number of draws, and with it the control flow: 2 + 3 a bounce +
1 a roulette test), prob > 0 and the discrete state of each offset (w == 0, w == 1, contrib == 0) are equal, and the continuous
fields hold |got - want| / max(1, |want|). What the unmodified reference is authoritative for: radiance, contrib, prob and the state
at every depth; the offset fields only where the bounce loop runs at most once (max_depth <= 2: path_tracing.h:1007-1010 read empty
optionals at the end of an iteration that is followed by another); all of Integrator::Path.

What a film holds: each film test prints the share of pixels at which every compared buffer of the reference is not zero, and asserts
that ref_cases.EMPTY_FILMS lists exactly the films that compare nothing but zeros ("What the films hold").

Bounds: nothing here is derivable in advance, so MEASURED holds the worst figure per tolerance class against the golden, and the bound
is 16 times it, never looser than the class's tolerance in tests/test_gpu_route_matrix.py (1e-9 Lambertian, 1e-7 with transcendentals
or textures, 1e-6 with an environment map) and never under 16 ulp of a double (a figure of a few ulp moves with the C library's
transcendentals). While an entry is None the test fails and names its figure.
"""
import os

import numpy as np
import pytest

import ref_cases as RC
from helpers import ROOT, rel_l2, scene_variant
from test_poisson_oracle import lcg_fields

GOLDEN = os.path.join(ROOT, "tests", "golden")

# worst figure per (class, what) over the cases of that class, this module against the golden (None: not recorded yet)
# the renders: 0 on all 17 cases, samples and films alike (the oracle returns the reference's bits)
MEASURED = {
    ("lambert", "samples"): 0.0, ("lambert", "film"): 0.0,
    ("general", "samples"): 0.0, ("general", "film"): 0.0,
    ("envmap", "samples"): 0.0, ("envmap", "film"): 0.0,
    ("fourier", "scipy"): 1.498e-15, ("fourier", "c"): 7.686e-16,      # worst at 64x48 and at 40x30 with alpha 40
}
ULP16 = 16 * 2.220446049250313e-16


def bound_of(klass, what):
    m = MEASURED[(klass, what)]
    if m is None:
        return None
    cap = RC.CLASS_TOLERANCE.get(klass, 1e-9)
    return min(max(16 * m, ULP16), cap)


def check(figure, klass, what, where=""):
    b = bound_of(klass, what)
    print(f"  FIGURE {klass}/{what} {where}: {figure:.3e} (bound {b})")
    assert b is not None, f"MEASURED[{(klass, what)!r}] has not been recorded; this run measured {figure:.3e} {where}"
    assert figure <= b, f"{klass}/{what} {where}: {figure:.3e} > {b:.3e}"


def err(got, want):
    """|got - want| / max(1, |want|), the largest over the trailing axis; a value that is not finite on one side only counts as infinite."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both_bad = ~np.isfinite(got) & ~np.isfinite(want)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    e = np.where(both_bad, 0.0, np.where(np.isfinite(e), e, np.inf))
    return e.max(axis=-1) if e.ndim > 1 else e


@pytest.fixture(scope="module")
def fixtures():
    cache = {}

    def get(name):
        if name not in cache:
            with np.load(os.path.join(GOLDEN, f"ref_samples_{name}.npz")) as d:
                cache[name] = {k: d[k] for k in d.files}
        return cache[name]
    return get


def oracle_scene(G, O, tmp, case, film=None):
    xml = RC.variant_xml(scene_variant, tmp, case, film=film)
    sd = G.parse_scene(xml)
    d = sd.ptr.contents
    if film:
        assert (d.camera.width, d.camera.height) == film
    if case.integrator == "gradpath":       # the flag of oracle/ref_cases.py is the parsed depth's, not an opinion
        assert case.offsets == (d.max_depth in (1, 2)), (case.name, d.max_depth)
    ntri = sum(d.shapes[i].num_triangles for i in range(d.num_shapes))
    return sd, O.OracleScene(sd.ptr, use_bvh=ntri > 5000)       # brute force is the definition; the BVH returns the same hit


def grad_row(rec):
    return np.array(list(rec.radiance) + list(rec.contrib) + list(rec.contribX0) + list(rec.contribX1) + list(rec.contribY0)
                    + list(rec.contribY1) + [rec.prob, rec.wX0, rec.wY0, rec.wX1, rec.wY1])


@pytest.mark.parametrize("case", RC.CASES, ids=[c.name for c in RC.CASES])
def test_samples_against_the_reference(G, O, scene_tmp, fixtures, case):
    fx = fixtures(case.name)
    grad = case.integrator == "gradpath"
    sd, sc = oracle_scene(G, O, scene_tmp, case)
    n = case.count
    assert fx["record"].shape == (n, 23 if grad else 3)
    got = np.zeros_like(fx["record"])
    state = np.zeros(n, dtype=np.uint64)
    for i, (x, y, stream) in enumerate(fx["xy_stream"]):
        assert (int(x), int(y), int(stream)) == ((37 * i) % sc.width, (91 * i) % sc.height, case.stream_offset + i)
        s0, inc = O.pcg_init(int(stream))
        if grad:
            rec, s1 = sc.grad_sample(int(x), int(y), s0, inc)
            got[i] = grad_row(rec)
        else:
            got[i], s1 = sc.path_sample(int(x), int(y), s0, inc)[:2]
        state[i] = s1
    sc.close()
    want = fx["record"]
    ill = (fx["margin"] < RC.MARGIN_THRESHOLD) | fx["undefined"]
    print(f"  {case.name}: {int(ill.sum())} of {n} samples below margin {RC.MARGIN_THRESHOLD:g} or undefined ({int(fx['undefined'].sum())})")
    assert ill.mean() <= RC.MARGIN_CAP
    # ill-conditioned samples: finiteness only
    assert (np.isfinite(got[ill]) == np.isfinite(want[ill])).all()
    keep = ~ill
    # the draw count, i.e. the whole control flow
    bad = np.flatnonzero(keep & (state != fx["state"]))
    assert bad.size == 0, f"PCG state after the sample differs on {bad.size} samples, first {bad[:8]}"
    cols = slice(0, 3)
    if grad:
        assert ((got[keep, 18] > 0) == (want[keep, 18] > 0)).all(), "prob > 0 differs"
        if case.offsets:
            for k, (c0, wcol) in enumerate(((6, 19), (9, 21), (12, 20), (15, 22))):       # X0, X1, Y0, Y1 with wX0 wY0 wX1 wY1 at 19..22
                for pred in (lambda a: a[:, wcol] == 0, lambda a: a[:, wcol] == 1, lambda a: (a[:, c0:c0 + 3] == 0).all(axis=1)):
                    bad = np.flatnonzero(keep & (pred(got) != pred(want)))
                    assert bad.size == 0, f"offset {k}: validity differs on {bad.size} samples, first {bad[:8]}"
            cols = slice(0, 23)
        else:
            cols = np.r_[0:6, 18]
    print(f"  {case.name}: samples with non-zero radiance {float((want[:, 0:3] != 0).any(axis=1).mean()):.4f}"
          + (f", with non-zero contrib {float((want[:, 3:6] != 0).any(axis=1).mean()):.4f}" if grad else ""))
    e = err(got[keep][:, cols], want[keep][:, cols])
    worst = int(np.argmax(e))
    check(float(e.max()), case.klass, "samples", f"({case.name}, sample {np.flatnonzero(keep)[worst]})")


def film_figure(got, want, ill, names):
    """Worst relative L2 over the named buffers outside the pixels `ill` (those: finiteness only; the sets of non-finite pixels must
    be identical everywhere), and the share of pixels at which the reference's buffer is not zero, per buffer: a buffer of zeros
    compares nothing but zeros."""
    worst, shares = 0.0, {}
    for k, name in enumerate(names):
        g, w = got[k].copy(), want[k].copy()
        assert (np.isfinite(g) == np.isfinite(w)).all(), f"{name}: the sets of non-finite pixels differ"
        g[ill] = 0.0
        w[ill] = 0.0
        fin = np.isfinite(w)
        worst = max(worst, rel_l2(np.where(fin, g, 0.0), np.where(fin, w, 0.0)))
        shares[name] = round(float((w != 0).any(axis=-1).mean()), 4)
    return worst, shares


@pytest.mark.parametrize("case", RC.CASES, ids=[c.name for c in RC.CASES])
def test_film_against_the_reference(G, O, scene_tmp, fixtures, case):
    fx = fixtures(case.name)
    grad = case.integrator == "gradpath"
    sd, sc = oracle_scene(G, O, scene_tmp, case, film=RC.FILM)
    if grad:
        bufs, _ = sc.render(case.film_spp, G.RNG_TILE, threads=4)
        got = np.stack([bufs[k] for k in RC.FILM_BUFFERS])
    else:
        got = sc.path_render(case.film_spp, G.RNG_TILE, threads=4)[0][None]
    sc.close()
    want = fx["film"]
    assert got.shape == want.shape
    ill = (fx["film_margin"] < RC.MARGIN_THRESHOLD) | fx["film_undefined"]
    print(f"  {case.name}: {int(ill.sum())} of {ill.size} pixels below margin {RC.MARGIN_THRESHOLD:g} or undefined "
          f"({np.argwhere(fx['film_undefined']).tolist()}): {np.argwhere(ill).tolist()}")
    assert ill.mean() <= RC.MARGIN_CAP
    names = RC.FILM_BUFFERS if (grad and case.offsets) else ("img",)
    worst, shares = film_figure(got, want, ill, names)
    print(f"  {case.name}: non-zero pixels of the reference's buffers: {shares}")
    assert (max(shares.values()) > 0) == (case.name not in RC.EMPTY_FILMS), shares
    check(worst, case.klass, "film", f"({case.name})")


# ---- fourierSolve --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_fourier():
    with np.load(os.path.join(GOLDEN, "ref_fourier.npz")) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("w,h,alpha", RC.FOURIER_CASES, ids=[RC.fourier_key(*c) for c in RC.FOURIER_CASES])
def test_fourier_solve_against_the_reference(O, ref_fourier, w, h, alpha):
    want = ref_fourier[RC.fourier_key(w, h, alpha)]
    c, gx, gy = lcg_fields(w, h)
    figures = (("scipy", rel_l2(O.fourier_solve(c, gx, gy, alpha, float_lambda=True), want)), ("c", rel_l2(O.poisson_dct_c(c, gx, gy, alpha), want)))
    for what, figure in figures:
        print(f"  FIGURE fourier/{what} ({w}x{h}, alpha {alpha:g}): {figure:.3e}")
    for what, figure in figures:
        check(figure, "fourier", what, f"({w}x{h}, alpha {alpha:g})")


def test_the_scipy_made_poisson_fixture_agrees_with_the_reference(ref_fourier):
    with np.load(os.path.join(GOLDEN, "poisson_64x48.npz")) as d:
        c, gx, gy = lcg_fields(64, 48)
        assert float(d["alpha"]) == 0.04
        assert np.array_equal(d["c"], c) and np.array_equal(d["gx"], gx) and np.array_equal(d["gy"], gy)
        check(rel_l2(d["out"], ref_fourier[RC.fourier_key(64, 48, 0.04)]), "fourier", "scipy", "(poisson_64x48.npz)")
