"""The render kernels and the Poisson solvers against the reference's own output, with no oracle in between.

tests/golden/ref_samples_<case>.npz hold 40x24 films that the reference's unmodified grad_path_tracing / path_tracing produced in
render.cpp's tile order (one init_pcg32(tile) stream per tile; oracle/ref_samples.cpp, oracle/ref_cases.py), and
tests/golden/ref_fourier.npz its fourierSolve. Here Scene.render(spp, RNG_TILE) / Scene.path_render(spp, RNG_TILE) run on the same
variant XMLs (written into the test's own folder by the helper the generator used) and G.fourierSolve on the same LCG fields.

Compared: all five buffers where the offset fields are a function of the reference's source (max_depth <= 2), `img`
alone otherwise, and the Path image: relative L2 per buffer, the sets of non-finite pixels identical. A pixel whose recorded margin
is below 1e-6, or which the fixture marks `undefined` (the reference reads memory out of range there), is compared for
finiteness only (at most 2 % of a film; the pixels are printed). Each case first asserts the kernel
route (or the solver) it reached, prints the share of pixels at which each compared buffer of the reference is not zero, and asserts
that ref_cases.EMPTY_FILMS lists exactly the films that compare nothing but zeros ("What the films hold").

Bounds: MEASURED holds the worst figure per tolerance class as measured on an MI355X; the bound is 16 times it, never looser than
the class's tolerance in tests/test_gpu_route_matrix.py and never under 16 ulp of a double. While an entry is None the test fails
and names its figure.
"""
import os

import numpy as np
import pytest

import ref_cases as RC
from helpers import ROOT, rel_l2, scene_variant
from test_oracle_vs_reference_samples import film_figure
from test_poisson_oracle import lcg_fields

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")

# worst figure per (class, what) on an MI355X (None: not recorded yet): lambert at grad_cbox_d2_rr1 (grad_small_pt, five buffers,
# 1.0e-16), general at path_sponza (five buffers: grad_disney_metal_d2 5.6e-16, grad_sponza_d2 1.2e-16), envmap at path_disney_glass;
# the direct solvers at 64x48, CG at 8x6. Every case's figure: DESIGN §6. The films of ref_cases.EMPTY_FILMS compare zeros only.
MEASURED = {
    ("lambert", "film"): 1.613e-16, ("general", "film"): 6.287e-15, ("envmap", "film"): 4.592e-14,
    ("fourier", "dct"): 1.602e-15, ("fourier", "dct_mfma"): 1.482e-15, ("fourier", "cg"): 1.364e-08,
}
ULP16 = 16 * 2.220446049250313e-16
# the CG solver stops at its own tolerance and solves without the reference's fp32 eigenvalue (include/gdpt.h: ~3e-9); its cap is the
# bound tests/test_gpu_poisson_and_pipeline.py holds it to
CAPS = dict(RC.CLASS_TOLERANCE, fourier=1e-9)
CG_CAP = 1e-6

# the kernel each case is meant to run (include/gdpt_debug.h: route names)
EXPECTED_ROUTE = {
    "grad_cbox": "tile_phases_lambert", "grad_cbox_d1_rr5": "tile_phases_lambert", "grad_cbox_d2_rr5": "tile_phases_lambert",
    "grad_cbox_d2_rr1": "tile_phases_lambert", "grad_cbox_dinf_rr1": "tile_phases_lambert", "grad_small_pt": "tile_phases_lambert",
    "grad_disney_metal": "tile_phases_general", "grad_disney_metal_d2": "tile_phases_general",
    "grad_sponza": "tile_phases_lambert", "grad_sponza_d2": "tile_phases_lambert",
    "path_cbox": "path/tile", "path_small_pt": "path/tile", "path_veach_mi": "path/tile", "path_disney_diffuse": "path/tile",
    "path_disney_glass": "path/tile", "path_matpreview": "path/tile", "path_sponza": "path/tile",
}


def check(figure, klass, what, where="", cap=None):
    m = MEASURED[(klass, what)]
    cap = CAPS[klass] if cap is None else cap
    b = None if m is None else min(max(16 * m, ULP16), cap)
    print(f"  FIGURE {klass}/{what} {where}: {figure:.3e} (bound {b})")
    assert b is not None, f"MEASURED[{(klass, what)!r}] has not been recorded; this run measured {figure:.3e} {where}"
    assert figure <= b, f"{klass}/{what} {where}: {figure:.3e} > {b:.3e}"


@pytest.mark.parametrize("case", RC.CASES, ids=[c.name for c in RC.CASES])
def test_film_against_the_reference(G, tmp_path, case):
    with np.load(os.path.join(GOLDEN, f"ref_samples_{case.name}.npz")) as d:
        want, margin, undefined = d["film"], d["film_margin"], d["film_undefined"]
    grad = case.integrator == "gradpath"
    sd = G.parse_scene(RC.variant_xml(scene_variant, tmp_path, case, film=RC.FILM))
    assert (sd.width, sd.height) == RC.FILM
    if grad:
        assert case.offsets == (sd.ptr.contents.max_depth in (1, 2)), (case.name, sd.ptr.contents.max_depth)
    sc = G.Scene(sd)
    try:
        if grad:
            bufs, _ = sc.render(case.film_spp, G.RNG_TILE)
            got = np.stack([bufs[k] for k in RC.FILM_BUFFERS])
        else:
            got = sc.path_render(case.film_spp, G.RNG_TILE)[0][None]
        route = G.debug_knobs.last_route()
    finally:
        sc.close()
    print(f"  ROUTE {case.name}: {route}")
    assert route == EXPECTED_ROUTE[case.name], route
    assert got.shape == want.shape
    ill = (margin < RC.MARGIN_THRESHOLD) | undefined
    print(f"  {case.name}: {int(ill.sum())} of {ill.size} pixels below margin {RC.MARGIN_THRESHOLD:g} or undefined "
          f"({np.argwhere(undefined).tolist()}): {np.argwhere(ill).tolist()}")
    assert ill.mean() <= RC.MARGIN_CAP
    names = RC.FILM_BUFFERS if (grad and case.offsets) else ("img",)
    worst, shares = film_figure(got, want, ill, names)
    print(f"  {case.name}: non-zero pixels of the reference's buffers: {shares}")
    assert (max(shares.values()) > 0) == (case.name not in RC.EMPTY_FILMS), shares
    check(worst, case.klass, "film", f"({case.name})")


@pytest.mark.parametrize("solver", ["dct", "dct_mfma", "cg"])
@pytest.mark.parametrize("w,h,alpha", RC.FOURIER_CASES, ids=[RC.fourier_key(*c) for c in RC.FOURIER_CASES])
def test_fourier_solve_against_the_reference(G, w, h, alpha, solver):
    with np.load(os.path.join(GOLDEN, "ref_fourier.npz")) as d:
        want = d[RC.fourier_key(w, h, alpha)]
    c, gx, gy = lcg_fields(w, h)
    which = {"dct": G.SOLVER_DCT, "dct_mfma": G.SOLVER_DCT_MFMA, "cg": G.SOLVER_CG}[solver]
    out, st = G.fourierSolve(w, h, c, gx, gy, alpha, solver=which, return_stats=True)
    assert st.solver == which, (st.solver, which)
    if solver == "cg":
        assert st.iterations > 0
    elif solver == "dct_mfma":
        assert G.debug_knobs.last_dct_shape() != ""
    check(rel_l2(out, want), "fourier", solver, f"({w}x{h}, alpha {alpha:g})", cap=CG_CAP if solver == "cg" else None)
