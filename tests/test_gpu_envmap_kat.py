"""The environment-map code under the Path kernels, case by case on the GPU (include/gdpt_debug.h: gdpt_debug_kat_envmap).

The family "envmap" of csrc/hip/debug_kat.hip calls upper_bound_index, table2d_sample, table2d_pdf, envmap_uv, envmap_emission,
envmap_sample_dir and envmap_pdf of csrc/hip/render_path.h as they are, one thread per case. Each test is one scene of
tests/envmap_cases.py (one upload, one launch) and compares with the CPU oracle, whose TableDist2D is pinned to the reference's own
code by tests/golden/ref_kat.json ("table2d"):
  - the four prepared tables with the oracle's, bit for bit, through the digests of gdpt_debug_prepare_scene (CPU, no launch);
  - sample_uv bit for bit on every random-number case, the ones on a CDF value and one ulp either side included (table2d_sample has
    no transcendental and no product-sum, so equal tables leave no room);
  - every output finite, on every case;
  - the discrete outcomes exactly: zero / non-zero pdf and the texel of table2d_pdf that dir_uv selects, on every direction case that
    tests/golden/envmap_kat_edges_dropped.json does not list under "all"; zero / non-zero sample_pdf likewise ("sample_all");
  - the continuous outputs under BOUNDS with the error measure |got - want| / max(1, |want|), each on the cases that keep that
    comparison (tests/envmap_cases.py: the conditioning rules); what the rules take out is reported with its measured figure.

Bounds: the starting bounds are 1e-11 for sample_dir, sample_pdf, dir_pdf and dir_uv (the light family's) and 1e-12 for both
emissions (the texture family's); a starting bound stays where the worst figure measured on an MI355X is at least four times under
it, otherwise the bound is sixteen times that figure, never above 1e-9. MEASURED holds the worst figure of each quantity over all
scenes as measured on an MI355X; while an entry is None the tests fail and name the figure they measured. Measured, worst over the 14
scenes: sample_dir 4.0e-16 (1x2/rotated), sample_pdf 1.2e-13 (1x2/identity), sample_emission 3.4e-14 (matpreview), dir_uv 3.5e-13
(every rotated scene), dir_pdf 4.5e-13 (64x32/rotated), dir_emission 6.6e-14 (6x4/rotated): each at least 15 times under its starting
bound, so all six stay. Reported, not bounded (the cases the rules take out, 80 .. 2090 a quantity): up to 3.5e6 for the two pdfs (a
pdf of 1e8 beside a pole against 0), 1 for dir_uv (the seam), 27 and 1.1 for the emissions. sample_uv: equal bits on all 5002 cases.
Each test prints its figures; DESIGN.md 6 has the table per scene class, and what six builds with a planted defect did to this module.
"""
import os
import sys

import numpy as np
import pytest

import envmap_cases as E
from helpers import ROOT

# worst figure per quantity over the 14 scenes, measured on an MI355X (None: not recorded yet)
MEASURED = {"sample_dir": 3.952e-16, "sample_pdf": 1.173e-13, "sample_emission": 3.423e-14, "dir_uv": 3.534e-13, "dir_pdf": 4.471e-13,
            "dir_emission": 6.628e-14}


def bound_of(quantity):
    start, m = E.START_BOUNDS[quantity], MEASURED[quantity]
    if m is None:
        return None
    return start if 4 * m <= start else min(16 * m, 1e-9)


BOUNDS = {q: bound_of(q) for q in MEASURED}


def err(got, want):
    """|got - want| / max(1, |want|) per case (the largest over a case's components); a value that is not finite counts as infinite."""
    got, want = np.asarray(got, dtype=np.float64).reshape(len(got), -1), np.asarray(want, dtype=np.float64).reshape(len(want), -1)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    return np.where(np.isfinite(e), e, np.inf).max(axis=1)


def fnv1a64(a):
    """The digest gdpt_debug_prepare_scene gives for a table of these doubles."""
    h = 0xcbf29ce484222325
    for byte in np.ascontiguousarray(a, dtype="<f8").tobytes():
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def run(G, scene, cases):
    query, result = G.KAT_STRUCTS["envmap"]
    q = np.zeros(len(cases["id"]), dtype=np.dtype(query))
    q["rnd"], q["dir"] = cases["rnd"], cases["dir"]
    out = G.debug_knobs.kat(scene, "envmap", 0, (query * len(q)).from_buffer(q))
    return np.frombuffer(out, dtype=np.dtype(result), count=len(q)).copy()


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("envmap_kat")


@pytest.mark.parametrize("scene", E.SCENE_NAMES)
def test_prepared_tables_equal_the_oracles(G, O, tmp, scene):
    """CPU: cdf_rows, pdf_rows, cdf_marginals and pdf_marginals of the host half of an upload (csrc/host/scene_prepare.cpp:
    build_envmap) against the oracle's make_table_2d, by size and by digest."""
    wd = E.World(G, O, tmp, scene)
    info = G.debug_knobs.prepare_scene(wd.sd)
    assert info["has_envmap"] == 1 and (info["env_w"], info["env_h"]) == (wd.w, wd.h)
    for name, table in wd.tables.items():
        assert info["count"]["env_" + name] == table.size, name
        assert info["digest"]["env_" + name] == fnv1a64(table), f"{wd.name}: env_{name} differs from the oracle's table"


@pytest.mark.gpu
@pytest.mark.parametrize("scene", E.SCENE_NAMES)
def test_envmap_cases_against_the_oracle(G, O, tmp, scene):
    wd = E.World(G, O, tmp, scene)
    c = wd.cases
    keep, sample_keep, ok = E.masks(c, E.load_dropped()[scene])
    want = dict(E.oracle_rnd(wd.osc, c["rnd"]), **E.oracle_dir(wd.osc, c["dir"]))
    sc = G.Scene(wd.sd)
    try:
        r = run(G, sc, c)
    finally:
        sc.close()
    is_rnd, is_dir = ~c["is_dir"], c["is_dir"]
    failed = []
    # ---- every output finite, on every case
    for f in r.dtype.names:
        bad = np.flatnonzero(~np.isfinite(r[f].reshape(len(r), -1)).all(axis=1))
        if bad.size:
            failed.append(f"{f} is not finite on {bad.size} cases, first {[c['id'][i] for i in bad[:4]]}")
    # ---- table sampling, bit for bit
    diff = np.flatnonzero(is_rnd & (r["sample_uv"].view(np.uint64) != np.ascontiguousarray(want["sample_uv"]).view(np.uint64)).any(axis=1))
    if diff.size:
        i = diff[0]
        failed.append(f"sample_uv differs in bits on {diff.size} of {int(is_rnd.sum())} cases, first {c['id'][i]}: rnd {c['rnd'][i].tolist()!r} got {r['sample_uv'][i].tolist()!r} want {want['sample_uv'][i].tolist()!r}")
    # ---- discrete outcomes
    zero = np.flatnonzero(keep & ((r["dir_pdf"] != 0) != (want["dir_pdf"] != 0)))
    if zero.size:
        failed.append(f"dir_pdf is zero on one side only on {zero.size} cases, first {[c['id'][i] for i in zero[:4]]}")
    texel = np.flatnonzero(keep & (E.texel_of(r["dir_uv"], wd.w, wd.h) != E.texel_of(want["dir_uv"], wd.w, wd.h)).any(axis=1))
    if texel.size:
        i = texel[0]
        failed.append(f"dir_uv selects another texel on {texel.size} cases, first {c['id'][i]}: got uv {r['dir_uv'][i].tolist()!r} want {want['dir_uv'][i].tolist()!r}")
    zero = np.flatnonzero(sample_keep & ((r["sample_pdf"] != 0) != (want["sample_pdf"] != 0)))
    if zero.size:
        failed.append(f"sample_pdf is zero on one side only on {zero.size} cases, first {[c['id'][i] for i in zero[:4]]}")
    # ---- continuous outputs
    which = {"sample_dir": is_rnd, "sample_pdf": ok["sample_pdf"], "sample_emission": ok["sample_emission"],
             "dir_uv": ok["dir_uv"], "dir_pdf": ok["dir_pdf"], "dir_emission": ok["dir_emission"]}
    whole = {"sample_dir": is_rnd, "sample_pdf": is_rnd, "sample_emission": is_rnd, "dir_uv": is_dir, "dir_pdf": is_dir, "dir_emission": is_dir}
    figures = {}
    for q, on in which.items():
        e = err(r[q], want[q])
        worst = float(e[on].max(initial=0.0))
        out = whole[q] & ~on
        figures[q] = worst
        where = c["id"][int(np.argmax(np.where(on, e, -1.0)))] if on.any() else "-"
        print(f"  {scene}: {q}: worst {worst:.3e} on {int(on.sum())} cases (at {where}), bound {BOUNDS[q]}; "
              f"reported, not bounded: {int(out.sum())} ill-conditioned cases, worst {float(e[out].max(initial=0.0)):.3e}")
        if BOUNDS[q] is None:
            failed.append(f"MEASURED['{q}'] has not been recorded; this run measured {worst:.3e}")
        elif not worst <= BOUNDS[q]:
            failed.append(f"{q}: {worst:.3e} > {BOUNDS[q]:.1e} at {where}")
    print("  FIGURES", scene, " ".join(f"{q}={v:.3e}" for q, v in figures.items()))
    assert not failed, "\n".join(failed)


@pytest.mark.gpu
def test_envmap_family_refuses_bad_arguments(G, O, tmp):
    """Refused on the host, before any launch: a scene without an environment map, a number that is not finite, a random number outside
    [0, 1], a zero direction, n above the family's cap; the light family still refuses the environment map's placeholder."""
    from helpers import Built, DescBuilder
    query, _ = G.KAT_STRUCTS["envmap"]
    one = np.zeros(1, dtype=np.dtype(query))
    one["rnd"], one["dir"] = [0.5, 0.5], [0.0, 1.0, 0.0]
    call = lambda sc, q, variant=0: G.debug_knobs.kat(sc, "envmap", variant, (query * len(q)).from_buffer(np.ascontiguousarray(q)))
    b = DescBuilder(G)
    plain = G.Scene(Built(b.finish(), 16, 16, b))
    with pytest.raises(G.GdptError, match="no environment map"):
        call(plain, one)
    plain.close()
    wd = E.World(G, O, tmp, "2x1/rotated")
    sc = G.Scene(wd.sd)
    try:
        assert len(call(sc, one)) == 1
        for field, k, value, text in (("rnd", 0, np.nan, "not finite"), ("dir", 2, np.inf, "not finite"), ("rnd", 1, 1.5, r"outside \[0, 1\]"),
                                      ("rnd", 0, -1e-300, r"outside \[0, 1\]")):
            bad = one.copy()
            bad[field][0, k] = value
            with pytest.raises(G.GdptError, match=text):
                call(sc, bad)
        bad = one.copy()
        bad["dir"] = 0.0
        with pytest.raises(G.GdptError, match="dir is zero"):
            call(sc, bad)
        with pytest.raises(G.GdptError, match="variant"):
            call(sc, one, variant=1)
        assert G.lib().gdpt_debug_kat_envmap(sc.handle, 0, (1 << 20) + 1, (query * 1).from_buffer(one.copy()), (G.KAT_STRUCTS["envmap"][1] * 1)()) != 0
        assert "n must be in [0, 1048576]" in G.lib().gdpt_last_error().decode()
        lq = np.zeros(1, dtype=np.dtype(G.KAT_STRUCTS["light"][0]))
        with pytest.raises(G.GdptError, match="the environment map is no area emitter"):
            G.debug_knobs.kat(sc, "light", 0, (G.KAT_STRUCTS["light"][0] * 1).from_buffer(lq))
    finally:
        sc.close()
    with pytest.raises(G.GdptError, match=r"unknown family 'env' \(bsdf, texture, filter, primary, shading, light, envmap, trace\)"):
        G.debug_knobs.kat_variants("env")


if __name__ == "__main__" and sys.argv[1:] == ["write-dropped"]:
    import json
    import tempfile
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import gdpt_amd as _G
    import oracle_py as _O
    with tempfile.TemporaryDirectory() as _tmp:
        found = E.find_dropped(_G, _O, _tmp)
    with open(E.DROPPED_FILE, "w") as f:
        json.dump(found, f, indent=0, sort_keys=True)
        f.write("\n")
    for scene, lists in found.items():
        print(scene, {k: len(v) for k, v in lists.items()})
