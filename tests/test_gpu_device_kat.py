"""The device functions under the render kernels, case by case on the GPU (include/gdpt_debug.h: gdpt_debug_kat_*).

Each test runs one family of csrc/hip/debug_kat.hip (the product's device functions, one thread per case) and compares
  (a) with the vectors the reference's own code computed (tests/golden/ref_kat.json): all 720 BSDF cases through every variant of the
      table whose material set admits them, every texture lookup, the 48 filter cases, every ray of the 3 cameras, the 24 + 6
      shading-info cases, the emitter meshes and the sphere;
  (b) the variants with each other, bit for bit: a reduced material set against the full switch, the inline Lambertian with
      kPlainConstTex against the one without;
  (c) with the CPU oracle on a deterministic list of edges the random cases do not reach (edge_bsdf_cases / edge_texture_cases below).

Error measure: |got - want| / max(1, |want|), NaN and Inf compared as NaN and Inf (a NaN where a number is wanted is an error).
Bounds (DESIGN.md 6 has the table; `BOUNDS` below): the ones the oracle is held to against the same vectors, 1e-11 on sampled
directions, 1e-10 on f and pdf, 1e-12 elsewhere; kept where the worst figure measured on an MI355X is at least four times under them,
otherwise sixteen times that figure, never above 1e-9. Measured on an MI355X, worst against the golden vectors / against the oracle
on the edge list: sampled direction 2.7e-15 / 2.1e-13 (bound 1e-11), eta and roughness 1.4e-17 / 1.4e-17 (1e-12), f and pdf, separate
and fused, 1.1e-12 / 6.0e-13 (1e-10), texture 2.6e-17 / 0 (1e-12), filter 1.1e-15, camera ray 2.2e-16, shading info 2.2e-16 (1e-12),
emitter point 6.7e-14, normal 2.7e-14, pdf 7.4e-16 (1e-11): every figure is at least 48 times under its starting bound, so all of
them stay. The fused eval_pdf differed from the separate eval and pdf by 0 in every variant. Each test prints its figures.

Conditioning. The kernels contract multiplications and additions into FMAs and call the device library's transcendentals, so their
intermediates sit a few ulps from the oracle's. An evaluation whose wanted value already moves by a tenth of its bound when ONE
component of ONE input direction or of the shading normal moves by ONE ulp (eval_sensitivity / sample_sensitivity below, the oracle alone: the move under one
ulp, and the move under 2^13 ulps scaled back, whichever is larger) cannot be held to
that bound by any code, and is ill-conditioned in the sense of the issue (the oracle's own output moves as much). Such evaluations
are near-singular: a lobe of roughness 0.01 a fraction of its width from the peak (values of 1e6 .. 1e13), or a direction exactly
on the horizon where the reference divides by a cosine that is 0 or 1e-18 depending on the last bit.
  - Golden cases are never dropped: all 720 are compared on validity, the reflect / refract choice, direction, eta and roughness, and
    every eval / pdf is compared unless the oracle shows that one evaluation ill-conditioned (at most 1 % of them, asserted; the
    count is printed and stated in DESIGN.md 6).
  - The edge list keeps a candidate only if the oracle's own answer is stable there: under a move of any one input by one part in 1e12
    its discrete outcome (validity, reflect or refract, which outputs are finite, the lobe of DisneyBSDF) stays and no output moves by
    more than 1e-6, and its sample and both evaluations pass the one-ulp rule above. The candidates that fail are listed by id in
    tests/golden/device_kat_edges_dropped.json (written by `python tests/test_gpu_device_kat.py write-dropped`, on the CPU, with the
    oracle alone); the GPU tests take every candidate that is not in that file and skip none; test_edge_list_is_stable (CPU) repeats
    the check on every kept case, so the list cannot rot.
"""
import json
import math
import os
import sys

import numpy as np
import pytest

from helpers import DescBuilder, ROOT
from test_oracle_vs_reference_kat import _emitter_mesh, _emitter_sphere, _materials, _shading_mesh, _textures, _vertex

DROPPED_FILE = os.path.join(ROOT, "tests", "golden", "device_kat_edges_dropped.json")

# bound per (family, quantity)
BOUNDS = {
    ("bsdf", "dir"): 1e-11, ("bsdf", "eta_rough"): 1e-12, ("bsdf", "f"): 1e-10, ("bsdf", "pdf"): 1e-10,
    ("texture", "value"): 1e-12, ("filter", "offset"): 1e-12, ("primary", "org"): 1e-12, ("primary", "dir"): 1e-12,
    ("shading", "uv"): 1e-12, ("shading", "frame"): 1e-12, ("shading", "inv_uv_size"): 1e-12,
    ("light", "position"): 1e-11, ("light", "normal"): 1e-11, ("light", "pdf"): 1e-11,
}
MEASURED = {}     # filled by the tests: (family, quantity, "golden" | "oracle") -> worst figure of this run (printed by each test)


def err(got, want):
    """|got - want| / max(1, |want|) elementwise; NaN wanted: 0 if NaN came; Inf wanted: 0 if the same Inf came; otherwise inf."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    special = ~np.isfinite(want)
    same = (np.isnan(want) & np.isnan(got)) | (np.isinf(want) & (got == want))
    e = np.where(special, np.where(same, 0.0, np.inf), e)
    return np.where(np.isnan(e), np.inf, e)


def worst(family, quantity, against, got, want):
    e = err(got, want)
    w = float(e.max()) if e.size else 0.0
    key = (family, quantity, against)
    MEASURED[key] = max(MEASURED.get(key, 0.0), w)
    return w


FAILED = []       # bounds missed by the running test: every figure is printed before finish() asserts


def check(family, quantity, against, got, want, what=""):
    w = worst(family, quantity, against, got, want)
    print(f"  {family}.{quantity} vs {against}{' ' + what if what else ''}: worst {w:.3e} (bound {BOUNDS[(family, quantity)]:.0e})")
    if not w <= BOUNDS[(family, quantity)]:
        e = err(got, want)
        i = np.unravel_index(int(np.argmax(e)), e.shape)
        FAILED.append(f"{family}.{quantity} vs {against} {what}: {w:.3e} > {BOUNDS[(family, quantity)]:.0e} at {tuple(int(x) for x in i)}: got {np.asarray(got)[i]!r}, want {np.asarray(want)[i]!r}")


def finish():
    missed = list(FAILED)
    FAILED.clear()
    assert not missed, "\n".join(missed)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class Built:
    """Duck-typed SceneDesc (ptr, width, height) over a DescBuilder."""

    def __init__(self, b):
        self.owner, self.ptr = b, b.finish()
        self.width, self.height = b.desc.camera.width, b.desc.camera.height


def run(G, scene, family, variant, q):
    """q: numpy structured array of the family's query struct -> numpy structured array of results."""
    query, result = G.KAT_STRUCTS[family]
    q = np.ascontiguousarray(q)
    out = G.debug_knobs.kat(scene, family, variant, (query * len(q)).from_buffer(q))
    return np.frombuffer(out, dtype=np.dtype(result), count=len(q)).copy()


def queries(G, family, n):
    return np.zeros(n, dtype=np.dtype(G.KAT_STRUCTS[family][0]))


# ---- the BSDF scene: the 15 materials of the golden file, then the edge list's variants of them -------------------------------------
def edge_materials(G, b):
    """Variants of the golden materials for the edge list: roughness and anisotropy (and the other scalar textures of the single
    lobes) at 0 and 1, eta = 1 + 1e-6. name -> (material id, golden material the cases count for)."""
    ct = lambda v: DescBuilder.const_tex(G, v)
    bc = (0.82, 0.67, 0.16)
    eta1 = 1.0 + 1e-6
    out = {}

    def add(name, base, mtype, texs, eta=1.5):
        out[name] = (b.material(mtype, texs, eta=eta), base)
    for r in (0.0, 1.0):
        add(f"disneydiffuse@rough{r:g}", "disneydiffuse", G.MAT_DISNEY_DIFFUSE, [ct(bc), ct(r), ct(1.0 - r)])
        add(f"disneyclearcoat@gloss{r:g}", "disneyclearcoat", G.MAT_DISNEY_CLEARCOAT, [ct(r)])
        add(f"disneysheen@tint{r:g}", "disneysheen", G.MAT_DISNEY_SHEEN, [ct(bc), ct(r)])
        add(f"roughplastic@rough{r:g}", "roughplastic", G.MAT_ROUGHPLASTIC, [ct((0.6, 0.3, 0.2)), ct((0.9, 0.9, 0.8)), ct(r)], eta=1.49)
        add(f"roughdielectric@rough{r:g}", "roughdielectric", G.MAT_ROUGHDIELECTRIC, [ct((0.95, 0.9, 1.0)), ct((0.8, 0.9, 0.7)), ct(r)], eta=1.5)
        for a in (0.0, 1.0):
            add(f"disneymetal@rough{r:g}aniso{a:g}", "disneymetal", G.MAT_DISNEY_METAL, [ct(bc), ct(r), ct(a)])
            add(f"disneyglass@rough{r:g}aniso{a:g}", "disneyglass", G.MAT_DISNEY_GLASS, [ct(bc), ct(r), ct(a)], eta=1.5)
            add(f"disneybsdf@rough{r:g}aniso{a:g}", "disneybsdf", G.MAT_DISNEY_BSDF,
                [ct(bc)] + [ct(v) for v in (0.5, 0.5, 0.5, 0.5, r, 0.5, a, 0.5, 0.5, 0.5, 0.5)], eta=1.5)
    add("disneyglass@eta1", "disneyglass", G.MAT_DISNEY_GLASS, [ct(bc), ct(0.15), ct(0.3)], eta=eta1)
    add("disneybsdf@eta1", "disneybsdf", G.MAT_DISNEY_BSDF, [ct(bc)] + [ct(v) for v in (0.5, 0.5, 0.5, 0.5, 0.1, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5)], eta=eta1)
    add("roughplastic@eta1", "roughplastic", G.MAT_ROUGHPLASTIC, [ct((0.6, 0.3, 0.2)), ct((0.9, 0.9, 0.8)), ct(0.25)], eta=eta1)
    add("roughdielectric@eta1", "roughdielectric", G.MAT_ROUGHDIELECTRIC, [ct((0.95, 0.9, 1.0)), ct((0.8, 0.9, 0.7)), ct(0.3)], eta=eta1)
    return out


class BsdfWorld:
    """One description holding the golden materials and the edge variants (no geometry: the cases fix none)."""

    def __init__(self, G):
        self.G, self.b = G, DescBuilder(G)
        self.ids = _materials(G, self.b)                                   # golden name -> material id
        self.edge = edge_materials(G, self.b)                              # edge name -> (material id, golden name)
        self.built = Built(self.b)
        self.type_of = [m.type for m in self.b.materials]

    def mid(self, name):
        return self.ids[name] if name in self.ids else self.edge[name][0]

    def base(self, name):
        return name if name in self.ids else self.edge[name][1]

    def admits(self, row, mid):
        """Does the variant's kernel carry the arms of this material? (device_bsdf.h: the dispatch; render_device.h: the inline lobe)"""
        G, t = self.G, self.type_of[mid]
        if row["inline_lambert"]:
            return t == G.MAT_LAMBERTIAN and (not (row["plain"] & 2) or self.b.materials[mid].tex[0].type == G.TEX_CONSTANT)
        if t in (G.MAT_ROUGHPLASTIC, G.MAT_ROUGHDIELECTRIC):
            return row["rough"]
        if t in (G.MAT_DISNEY_GLASS, G.MAT_DISNEY_BSDF) and not row["twosided"]:
            return False
        return bool((row["mask"] >> t) & 1)


def bsdf_queries(G, world, cases):
    q = queries(G, "bsdf", len(cases))
    q["material_id"] = [world.mid(c["mat"]) for c in cases]
    for field, key in (("gn", "gn"), ("fx", "fx"), ("fy", "fy"), ("fn", "fn"), ("uv", "uv")):
        q["vertex"][field] = [c[key] for c in cases]
    q["vertex"]["uv_screen_size"] = [c["uvss"] for c in cases]
    for field in ("dir_in", "dir_out2", "ruv", "rw"):
        q[field] = [c[field] for c in cases]
    return q


def bsdf_expected(cases):
    """Expected arrays from cases in the golden file's format (edge cases carry the oracle's answers under the same keys)."""
    n = len(cases)
    nan3 = [math.nan] * 3
    return {
        "valid": np.array([c["sample_valid"] for c in cases], dtype=np.int32),
        "s_dir": np.array([c.get("s_dir", nan3) for c in cases]).reshape(n, 3),
        "s_eta_rough": np.array([[c.get("s_eta", math.nan), c.get("s_rough", math.nan)] for c in cases]).reshape(n, 2),
        "s_f": np.array([c.get("s_f", nan3) for c in cases]).reshape(n, 3), "s_pdf": np.array([c.get("s_pdf", math.nan) for c in cases]),
        "f2": np.array([c["f2"] for c in cases]).reshape(n, 3), "pdf2": np.array([c["pdf2"] for c in cases]),
    }


def compare_bsdf(r, at_s, want, row, against, what, ok_s=None, ok_2=None):
    """Validity exactly; then direction, eta, roughness; separate eval / pdf; fused eval_pdf. `r`: the cases as they are; `at_s`: the
    same cases with dir_out2 replaced by the WANTED sampled direction, so that eval and pdf "at the sampled direction" are compared
    on the same direction bits as the reference evaluated (as the oracle's own test does), not on a direction one rounding away.
    (What the kernel evaluated at the direction it sampled itself takes part in the bit-for-bit comparison of the variants.)
    ok_s / ok_2 (golden cases): False where the oracle shows the evaluation at the sampled direction / at dir_out2 ill-conditioned.
    Returns the largest fused-separate gap."""
    n = len(want["valid"])
    ok_s = np.ones(n, dtype=bool) if ok_s is None else ok_s
    ok_2 = np.ones(n, dtype=bool) if ok_2 is None else ok_2
    bad = np.flatnonzero(r["sample_valid"] != want["valid"])
    assert bad.size == 0, f"{what}: sample validity differs at cases {bad[:8].tolist()} (got {r['sample_valid'][bad[:8]].tolist()})"
    v = want["valid"] == 1
    # reflect or refract is a choice, not a number: eta is 0 for a reflection and the medium's ratio for a refraction
    choice = (r["s_eta"][v] != 0) == (want["s_eta_rough"][v, 0] != 0)
    assert choice.all(), f"{what}: reflect / refract choice differs at {np.flatnonzero(v)[~choice][:8].tolist()}"
    check("bsdf", "dir", against, r["s_dir"][v], want["s_dir"][v], what)
    check("bsdf", "eta_rough", against, np.stack([r["s_eta"][v], r["s_rough"][v]], axis=1), want["s_eta_rough"][v], what)
    vs = v & ok_s
    if not row["inline_lambert"]:                                   # the inline Lambertian has no separate eval
        check("bsdf", "f", against, at_s["f"][vs, 1], want["s_f"][vs], what + " eval(sampled)")
        check("bsdf", "f", against, r["f"][ok_2, 1], want["f2"][ok_2], what + " eval(dir_out2)")
    check("bsdf", "pdf", against, at_s["pdf"][vs, 1], want["s_pdf"][vs], what + " pdf(sampled)")
    check("bsdf", "pdf", against, r["pdf"][ok_2, 1], want["pdf2"][ok_2], what + " pdf(dir_out2)")
    check("bsdf", "f", against, at_s["fused_f"][vs, 1], want["s_f"][vs], what + " eval_pdf(sampled).f")
    check("bsdf", "f", against, r["fused_f"][ok_2, 1], want["f2"][ok_2], what + " eval_pdf(dir_out2).f")
    check("bsdf", "pdf", against, at_s["fused_pdf"][vs, 1], want["s_pdf"][vs], what + " eval_pdf(sampled).pdf")
    check("bsdf", "pdf", against, r["fused_pdf"][ok_2, 1], want["pdf2"][ok_2], what + " eval_pdf(dir_out2).pdf")
    if not (ok_s[v].all() and ok_2.all()):
        ill = max(float(err(at_s["fused_f"][v & ~ok_s, 1], want["s_f"][v & ~ok_s]).max(initial=0.0)), float(err(at_s["fused_pdf"][v & ~ok_s, 1], want["s_pdf"][v & ~ok_s]).max(initial=0.0)),
                  float(err(r["fused_f"][~ok_2, 1], want["f2"][~ok_2]).max(initial=0.0)), float(err(r["fused_pdf"][~ok_2, 1], want["pdf2"][~ok_2]).max(initial=0.0)))
        print(f"  (reported, not bounded) {what}: {int((v & ~ok_s).sum())} + {int((~ok_2).sum())} ill-conditioned evaluations, worst {ill:.3e}")
    own = max(float(err(r["fused_f"][v, 0], want["s_f"][v]).max(initial=0.0)), float(err(r["fused_pdf"][v, 0], want["s_pdf"][v]).max(initial=0.0)))
    print(f"  (reported, not bounded) {what}: eval_pdf at the kernel's own sampled direction against the wanted values: worst {own:.3e}")
    gap = 0.0
    if not row["inline_lambert"]:
        for res in (r, at_s):
            fin = np.isfinite(res["f"][:, 1]).all(axis=1) & np.isfinite(res["pdf"][:, 1])
            gap = max(gap, float(err(res["fused_f"][fin, 1], res["f"][fin, 1]).max(initial=0.0)), float(err(res["fused_pdf"][fin, 1], res["pdf"][fin, 1]).max(initial=0.0)))
    return gap


def run_variants(G, world, scene, rows, cases):
    """Every variant on the cases its kernel admits: variant index -> (case indices, results, results with dir_out2 := wanted s_dir)."""
    q = bsdf_queries(G, world, cases)
    q_s = q.copy()
    for i, c in enumerate(cases):
        if c["sample_valid"]:
            q_s["dir_out2"][i] = c["s_dir"]
    runs = {}
    for vi, row in enumerate(rows):
        idx = np.array([i for i, c in enumerate(cases) if world.admits(row, world.mid(c["mat"]))], dtype=np.int64)
        runs[vi] = (idx, run(G, scene, "bsdf", vi, q[idx]), run(G, scene, "bsdf", vi, q_s[idx])) if idx.size else (idx, None, None)
    return runs


@pytest.fixture(scope="module")
def world(G):
    return BsdfWorld(G)


@pytest.fixture(scope="module")
def bsdf_scene(G, world):
    sc = G.Scene(world.built)
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def bsdf_rows(G):
    return G.debug_knobs.kat_variants("bsdf")


@pytest.fixture(scope="module")
def golden_runs(G, world, bsdf_scene, bsdf_rows, golden):
    """One run of every variant on the golden cases, shared by the tests."""
    return run_variants(G, world, bsdf_scene, bsdf_rows, golden["bsdf"])


@pytest.fixture(scope="module")
def golden_conditioning(G, O, world, golden):
    """Per golden case: is the evaluation at the sampled direction / at dir_out2 well-conditioned (the one-ulp rule, oracle alone)?"""
    sc = O.OracleScene(world.built.ptr)
    limit = ULP_MOVE * BOUNDS[("bsdf", "f")]
    ok_s, ok_2 = [], []
    for c in golden["bsdf"]:
        mat = world.b.materials[world.mid(c["mat"])]
        ok_s.append(not c["sample_valid"] or eval_sensitivity(O, sc, mat, c, c["s_dir"]) <= limit)
        ok_2.append(eval_sensitivity(O, sc, mat, c, c["dir_out2"]) <= limit)
    return np.array(ok_s), np.array(ok_2)


# ---- (a) against the reference's own vectors ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bsdf_golden_cases_through_every_variant(G, world, bsdf_rows, golden_runs, golden, golden_conditioning):
    """720 cases = 15 materials x 48 under the full switch, and through every other variant the cases of the materials in its set.
    MI355X: direction 2.7e-15, eta / roughness 1.4e-17, f and pdf 1.1e-12; the 73 ill-conditioned evaluations 1e-8 .. 1.2e-7 and one
    finite value where the reference's pdf is infinite (reported, not bounded)."""
    cases = golden["bsdf"]
    names = sorted({c["mat"] for c in cases})
    assert len(names) == 15
    ok_s, ok_2 = golden_conditioning
    ill = [(cases[i]["mat"], i % 48, "sampled") for i in np.flatnonzero(~ok_s)] + [(cases[i]["mat"], i % 48, "dir_out2") for i in np.flatnonzero(~ok_2)]
    print(f"  ill-conditioned golden evaluations (one-ulp rule, oracle alone): {len(ill)} of {2 * len(cases)}: {ill}")
    # they are the sampled directions of the lobes whose roughness clamps to 0.01 or is 0.02 (every sample lands on the peak, where
    # GTR2's 1 + (a^2 - 1) cos^2 cancels to 1e-8), and one direction on the horizon whose reference pdf is infinite
    smooth = ("roughplastic_checker", "roughdielectric_smooth")
    assert sum(m not in smooth for m, _, _ in ill) <= 2 and not any(which == "dir_out2" for _, _, which in ill), ill
    gaps = {}
    for vi, row in enumerate(bsdf_rows):
        idx, r, at_s = golden_runs[vi]
        admitted = [n for n in names if world.admits(row, world.mid(n))]
        assert admitted, f"variant {row['name']} admits no golden material"
        ran = {}
        for i in idx:
            ran[cases[i]["mat"]] = ran.get(cases[i]["mat"], 0) + 1
        assert sorted(ran) == admitted and all(n == 48 for n in ran.values()), (row["name"], ran)      # a variant without cases fails here
        if row["name"] == "full":
            assert len(idx) == 720 and len(ran) == 15
        gaps[row["name"]] = compare_bsdf(r, at_s, bsdf_expected([cases[i] for i in idx]), row, "golden", row["name"], ok_s[idx], ok_2[idx])
        # every lobe the kernel's set holds is among the golden materials it ran
        lobes = {world.type_of[world.mid(n)] for n in admitted}
        if not row["inline_lambert"]:
            one_sided = {t for t in range(9) if (row["mask"] >> t) & 1 and t not in (G.MAT_ROUGHPLASTIC, G.MAT_ROUGHDIELECTRIC, G.MAT_DISNEY_GLASS, G.MAT_DISNEY_BSDF)}
            assert one_sided <= lobes, (row["name"], one_sided, lobes)
    print("  largest fused-against-separate difference per variant:", {k: f"{v:.2e}" for k, v in gaps.items()})
    full = bsdf_rows[0]
    assert full["name"] == "full" and {world.type_of[world.mid(n)] for n in names} == set(range(9))       # all nine lobes under the full switch
    finish()


@pytest.mark.gpu
def test_texture_golden_lookups(G, golden):
    """Every textures.lookups entry, all four textures (image 5x3 and 16x16 three-channel, 4x4 one-channel, checker), through tex3, and
    tex1 = its first channel; the mip chain is the one the upload built."""
    b = DescBuilder(G)
    tex = _textures(G, b, golden)
    slot = {name: b.material(G.MAT_LAMBERTIAN, [t]) for name, t in tex.items()}
    sc = G.Scene(Built(b))
    lks = golden["textures"]["lookups"]
    q = queries(G, "texture", len(lks))
    q["material_id"], q["slot"] = [slot[lk["tex"]] for lk in lks], 0
    q["uv"], q["uv_screen_size"] = [lk["uv"] for lk in lks], [lk["footprint"] for lk in lks]
    r = run(G, sc, "texture", 0, q)
    sc.close()
    assert {lk["tex"] for lk in lks} == {"img", "img2", "chk", "f"} and len(r) == len(lks) == 60
    want = np.array([lk["out"] for lk in lks])
    check("texture", "value", "golden", r["tex3"], want)
    check("texture", "value", "golden", r["tex1"], want[:, 0], "tex1")
    finish()


@pytest.mark.gpu
def test_filter_and_primary_golden_cases(G, golden):
    """The 48 filter cases, and every ray of the 3 cameras (512x512 Gaussian: the power-of-two fast path of PIXEL_SPACE; 683x512 box,
    1280x720 tent) through sample_primary on the screen position and on the pixel-space numbers."""
    sc = G.Scene(Built(DescBuilder(G)))
    fc = golden["filters"]
    assert len(fc) == 48
    q = queries(G, "filter", len(fc))
    q["type"], q["param"], q["u"] = [c["type"] for c in fc], [c["param"] for c in fc], [c["u"] for c in fc]
    r = run(G, sc, "filter", 0, q)
    sc.close()
    check("filter", "offset", "golden", r["out"], np.array([c["out"] for c in fc]))
    assert len(golden["cameras"]) == 3
    rays = 0
    for cam in golden["cameras"]:
        b = DescBuilder(G)
        c = b.desc.camera
        for i in range(16):
            c.sample_to_cam[i], c.cam_to_world[i] = cam["sample_to_cam"][i], cam["cam_to_world"][i]
        c.width, c.height, c.filter_type, c.filter_param = cam["width"], cam["height"], cam["filter_type"], cam["filter_param"]
        sc = G.Scene(Built(b))
        for variant, name in enumerate(r_["name"] for r_ in G.debug_knobs.kat_variants("primary")):
            q = queries(G, "primary", len(cam["rays"]))
            if name == "screen":
                q["s"] = [ray["screen"] for ray in cam["rays"]]
            else:
                q["s"] = [[ray["x"] + ray["rng"][0], ray["y"] + ray["rng"][1]] for ray in cam["rays"]]
            r = run(G, sc, "primary", variant, q)
            check("primary", "org", "golden", r["org"], np.array([ray["org"] for ray in cam["rays"]]), f"{cam['width']}x{cam['height']} {name}")
            check("primary", "dir", "golden", r["dir"], np.array([ray["dir"] for ray in cam["rays"]]), f"{cam['width']}x{cam['height']} {name}")
        rays += len(cam["rays"])
        sc.close()
    assert rays == 72
    finish()


def table_normal(mesh, prim):
    """The geometric normal the upload stores for a triangle (csrc/host/tri_precompute.cpp): the cross product of the fp32 edges in fp32,
    every operation rounded once, normalised in fp64. It is what the traversal reports and what intersect() hands to
    compute_shading_info in the reference, whose Embree returns Ng in fp32 (src/intersection.cpp:41)."""
    pos = np.array(mesh["positions"], dtype=np.float64).reshape(-1, 3).astype(np.float32)
    i0, i1, i2 = mesh["indices"][3 * prim:3 * prim + 3]
    e1, e2 = pos[i1] - pos[i0], pos[i2] - pos[i0]
    ng = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], dtype=np.float32).astype(np.float64)
    return ng * (1.0 / math.sqrt(float(ng[0] * ng[0] + ng[1] * ng[1] + ng[2] * ng[2])))


@pytest.mark.gpu
def test_shading_info_golden_cases(G, O, golden):
    """The 24 triangle cases (4 mesh variants x 6) with need_uv both ways, and the 6 sphere cases, all at 1e-12.
    Where a triangle's frame depends on its geometric normal, shading_info_tri takes it from the uploaded table (table_normal above)
    and does not read the `gn` it is given: a triangle without vertex normals has a flat frame made at upload from that normal
    (mesh variant 0), and one with degenerate uvs a tangent made from it (variant 3). The golden cases pass a normal from an fp64
    cross product, 5e-8 away. For these 12 the wanted frame is therefore the oracle's shading_info_tri (pinned to the same golden
    cases at 1e-12 by tests/test_oracle_vs_reference_kat.py) on the normal the table holds, and the golden frame itself must agree
    with it to fp32 rounding (2^-22). uv and inv_uv_size of these cases, and everything of the other 12, are compared with the
    golden values."""
    cases = golden["shading_info"]
    assert len(cases) == 24 and len(golden["sphere_shading"]) == 6
    flat_cases = 0
    for variant in range(4):
        sub = [c for c in cases if c["variant"] == variant]
        assert len(sub) == 6
        built = Built(_shading_mesh(G, golden, variant))
        sc = G.Scene(built)
        frames = np.array([c["fx"] + c["fy"] + c["fn"] for c in sub])
        if variant in (0, 3):                               # no vertex normals: flat frames; degenerate uvs: tangent from the normal
            osc = O.OracleScene(built.ptr)
            golden_frames = frames
            frames = np.array([osc.shading_info_tri(c["prim"], c["st"], table_normal(golden["shading_mesh"], c["prim"]))[2:11] for c in sub])
            assert float(np.abs(frames - golden_frames).max()) <= 2.0 ** -22
            flat_cases += len(sub)
        for need_uv in (1, 0):
            q = queries(G, "shading", len(sub))
            q["index"], q["need_uv"] = [c["prim"] for c in sub], need_uv
            q["st"], q["gn"] = [c["st"] for c in sub], [c["gn"] for c in sub]
            r = run(G, sc, "shading", 0, q)
            what = f"mesh variant {variant} need_uv={need_uv}"
            check("shading", "uv", "golden", r["uv"], np.array([c["uv"] for c in sub]) if need_uv else np.zeros((len(sub), 2)), what)
            check("shading", "frame", "golden", np.concatenate([r["fx"], r["fy"], r["fn"]], axis=1), frames, what)
            check("shading", "inv_uv_size", "golden", r["inv_uv_size"], np.array([c["inv_uv_size"] for c in sub]), what)
        sc.close()
    assert flat_cases == 12
    sh = golden["sphere_hits"]
    b = DescBuilder(G)
    b.sphere(sh["center"], sh["radius"], b.material(G.MAT_LAMBERTIAN, [DescBuilder.const_tex(G, 0.5)]))
    sc = G.Scene(Built(b))
    sub = golden["sphere_shading"]
    q = queries(G, "shading", len(sub))
    q["is_sphere"], q["index"], q["st"], q["gn"] = 1, 0, [c["st"] for c in sub], [c["gn"] for c in sub]
    r = run(G, sc, "shading", 0, q)
    sc.close()
    check("shading", "uv", "golden", r["uv"], np.array([c["uv"] for c in sub]), "sphere")
    check("shading", "frame", "golden", np.concatenate([r["fx"], r["fy"], r["fn"]], axis=1), np.array([c["fx"] + c["fy"] + c["fn"] for c in sub]), "sphere")
    check("shading", "inv_uv_size", "golden", r["inv_uv_size"], np.array([c["inv_uv_size"] for c in sub]), "sphere")
    finish()


@pytest.mark.gpu
def test_light_sampling_golden_cases(G, golden):
    """sample_point_on_light and pdf_point_on_light for the two emitter meshes (without and with vertex normals) and the sphere
    (reference points outside and inside it)."""
    ls = golden["light_sampling"]
    assert len(ls["meshes"]) == 2
    for rec in ls["meshes"] + [ls["sphere"]]:
        is_sphere = "radius" in rec
        b, sid = _emitter_sphere(G, golden) if is_sphere else _emitter_mesh(G, golden, rec)
        light_id = b.shapes[sid].area_light_id
        sc = G.Scene(Built(b))
        cs = rec["cases"]
        q = queries(G, "light", len(cs))
        q["light_id"], q["ref"], q["uv"] = light_id, [c["ref"] for c in cs], [c["uv"] for c in cs]
        q["w"] = [c.get("w", 0.5) for c in cs]
        r = run(G, sc, "light", 0, q)
        sc.close()
        what = "sphere" if is_sphere else rec["file"]
        assert len(cs) == (20 if is_sphere else 16)
        check("light", "position", "golden", r["position"], np.array([c["position"] for c in cs]), what)
        check("light", "normal", "golden", r["normal"], np.array([c["normal"] for c in cs]), what)
        check("light", "pdf", "golden", r["pdf"], np.array([c["pdf"] for c in cs]), what)
    finish()


# ---- (c) the edge list -------------------------------------------------------------------------------------------------------------
# shading frame of every edge case: an orthonormal triple of thirds (x cross y = n), so that no world component is zero
FX, FY, FN = (1 / 3, 2 / 3, 2 / 3), (2 / 3, 1 / 3, -2 / 3), (-2 / 3, 2 / 3, -1 / 3)
ONE_BELOW = math.nextafter(1.0, 0.0)


def _world(local):
    return [FX[k] * local[0] + FY[k] * local[1] + FN[k] * local[2] for k in range(3)]


def _polar(cos_t, phi):
    s = math.sqrt(max(0.0, 1.0 - cos_t * cos_t))
    return (s * math.cos(phi), s * math.sin(phi), cos_t)


def edge_bsdf_candidates(world):
    """Every candidate of the BSDF edge list, kept or not: dicts in the golden file's format plus "id"."""
    # dir_in (local to the shading frame), with the geometric normal that goes with it (local; the default is the shading normal)
    n_local = (0.0, 0.0, 1.0)
    dins = [("normal", (0.0, 0.0, 1.0), n_local), ("cos+1e-3", _polar(1e-3, 0.7), n_local), ("cos+1e-6", _polar(1e-6, 0.7), n_local),
            ("cos-1e-3", _polar(-1e-3, 0.7), n_local), ("cos-1e-6", _polar(-1e-6, 0.7), n_local),
            ("above", _polar(0.8, 2.1), n_local), ("below", _polar(-0.8, 2.1), n_local),
            ("inside_past_tir", _polar(-0.6, 0.4), n_local),                       # sin = 0.8 > 1 / eta for every eta >= 1.33 used
            ("gn_below_n_above", (0.9, 0.0, math.sqrt(0.19)), (-0.6, 0.0, 0.8)),   # gn . in < 0 < n . in
            ("gn_above_n_below", (-0.9 / math.sqrt(0.85), 0.0, -0.2 / math.sqrt(0.85)), (-0.6, 0.0, 0.8))]   # n . in < 0 < gn . in
    douts = ["mirror", "minus_in", "below_horizon", "above", "grazing"]
    ruvs = [(a, b) for a in (0.0, 0.5, ONE_BELOW) for b in (0.0, 0.5, ONE_BELOW)] + \
           [(t + s * 1e-3, 0.3) for t in (0.25, 0.5, 0.75) for s in (-1, 1)] + [(0.1, 0.9)]            # the lobe thresholds act on ruv.x
    rws = [t + s * 1e-3 for t in (0.0, 0.25, 0.5, 0.75, 1.0) for s in (-1, 1)] + [0.5]
    out = []
    names = list(world.ids) + list(world.edge)
    for name in names:
        rounds, step = (2, 1) if name in world.ids else (1, 2)         # the variants of a material take every other pair, once
        for idx in range(0, rounds * len(dins) * len(douts), step):
            i, j = (idx // len(douts)) % len(dins), idx % len(douts)
            tag, din, gnl = dins[i]
            dout = {"mirror": (-din[0], -din[1], din[2]), "minus_in": (-din[0], -din[1], -din[2]), "below_horizon": _polar(-0.8, 1.1),
                    "above": _polar(math.sqrt(0.66), 4.0), "grazing": _polar(1e-3, 5.0)}[douts[j]]
            out.append({"id": f"{name}/{tag}/{douts[j]}/{idx // (len(dins) * len(douts))}", "mat": name,
                        "gn": _world(gnl), "fx": list(FX), "fy": list(FY), "fn": list(FN), "uv": [0.3 + 0.01 * j, 0.6], "uvss": 0.0,
                        "dir_in": _world(din), "dir_out2": _world(dout), "ruv": list(ruvs[idx % len(ruvs)]), "rw": rws[idx % len(rws)]})
    return out


def edge_texture_setup(G, b):
    """Images of the texture edge list: 8x4 three-channel (non-square, four mip levels), 1x1 one-channel, 4x4 one-channel with a
    scale and an offset, and a checker. name -> (material id, largest extent x scale of an image texture)."""
    tex = {
        "rgb8x4": (b.image_tex([((i * 7 + 3) % 11) / 10 for i in range(8 * 4 * 3)], 8, 4, 3, 1.0, 1.0, 0.0, 0.0), 8.0),
        "one1x1": (b.image_tex([0.375], 1, 1, 1, 1.0, 1.0, 0.0, 0.0), 1.0),
        "mono4x4": (b.image_tex([((i * 5 + 1) % 7) / 8 for i in range(16)], 4, 4, 1, 2.0, 0.5, 0.25, -0.75), 8.0),
        "checker": (b.checker_tex((0.4, 0.5, 0.6), (0.1, 0.2, 0.3), 4.0, 2.0, 0.125, 0.0), 0.0),
    }
    return {name: (b.material(G.MAT_LAMBERTIAN, [t]), t, ext) for name, (t, ext) in tex.items()}


def edge_texture_candidates():
    """uv at texel centres and edges, negative and above 1; footprints that put the level at 0 and below, on an integer level, between the
    last two levels, on the last and past it."""
    levels = {"rgb8x4": 4, "one1x1": 1, "mono4x4": 3}
    extent = {"rgb8x4": 8.0, "one1x1": 1.0, "mono4x4": 8.0, "checker": 1.0}
    out = []
    for name in ("rgb8x4", "one1x1", "mono4x4", "checker"):
        n = levels.get(name, 1)
        lv = [-1.0, 0.0, 0.5, 1.0, n - 1.5, float(n - 1), n + 1.0]
        fps = [0.0] + [2.0 ** l / extent[name] for l in lv]
        uvs = [((x + 0.5) / 8, (y + 0.5) / 4) for x, y in ((0, 0), (3, 2), (7, 3))] + [(x / 8, y / 4) for x, y in ((0, 0), (3, 2), (8, 4))] + \
              [(-0.25, -1.5), (-0.0625, 0.3), (1.25, 2.75), (1.0, 1.0), (0.3, -3.0625), (5.5, 0.99)]
        for k, uv in enumerate(uvs):
            for m, fp in enumerate(fps):
                out.append({"id": f"{name}/uv{k}/fp{m}", "tex": name, "uv": list(uv), "footprint": fp})
    return out


def _dropped():
    with open(DROPPED_FILE) as f:
        return json.load(f)


def edge_bsdf_cases(world):
    drop = set(_dropped()["bsdf"])
    return [c for c in edge_bsdf_candidates(world) if c["id"] not in drop]


def edge_texture_cases():
    drop = set(_dropped()["texture"])
    return [c for c in edge_texture_candidates() if c["id"] not in drop]


def oracle_bsdf(O, sc, world, case):
    """The oracle's answers to one case, under the golden file's keys."""
    mat = world.b.materials[world.mid(case["mat"])]
    v = _vertex(O, case)
    out = {"sample_valid": 0}
    s = sc.bsdf_sample(mat, case["dir_in"], v, case["ruv"], case["rw"])
    if s is not None:
        d, eta, rough = s
        out.update(sample_valid=1, s_dir=d.tolist(), s_eta=eta, s_rough=rough,
                   s_f=sc.bsdf_eval(mat, case["dir_in"], d, v).tolist(), s_pdf=sc.bsdf_pdf(mat, case["dir_in"], d, v))
    out["f2"] = sc.bsdf_eval(mat, case["dir_in"], case["dir_out2"], v).tolist()
    out["pdf2"] = sc.bsdf_pdf(mat, case["dir_in"], case["dir_out2"], v)
    return out


def _flat(ans):
    nan3 = [math.nan] * 3
    return np.array(ans.get("s_dir", nan3) + [ans.get("s_eta", math.nan), ans.get("s_rough", math.nan)] + ans.get("s_f", nan3) +
                    [ans.get("s_pdf", math.nan)] + ans["f2"] + [ans["pdf2"]])


def _discrete(case, ans):
    """Validity, reflect or refract, which outputs are finite, and for DisneyBSDF the lobe (its fixed thresholds act on ruv.x)."""
    lobe = min(3, int(case["ruv"][0] * 4)) if case["mat"].startswith("disneybsdf") else 0
    return (ans["sample_valid"], ans.get("s_eta", 0.0) != 0.0, tuple(np.isfinite(_flat(ans)).tolist()), lobe)


STEP, MOVE, ULP_MOVE = 1e-12, 1e-6, 0.1


def _moved(a, b):
    """Largest |a - b| / max(1, |b|) over two vectors; a change of finiteness counts as infinite."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    if not np.array_equal(np.isfinite(a), np.isfinite(b)) or not np.array_equal(np.isnan(a), np.isnan(b)):
        return math.inf
    fin = np.isfinite(b)
    return float((np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))).max(initial=0.0))


def _steps(x):
    """x one ulp away, and 2^13 ulps away (about one part in 1e12) with the factor that scales the move back to one ulp: the first sees
    a singularity the last bit decides, the second the slope where a single ulp happens to round away."""
    for toward in (-math.inf, math.inf):
        yield math.nextafter(x, toward), 1.0
        yield x + (math.nextafter(x, toward) - x) * 8192.0, 1.0 / 8192.0


def eval_sensitivity(O, sc, mat, case, dir_out):
    """How far the oracle's eval and pdf of one direction pair move when one component of dir_in, dir_out or the shading normal moves
    by one ulp. (The normal counts: at the peak of a narrow lobe cos(n, h) is stationary in the directions, and what the value hangs
    on is the last bit of that cosine.)"""
    v = _vertex(O, case)
    f0, p0 = sc.bsdf_eval(mat, case["dir_in"], dir_out, v), sc.bsdf_pdf(mat, case["dir_in"], dir_out, v)
    worst_move = 0.0
    for which in ("dir_in", "dir_out", "fn"):
        for k in range(3):
            base = {"dir_in": case["dir_in"], "dir_out": dir_out, "fn": case["fn"]}
            for x, scale in _steps(base[which][k]):
                d = {key: list(val) for key, val in base.items()}
                d[which][k] = x
                v2 = _vertex(O, dict(case, fn=d["fn"])) if which == "fn" else v
                worst_move = max(worst_move, scale * _moved(sc.bsdf_eval(mat, d["dir_in"], d["dir_out"], v2), f0),
                                 scale * _moved(sc.bsdf_pdf(mat, d["dir_in"], d["dir_out"], v2), p0))
    return worst_move


def sample_sensitivity(sc, mat, v, case):
    """... the oracle's sampled direction, eta and roughness, when one component of dir_in, ruv (inside [0, 1)) or rw moves by one ulp."""
    s0 = sc.bsdf_sample(mat, case["dir_in"], v, case["ruv"], case["rw"])
    if s0 is None:
        return 0.0
    flat0 = np.array(list(s0[0]) + [s0[1], s0[2]])
    worst_move = 0.0
    for key in ("dir_in", "ruv", "rw"):
        vals = case[key] if isinstance(case[key], list) else [case[key]]
        for k in range(len(vals)):
            for x, scale in _steps(vals[k]):
                moved = list(vals)
                moved[k] = min(max(x, 0.0), ONE_BELOW) if key == "ruv" else x
                args = {"dir_in": case["dir_in"], "ruv": case["ruv"], "rw": case["rw"]}
                args[key] = moved if isinstance(case[key], list) else moved[0]
                s1 = sc.bsdf_sample(mat, args["dir_in"], v, args["ruv"], args["rw"])
                if s1 is None:
                    return math.inf
                worst_move = max(worst_move, scale * _moved(np.array(list(s1[0]) + [s1[1], s1[2]]), flat0))
    return worst_move


def bsdf_case_is_stable(O, sc, world, case, base=None):
    """The rule of the module docstring for one BSDF case."""
    base = base or oracle_bsdf(O, sc, world, case)
    d0, f0 = _discrete(case, base), _flat(base)
    for key in ("dir_in", "dir_out2", "gn", "ruv", "rw"):
        vals = case[key] if isinstance(case[key], list) else [case[key]]
        for k in range(len(vals)):
            for sign in (-1.0, 1.0):
                moved = list(vals)
                if key == "ruv":
                    moved[k] = min(max(vals[k] * (1.0 + sign * STEP), 0.0), ONE_BELOW)       # stays inside [0, 1)
                else:
                    moved[k] = vals[k] + sign * STEP * max(1.0, abs(vals[k]))
                if moved[k] == vals[k]:
                    continue
                c2 = dict(case)
                c2[key] = moved if isinstance(case[key], list) else moved[0]
                a2 = oracle_bsdf(O, sc, world, c2)
                if _discrete(c2, a2) != d0 or _moved(_flat(a2), f0) > MOVE:
                    return False
    mat, v = world.b.materials[world.mid(case["mat"])], _vertex(O, case)
    if sample_sensitivity(sc, mat, v, case) > ULP_MOVE * BOUNDS[("bsdf", "dir")]:
        return False
    if base["sample_valid"] and eval_sensitivity(O, sc, mat, case, base["s_dir"]) > ULP_MOVE * BOUNDS[("bsdf", "f")]:
        return False
    return eval_sensitivity(O, sc, mat, case, case["dir_out2"]) <= ULP_MOVE * BOUNDS[("bsdf", "f")]


def texture_case_is_stable(sc, tex, case):
    base = sc.texture_eval(tex, case["uv"], case["footprint"])
    for k in range(3):
        for sign in (-1.0, 1.0):
            uv, fp = list(case["uv"]), case["footprint"]
            if k < 2:
                uv[k] += sign * STEP * max(1.0, abs(uv[k]))
            else:
                fp = max(0.0, fp + sign * STEP * max(1.0, abs(fp)))
            got = sc.texture_eval(tex, uv, fp)
            if not np.isfinite(got).all() or float((np.abs(got - base) / np.maximum(1.0, np.abs(base))).max()) > MOVE:
                return False
    return True


def _texture_world(G):
    b = DescBuilder(G)
    return b, edge_texture_setup(G, b)


def find_unstable(G, O, only_kept):
    """ids of the candidates that fail the rule (only_kept: among the kept ones alone)."""
    world = BsdfWorld(G)
    sc = O.OracleScene(world.built.ptr)
    cand = edge_bsdf_cases(world) if only_kept else edge_bsdf_candidates(world)
    bad_bsdf = [c["id"] for c in cand if not bsdf_case_is_stable(O, sc, world, c)]
    b, texs = _texture_world(G)
    tsc = O.OracleScene(b.finish())
    tc = edge_texture_cases() if only_kept else edge_texture_candidates()
    bad_tex = [c["id"] for c in tc if not texture_case_is_stable(tsc, texs[c["tex"]][1], c)]
    return {"bsdf": bad_bsdf, "texture": bad_tex}, len(cand), len(tc)


def test_edge_list_is_stable(G, O):
    """CPU: every kept edge case passes the stability rule with the oracle alone; the list covers every golden material with at least
    24 cases, every required direction, random number and texture edge; nothing is dropped twice or unknown."""
    world = BsdfWorld(G)
    bad, n_bsdf, n_tex = find_unstable(G, O, only_kept=True)
    assert bad == {"bsdf": [], "texture": []}, bad
    cand, kept = edge_bsdf_candidates(world), edge_bsdf_cases(world)
    drop = _dropped()
    ids = [c["id"] for c in cand]
    assert len(set(ids)) == len(ids) and set(drop["bsdf"]) <= set(ids) and len(set(drop["bsdf"])) == len(drop["bsdf"])
    tids = [c["id"] for c in edge_texture_candidates()]
    assert len(set(tids)) == len(tids) and set(drop["texture"]) <= set(tids)
    per = {}
    for c in kept:
        per[world.base(c["mat"])] = per.get(world.base(c["mat"]), 0) + 1
    print("  bsdf edge cases kept per material:", per, "dropped:", len(drop["bsdf"]), "of", len(cand))
    print("  texture edge cases kept:", len(edge_texture_cases()), "dropped:", len(drop["texture"]), "of", len(tids))
    assert sorted(per) == sorted(world.ids) and len(per) == 15 and min(per.values()) >= 24, per
    tags = {c["id"].split("/")[1] for c in kept}
    assert tags == {"normal", "cos+1e-3", "cos+1e-6", "cos-1e-3", "cos-1e-6", "above", "below", "inside_past_tir", "gn_below_n_above", "gn_above_n_below"}
    assert {c["id"].split("/")[2] for c in kept} == {"mirror", "minus_in", "below_horizon", "above", "grazing"}
    for comp in (0, 1):
        assert {0.0, 0.5, ONE_BELOW} <= {c["ruv"][comp] for c in kept}
    assert {t + s * 1e-3 for t in (0.0, 0.25, 0.5, 0.75, 1.0) for s in (-1, 1)} <= {c["rw"] for c in kept}
    assert {t + s * 1e-3 for t in (0.25, 0.5, 0.75) for s in (-1, 1)} <= {c["ruv"][0] for c in kept}
    for tex in ("rgb8x4", "one1x1", "mono4x4", "checker"):
        assert sum(c["tex"] == tex for c in edge_texture_cases()) >= 24, tex
    # glass and the rough dielectric from inside, past total internal reflection for their eta (about the shading normal; a sampled
    # micro-normal may still let the ray out): the oracle reflects or refuses most of them, and refracts none about the normal itself
    sc = O.OracleScene(world.built.ptr)
    tir = [c for c in kept if "/inside_past_tir/" in c["id"] and world.base(c["mat"]) in ("disneyglass", "roughdielectric", "roughdielectric_smooth")]
    assert len(tir) >= 12
    not_refracted = 0
    for c in tir:
        eta = world.b.materials[world.mid(c["mat"])].eta
        cos_in = sum(a * n for a, n in zip(c["dir_in"], c["gn"]))
        assert cos_in < 0 and math.sqrt(1 - cos_in * cos_in) > 1 / eta, c["id"]
        a = oracle_bsdf(O, sc, world, c)
        not_refracted += int(a["sample_valid"] == 0 or a["s_eta"] == 0.0)
    assert not_refracted >= len(tir) // 2, (not_refracted, len(tir))


@pytest.fixture(scope="module")
def edge_reference(G, O, world):
    """The kept BSDF edge cases with the oracle's answers merged in (computed once, shared)."""
    sc = O.OracleScene(world.built.ptr)
    return [dict(c, **oracle_bsdf(O, sc, world, c)) for c in edge_bsdf_cases(world)]


@pytest.fixture(scope="module")
def edge_runs(G, world, bsdf_scene, bsdf_rows, edge_reference):
    return run_variants(G, world, bsdf_scene, bsdf_rows, edge_reference)


@pytest.mark.gpu
def test_bsdf_edges_against_the_oracle(G, world, bsdf_rows, edge_reference, edge_runs):
    """Every kept edge case (none skipped) through every variant that admits its material, against the CPU oracle, under the bounds of
    the golden comparison. MI355X: direction 2.1e-13, eta / roughness 1.4e-17, f and pdf 6.0e-13."""
    total = 0
    for vi, row in enumerate(bsdf_rows):
        idx, r, at_s = edge_runs[vi]
        assert idx.size, row["name"]
        if row["name"] == "full":
            assert idx.size == len(edge_reference)
        gap = compare_bsdf(r, at_s, bsdf_expected([edge_reference[i] for i in idx]), row, "oracle", row["name"])
        print(f"  {row['name']}: {idx.size} cases, largest fused-against-separate difference {gap:.2e}")
        total += idx.size
    assert total >= len(edge_reference)
    finish()


@pytest.mark.gpu
def test_texture_edges_against_the_oracle(G, O):
    b, texs = _texture_world(G)
    built = Built(b)
    osc = O.OracleScene(built.ptr)
    cases = edge_texture_cases()
    want = np.array([osc.texture_eval(texs[c["tex"]][1], c["uv"], c["footprint"]) for c in cases])
    sc = G.Scene(built)
    q = queries(G, "texture", len(cases))
    q["material_id"], q["slot"] = [texs[c["tex"]][0] for c in cases], 0
    q["uv"], q["uv_screen_size"] = [c["uv"] for c in cases], [c["footprint"] for c in cases]
    r = run(G, sc, "texture", 0, q)
    sc.close()
    assert len(r) == len(cases) and {c["tex"] for c in cases} == {"rgb8x4", "one1x1", "mono4x4", "checker"}
    check("texture", "value", "oracle", r["tex3"], want)
    check("texture", "value", "oracle", r["tex1"], want[:, 0], "tex1")
    finish()


# ---- (b) variants against each other, bit for bit ----------------------------------------------------------------------------------
FIELDS = ("s_dir", "s_eta", "s_rough", "f", "pdf", "fused_f", "fused_pdf")


@pytest.mark.gpu
def test_reduced_sets_give_the_full_switch_s_bits(G, world, bsdf_rows, golden_runs, edge_runs):
    """"Same arithmetic on every path": sample, eval, pdf and eval_pdf of every reduced variant equal the full switch's raw doubles on
    every golden and edge case of the materials in its set; the inline Lambertian with kPlainConstTex equals the one without."""
    by_name = {row["name"]: vi for vi, row in enumerate(bsdf_rows)}
    compared = 0
    for runs, label in ((golden_runs, "golden"), (edge_runs, "edges")):
        full_idx = runs[by_name["full"]][0]
        pos = {int(i): k for k, i in enumerate(full_idx)}
        idx0 = runs[by_name["lambert_inline"]][0]
        idx2 = runs[by_name["lambert_inline_const_tex"]][0]
        assert idx2.size and set(idx2.tolist()) <= set(idx0.tolist())
        at = {int(i): k for k, i in enumerate(idx0)}
        for batch in (1, 2):                                   # the cases as they are; with dir_out2 := the wanted sampled direction
            full = runs[by_name["full"]][batch]
            for vi, row in enumerate(bsdf_rows):
                if row["name"] == "full" or row["inline_lambert"]:
                    continue
                idx, r = runs[vi][0], runs[vi][batch]
                assert idx.size, (row["name"], label)
                ref = full[[pos[int(i)] for i in idx]]
                assert np.array_equal(r["sample_valid"], ref["sample_valid"]), (row["name"], label)
                for f in FIELDS:
                    assert same_bits(r[f], ref[f]), f"{row['name']} ({label}): {f} differs from the full switch in {int((r[f] != ref[f]).sum())} numbers"
                compared += idx.size
            plain0, plain2 = runs[by_name["lambert_inline"]][batch], runs[by_name["lambert_inline_const_tex"]][batch]
            ref = plain0[[at[int(i)] for i in idx2]]
            assert np.array_equal(plain2["sample_valid"], ref["sample_valid"])
            for f in ("s_dir", "s_eta", "s_rough", "pdf", "fused_f", "fused_pdf"):
                assert same_bits(plain2[f], ref[f]), f"kPlainConstTex ({label}): {f} differs"
            compared += idx2.size
    print(f"  {compared} (variant, case) pairs compared bit for bit")


# ---- refusals: a bad argument never reaches a kernel -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bad_arguments_are_refused(G, world, bsdf_scene, bsdf_rows):
    q = bsdf_queries(G, world, [dict(mat="lambertian", gn=FN, fx=FX, fy=FY, fn=FN, uv=[0, 0], uvss=0, dir_in=FN, dir_out2=FN, ruv=[0.5, 0.5], rw=0.5)])
    with pytest.raises(G.GdptError, match="variant"):
        run(G, bsdf_scene, "bsdf", len(bsdf_rows), q)
    with pytest.raises(G.GdptError, match="variant"):
        run(G, bsdf_scene, "bsdf", -1, q)
    bad = q.copy()
    bad["material_id"] = len(world.type_of)
    with pytest.raises(G.GdptError, match="material id"):
        run(G, bsdf_scene, "bsdf", 0, bad)
    bad["material_id"] = world.mid("disneymetal")
    inline = next(i for i, r in enumerate(bsdf_rows) if r["inline_lambert"])
    with pytest.raises(G.GdptError, match="Lambertian materials only"):
        run(G, bsdf_scene, "bsdf", inline, bad)
    t = queries(G, "texture", 1)
    t["slot"] = 12
    with pytest.raises(G.GdptError, match="texture slot"):
        run(G, bsdf_scene, "texture", 0, t)
    lq = queries(G, "light", 1)
    with pytest.raises(G.GdptError, match="light id"):                # the scene has no emitter
        run(G, bsdf_scene, "light", 0, lq)
    sq = queries(G, "shading", 1)
    with pytest.raises(G.GdptError, match="triangle id"):             # ... and no geometry
        run(G, bsdf_scene, "shading", 0, sq)
    sq["is_sphere"] = 1
    with pytest.raises(G.GdptError, match="sphere index"):
        run(G, bsdf_scene, "shading", 0, sq)
    fq = queries(G, "filter", 1)
    fq["type"] = 3
    with pytest.raises(G.GdptError, match="filter type"):
        run(G, bsdf_scene, "filter", 0, fq)
    assert G.lib().gdpt_debug_kat_bsdf(None, 0, 0, None, None) != 0


if __name__ == "__main__" and sys.argv[1:] == ["write-dropped"]:
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import gdpt_amd as _G
    import oracle_py as _O
    if not os.path.exists(DROPPED_FILE):
        with open(DROPPED_FILE, "w") as f:
            json.dump({"bsdf": [], "texture": []}, f)
    found, nb, nt = find_unstable(_G, _O, only_kept=False)
    with open(DROPPED_FILE, "w") as f:
        json.dump(found, f, indent=0)
        f.write("\n")
    print(f"dropped {len(found['bsdf'])} of {nb} bsdf candidates, {len(found['texture'])} of {nt} texture candidates")
