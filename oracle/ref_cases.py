"""The scenes, variants and sizes of the reference-made fixtures tests/golden/ref_samples_*.npz and ref_fourier.npz.

One list, read by oracle/gen_golden.py (which writes the fixtures from the reference's own integrators) and by
tests/test_oracle_vs_reference_samples.py and tests/test_gpu_reference_samples.py (which hold the oracle and the kernels
against them), so that the XML a fixture was made from and the XML a test renders cannot drift apart.
"""
import collections

FILM = (40, 24)             # 3 x 2 tiles of 16 x 16, ragged in both directions
MARGIN_THRESHOLD = 1e-6     # a sample (pixel) whose `margin` is below this keeps only the finiteness check
MARGIN_CAP = 0.02           # ... and at most this share of a scene's samples (a film's pixels) may be such

# klass: the tolerance class of tests/test_gpu_route_matrix.py (lambert 1e-9, general 1e-7: transcendentals or
# textures, envmap 1e-6). offsets: the offset fields are a function of the source (the scene's max_depth, as shipped or as edited,
# is 1 or 2; the tests check the flag against the parsed depth).
Case = collections.namedtuple("Case", "name scene integrator max_depth rr_depth count film_spp stream_offset klass offsets")

CASES = [
    # ---- Integrator::GradPath ----
    Case("grad_cbox", "cbox/cbox_gdpt.xml", "gradpath", None, None, 1024, 2, 0, "lambert", False),
    Case("grad_cbox_d1_rr5", "cbox/cbox_gdpt.xml", "gradpath", 1, 5, 1024, 2, 0, "lambert", True),
    Case("grad_cbox_d2_rr5", "cbox/cbox_gdpt.xml", "gradpath", 2, 5, 1024, 2, 0, "lambert", True),
    Case("grad_cbox_d2_rr1", "cbox/cbox_gdpt.xml", "gradpath", 2, 1, 1024, 2, 0, "lambert", True),
    Case("grad_cbox_dinf_rr1", "cbox/cbox_gdpt.xml", "gradpath", -1, 1, 1024, 2, 0, "lambert", False),
    Case("grad_small_pt", "cbox/small_pt_compare.xml", "gradpath", None, None, 1024, 2, 0, "lambert", True),     # ships with maxDepth 2
    Case("grad_disney_metal", "disney_bsdf_test/disney_metal.xml", "gradpath", None, None, 1024, 2, 0, "general", False),
    Case("grad_disney_metal_d2", "disney_bsdf_test/disney_metal.xml", "gradpath", 2, 5, 1024, 2, 0, "general", True),
    Case("grad_sponza", "sponza/sponza.xml", "gradpath", None, None, 256, 1, 0, "general", False),
    Case("grad_sponza_d2", "sponza/sponza.xml", "gradpath", 2, 5, 256, 1, 0, "general", True),
    # ---- Integrator::Path ----
    Case("path_cbox", "cbox/cbox_gdpt.xml", "path", None, None, 1024, 2, 0, "lambert", False),
    Case("path_small_pt", "cbox/small_pt_compare.xml", "path", None, None, 1024, 2, 0, "lambert", False),
    Case("path_veach_mi", "veach_mi/mi.xml", "path", None, None, 1024, 2, 0, "general", False),
    Case("path_disney_diffuse", "disney_bsdf_test/disney_diffuse.xml", "path", None, None, 1024, 2, 0, "envmap", False),
    Case("path_disney_glass", "disney_bsdf_test/disney_glass.xml", "path", None, None, 1024, 2, 0, "envmap", False),
    Case("path_matpreview", "matpreview/matpreview.xml", "path", None, None, 256, 2, 0, "envmap", False),
    Case("path_sponza", "sponza/sponza.xml", "path", None, None, 256, 1, 0, "general", False),
]
BY_NAME = {c.name: c for c in CASES}

# Films whose compared buffers are zero at every pixel in the reference's own output, so that the film comparison of these cases
# holds the route, the finiteness and "nothing but zeros" only (the tests assert that this list is exact): GradPath radiance arrives
# through BSDF-sampled emitter hits alone, and at unbounded depth only `img` is authoritative. Their scattered samples still pin
# contrib, prob and the draw count, and each GradPath one has a max_depth 2 sibling whose gradient buffers are not empty.
# path_small_pt: the camera of small_pt_compare never sees light under the parsing quirks the reference has (`x="1e5+1"`
# -> 1e5), at any depth, so every radiance of that case is zero, scattered samples included: it pins the draw count alone.
EMPTY_FILMS = ("grad_disney_metal", "grad_sponza", "path_small_pt")

CLASS_TOLERANCE = {"lambert": 1e-9, "general": 1e-7, "envmap": 1e-6}

GRAD_COLUMNS = ("radiance", "contrib", "contribX0", "contribX1", "contribY0", "contribY1")     # 3 each, then the scalars
GRAD_SCALARS = ("prob", "wX0", "wY0", "wX1", "wY1")
FILM_BUFFERS = ("img", "cx0", "cy0", "cx1", "cy1")

# fourierSolve(w, h, c, cx, cy, alpha, out) on tests/test_poisson_oracle.lcg_fields(w, h)
FOURIER_CASES = [(8, 6, 0.04), (3, 2, 0.04), (2, 2, 0.04), (33, 20, 0.04), (64, 48, 0.04), (40, 30, 0.4), (40, 30, 40.0)]


def fourier_key(w, h, alpha):
    return f"{w}x{h}_a{alpha:g}"


def variant_xml(scene_variant, tmp_dir, case, film=None):
    """The XML a case is made from and tested on: tests/helpers.scene_variant's edits. film=None keeps the scene's own
    film (the scattered samples), film=(W, H) is the small film."""
    w, h = film if film else (None, None)
    return scene_variant(tmp_dir, case.scene, width=w, height=h, integrator=case.integrator, max_depth=case.max_depth,
                         rr_depth=case.rr_depth, tag=case.name + ("_film" if film else ""))
