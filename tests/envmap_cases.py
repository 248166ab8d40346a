"""Scenes and cases of the environment-map KAT (tests/test_envmap_cases.py on the CPU, tests/test_gpu_envmap_kat.py on the GPU).

Scenes: one small emitter-free rectangle under an environment map, parsed from an XML the test writes, the map a PFM beside it, so that
`to_local` is the inverse the loader makes. Every synthetic map under the identity and under a rotation about a skew axis with a scale
of 1.7; scenes/matpreview/envmap.exr under the transform of scenes/matpreview/matpreview.xml; an all-black map (it loads: both tables
take their uniform fallback).

Cases: one deterministic list per scene, built from the oracle's tables (build_cases). A case is a pair of random numbers (classes
rnd_*) or a direction (classes dir_*), given in the map's frame and mapped through `to_world` unless its id says "world".

Conditioning (condition_cases; the oracle alone):
  rule 2  a direction case keeps the exact comparisons only if, under a move of any one component by one part in 1e12 (a relative
          move: a zero stays zero, so that under the identity, where the local direction is the input itself, the seam and the borders
          stay), its discrete outcome (zero / non-zero pdf, which outputs are finite, the texel that dir_uv selects) stays; a quantity
          (dir_uv, dir_pdf, dir_emission) keeps its continuous comparison only if it moves by no more than 1e-6 under that move, and
  rule 1  only if the oracle's own value moves by less than a tenth of that quantity's bound under one ulp of any one component (the
          two-step form of tests/test_gpu_device_kat.py: one ulp, and 2^13 ulps scaled back).
What fails is listed by id in tests/golden/envmap_kat_edges_dropped.json: per scene "all" (the discrete outcome changes under rule 2: the
case keeps the comparison on finiteness alone) and one list per quantity (it moves by more than 1e-6 under rule 2, or fails rule 1: the
case stays under the exact comparisons, the quantity is reported, not bounded). A random-number case always keeps sample_uv (bit for bit)
and sample_dir; the pdf and the emission at its sampled direction follow the same rules at that direction (condition_cases)."""
import json
import math
import os

import numpy as np

from helpers import ROOT, SCENES

DROPPED_FILE = os.path.join(ROOT, "tests", "golden", "envmap_kat_edges_dropped.json")
ONE_BELOW = math.nextafter(1.0, 0.0)
STEP, MOVE, ULP_MOVE = 1e-12, 1e-6, 0.1
# starting bounds (the light family's and the texture family's) ; tests/test_gpu_envmap_kat.py holds the ones in force
START_BOUNDS = {"sample_dir": 1e-11, "sample_pdf": 1e-11, "dir_pdf": 1e-11, "dir_uv": 1e-11, "sample_emission": 1e-12, "dir_emission": 1e-12}
QUANTITIES = ("dir_uv", "dir_pdf", "dir_emission")
SEAM_X = (0.0, 1e-300, 1e-20, 1e-17, 1e-16, 1e-12, 1e-9, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)   # 1e-7 and up: so that the rotated scenes keep half
SEAM_Y = 0.3                  # the seam and the half line are walked at this height: y = 0 is a texel border of every map of even height
POLE_OFFSETS = (1e-12, 1e-9, 1e-6, 1e-4, 1e-3, 1e-2, 3e-2, 1e-1, 3e-1)     # 3e-2 and up: so that the class keeps more than half (a move of one
#                               part in 1e12 pushes cos(1e-6) above 1, and the pdf to 0)
BORDER_OFFSET = 1e-9
CDF_ENTRIES_MAX = 65          # a CDF with more entries gives every (n - 1) / 32-th of them, the first and the last included


# ---- maps (float32, as a PFM stores them) -------------------------------------------------------------------------------------------
def _smooth(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w, 3))
    for c in range(3):
        m[:, :, c] = 1.0 + 0.5 * np.cos(2 * np.pi * (x / w + rng.random())) * np.sin(np.pi * (y + 0.5) / h) + 0.3 * np.cos(2 * np.pi * (2 * y / h + rng.random()))
    return m + 0.15 * rng.random((h, w, 3))


def _bright6x4():
    m = np.array([[[0.2 + 0.1 * x + 0.05 * y, 0.3 + 0.02 * x * y, 0.25 + 0.04 * (5 - x)] for x in range(6)] for y in range(4)])
    m[2] = 0.0                 # a black row
    m[0, 1:3] = 0.0            # zero-width texels inside a lit row
    m[3, 4] = 0.0
    m[1, 4] = 50.0             # the single bright texel
    return m


def _columns5x3():
    m = np.array([[[0.4 + 0.1 * x + 0.2 * y, 0.5, 0.3 + 0.1 * y] for x in range(5)] for y in range(3)])
    m[:, 0] = 0.0
    m[:, 4] = 0.0
    return m


MAPS = {
    "1x1": lambda: np.array([[[0.7, 0.5, 0.3]]]),
    "2x1": lambda: np.array([[[0.9, 0.2, 0.1], [0.1, 0.4, 0.8]]]),
    "1x2": lambda: np.array([[[0.9, 0.2, 0.1]], [[0.1, 0.4, 0.8]]]),
    "6x4": _bright6x4,
    "5x3": _columns5x3,
    "64x32": lambda: _smooth(64, 32, 20240611),
    "black4x2": lambda: np.zeros((2, 4, 3)),
}


def _rotation(axis, angle, scale):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return scale * (np.eye(3) + math.sin(angle) * k + (1 - math.cos(angle)) * (k @ k))


TRANSFORMS = {"identity": np.eye(3), "rotated": _rotation((0.3, -0.5, 0.81), 1.1, 1.7)}
MATPREVIEW_TRANSFORM = """<rotate y="1" angle="-180"/>
      <matrix value="-0.224951 -0.000001 -0.974370 0.000000 -0.974370 0.000000 0.224951 0.000000 0.000000 1.000000 -0.000001 8.870000 0.000000 0.000000 0.000000 1.000000 "/>"""

# (scene, map, transform)
SCENE_LIST = [(f"{m}/{t}", m, t) for m in ("1x1", "2x1", "1x2", "6x4", "5x3", "64x32") for t in ("identity", "rotated")] + \
             [("black4x2/rotated", "black4x2", "rotated"), ("matpreview", "matpreview", "matpreview")]
SCENE_NAMES = [s for s, _, _ in SCENE_LIST]

XML = """<?xml version="1.0" encoding="utf-8"?>
<scene version="0.5.0">
  <integrator type="path"><integer name="maxDepth" value="3"/></integrator>
  <sensor type="perspective">
    <float name="fov" value="45"/>
    <transform name="toWorld"><lookAt origin="0, 0, 4" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="independent"><integer name="sampleCount" value="1"/></sampler>
    <film type="hdrfilm"><integer name="width" value="16"/><integer name="height" value="16"/></film>
  </sensor>
  <bsdf type="diffuse" id="grey"><rgb name="reflectance" value="0.5 0.5 0.5"/></bsdf>
  <shape type="rectangle"><ref name="bsdf" id="grey"/></shape>
  <emitter type="envmap">
    <string name="filename" value="%s"/>
    <transform name="toWorld">
      %s
    </transform>
    <float name="scale" value="%s"/>
  </emitter>
</scene>
"""


def write_pfm(path, rgb):
    """rgb: (h, w, 3); rows in file order (the loader does not flip them)."""
    rgb = np.ascontiguousarray(rgb, dtype="<f4")
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())


def write_scene(tmp_dir, scene):
    """Writes the scene's XML (and its map) into tmp_dir; returns the XML's path."""
    _, map_name, transform = next(s for s in SCENE_LIST if s[0] == scene)
    stem = scene.replace("/", "_")
    if map_name == "matpreview":
        filename, xform, scale = os.path.join(SCENES, "matpreview", "envmap.exr"), MATPREVIEW_TRANSFORM, "3"
    else:
        filename = os.path.join(str(tmp_dir), stem + ".pfm")
        write_pfm(filename, MAPS[map_name]())
        m = np.eye(4)
        m[:3, :3] = TRANSFORMS[transform]
        xform, scale = '<matrix value="%s"/>' % " ".join(repr(float(x)) for x in m.ravel()), "1.5"
    xml = os.path.join(str(tmp_dir), stem + ".xml")
    with open(xml, "w") as f:
        f.write(XML % (filename, xform, scale))
    return xml


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def _entries(n):
    """Indices of a CDF of n entries that the list takes."""
    return list(range(n)) if n <= CDF_ENTRIES_MAX else sorted({round(k * (n - 1) / 32) for k in range(33)})


def _around(v):
    """v exactly and one ulp either side, inside [0, 1)."""
    return [(tag, x) for tag, x in (("-", math.nextafter(v, -math.inf)), ("", v), ("+", math.nextafter(v, math.inf))) if 0.0 <= x <= ONE_BELOW]


def cdf_rows_of(t, black_rows=()):
    """The three rows whose CDF values the list takes: the first row that is not black, a black row (the middle row where the map
    has none), the last."""
    h = len(t["pdf_marginals"])
    lit = [y for y in range(h) if y not in black_rows]
    return sorted({lit[0] if lit else 0, black_rows[0] if len(black_rows) else h // 2, h - 1})


def _row_selector(t, y):
    """A rnd.y for row y: the middle of its marginal interval, or the interval's one point where it has no width."""
    a, b = t["cdf_marginals"][y], t["cdf_marginals"][y + 1]
    return min(a + 0.5 * (b - a), ONE_BELOW)


def dir_of_uv(u, v):
    az, el = 2 * math.pi * u, math.pi * v
    return (math.sin(az) * math.sin(el), math.cos(el), -math.cos(az) * math.sin(el))


def build_cases(osc, to_world, black_rows=(), seed=7):
    """The scene's list: dict of `id` (list of str), `cls` (list of str), `rnd` (n, 2), `dir` (n, 3; world), `is_dir` (n, bool).
    A random-number case carries the direction (1, 2, 3) / sqrt(14) in the map's frame, a direction case rnd = (0.5, 0.5).
    black_rows: the rows of the map that hold no light. (make_table_dist_2d gives such a row the weight 1 of its uniform fallback, so
    its interval of the marginal CDF has a width and sampling reaches it; a black texel of a lit row has none.)"""
    t = osc.envmap_tables()
    w, h = osc.envmap_size()
    to_world = np.asarray(to_world, dtype=np.float64).reshape(4, 4)[:3, :3]
    rng = np.random.default_rng(seed)
    rnd = []                                            # (class, id, rx, ry)
    for k, (a, b) in enumerate(rng.random((200, 2))):
        rnd.append(("rnd_interior", f"rnd_interior/{k}", a, b))
    for i, a in enumerate((0.0, ONE_BELOW, 0.37)):
        for j, b in enumerate((0.0, ONE_BELOW, 0.61)):
            if (i, j) != (2, 2):
                rnd.append(("rnd_ends", f"rnd_ends/{i}{j}", a, b))
    for y in _entries(h + 1):
        for tag, v in _around(t["cdf_marginals"][y]):
            rnd.append(("rnd_cdf_marginal", f"rnd_cdf_marginal/{y}{tag}", 0.37, v))
    black = list(black_rows)
    for y in cdf_rows_of(t, black):
        for x in _entries(w + 1):
            for tag, v in _around(t["cdf_rows"][y, x]):
                rnd.append(("rnd_cdf_row", f"rnd_cdf_row/{y}/{x}{tag}", v, _row_selector(t, y)))
    for y in black[:16]:                                # inside the interval of a black row, and on its two ends ...
        for k, a in enumerate((0.25, 0.75)):
            rnd.append(("rnd_zero_width", f"rnd_zero_width/row{y}/{k}", a, _row_selector(t, y)))
            rnd.append(("rnd_zero_width", f"rnd_zero_width/row{y}/end{k}", a, min(t["cdf_marginals"][y + k], ONE_BELOW)))
    zero = [(y, x) for y in range(h) for x in range(w) if t["cdf_rows"][y, x + 1] == t["cdf_rows"][y, x]]
    for y, x in zero[:32]:                              # ... and inside the zero-width interval of a black texel in a lit row
        if t["cdf_rows"][y, x] <= ONE_BELOW:
            rnd.append(("rnd_zero_width", f"rnd_zero_width/texel{y}_{x}", t["cdf_rows"][y, x], _row_selector(t, y)))
    for name, (x, y) in (("first", (0, 0)), ("last", (w - 1, h - 1))):
        a = 0.5 * (t["cdf_rows"][y, x] + t["cdf_rows"][y, x + 1])
        rnd.append(("rnd_cell_mid", f"rnd_cell_mid/{name}", min(a, ONE_BELOW), _row_selector(t, y)))

    dirs = []                                           # (class, id, local direction or None, world direction or None)
    g = rng.standard_normal((400, 3))
    for k, v in enumerate(g / np.linalg.norm(g, axis=1, keepdims=True)):
        dirs.append(("dir_sphere", f"dir_sphere/{k}", tuple(v), None))
    for s, name in ((1.0, "+y"), (-1.0, "-y")):
        dirs.append(("dir_pole", f"dir_pole/{name}", (0.0, s, 0.0), None))
        dirs.append(("dir_pole", f"dir_pole/{name}/world", None, (0.0, s, 0.0)))
        for e in POLE_OFFSETS:
            for k in range(4):
                az = 0.3 + k * math.pi / 2
                dirs.append(("dir_pole", f"dir_pole/{name}/{e:g}/{k}", (math.sin(e) * math.cos(az), s * math.cos(e), math.sin(e) * math.sin(az)), None))
    for cls, z in (("dir_seam", -1.0), ("dir_half", 1.0)):
        for x in SEAM_X:
            for s, sign in ((1.0, "+"), (-1.0, "-")):
                dirs.append((cls, f"{cls}/{sign}{x:g}", (s * x, SEAM_Y, z), None))
    if w * h <= 64:
        for y in range(h):
            for x in range(w):
                dirs.append(("dir_texel_centre", f"dir_texel_centre/{x}_{y}", dir_of_uv((x + 0.5) / w, (y + 0.5) / h), None))
    us, vs = _entries(w + 1) if w <= 8 else [round(k * w / 8) for k in range(9)], list(range(1, h)) if h <= 8 else [round(k * h / 8) for k in range(1, 8)]
    v_mid = [(y + 0.5) / h for y in sorted({0, h // 2, h - 1})]
    u_mid = [(x + 0.5) / w for x in sorted({0, w // 2, w - 1})]
    for i in us:
        for tag, off in (("-", -BORDER_OFFSET), ("", 0.0), ("+", BORDER_OFFSET)):
            for k, v in enumerate(v_mid):
                dirs.append(("dir_border", f"dir_border/u{i}{tag}/{k}", dir_of_uv(i / w + off, v), None))
    for j in vs:
        for tag, off in (("-", -BORDER_OFFSET), ("", 0.0), ("+", BORDER_OFFSET)):
            for k, u in enumerate(u_mid):
                dirs.append(("dir_border", f"dir_border/v{j}{tag}/{k}", dir_of_uv(u, j / h + off), None))

    rnd_arr = np.array([[a, b] for _, _, a, b in rnd])
    fed = osc.envmap_sample_dir(rnd_arr)                 # the sampled directions of the random-number cases, fed back
    for k, (cls, rid, _, _) in enumerate(rnd):           # (not those of the CDF values: they lie on texel borders by construction,
        if not cls.startswith("rnd_cdf_"):               # where rule 2 keeps none; dir_border holds such directions, a third of them exact)
            dirs.append(("dir_fed_back", f"dir_fed_back/{rid}", None, tuple(fed[k])))
    if (len(rnd) + len(dirs)) % 64 == 0:                 # never whole waves: the last one keeps idle lanes
        rnd.append(("rnd_interior", "rnd_interior/extra", 0.123456789, 0.987654321))
        rnd_arr = np.vstack([rnd_arr, [[0.123456789, 0.987654321]]])

    default_dir = to_world @ (np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0))
    world = np.array([wd if wd is not None else tuple(to_world @ np.array(ld)) for _, _, ld, wd in dirs])
    n_r, n_d = len(rnd), len(dirs)
    return {
        "id": [r[1] for r in rnd] + [d[1] for d in dirs], "cls": [r[0] for r in rnd] + [d[0] for d in dirs],
        "rnd": np.vstack([rnd_arr, np.full((n_d, 2), 0.5)]), "dir": np.vstack([np.tile(default_dir, (n_r, 1)), world]),
        "is_dir": np.array([False] * n_r + [True] * n_d),
    }


# ---- the oracle's answers and the conditioning rules ---------------------------------------------------------------------------------
def oracle_dir(osc, d):
    """dir_uv (n, 2), dir_pdf (n), dir_emission (n, 3) for world directions d, as the KAT kernel forms them."""
    d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1, 3)
    return {"dir_uv": osc.envmap_dir_uv(d), "dir_pdf": osc.envmap_pdf(-d), "dir_emission": osc.envmap_emission(-d)}


def oracle_rnd(osc, rnd):
    sd = osc.envmap_sample_dir(rnd)
    return {"sample_uv": osc.envmap_table_sample(rnd), "sample_dir": sd, "sample_pdf": osc.envmap_pdf(-sd), "sample_emission": osc.envmap_emission(-sd)}


def texel_of(uv, w, h):
    """The texel of table2d_pdf that uv selects: (int) of uv.x w and of uv.y h, each clamped to the table as table2d_pdf clamps it."""
    uv = np.asarray(uv, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.stack([np.trunc(np.clip(uv[:, 0] * w, 0.0, w - 1.0)), np.trunc(np.clip(uv[:, 1] * h, 0.0, h - 1.0))], axis=1)


def discrete(ans, w, h):
    """Per case: pdf zero or not, which outputs are finite, the texel."""
    flat = np.column_stack([ans["dir_uv"], ans["dir_pdf"], ans["dir_emission"]])
    return np.column_stack([ans["dir_pdf"] != 0, np.isfinite(flat), np.nan_to_num(texel_of(ans["dir_uv"], w, h), nan=-1.0)])


def moved(a, b):
    """Per case: largest |a - b| / max(1, |b|) over the row; a change of finiteness counts as infinite."""
    a, b = np.asarray(a, dtype=np.float64).reshape(len(a), -1), np.asarray(b, dtype=np.float64).reshape(len(b), -1)
    with np.errstate(invalid="ignore"):
        e = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    fin = np.isfinite(a) & np.isfinite(b)
    same_special = (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & (a == b))
    e = np.where(fin, e, np.where(same_special, 0.0, np.inf))
    return e.max(axis=1)


def condition_dirs(osc, d, bounds=None):
    """The two rules on world directions d: (unstable (n): rule 2's discrete outcome changes; ill: quantity -> (n), the quantity moves
    by more than 1e-6 under rule 2's move or fails rule 1)."""
    bounds = bounds or START_BOUNDS
    w, h = osc.envmap_size()
    d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1, 3)
    base = oracle_dir(osc, d)
    d0 = discrete(base, w, h)
    unstable = np.zeros(len(d), dtype=bool)
    ill = {q: np.zeros(len(d), dtype=bool) for q in QUANTITIES}
    for k in range(3):                                                   # rule 2
        for sign in (-1.0, 1.0):
            d2 = d.copy()
            d2[:, k] = d[:, k] * (1.0 + sign * STEP)
            a2 = oracle_dir(osc, d2)
            unstable |= (discrete(a2, w, h) != d0).any(axis=1)
            for q in QUANTITIES:
                ill[q] |= moved(a2[q], base[q]) > MOVE
    for k in range(3):                                                   # rule 1
        for toward in (-math.inf, math.inf):
            one = np.nextafter(d[:, k], toward)
            for x, scale in ((one, 1.0), (d[:, k] + (one - d[:, k]) * 8192.0, 1.0 / 8192.0)):
                d2 = d.copy()
                d2[:, k] = x
                bad = ~(np.isfinite(d2).all(axis=1) & (d2 != 0).any(axis=1))
                d2[bad] = d[bad]
                a2 = oracle_dir(osc, d2)
                for q in QUANTITIES:
                    ill[q] |= scale * moved(a2[q], base[q]) > ULP_MOVE * bounds[q]
    return unstable, ill


def condition_cases(osc, cases, bounds=None):
    """Applies the rules to the scene's list. Direction cases: "all" = ids that leave every comparison but the one on finiteness,
    quantity = ids that lose that quantity's continuous comparison (among those that stay). Random-number cases: the pdf and the emission
    of a sampled direction are evaluated at a direction a few ulps from the oracle's, so they follow the rules at the oracle's
    sampled direction: "sample_all" = ids that lose the zero / non-zero and the continuous comparison of sample_pdf (the texel is the
    pdf's alone: the emission is continuous across a texel border), "sample_pdf" / "sample_emission" = ids that lose that continuous
    comparison. sample_uv and sample_dir are compared for every case."""
    is_dir = cases["is_dir"]
    ids = np.array(cases["id"], dtype=object)
    unstable, ill = condition_dirs(osc, cases["dir"][is_dir], bounds)
    out = {"all": ids[is_dir][unstable].tolist()}
    for q in QUANTITIES:
        out[q] = ids[is_dir][ill[q] & ~unstable].tolist()
    sd = osc.envmap_sample_dir(cases["rnd"][~is_dir])
    unstable, ill = condition_dirs(osc, sd, bounds)
    out["sample_all"] = ids[~is_dir][unstable].tolist()
    out["sample_pdf"] = ids[~is_dir][ill["dir_pdf"] & ~unstable].tolist()
    out["sample_emission"] = ids[~is_dir][ill["dir_emission"]].tolist()
    return out


def load_dropped():
    with open(DROPPED_FILE) as f:
        return json.load(f)


def masks(cases, dropped):
    """keep (n): the direction case stays under the exact comparisons; ok[quantity] (n): the case keeps that quantity's continuous
    comparison; sample_keep (n): the random-number case keeps the zero / non-zero comparison of sample_pdf."""
    ids = cases["id"]
    member = lambda key: np.array([i in set_ for i in ids]) if (set_ := set(dropped[key])) else np.zeros(len(ids), dtype=bool)
    is_dir = cases["is_dir"]
    keep = is_dir & ~member("all")
    ok = {q: keep & ~member(q) for q in QUANTITIES}
    sample_keep = ~is_dir & ~member("sample_all")
    ok["sample_pdf"], ok["sample_emission"] = sample_keep & ~member("sample_pdf"), ~is_dir & ~member("sample_emission")
    return keep, sample_keep, ok


def black_rows_of(scene):
    """Rows of the scene's map without light (the shipped map has none)."""
    _, map_name, _ = next(s for s in SCENE_LIST if s[0] == scene)
    return [y for y, row in enumerate(MAPS[map_name]()) if not row.any()] if map_name in MAPS else []


class World:
    """One scene of the list: the parsed description, the oracle on it, its cases."""

    def __init__(self, G, O, tmp_dir, scene):
        self.name = scene
        self.sd = G.parse_scene(write_scene(tmp_dir, scene))
        self.osc = O.OracleScene(self.sd.ptr)
        self.w, self.h = self.osc.envmap_size()
        self.tables = self.osc.envmap_tables()
        self.black = black_rows_of(scene)
        self.cases = build_cases(self.osc, list(self.sd.desc.envmap.to_world), self.black)


def find_dropped(G, O, tmp_dir):
    """scene -> the lists of condition_cases, for every scene."""
    out = {}
    for scene in SCENE_NAMES:
        wd = World(G, O, tmp_dir, scene)
        out[scene] = condition_cases(wd.osc, wd.cases)
    return out
