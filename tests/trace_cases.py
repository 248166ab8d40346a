"""Scenes and ray lists of the ray-by-ray traversal tests (tests/test_trace_cases.py on the CPU, tests/test_gpu_trace_kat.py on the GPU).

Everything is deterministic (numpy generators with fixed seeds). Origins stay inside the scene bounds or at the camera: the host's box
padding (csrc/hip/device_trace.h, box_hit) promises nothing outside that range. A ray list is a numpy array of RAY records, the layout
of GdptKatTraceQuery; the oracle's answer to a list is `Case.want(name)` = (gid, float32 [n, 6] = t, u, v, ng), computed once.

Scenes: cbox; odd_room (tests/helpers.py) with a sphere emitter, leaves of 1 .. 4 records; a lattice of axis-aligned unit
quads on integer coordinates with every fifth quad listed twice (exact ties in t), in two listing orders; a chain of triangles whose
sizes grow geometrically along a line (a BVH4 whose stack bound exceeds the 16 LDS levels of the wavefront trace kernel); sponza.
Classes: (a) camera rays, (b) bounce rays off their hits, (c) axis-parallel rays on lattice coordinates, (d) one tiny direction
component, (e) [tnear, tfar) windows at the hit distance and one ulp beside it, (f) ties, (g) shadow rays, (h) sphere edges.
"""
import numpy as np

from helpers import DescBuilder, _camera, _quad, odd_room_builder, scene_variant

RAY = np.dtype([("org", "f8", 3), ("dir", "f8", 3), ("tnear", "f8"), ("tfar", "f8"), ("any_hit", "i4"), ("pad", "i4")])
RESULT = np.dtype([("gid", "i4"), ("t", "f4"), ("u", "f4"), ("v", "f4"), ("ng", "f4", 3)])
FILM = (48, 32)
TINY = (1e-30, 1e-36, 1e-37, 1e-38, 2e-39, 1e-42)
WF_LDS_LEVELS = 16          # kWfLdsLevels (csrc/hip/render_wavefront.h); the table's wavefront rows report it, the GPU test compares


def rays(org, dirv, tnear=0.0, tfar=np.inf, any_hit=0):
    org, dirv = np.atleast_2d(np.asarray(org, float)), np.atleast_2d(np.asarray(dirv, float))
    n = max(len(org), len(dirv))
    r = np.zeros(n, RAY)
    r["org"], r["dir"], r["tnear"], r["tfar"], r["any_hit"] = org, dirv, tnear, tfar, any_hit
    return r


def as_oracle(r):
    return np.concatenate([r["org"], r["dir"], r["tnear"][:, None], r["tfar"][:, None]], axis=1)


def overflows(r):
    """Rays with an axis whose fp32 1/d or o/d is not finite although d is not zero: the slab arithmetic of that axis degenerates."""
    o, d = r["org"].astype(np.float32), r["dir"].astype(np.float32)
    with np.errstate(all="ignore"):
        inv = np.float32(1) / d
        oi = o * inv
    return np.any((d != 0) & ~(np.isfinite(inv) & np.isfinite(oi)), axis=1)


def unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def cosine_dirs(normals, rng):
    """Cosine-distributed directions about unit normals."""
    n = unit(normals)
    a = np.where(np.abs(n[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    t = unit(np.cross(n, a))
    b = np.cross(n, t)
    u1, u2 = rng.random(len(n)), rng.random(len(n))
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    return unit(t * (r * np.cos(phi))[:, None] + b * (r * np.sin(phi))[:, None] + n * np.sqrt(1 - u1)[:, None])


class Built:
    """Duck-typed SceneDesc (ptr, width, height) over a DescBuilder."""

    def __init__(self, b):
        self.owner, self.ptr = b, b.finish()
        self.desc = b.desc
        self.width, self.height = b.desc.camera.width, b.desc.camera.height


class Case:
    """A scene, how to upload it, and its ray lists with the oracle's answers."""

    def __init__(self, G, O, name, sd, upload_knobs=None, oracle_bvh=False):
        self.G, self.name, self.sd, self.upload_knobs = G, name, sd, dict(upload_knobs or {})
        with G.debug_knobs(**self.upload_knobs):
            self.prepared = G.debug_knobs.prepare_scene(sd)
        self.eps = self.prepared["isect_eps"]
        self.lo, self.hi = np.array(self.prepared["bounds"][:3], float), np.array(self.prepared["bounds"][3:], float)
        self.oracle = O.OracleScene(sd.ptr, use_bvh=oracle_bvh)
        self.brute = self.oracle if not oracle_bvh else O.OracleScene(sd.ptr, use_bvh=False)
        self.oracle_bvh = oracle_bvh
        self.lists, self._want = {}, {}
        self.cam = np.array(self.oracle.sample_primary(0.5, 0.5)[0])

    def upload(self):
        with self.G.debug_knobs(**self.upload_knobs):
            return self.G.Scene(self.sd)

    def add(self, name, r):
        assert name not in self.lists and len(r) % 64 != 0, (name, len(r))
        o = r["org"]
        inside = np.all((o >= self.lo) & (o <= self.hi), axis=1) | np.all(o == self.cam, axis=1)
        assert inside.all(), (self.name, name, "origin outside the scene bounds", o[~inside][:3])
        self.lists[name] = r
        return r

    def want(self, name):
        """The oracle's answer to a list: the brute force; on a scene whose oracle walks its own BVH (sponza) the brute force still
        answers the one-ulp windows, the class in which a tree's boxes decide most."""
        if name not in self._want:
            osc = self.brute if name.startswith("e_") else self.oracle
            self._want[name] = osc.closest_hits(as_oracle(self.lists[name]))
        return self._want[name]

    def hit_rate(self, name):
        return float(np.mean(self.want(name)[0] >= 0))

    def interior(self, n, rng, margin=0.02):
        ext = self.hi - self.lo
        return self.lo + ext * (margin + (1 - 2 * margin) * rng.random((n, 3)))

    # ---- the classes every scene gets --------------------------------------------------------------------------------------------
    def add_camera(self, n, seed):
        rng = np.random.default_rng(seed)
        o, d = zip(*[self.oracle.sample_primary(float(x), float(y)) for x, y in rng.random((n, 2))])
        return self.add("a_camera", rays(np.array(o), np.array(d)))

    def hit_points(self, name):
        """(rays that hit, their points, unit normals turned against the ray, fp32 t)."""
        r = self.lists[name]
        gid, h = self.want(name)
        k = gid >= 0
        t = h[k, 0]
        p = r["org"][k] + r["dir"][k] * t.astype(float)[:, None]
        n = unit(h[k, 3:6].astype(float))
        n = np.where(np.sum(n * r["dir"][k], axis=1, keepdims=True) > 0, -n, n)
        return r[k], p, n, t

    def add_bounce(self, seed, source="a_camera", name="b_bounce", through=False):
        """through: every second ray leaves on the far side of its surface (an open scene, whose reflected rays nearly all escape)."""
        rng = np.random.default_rng(seed)
        _, p, n, _ = self.hit_points(source)
        p = np.clip(p, self.lo, self.hi)
        if len(p) % 64 == 0:
            p, n = p[:-1], n[:-1]
        if through:
            n = n * np.where(np.arange(len(n)) % 2, -1.0, 1.0)[:, None]
        return self.add(name, rays(p, cosine_dirs(n, rng), tnear=self.eps))

    def add_windows(self, sources=("a_camera", "b_bounce"), cap=1500):
        """From the oracle's fp32 t of each hit: tnear = t (the same hit), tnear = nextafter(t) (not that hit), tfar = t (not that
        hit), tfar = nextafter(t) (that hit). Lists e_near0 / e_near1 and e_far0 / e_far1 pair up ray by ray."""
        src = np.concatenate([self.hit_points(s)[0] for s in sources])
        t = np.concatenate([self.hit_points(s)[3] for s in sources])
        keep = np.flatnonzero(t.astype(float) >= src["tnear"])[:cap]
        if len(keep) % 64 == 0:
            keep = keep[:-1]
        src, t = src[keep], t[keep]
        up = np.nextafter(t, np.float32(np.inf)).astype(float)
        for name, field, value in (("e_near0", "tnear", t.astype(float)), ("e_near1", "tnear", up), ("e_far0", "tfar", t.astype(float)), ("e_far1", "tfar", up)):
            r = src.copy()
            r[field] = value
            if field == "tfar":
                r["tnear"] = np.minimum(r["tnear"], value)
            self.add(name, r)

    def add_shadow(self, seed, n, sources=("a_camera", "b_bounce")):
        """any_hit rays between pairs of surface points, as render_path.h forms its shadow rays: dir = normalize(q - p), tnear = eps,
        tfar = (1 - eps) |q - p|."""
        rng = np.random.default_rng(seed)
        pts = np.clip(np.concatenate([self.hit_points(s)[1] for s in sources]), self.lo, self.hi)
        # eight candidates per ray wanted; the oracle says which are occluded, and the list takes the first n / 2 of either kind it
        # finds (a closed room with a few blocks occludes one pair in eight, too few to exercise the early exit)
        i, j = rng.integers(0, len(pts), 8 * n), rng.integers(0, len(pts), 8 * n)
        d = pts[j] - pts[i]
        dist = np.linalg.norm(d, axis=1)
        k = dist > 50 * self.eps
        i, d, dist = i[k], d[k], dist[k]
        cand = rays(pts[i], d / dist[:, None], tnear=self.eps, tfar=(1 - self.eps) * dist, any_hit=1)
        occ = self.oracle.closest_hits(as_oracle(cand))[0] >= 0
        take = np.sort(np.concatenate([np.flatnonzero(occ)[:n // 2], np.flatnonzero(~occ)[:n - n // 2]]))
        if len(take) % 64 == 0:
            take = take[:-1]
        return self.add("g_shadow", cand[take])

    def add_axis_parallel(self, seed, n, origins):
        """One and two direction components exactly +0.0 and -0.0."""
        rng = np.random.default_rng(seed)
        d = unit(rng.normal(size=(n, 3)))
        for i in range(n):
            zero = rng.permutation(3)[:1 + (i % 2)]
            d[i, zero] = np.where(rng.random(len(zero)) < 0.5, 0.0, -0.0)
        return self.add("c_axis", rays(origins[:n], unit(d)))

    def add_tiny(self, seed, n, origins):
        """One direction component in +-TINY, the others generic."""
        rng = np.random.default_rng(seed)
        d = unit(rng.normal(size=(n, 3)))
        for i in range(n):
            d[i, rng.integers(0, 3)] = TINY[i % len(TINY)] * (1 if (i // len(TINY)) % 2 else -1)
        return self.add("d_tiny", rays(origins[:n], d))


def targeted_origins(case, n, seed, step=None):
    """Origins: the camera (every third) and interior points, those snapped to multiples of `step` if given."""
    rng = np.random.default_rng(seed)
    o = case.interior(n, rng)
    if step:
        o = np.clip(np.round(o / step) * step, case.lo, case.hi)
    o[::3] = case.cam
    return o


# ---- the scenes ------------------------------------------------------------------------------------------------------------------
def cbox(G, O, tmp):
    c = Case(G, O, "cbox", G.parse_scene(scene_variant(tmp, "cbox/cbox_gdpt.xml", width=FILM[0], height=FILM[1])))
    c.add_camera(1501, 11)
    c.add_bounce(12)
    c.add_axis_parallel(13, 1001, targeted_origins(c, 1001, 14, step=8.0))
    c.add_tiny(15, 1201, targeted_origins(c, 1201, 16))
    c.add_windows()
    c.add_shadow(17, 1500)
    return c


def odd_room_case(G, O):
    b = odd_room_builder(G, FILM)
    dark = b.material(G.MAT_LAMBERTIAN, [DescBuilder.const_tex(G, 0.0)])
    centre, radius = np.array([1.0, -1.2, -0.8]), 0.5
    b.sphere(tuple(centre), radius, dark, light=(5.0, 4.0, 3.0))
    c = Case(G, O, "odd_room", Built(b), upload_knobs={"bvh_leaf_max": 4, "bvh_leaf_factor": 0.8})
    c.sphere = (centre, radius)
    c.add_camera(1501, 21)
    c.add_bounce(22)
    c.add_axis_parallel(23, 1001, targeted_origins(c, 1001, 24, step=0.25))
    # (coordinates of +-2 at most: o / d overflows from |d| = 1e-38 down, 1 / d from the denormals on)
    c.add_tiny(25, 1201, targeted_origins(c, 1201, 26))
    c.add_windows()
    c.add_shadow(27, 1500)
    # (h) the sphere: tangent rays and small offsets to both sides, from near origins and from the far corner of the room; origins
    # inside the sphere; a sphere hit and a triangle hit at nearly the same distance (the sphere's lowest point is 0.3 above the
    # floor: rays that graze its underside meet the floor a little later; and rays through the sphere's silhouette onto the block)
    rng = np.random.default_rng(28)
    far = np.array([-1.95, 1.95, 1.95])
    out = []
    for k in range(900):
        o = far if k % 3 == 0 else centre + unit(rng.normal(size=3)) * radius * (1.05 + 2.0 * rng.random())
        o = np.clip(o, c.lo + 1e-3, c.hi - 1e-3)
        to_c = centre - o
        dist = np.linalg.norm(to_c)
        side = unit(np.cross(to_c, rng.normal(size=3)))
        # the tangent direction touches the sphere at angle asin(r / dist) off the line to the centre
        off = (0.0, 1e-7, -1e-7, 1e-5, -1e-5, 1e-3, -1e-3, 3e-2, -3e-2, 0.3)[k % 10]
        ang = np.arcsin(min(1.0, radius / dist)) * (1 + off)
        out.append((o, unit(unit(to_c) * np.cos(ang) + side * np.sin(ang))))
    for k in range(200):
        out.append((centre + unit(rng.normal(size=3)) * radius * 0.98 * rng.random(), unit(rng.normal(size=3))))
    for k in range(201):
        # down past the sphere's underside onto the floor (y = -2): the two hits lie within 0.3 of each other
        p = centre + np.array([0.3 * rng.normal(), -radius, 0.3 * rng.normal()]) * np.array([radius, 1.0, radius])
        o = np.clip(p + np.array([rng.normal(), 2.0 + rng.random(), rng.normal()]), c.lo + 1e-3, c.hi - 1e-3)
        out.append((o, unit(p - o)))
    o, d = zip(*out)
    c.add("h_sphere", rays(np.array(o), np.array(d)))
    return c


def lattice_builder(G, twins_first):
    """Unit quads on the integer planes of [0, 6]^3, about a third of all cells, one mesh each; every fifth quad has a twin: the same
    four corners and indices again, so v0, e1, e2 of its triangles are identical. twins_first: the twins are listed before all the
    originals instead of after them, so the lower id of a pair is the twin's. Returns (builder, pairs of triangle ids)."""
    N = 6
    rng = np.random.default_rng(31)
    b = DescBuilder(G)
    grey = b.material(G.MAT_LAMBERTIAN, [DescBuilder.const_tex(G, 0.6)])
    quads = []
    for axis in range(3):
        u, v = [k for k in range(3) if k != axis]
        for c in range(N + 1):
            for i in range(N):
                for j in range(N):
                    if rng.random() < 0.20:
                        pts = []
                        for a, bb in ((0, 0), (1, 0), (1, 1), (0, 1)):
                            q = [0.0] * 3
                            q[axis], q[u], q[v] = c, i + a, j + bb
                            pts.append(q)
                        quads.append(pts)
    twin_of = [k for k in range(len(quads)) if k % 5 == 0]
    order = [("twin", k) for k in twin_of] + [("orig", k) for k in range(len(quads))] if twins_first else \
            [("orig", k) for k in range(len(quads))] + [("twin", k) for k in twin_of]
    shape_of = {}
    for s, (kind, k) in enumerate(order):
        _quad(b, quads[k], grey, (3.0, 3.0, 3.0), light=(4.0, 4.0, 4.0) if s == 0 else None)
        shape_of[(kind, k)] = s
    pairs = [(2 * shape_of[("orig", k)] + tri, 2 * shape_of[("twin", k)] + tri) for k in twin_of for tri in (0, 1)]
    _camera(G, b.desc.camera, *FILM, pos=(3.3, 3.4, 5.9), fov=100.0)
    return b, pairs, [quads[k] for k in twin_of]


def lattice(G, O, twins_first=False):
    b, pairs, twin_quads = lattice_builder(G, twins_first)
    c = Case(G, O, "lattice_twins_first" if twins_first else "lattice", Built(b))
    c.pairs = pairs
    c.add_camera(1501, 32)
    c.add_bounce(33)
    # (c) origins ON lattice coordinates: the rays lie in box planes and pass through shared edges and vertices
    rng = np.random.default_rng(34)
    c.add_axis_parallel(35, 1501, rng.integers(0, 7, (1501, 3)).astype(float))
    c.add_tiny(36, 1201, np.where(rng.random((1201, 1)) < 0.5, rng.integers(0, 7, (1201, 3)).astype(float), c.interior(1201, rng)))
    c.add_windows()
    c.add_shadow(37, 1500)
    # (f) rays onto the twin quads: interior points, points on their edges and their corners
    o, d = [], []
    for k in range(1201):
        q = np.array(twin_quads[k % len(twin_quads)], float)
        s, t = ((rng.random(), rng.random()), (rng.random(), 0.0), (1.0, rng.random()), (0.0, 0.0), (0.5, 0.5))[k % 5]
        target = q[0] + s * (q[1] - q[0]) + t * (q[3] - q[0])
        org = c.interior(1, rng)[0] if k % 2 else rng.integers(0, 7, 3).astype(float)
        if np.linalg.norm(target - org) < 1e-6:
            org = c.cam
        o.append(org)
        d.append(unit(target - org))
    c.add("f_ties", rays(np.array(o), np.array(d)))
    return c


def deep(G, O):
    """26 triangles across the z axis whose sizes and distances grow by half from one to the next, one record per leaf. The SAH builder
    splits such a row unevenly (BVH2 depth 11), and the collapsed BVH4 keeps up to three pushes per node along its longest path: a
    stack bound of 23, above the 16 LDS levels of the wavefront trace kernel, while the BVH2 still fits the 12-slot LDS column. The
    camera looks along the chain from its small end, so a ray's nearest child is the rest of the chain and the leaves beside it are
    pushed."""
    b = DescBuilder(G)
    grey = b.material(G.MAT_LAMBERTIAN, [DescBuilder.const_tex(G, 0.6)])
    n = 26
    for i in range(n):
        s, z = 0.3 * 1.5 ** i, -(1.5 ** i)
        ang = 2.4 * i
        cx, cy = 0.45 * s * np.cos(ang), 0.45 * s * np.sin(ang)
        b.mesh([cx - s, cy - s, z, cx + s, cy - s, z, cx, cy + s, z], [0, 1, 2], grey, light=(3.0, 3.0, 3.0) if i == 0 else None)
    _camera(G, b.desc.camera, *FILM, pos=(0.0, 0.0, -0.5), fov=60.0)
    c = Case(G, O, "deep", Built(b), upload_knobs={"bvh_leaf_max": 1})
    c.add_camera(1501, 41)
    c.add_bounce(42, through=True)
    rng = np.random.default_rng(43)
    # from the small end into the chain, and between random points of the bounds
    o = np.tile(c.cam, (1001, 1))
    o[1::2] = c.interior(1001, rng)[1::2]
    c.add("c_along", rays(o, unit(np.array([0.0, 0.0, -1.0]) + 0.35 * rng.normal(size=(1001, 3)))))
    c.add_windows()
    c.add_shadow(44, 1200)
    return c


def sponza(G, O, tmp):
    """sponza at the product's upload defaults (spatial splits: one triangle is reached from several leaves), against the oracle's own
    BVH, which the CPU tests hold equal to its brute force."""
    c = Case(G, O, "sponza", G.parse_scene(scene_variant(tmp, "sponza/sponza.xml", width=FILM[0], height=FILM[1])), oracle_bvh=True)
    c.add_camera(2001, 51)
    c.add_bounce(52)
    c.add_windows(cap=2001)
    c.add_shadow(53, 2000)
    return c


SMALL = ("cbox", "odd_room", "lattice", "lattice_twins_first", "deep")


def build(G, O, tmp, name):
    return {"cbox": lambda: cbox(G, O, tmp), "odd_room": lambda: odd_room_case(G, O), "lattice": lambda: lattice(G, O),
            "lattice_twins_first": lambda: lattice(G, O, True), "deep": lambda: deep(G, O), "sponza": lambda: sponza(G, O, tmp)}[name]()


_CACHE = {}


def get(G, O, tmp, name):
    """The case `name`, built once per process (both test modules and every test of them share it and leave it unchanged)."""
    if name not in _CACHE:
        _CACHE[name] = build(G, O, tmp, name)
    return _CACHE[name]
