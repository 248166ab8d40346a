"""Shared helpers for the test-suite (scene variants, error metrics)."""
import math
import os
import re
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
ORACLE_DIR = os.path.join(ROOT, "oracle")
if ORACLE_DIR not in sys.path:
    sys.path.insert(0, ORACLE_DIR)

SCENES = os.path.join(ROOT, "scenes")


def scene_variant(tmp_dir, scene_rel, width=None, height=None, integrator=None, max_depth=None, spp=None, rr_depth=None, tag="variant"):
    """Copies the scene's folder tree (XML + meshes; sibling folders it references) to tmp_dir and edits
    film size / integrator type / maxDepth / rrDepth / sampleCount. Returns the path of the edited XML, <scene>_<tag>.xml."""
    src_dir = os.path.dirname(os.path.join(SCENES, scene_rel))
    dst_root = os.path.join(str(tmp_dir), "scenes")
    if not os.path.exists(dst_root):
        shutil.copytree(SCENES, dst_root)
    dst = os.path.join(dst_root, scene_rel)
    text = open(dst).read()
    if width is not None:
        text = re.sub(r'(<integer name="width" value=")\d+(")', r"\g<1>%d\2" % width, text)
    if height is not None:
        text = re.sub(r'(<integer name="height" value=")\d+(")', r"\g<1>%d\2" % height, text)
    if integrator is not None:
        text = re.sub(r'(<integrator type=")\w+(")', r"\g<1>%s\2" % integrator, text)
    if max_depth is not None:
        text = re.sub(r'(<integer name="maxDepth" value=")-?\d+(")', r"\g<1>%d\2" % max_depth, text)
    if rr_depth is not None:
        if 'name="rrDepth"' in text:
            text = re.sub(r'(<integer name="rrDepth" value=")-?\d+(")', r"\g<1>%d\2" % rr_depth, text)
        else:       # next to the first (the live) integrator's maxDepth
            text, n = re.subn(r'(<integer name="maxDepth" value="-?\d+"\s*/>)', r'\1<integer name="rrDepth" value="%d"/>' % rr_depth, text, count=1)
            assert n == 1, "no maxDepth to put rrDepth next to"
    if spp is not None:
        text = re.sub(r'(<integer name="sampleCount" value=")\d+(")', r"\g<1>%d\2" % spp, text)
    out = dst.replace(".xml", "_%s.xml" % tag)
    with open(out, "w") as f:
        f.write(text)
    return out


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    d = np.linalg.norm((a - b).ravel())
    n = np.linalg.norm(b.ravel())
    return d / n if n > 0 else d


# ---- building GdptSceneDesc objects from Python (tests only) -------------------------------------
import ctypes as _C


class DescBuilder:
    """Owns the ctypes arrays behind a GdptSceneDesc assembled in Python."""

    def __init__(self, G):
        self.G = G
        self.keep = []
        self.materials, self.shapes, self.lights, self.images = [], [], [], []
        self.desc = G.GdptSceneDesc()
        cam = self.desc.camera
        for i in range(16):
            cam.sample_to_cam[i] = 1.0 if i % 5 == 0 else 0.0
            cam.cam_to_world[i] = 1.0 if i % 5 == 0 else 0.0
        cam.width, cam.height, cam.filter_type, cam.filter_param = 16, 16, G.FILTER_BOX, 1.0
        self.desc.integrator, self.desc.samples_per_pixel = G.INTEGRATOR_GRADPATH, 4
        self.desc.max_depth, self.desc.rr_depth = -1, 5

    @staticmethod
    def const_tex(G, v):
        t = G.GdptTexture()
        t.type, t.image_id = G.TEX_CONSTANT, -1
        vals = [v, v, v] if not hasattr(v, "__len__") else list(v)
        for i in range(3):
            t.v0[i] = vals[i]
        t.uscale = t.vscale = 1.0
        return t

    def checker_tex(self, c0, c1, us, vs, uo, vo):
        t = self.G.GdptTexture()
        t.type, t.image_id = self.G.TEX_CHECKERBOARD, -1
        for i in range(3):
            t.v0[i], t.v1[i] = c0[i], c1[i]
        t.uscale, t.vscale, t.uoffset, t.voffset = us, vs, uo, vo
        return t

    def image_tex(self, texels, w, h, channels, us, vs, uo, vo):
        arr = (_C.c_double * len(texels))(*texels)
        self.keep.append(arr)
        im = self.G.GdptImage()
        im.width, im.height, im.channels = w, h, channels
        im.texels = _C.cast(arr, _C.POINTER(_C.c_double))
        self.images.append(im)
        t = self.G.GdptTexture()
        t.type, t.image_id = self.G.TEX_IMAGE, len(self.images) - 1
        t.uscale, t.vscale, t.uoffset, t.voffset = us, vs, uo, vo
        return t

    def material(self, mtype, texs, eta=1.5):
        m = self.G.GdptMaterial()
        m.type, m.eta = mtype, eta
        for i in range(12):
            m.tex[i] = texs[i] if i < len(texs) else self.const_tex(self.G, 0.0)
        self.materials.append(m)
        return len(self.materials) - 1

    def mesh(self, positions, indices, material_id, normals=None, uvs=None, light=None):
        G = self.G
        s = G.GdptShape()
        s.type, s.material_id, s.area_light_id = G.SHAPE_TRIMESH, material_id, -1
        s.num_vertices, s.num_triangles = len(positions) // 3, len(indices) // 3
        p = (_C.c_double * len(positions))(*positions)
        ix = (_C.c_int32 * len(indices))(*indices)
        self.keep += [p, ix]
        s.positions = _C.cast(p, _C.POINTER(_C.c_double))
        s.indices = _C.cast(ix, _C.POINTER(_C.c_int32))
        if normals is not None:
            n = (_C.c_double * len(normals))(*normals)
            self.keep.append(n)
            s.normals = _C.cast(n, _C.POINTER(_C.c_double))
        if uvs is not None:
            u = (_C.c_double * len(uvs))(*uvs)
            self.keep.append(u)
            s.uvs = _C.cast(u, _C.POINTER(_C.c_double))
        if light is not None:
            l = G.GdptLight()
            l.shape_id = len(self.shapes)
            for i in range(3):
                l.intensity[i] = light[i]
            s.area_light_id = len(self.lights)
            self.lights.append(l)
        self.shapes.append(s)
        return len(self.shapes) - 1

    def sphere(self, center, radius, material_id, light=None):
        G = self.G
        s = G.GdptShape()
        s.type, s.material_id, s.area_light_id = G.SHAPE_SPHERE, material_id, -1
        for i in range(3):
            s.center[i] = center[i]
        s.radius = radius
        if light is not None:
            l = G.GdptLight()
            l.shape_id = len(self.shapes)
            for i in range(3):
                l.intensity[i] = light[i]
            s.area_light_id = len(self.lights)
            self.lights.append(l)
        self.shapes.append(s)
        return len(self.shapes) - 1

    def finish(self):
        G, d = self.G, self.desc

        def arr(lst, typ):
            a = (typ * max(1, len(lst)))(*lst)
            self.keep.append(a)
            return a
        self._m = arr(self.materials, G.GdptMaterial)
        self._s = arr(self.shapes, G.GdptShape)
        self._l = arr(self.lights, G.GdptLight)
        self._i = arr(self.images, G.GdptImage)
        d.num_materials, d.num_shapes, d.num_lights, d.num_images = len(self.materials), len(self.shapes), len(self.lights), len(self.images)
        d.materials = _C.cast(self._m, _C.POINTER(G.GdptMaterial))
        d.shapes = _C.cast(self._s, _C.POINTER(G.GdptShape))
        d.lights = _C.cast(self._l, _C.POINTER(G.GdptLight))
        d.images = _C.cast(self._i, _C.POINTER(G.GdptImage))
        return _C.pointer(d)


# ---- the 4x4x4 test room and its parts (tests/test_gpu_route_matrix.py and the modules that build on it) ----------------------------
def _camera(G, cam, w, h, pos=(0.0, 0.0, 1.6), fov=60.0):
    """Perspective camera at `pos` looking down -z (the loader's maths for fovAxis x, as test_gpu_render_parity.py)."""
    cam.width, cam.height, cam.filter_type, cam.filter_param = w, h, G.FILTER_BOX, 1.0
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = [-1, 0, 0], [0, 1, 0], [0, 0, -1], pos
    aspect = w / h
    cot = 1.0 / math.tan(math.radians(fov / 2))
    persp = np.array([[cot, 0, 0, 0], [0, cot, 0, 0], [0, 0, 1, -1], [0, 0, 1, 0]], dtype=float)
    c2s = np.diag([-0.5, -0.5 * aspect, 1, 1]) @ np.array([[1, 0, 0, -1], [0, 1, 0, -1 / aspect], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=float) @ persp
    s2c = np.linalg.inv(c2s)
    for i in range(16):
        cam.sample_to_cam[i] = s2c.ravel()[i]
        cam.cam_to_world[i] = c2w.ravel()[i]


def _quad(b, pts, material, toward, light=None, uvs=None):
    """Two triangles over pts[0..3], wound so that the geometric normal faces the point `toward`."""
    p = np.asarray(pts, dtype=float)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    idx = [0, 1, 2, 0, 2, 3] if np.dot(n, np.asarray(toward, float) - p[0]) > 0 else [0, 2, 1, 0, 3, 2]
    return b.mesh(list(p.ravel()), idx, material, uvs=uvs, light=light)


def _box(b, lo, hi, material, faces_in, lights=None):
    """Axis-aligned box of six quads (face 2 * axis + side, side 1 = the high one); faces_in: normals point inside (a
    room) or outside (a block); lights: {face: intensity} makes those faces emitters."""
    c = [(lo[k] + hi[k]) / 2 for k in range(3)]
    for axis in range(3):
        for side in (lo[axis], hi[axis]):
            u, v = [k for k in range(3) if k != axis]
            pts = []
            for a, bb in ((0, 0), (1, 0), (1, 1), (0, 1)):
                q = [0.0] * 3
                q[axis], q[u], q[v] = side, (lo[u], hi[u])[a], (lo[v], hi[v])[bb]
                pts.append(q)
            face = axis * 2 + (side == hi[axis])
            mat = material[face] if isinstance(material, list) else material
            outward = [c[k] + (2 * (side - c[k]) if k == axis else 0.0) for k in range(3)]
            _quad(b, pts, mat, c if faces_in else outward, light=(lights or {}).get(face))


def room(G, kind, w, h, max_depth, rr_depth):
    """Closed 4x4x4 room seen from inside: Lambertian walls, an emitter on the back wall in the camera's line of sight
    and glowing walls, a block and the floor made of the lobe under test; `kind` picks that lobe."""
    b = DescBuilder(G)
    ct = lambda v: DescBuilder.const_tex(G, v)
    lam = lambda c: b.material(G.MAT_LAMBERTIAN, [ct(c)])
    if kind == "metal_box":
        # every wall, the emitting one included, of one material: DisneyMetal, base colour 1, low roughness -> throughput
        # stays near 1, paths in the closed box run to maxDepth and no offset fails the replay's material test. (A
        # metallic DisneyBSDF would not do: the reference samples its glass lobe a quarter of the time, whatever the
        # weights, and the refracted path leaves the box.) The small glass sphere makes the scene two-sided.
        m = b.material(G.MAT_DISNEY_METAL, [ct(1.0), ct(0.1), ct(0.0)])
        _box(b, (-2, -2, -2), (2, 2, 2), m, True, lights={4: (1.0, 0.8, 0.6)})       # the back wall emits
        b.sphere((1.8, 1.8, -1.8), 0.1, b.material(G.MAT_DISNEY_GLASS, [ct(1.0), ct(0.2), ct(0.0)], eta=1.5))
        _camera(G, b.desc.camera, w, h)
        b.desc.max_depth, b.desc.rr_depth = max_depth, rr_depth
        return b
    white, red, green, dark = lam((0.7, 0.7, 0.7)), lam((0.7, 0.15, 0.1)), lam((0.1, 0.6, 0.2)), lam(0.0)
    lobe = {
        "disney_diffuse": lambda: b.material(G.MAT_DISNEY_DIFFUSE, [ct((0.8, 0.6, 0.3)), ct(0.6), ct(0.4)]),
        "disney_metal": lambda: b.material(G.MAT_DISNEY_METAL, [ct((0.9, 0.7, 0.5)), ct(0.3), ct(0.25)]),
        "disney_clearcoat": lambda: b.material(G.MAT_DISNEY_CLEARCOAT, [ct(0.6)]),
        "disney_sheen": lambda: b.material(G.MAT_DISNEY_SHEEN, [ct((0.8, 0.5, 0.6)), ct(0.5)]),
        "bsdf": lambda: b.material(G.MAT_DISNEY_BSDF, [ct((0.8, 0.4, 0.3))] + [ct(v) for v in (0.4, 0.3, 0.2, 0.5, 0.35, 0.2, 0.3, 0.4, 0.5, 0.3, 0.6)], eta=1.4),
        "glass": lambda: b.material(G.MAT_DISNEY_GLASS, [ct((0.9, 0.85, 0.8)), ct(0.25), ct(0.3)], eta=1.5),
        "rough": lambda: b.material(G.MAT_ROUGHPLASTIC, [ct((0.6, 0.4, 0.3)), ct(0.5), ct(0.2)], eta=1.5),
    }
    if kind in lobe:
        floor = block = lobe[kind]()
    elif kind == "general_mix":
        floor, block = lobe["disney_diffuse"](), lobe["disney_metal"]()
    elif kind == "lambert_tex":
        rng = np.random.default_rng(7)
        floor = b.material(G.MAT_LAMBERTIAN, [b.image_tex(list(0.2 + 0.6 * rng.random(16 * 8 * 3)), 16, 8, 3, 2.0, 3.0, 0.1, 0.3)])
        block = lam((0.5, 0.5, 0.6))
    else:
        floor, block = white, lam((0.5, 0.5, 0.6))
    # walls: -x, +x, -y (floor), +y, -z (back), +z (behind the camera)
    # every wall glows a little: a sample whose primary ray meets a wall sees emission at any depth, so an all-zero
    # image would mean the film saw nothing but the block
    _box(b, (-2, -2, -2), (2, 2, 2), [red, green, floor, white, white, white], True, lights={f: (0.3, 0.3, 0.3) for f in range(6)})
    _box(b, (-1.7, -2.0, -1.3), (-0.7, -0.7, -0.3), block, False)
    _quad(b, [[-0.8, -0.8, -1.95], [0.8, -0.8, -1.95], [0.8, 0.8, -1.95], [-0.8, 0.8, -1.95]], dark, (0, 0, 0), light=(6.0, 5.0, 4.0))
    if kind == "lambert_sphere":
        b.sphere((1.0, -1.4, -0.8), 0.6, lam((0.6, 0.6, 0.3)))
    _camera(G, b.desc.camera, w, h)
    b.desc.max_depth, b.desc.rr_depth = max_depth, rr_depth
    return b


class Built:
    """Duck-typed SceneDesc (ptr, width, height) over a DescBuilder or a parsed scene file."""

    def __init__(self, ptr, w, h, owner):
        self.ptr, self.width, self.height, self.owner = ptr, w, h, owner


def odd_room_builder(G, film):
    """The Lambertian room above plus a fan of three triangles on the floor and two lone triangles on a wall and the
    ceiling: 31 triangles that do not pair up, so the builder at its default leaf factor makes leaves of every size up to bvh_leaf_max
    (histograms [31], [3, 14], [1, 12, 2], [1, 10, 2, 1]). cbox, 19 quads, never yields a three-record leaf."""
    b = room(G, "lambert", *film, -1, 5)
    m = b.material(G.MAT_LAMBERTIAN, [DescBuilder.const_tex(G, 0.5)])
    b.mesh([0.9, -2.0, 0.2, 1.7, -2.0, 0.4, 1.2, -1.0, 0.3, 0.6, -1.0, 0.5, 0.4, -2.0, 0.6], [0, 1, 2, 0, 2, 3, 0, 3, 4], m)
    b.mesh([-1.9, 1.0, 0.5, -1.9, 1.6, 0.9, -1.9, 1.2, 1.4], [0, 1, 2], m)
    b.mesh([1.0, 1.9, -1.0, 1.6, 1.9, -0.6, 1.2, 1.9, -0.2], [0, 1, 2], m)
    return b
