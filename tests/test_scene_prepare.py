"""The host half of a scene upload through gdpt_debug_prepare_scene (include/gdpt_debug.h), against the oracle and the description.
CPU only: nothing here touches a device."""
import os

import numpy as np
import pytest

from helpers import SCENES

SCENE_FILES = ["cbox/cbox_gdpt.xml", "disney_bsdf_test/simple_sphere.xml", "matpreview/matpreview.xml", "veach_mi/mi.xml", "sponza/sponza.xml"]


@pytest.fixture(scope="module")
def prepared(G):
    """{scene: (description, prepare_scene's dict)} at a 32x32 film, made once."""
    out = {}
    for s in SCENE_FILES + ["disney_bsdf_test/disney_glass.xml"]:
        sd = G.parse_scene(os.path.join(SCENES, s), film=(32, 32))
        out[s] = (sd, G.debug_knobs.prepare_scene(sd))
    return out


@pytest.mark.parametrize("scene", SCENE_FILES)
def test_tables_equal_the_oracle_exactly(G, O, prepared, scene):
    """The emitter selection table and the intersection epsilon are the oracle's formulas in the oracle's order, both in fp64 and
    both compiled without contraction: tolerance zero. The primitive counts are the description's."""
    sd, p = prepared[scene]
    osc = O.OracleScene(sd.ptr)
    n = sd.desc.num_lights
    assert n > 0 and p["count"]["light_pmf"] == n and p["count"]["light_cdf"] == n + 1
    pmf, cdf = osc.light_table(n)
    print(scene, "light_pmf", p["light_pmf"], "oracle", pmf, "isect_eps", p["isect_eps"], "oracle", osc.intersection_epsilon)
    assert np.array_equal(p["light_pmf"], pmf) and np.array_equal(p["light_cdf"], cdf)
    assert p["isect_eps"] == osc.intersection_epsilon
    d = sd.desc
    assert p["count"]["tris"] == len(G.shape_triangles(sd))
    assert p["count"]["spheres"] == sum(1 for i in range(d.num_shapes) if d.shapes[i].type == G.SHAPE_SPHERE)
    assert p["count"]["prims"] >= p["count"]["tris"] + p["count"]["spheres"]
    assert p["count"]["nodes4q"] == p["count"]["nodes4"] and p["count"]["nodes8"] == 0       # a product upload has no 8-wide tree
    assert bool(p["has_envmap"]) == bool(d.has_envmap)


def test_traits(prepared):
    cbox = prepared["cbox/cbox_gdpt.xml"][1]
    assert cbox["lambert_only"] and cbox["one_sided"] and not cbox["has_rough"] and cbox["plan_take_pct"] == 0
    assert cbox["material_mask"] == 1 and cbox["all_textures_constant"]
    assert sum(cbox["leaf_hist"]) > 0 and 0 < cbox["bvh_depth"] <= 32 and 0 < cbox["wide_stack_need"] <= 32
    glass = prepared["disney_bsdf_test/disney_glass.xml"][1]
    assert not glass["one_sided"] and not glass["lambert_only"] and glass["plan_take_pct"] == 40


@pytest.mark.parametrize("scene", ["cbox/cbox_gdpt.xml", "matpreview/matpreview.xml"])
def test_two_calls_give_identical_digests(G, prepared, scene):
    sd, p = prepared[scene]
    again = G.debug_knobs.prepare_scene(sd)
    assert again["digest"] == p["digest"] and again["count"] == p["count"]
    assert len(set(p["digest"][k] for k in p["count"] if p["count"][k])) > 1


def test_a_defective_description_gives_the_upload_message(G):
    from helpers import DescBuilder

    class Borrowed:          # a description the test owns: what prepare_scene reads of a SceneDesc
        def __init__(self, p):
            self.ptr, self.desc = p, p.contents
    b = DescBuilder(G)
    m = b.material(G.MAT_LAMBERTIAN, [DescBuilder.const_tex(G, 0.5)])
    b.mesh([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 1, 3], m)
    with pytest.raises(G.GdptError, match="gdpt_scene_upload: mesh index out of range"):
        G.debug_knobs.prepare_scene(Borrowed(b.finish()))
