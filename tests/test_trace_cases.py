"""The inputs of tests/test_gpu_trace_kat.py, checked on the CPU with the oracle alone (tests/trace_cases.py builds them): every ray
class must contain what it is there for before any GPU time is spent on it.

  (a) camera, (b) bounce and (c) axis-parallel rays: between 10 % and 90 % hits on every open scene. odd_room is a closed room and
      sponza nearly one (98 % of its camera rays hit): every ray from inside hits something whatever the list, so there the
      condition is that the hits spread over the scene (at least 8 primitives, a quarter of odd_room's, none with more than half of the hits);
  (d) tiny direction components: at least 50 rays whose fp32 1/d or o/d overflows and that the brute force hits, and rays that do not
      overflow;
  (e) windows: the answer differs between the two members of a pair in at least 90 % of the pairs;
  (f) ties: at least 100 rays whose hit is a twin quad, the lower id reported, in both listing orders;
  (g) shadow rays: 25 % to 75 % occluded;
  (h) sphere edges: at least 20 % hit the sphere and at least 20 % miss it;
  the oracle's brute force equals its own BVH, bit for bit, on every list of the small scenes; odd_room has leaves of 1, 2, 3 and 4
  records; the deep scene's and sponza's BVH4 stack bounds exceed the LDS levels of the wavefront trace kernel; sponza's window lists
  get the same answers from the brute force and from the oracle's BVH."""
import numpy as np
import pytest

import trace_cases as T

OPEN = ("cbox", "lattice", "lattice_twins_first", "deep")


@pytest.fixture(params=T.SMALL + ("sponza",))
def case(request, G, O, scene_tmp):
    return T.get(G, O, scene_tmp, request.param)


def test_hit_rates(case):
    for name in ("a_camera", "b_bounce", "c_axis", "c_along"):
        if name not in case.lists:
            continue
        gid = case.want(name)[0]
        rate = float(np.mean(gid >= 0))
        print(case.name, name, "rays", len(gid), "hit rate", rate)
        if case.name in OPEN:
            assert 0.10 <= rate <= 0.90, (case.name, name, rate)
        else:
            ids, counts = np.unique(gid[gid >= 0], return_counts=True)
            assert rate > 0.9 and len(ids) >= 8 and counts.max() <= 0.5 * len(gid), (case.name, name, rate, len(ids), counts.max())
    assert "a_camera" in case.lists and "b_bounce" in case.lists and all(len(r) % 64 for r in case.lists.values())
    assert all(1000 <= len(r) <= 4000 or k == "b_bounce" and len(r) > 900 for k, r in case.lists.items()), {k: len(r) for k, r in case.lists.items()}


@pytest.mark.parametrize("scene", ["cbox", "odd_room", "lattice"])
def test_tiny_components_overflow_and_do_not(G, O, scene_tmp, scene):
    case = T.get(G, O, scene_tmp, scene)
    r = case.lists["d_tiny"]
    ov, hit = T.overflows(r), case.want("d_tiny")[0] >= 0
    print(case.name, "overflowing", int(ov.sum()), "of them hit", int(np.sum(ov & hit)), "not overflowing", int(np.sum(~ov)), "of them hit", int(np.sum(~ov & hit)))
    assert np.sum(ov & hit) >= 50 and np.sum(~ov & hit) >= 50
    for other in case.lists:
        if other != "d_tiny":
            assert not T.overflows(case.lists[other]).any(), other          # the defect of that class cannot hide a failure elsewhere


def test_windows_change_the_answer(case):
    for a, b in (("e_near0", "e_near1"), ("e_far0", "e_far1")):
        (ga, ha), (gb, hb) = case.want(a), case.want(b)
        differ = (ga != gb) | ((ga >= 0) & (ha[:, 0].view(np.uint32) != hb[:, 0].view(np.uint32)))
        print(case.name, a, b, "pairs", len(ga), "differ", float(differ.mean()))
        assert differ.mean() >= 0.90, (case.name, a, b, differ.mean())
    # tnear = t keeps the hit, tfar = nextafter(t) keeps it: the same primitive at the same distance
    # (triangles; the sphere's fp64 root may lie below its own fp32 rounding, and tnear = t then takes the far root)
    (g0, h0), (g1, h1) = case.want("e_near0"), case.want("e_far1")
    tri = g1 < case.prepared["count"]["tris"]
    assert np.all(g1 >= 0) and tri.mean() > 0.9 and np.array_equal(g0[tri], g1[tri]) and np.array_equal(h0[tri, 0].view(np.uint32), h1[tri, 0].view(np.uint32))


def test_ties_report_the_lower_id(G, O, scene_tmp):
    seen = []
    for name in ("lattice", "lattice_twins_first"):
        c = T.get(G, O, scene_tmp, name)
        gid = c.want("f_ties")[0]
        lower, higher = {min(p) for p in c.pairs}, {max(p) for p in c.pairs}
        n_low, n_high = int(np.isin(gid, list(lower)).sum()), int(np.isin(gid, list(higher)).sum())
        print(name, "rays whose hit is a twin quad:", n_low, "reported with the higher id:", n_high)
        assert n_low >= 100 and n_high == 0
        seen.append(gid)
    # the listing order changes which id is the lower one: the two scenes give different ids for the same rays
    assert np.count_nonzero(seen[0] != seen[1]) >= 100


def test_shadow_rays_are_half_occluded(case):
    r = case.lists["g_shadow"]
    occ = float(np.mean(case.want("g_shadow")[0] >= 0))
    print(case.name, "shadow rays", len(r), "occluded", occ)
    assert 0.25 <= occ <= 0.75 and np.all(r["any_hit"] == 1) and np.all(np.isfinite(r["tfar"])) and np.all(r["tnear"] == case.eps)


def test_sphere_list_hits_and_misses(G, O, scene_tmp):
    c = T.get(G, O, scene_tmp, "odd_room")
    sphere_gid = c.prepared["count"]["tris"]
    gid, h = c.want("h_sphere")
    on = float(np.mean(gid == sphere_gid))
    print("sphere list: rays", len(gid), "hit the sphere", on)
    assert c.prepared["count"]["spheres"] == 1 and 0.20 <= on <= 0.80
    # a sphere hit and a triangle hit at nearly the same distance: rays that miss the sphere by a hair hit the floor close behind it
    centre, radius = c.sphere
    r = c.lists["h_sphere"]
    miss = gid != sphere_gid
    p = r["org"][miss] + r["dir"][miss] * h[miss, 0].astype(float)[:, None]
    assert np.count_nonzero(np.linalg.norm(p - centre, axis=1) < radius + 0.35) >= 20


@pytest.mark.parametrize("scene", T.SMALL)
def test_brute_force_equals_the_oracles_bvh(G, O, scene_tmp, scene):
    case = T.get(G, O, scene_tmp, scene)
    other = O.OracleScene(case.sd.ptr, use_bvh=True)
    for name, r in case.lists.items():
        gid, h = case.want(name)
        g2, h2 = other.closest_hits(T.as_oracle(r))
        if np.all(r["any_hit"] == 1):
            assert np.array_equal(gid >= 0, g2 >= 0), (case.name, name)
        else:
            assert np.array_equal(gid, g2) and np.array_equal(h.view(np.uint32), h2.view(np.uint32)), (case.name, name)


def test_sponzas_windows_by_brute_force_equal_its_bvh(G, O, scene_tmp):
    """sponza's lists are answered by the oracle's BVH, its four window lists by the brute force (Case.want); here the two are held
    equal on the windows, bit for bit, so that the BVH's answers to the other lists rest on a tree that keeps hits an ulp from a bound."""
    case = T.get(G, O, scene_tmp, "sponza")
    assert case.oracle_bvh and case.brute is not case.oracle
    for name in ("e_near0", "e_near1", "e_far0", "e_far1"):
        gid, h = case.want(name)
        g2, h2 = case.oracle.closest_hits(T.as_oracle(case.lists[name]))
        assert np.array_equal(gid, g2) and np.array_equal(h.view(np.uint32), h2.view(np.uint32)), name


def test_leaf_sizes_and_stack_bounds(G, O, scene_tmp):
    odd = T.get(G, O, scene_tmp, "odd_room")
    print("odd_room leaf histogram", odd.prepared["leaf_hist"])
    assert all(h > 0 for h in odd.prepared["leaf_hist"])
    for name in ("deep", "sponza"):
        c = T.get(G, O, scene_tmp, name)
        print(name, "wide_stack_need", c.prepared["wide_stack_need"], "bvh_depth", c.prepared["bvh_depth"])
        assert c.prepared["wide_stack_need"] > T.WF_LDS_LEVELS
    # the chain: too deep for the BVH4's LDS column, not for the BVH2's (kLdsSceneLevels = 12)
    deep = T.get(G, O, scene_tmp, "deep").prepared
    assert deep["bvh_depth"] <= 12 < deep["wide_stack_need"] and deep["leaf_hist"][1:] == [0, 0, 0]
    lat = T.get(G, O, scene_tmp, "lattice")
    assert 300 <= lat.prepared["count"]["tris"] <= 1500 and len(lat.pairs) >= 40
