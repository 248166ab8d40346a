"""The case lists of the environment-map KAT (tests/envmap_cases.py), on the CPU with the oracle alone: every scene's list holds the
classes it is meant to hold, every CDF value it promises, only finite answers; the conditioning file is current and within its caps."""
import math

import numpy as np
import pytest

import envmap_cases as E


@pytest.fixture(scope="module")
def worlds(G, O, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("envmap_cases")
    return {scene: E.World(G, O, tmp, scene) for scene in E.SCENE_NAMES}


def _count(cases, cls):
    return sum(c == cls for c in cases["cls"])


def test_scene_list_and_maps(G, worlds):
    """Six synthetic maps under both transforms, the all-black map, the shipped map; the 6 x 4 map has its black row, its zero-width
    texels and its bright texel, the 5 x 3 map its black columns; the rotated transform is no rotation alone."""
    assert len(E.SCENE_NAMES) == 14 and len(set(E.SCENE_NAMES)) == 14
    sizes = {s: (wd.w, wd.h) for s, wd in worlds.items()}
    for m, size in (("1x1", (1, 1)), ("2x1", (2, 1)), ("1x2", (1, 2)), ("6x4", (6, 4)), ("5x3", (5, 3)), ("64x32", (64, 32))):
        assert sizes[m + "/identity"] == sizes[m + "/rotated"] == size
    assert sizes["black4x2/rotated"] == (4, 2) and sizes["matpreview"] == (512, 256)
    for s, wd in worlds.items():
        e = wd.sd.desc.envmap
        m = np.array(list(e.to_world)).reshape(4, 4)[:3, :3]
        if s.endswith("identity"):
            assert np.array_equal(m, np.eye(3)) and np.array_equal(np.array(list(e.to_local)).reshape(4, 4), np.eye(4))
        else:
            assert np.count_nonzero(m) >= 7
            if s.endswith("rotated"):                                                            # skew axis, scale != 1
                assert np.count_nonzero(m) == 9 and abs(np.linalg.det(m) - 1.7 ** 3) < 1e-5       # (the loader reads fp32 numbers)
            assert np.abs(np.array(list(e.to_local)).reshape(4, 4)[:3, :3] @ m - np.eye(3)).max() < 1e-14
        assert wd.sd.desc.num_lights == 1 and wd.sd.desc.lights[0].shape_id == -1               # the envmap is the only light
    t = worlds["6x4/identity"].tables
    assert worlds["6x4/identity"].black == [2] and np.array_equal(t["pdf_rows"][2], np.full(6, 1 / 6)) and t["pdf_marginals"][2] > 0
    zero = [(y, x) for y in range(4) for x in range(6) if t["cdf_rows"][y, x + 1] == t["cdf_rows"][y, x]]
    assert zero == [(0, 1), (0, 2), (3, 4)] and t["pdf_rows"][1, 4] > 0.9
    t = worlds["5x3/identity"].tables
    assert (t["pdf_rows"][:, 0] == 0).all() and (t["pdf_rows"][:, 4] == 0).all() and (t["pdf_rows"][:, 1:4] > 0).all()
    t = worlds["black4x2/rotated"].tables                                                    # the uniform fallback of both tables
    assert np.array_equal(t["pdf_rows"], np.full((2, 4), 0.25)) and np.array_equal(t["cdf_marginals"], [0, 0.5, 1]) and np.array_equal(t["cdf_rows"][0], [0, 0.25, 0.5, 0.75, 1])
    info = G.debug_knobs.prepare_scene(worlds["black4x2/rotated"].sd)                        # the host half of an upload takes it
    assert info["has_envmap"] == 1 and (info["env_w"], info["env_h"]) == (4, 2) and info["light_pmf"][0] == 1.0
    assert (worlds["64x32/identity"].tables["pdf_rows"] > 0).all()


@pytest.mark.parametrize("scene", E.SCENE_NAMES)
def test_list_is_what_it_is_meant_to_be(worlds, scene):
    wd = worlds[scene]
    c, t, w, h = wd.cases, wd.tables, wd.w, wd.h
    n = len(c["id"])
    assert len(set(c["id"])) == n and 900 <= n <= 3000 and n % 64 != 0, n
    assert c["rnd"].shape == (n, 2) and c["dir"].shape == (n, 3) and np.isfinite(c["rnd"]).all() and np.isfinite(c["dir"]).all()
    assert (c["rnd"] >= 0).all() and (c["rnd"] <= E.ONE_BELOW).all() and (c["dir"] != 0).any(axis=1).all()      # rnd = 1 is not in the list
    rnd = c["rnd"][~c["is_dir"]]
    # no case needs table2d_sample's clamp of y_offset: the search alone stays inside the table
    y_offset = np.searchsorted(t["cdf_marginals"], c["rnd"][:, 1], side="right") - 1
    assert t["cdf_marginals"][0] == 0 and t["cdf_marginals"][-1] == 1 and y_offset.min() >= 0 and y_offset.max() <= h - 1
    # counts per class
    assert _count(c, "rnd_interior") in (200, 201) and _count(c, "rnd_ends") == 8 and _count(c, "rnd_cell_mid") == 2
    assert _count(c, "dir_sphere") == 400 and _count(c, "dir_pole") == 4 + 8 * len(E.POLE_OFFSETS) == 76
    assert _count(c, "dir_seam") == _count(c, "dir_half") == 2 * len(E.SEAM_X) == 28
    assert _count(c, "dir_texel_centre") == (w * h if w * h <= 64 else 0)
    assert _count(c, "dir_border") >= 6 and _count(c, "dir_fed_back") == sum(not cl.startswith("rnd_cdf_") for cl in c["cls"] if cl.startswith("rnd_")) - ("rnd_interior/extra" in c["id"])
    for comp in (0, 1):
        assert {0.0, E.ONE_BELOW} <= set(rnd[:, comp].tolist())
    # every CDF value, exactly and one ulp either side (inside [0, 1)): the marginal's in rnd.y, three rows' in rnd.x
    def around(v):
        return {x for x in (math.nextafter(v, -math.inf), v, math.nextafter(v, math.inf)) if 0 <= x <= E.ONE_BELOW}
    marg = [i for i, cl in enumerate(c["cls"]) if cl == "rnd_cdf_marginal"]
    have = set(c["rnd"][marg, 1].tolist())
    ys = range(h + 1) if h + 1 <= E.CDF_ENTRIES_MAX else E._entries(h + 1)
    assert len(ys) >= min(h + 1, 33) and ys[0] == 0 and ys[-1] == h
    for y in ys:
        assert around(t["cdf_marginals"][y]) <= have, y
    rows = E.cdf_rows_of(t, wd.black)
    assert len(rows) == min(h, 3) and (not wd.black or wd.black[0] in rows)
    for y in rows:
        mine = [i for i, ident in enumerate(c["id"]) if ident.startswith(f"rnd_cdf_row/{y}/")]
        have = set(c["rnd"][mine, 0].tolist())
        for x in (range(w + 1) if w + 1 <= E.CDF_ENTRIES_MAX else E._entries(w + 1)):
            assert around(t["cdf_rows"][y, x]) <= have, (y, x)
        got_rows = np.trunc(wd.osc.envmap_table_sample(c["rnd"][mine])[:, 1] * h)
        assert (got_rows == y).all(), (y, got_rows)                                        # rnd.y does select that row, a black one included
    zero_texels = int(((t["cdf_rows"][:, 1:] == t["cdf_rows"][:, :-1]) & (t["cdf_rows"][:, :-1] < 1)).sum())      # (rnd.x = 1 is no case)
    assert _count(c, "rnd_zero_width") == 4 * len(wd.black[:16]) + min(zero_texels, 32)
    # poles exactly, in the map's frame and in world space; the seam and the half line
    ids = set(c["id"])
    assert {"dir_pole/+y", "dir_pole/-y", "dir_pole/+y/world", "dir_pole/-y/world", "dir_seam/+0", "dir_seam/-0", "dir_half/-1e-300"} <= ids
    world_pole = c["dir"][c["id"].index("dir_pole/-y/world")]
    assert np.array_equal(world_pole, [0.0, -1.0, 0.0])
    # the oracle's answers: all finite; pdf(sample(rnd)) > 0 wherever the table has mass there
    a_dir, a_rnd = E.oracle_dir(wd.osc, c["dir"]), E.oracle_rnd(wd.osc, c["rnd"])
    assert all(np.isfinite(v).all() for v in a_dir.values()) and all(np.isfinite(v).all() for v in a_rnd.values())
    uv = a_rnd["sample_uv"]
    x = np.minimum(np.trunc(uv[:, 0] * w), w - 1).astype(int)
    y = np.minimum(np.trunc(uv[:, 1] * h), h - 1).astype(int)
    mass = t["pdf_marginals"][y] * t["pdf_rows"][y, x] > 0
    interior = (uv[:, 1] > 0) & (uv[:, 1] < 1)                     # (at a pole the solid-angle pdf is 0 by definition)
    assert mass[~c["is_dir"]].mean() > 0.5
    wrong = np.flatnonzero(mass & interior & ~(a_rnd["sample_pdf"] > 0))
    keep, sample_keep, _ = E.masks(c, E.load_dropped()[scene])
    assert not (set(wrong.tolist()) & set(np.flatnonzero(sample_keep | c["is_dir"]).tolist())), [c["id"][i] for i in wrong[:8]]


def test_dropped_file_is_current_and_within_its_caps(G, O, worlds):
    """The conditioning rules, repeated with the oracle alone, give the file as it is committed; per scene no class loses more than half
    of its cases from every comparison and every class keeps at least 8 under the exact ones (a class of fewer: all but the half);
    over all scenes at most 30 % of the direction candidates lose a continuous comparison."""
    dropped = E.load_dropped()
    assert sorted(dropped) == sorted(E.SCENE_NAMES)
    lost_any = total = 0
    for scene, wd in worlds.items():
        now = E.condition_cases(wd.osc, wd.cases)
        assert now == dropped[scene], (scene, {k: (len(now[k]), len(dropped[scene][k])) for k in now})
        c = wd.cases
        keep, sample_keep, ok = E.masks(c, dropped[scene])
        cls = np.array(c["cls"])
        for name in sorted(set(c["cls"])):
            mine = cls == name
            if name.startswith("dir_"):
                assert 2 * int((mine & ~keep).sum()) <= int(mine.sum()), (scene, name, int((mine & ~keep).sum()), int(mine.sum()))
                assert int((mine & keep).sum()) >= min(8, (int(mine.sum()) + 1) // 2), (scene, name)
        d = c["is_dir"]
        total += int(d.sum())
        lost_any += int((d & ~(ok["dir_uv"] & ok["dir_pdf"] & ok["dir_emission"])).sum())
        # the rule never drops a whole family of inputs: the sphere class keeps every comparison nearly everywhere
        sph = cls == "dir_sphere"
        assert (ok["dir_uv"] & ok["dir_pdf"] & ok["dir_emission"])[sph].mean() > 0.98, scene
    print(f"  direction candidates: {total}, losing a continuous comparison: {lost_any} ({100 * lost_any / total:.1f} %)")
    assert lost_any <= 0.3 * total
