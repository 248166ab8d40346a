"""The BVH walks of the render kernels, ray by ray against brute force (include/gdpt_debug.h: gdpt_debug_kat_trace).

Every row of the instrument's table — one per (TraceCfg, residency) a product kernel instantiates, and the wavefront pipeline's own
trace kernel with and without sphere code — walks the ray lists of tests/trace_cases.py on every scene the host admits the row for, and
must return the oracle's hit: the brute force over the same fp32 arithmetic (sponza: the oracle's BVH, except for the one-ulp windows,
which trace_cases.Case.want answers by brute force; the CPU module holds the two equal there). Triangles: gid and the bits of t, u, v. Spheres: gid and the bits of t and ng; u and v, which pass
through acos / atan2, within one fp32 ulp (a few fp64 ulps between libm and the device library move an fp32 rounding by one step at
most); the count of differing values is printed. any_hit queries: the boolean. tests/test_trace_cases.py (CPU) shows that the lists
contain what they are there for.

The closest hit is defined without the tree, so no schedule may change it: the same lists under a fixed permutation of the rays
(other rays share a wave), keep_frac 0 / 128 / 224 (how early a walk is left and resumed) and search_frac 0 / 200 (how early the
node loop is left) give the same bits. The host's refusals are checked with their messages and leave the result array untouched.

On an MI355X: 38 (scene, row) pairs of 6667 .. 14 206 rays, every ray equal; 0 of 2146 sphere u / v values differ at all; 13 tests,
2.3 s together. DESIGN.md 6 ("Walks ray by ray") has the findings and what planted defects the module catches.
"""
import ctypes as C

import numpy as np
import pytest

import trace_cases as T

SCENES = T.SMALL + ("sponza",)
_STATE = {"scenes": {}}


@pytest.fixture(scope="module")
def rows(G):
    return G.debug_knobs.kat_trace_variants()


@pytest.fixture(scope="module")
def uploaded(G, O, scene_tmp):
    """name -> (case, uploaded scene); every scene is uploaded once for the module."""
    def get(name):
        if name not in _STATE["scenes"]:
            case = T.get(G, O, scene_tmp, name)
            _STATE["scenes"][name] = (case, case.upload())
        return _STATE["scenes"][name]
    yield get
    for _, sc in _STATE["scenes"].values():
        sc.close()
    _STATE["scenes"].clear()


def trace(G, sc, variant, r):
    r = np.ascontiguousarray(r)
    assert r.dtype == T.RAY and C.sizeof(G.GdptKatTraceQuery) == T.RAY.itemsize and C.sizeof(G.GdptKatTraceResult) == T.RESULT.itemsize
    out = G.debug_knobs.kat_trace(sc, variant, (G.GdptKatTraceQuery * len(r)).from_buffer(r))
    return np.frombuffer(out, dtype=T.RESULT, count=len(r)).copy()


def admits(G, sc, variant):
    """Whether the host takes the row for the scene (a call without rays). Only the two refusals a scene can earn count as "no"; any
    other error is one."""
    try:
        G.debug_knobs.kat_trace(sc, variant, (G.GdptKatTraceQuery * 0)())
        return True
    except G.GdptError as e:
        if "does not fit there" in str(e) or "this scene has spheres" in str(e):
            return False
        raise


def all_rays(case, row):
    """Every list of the case in one array (one launch per row), with the list and index of each ray; a wavefront row takes the
    closest-hit rays to infinity."""
    names = sorted(case.lists)
    r = np.concatenate([case.lists[k] for k in names])
    gid = np.concatenate([case.want(k)[0] for k in names])
    h = np.concatenate([case.want(k)[1] for k in names])
    src = np.concatenate([np.full(len(case.lists[k]), i) for i, k in enumerate(names)])
    idx = np.concatenate([np.arange(len(case.lists[k])) for k in names])
    keep = (r["any_hit"] == 0) & np.isinf(r["tfar"]) if row["wavefront"] else np.ones(len(r), bool)
    if np.count_nonzero(keep) % 64 == 0:
        keep[np.flatnonzero(keep)[-1]] = False
    return r[keep], gid[keep], h[keep], [names[i] for i in src[keep]], idx[keep]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def compare(case, row, r, got, want_gid, want, names, idx):
    """Returns the number of sphere u / v values that differ at all; asserts everything else."""
    ntri = case.prepared["count"]["tris"]
    anyhit = r["any_hit"] == 1
    bad = np.where(anyhit, (got["gid"] >= 0) != (want_gid >= 0), got["gid"] != want_gid)
    hit = ~anyhit & (want_gid >= 0) & ~bad
    tri, sph = hit & (want_gid < ntri), hit & (want_gid >= ntri)
    tuv = np.stack([got["t"], got["u"], got["v"]], axis=1)
    bad |= tri & np.any(bits(tuv) != bits(want[:, :3]), axis=1)
    bad |= sph & ((bits(got["t"]) != bits(want[:, 0])) | np.any(bits(got["ng"]) != bits(want[:, 3:6]), axis=1))
    ulp = np.abs(bits(tuv[:, 1:]).astype(np.int64) - bits(want[:, 1:3]).astype(np.int64))      # (u in [-0.5, 0.5], v in [0, 1]: one sign each side of a step)
    same_sign = np.signbit(tuv[:, 1:]) == np.signbit(want[:, 1:3])
    bad |= sph & np.any(~same_sign | (ulp > 1), axis=1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"scene {case.name}, row {row['name']}, class {names[i]}, ray {int(idx[i])} ({int(bad.sum())} of {len(r)} rays differ): "
                             f"org {r['org'][i].tolist()} dir {r['dir'][i].tolist()} tnear {r['tnear'][i]!r} tfar {r['tfar'][i]!r} any_hit {int(r['any_hit'][i])}: "
                             f"got gid {int(got['gid'][i])} t {got['t'][i]!r} u {got['u'][i]!r} v {got['v'][i]!r} ng {got['ng'][i].tolist()}, "
                             f"want gid {int(want_gid[i])} t {want[i, 0]!r} u {want[i, 1]!r} v {want[i, 2]!r} ng {want[i, 3:6].tolist()}")
    return int(np.count_nonzero(ulp[sph] != 0)), int(2 * np.count_nonzero(sph))


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_every_admitted_row_returns_the_oracles_hits(G, rows, uploaded, scene):
    case, sc = uploaded(scene)
    ran = []
    for variant, row in enumerate(rows):
        if not admits(G, sc, variant):
            continue
        r, want_gid, want, names, idx = all_rays(case, row)
        got = trace(G, sc, variant, r)
        moved, of = compare(case, row, r, got, want_gid, want, names, idx)
        ran.append(row["name"])
        print(f"{scene} / {row['name']}: {len(r)} rays equal the oracle" + (f"; sphere u, v off by one ulp: {moved} of {of}" if of else ""))
    # what the host must admit for this scene: every row built for what the scene holds, on the residency it fits
    spheres = case.prepared["count"]["spheres"] > 0
    # (the chain: BVH2 depth 11 fits the 12-slot LDS column, its BVH4 stack bound of 23 does not)
    fits_wide, fits_bvh2 = scene in ("cbox", "odd_room"), scene in ("cbox", "odd_room", "deep")
    for row in rows:
        must = (row["spheres"] or not spheres) and (not row["lds_scene"] or (fits_wide if row["wide"] else fits_bvh2))
        assert (row["name"] in ran) == bool(must), (scene, row["name"], must)


@pytest.mark.gpu
def test_every_row_of_the_table_is_reachable(G, rows, uploaded):
    """A row that no scene admits is unreachable, and the table is wrong."""
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names) == 11 and sum(r["wavefront"] for r in rows) == 2
    assert all(r["lds_stack_levels"] == T.WF_LDS_LEVELS for r in rows if r["wavefront"])
    # the forms the kernels have: three box tests (BVH2, signed fp32 BVH4 in LDS, BVH4 walked from HBM), whole-leaf trips with tri_hit and
    # with the flat test, the cursor, one node per trip, while-while, while-while with a leaf set aside, the wavefront kernel
    have = {(r["ww"], r["wide"], r["flat"], r["spec"], r["leaf_k"] > 0, r["lds_scene"], r["wavefront"]) for r in rows}
    for need in ((0, 0, 0, 0, False, 1, 0), (0, 0, 0, 0, True, 1, 0), (1, 1, 0, 0, False, 1, 0), (1, 1, 0, 0, True, 1, 0), (1, 1, 1, 1, False, 0, 0),
                 (1, 1, 1, 0, False, 0, 0), (1, 1, 1, 0, False, 0, 1)):
        assert need in have, need
    for variant, row in enumerate(rows):
        on = [s for s in SCENES if admits(G, uploaded(s)[1], variant)]
        print(row["name"], "admitted for", on)
        assert on, row["name"]
        case, sc = uploaded(on[0])
        r = case.lists["a_camera"]
        want_gid, want = case.want("a_camera")
        compare(case, row, r, trace(G, sc, variant, r), want_gid, want, ["a_camera"] * len(r), np.arange(len(r)))


@pytest.mark.gpu
def test_the_lattice_is_walked_from_hbm(G, uploaded):
    case, sc = uploaded("lattice")
    sc.render(1, G.RNG_SAMPLE)
    route = G.debug_knobs.last_route()
    print("lattice route", route)
    assert "hbm" in route and "lds" not in route


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cbox", "odd_room", "lattice", "deep"])
def test_the_schedule_cannot_change_a_hit(G, rows, uploaded, scene):
    case, sc = uploaded(scene)
    for variant, row in enumerate(rows):
        if not admits(G, sc, variant):
            continue
        r = all_rays(case, row)[0]
        base = trace(G, sc, variant, r)
        perm = np.random.default_rng(5).permutation(len(r))
        runs = {"permuted": lambda: trace(G, sc, variant, r[perm])}
        for knobs in ({"keep_frac": 0}, {"keep_frac": 128}, {"keep_frac": 224}, {"search_frac": 0}, {"search_frac": 200}, {"keep_frac": 224, "search_frac": 200}):
            runs[str(knobs)] = (lambda k: lambda: _with(G, k, lambda: trace(G, sc, variant, r)))(knobs)
        for what, run in runs.items():
            got = run()
            want = base[perm] if what == "permuted" else base
            anyhit = (r[perm] if what == "permuted" else r)["any_hit"] == 1
            # (an occlusion query ends at the first primitive it meets: which one that is may depend on the schedule, that there is one may not)
            raw = lambda x: x.view(np.uint8).reshape(len(x), -1)
            same = np.where(anyhit, (got["gid"] >= 0) == (want["gid"] >= 0), np.all(raw(got) == raw(want), axis=1))
            assert same.all(), (scene, row["name"], what, int(np.flatnonzero(~same)[0]), got[~same][0], want[~same][0])
        print(f"{scene} / {row['name']}: {len(runs)} schedules, {len(r)} rays, same bits")


def _with(G, knobs, fn):
    with G.debug_knobs(**knobs):
        return fn()


@pytest.mark.gpu
def test_bad_calls_are_refused_on_the_host(G, rows, uploaded):
    by_name = {r["name"]: i for i, r in enumerate(rows)}
    cbox, odd, lat = uploaded("cbox")[1], uploaded("odd_room")[1], uploaded("lattice")[1]
    good = T.rays([[278.0, 273.0, -800.0]], [[0.0, 0.0, 1.0]])

    def refused(sc, variant, r, message):
        r = np.ascontiguousarray(r)
        q = (G.GdptKatTraceQuery * len(r)).from_buffer(r)
        out = (G.GdptKatTraceResult * max(1, len(r)))()
        C.memset(out, 0xA5, C.sizeof(out))
        rc = G.lib().gdpt_debug_kat_trace(sc.handle, variant, len(r), q, out)
        err = G.lib().gdpt_last_error().decode()
        assert rc != 0 and message in err, (message, rc, err)
        assert bytes(out) == b"\xa5" * C.sizeof(out), message            # nothing was written: no kernel ran

    def edit(**fields):
        r = good.copy()
        for k, v in fields.items():
            r[k] = v
        return r
    hbm, wf = by_name["hbm"], by_name["wavefront_tris"]
    refused(cbox, len(rows), good, "is not in the table")
    refused(cbox, -1, good, "is not in the table")
    for name in ("lds_wide_cursor", "lds_wide_whole", "lds_bvh2_cursor", "lds_bvh2_whole"):
        refused(lat, by_name[name], T.rays([[3.0, 3.0, 3.0]], [[0.0, 0.0, 1.0]]), "does not fit there")
    for name in ("lds_wide_cursor_tris", "lds_wide_whole_tris", "hbm_spec_tris", "wavefront_tris"):
        refused(odd, by_name[name], T.rays([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]]), "this scene has spheres")
    refused(cbox, wf, edit(tfar=1000.0), "a wavefront row takes closest-hit queries with tfar = infinity only")
    refused(cbox, wf, edit(any_hit=1), "a wavefront row takes closest-hit queries with tfar = infinity only")
    for bad in (np.nan, np.inf, -np.inf, 1e300):
        refused(cbox, hbm, edit(org=[[bad, 0.0, 0.0]]), "not a finite fp32 number")
        refused(cbox, hbm, edit(dir=[[0.0, bad, 1.0]]), "not a finite fp32 number")
    refused(cbox, hbm, edit(tnear=np.nan), "is not a number")
    refused(cbox, hbm, edit(tnear=np.inf), "is not a number")
    refused(cbox, hbm, edit(tfar=np.nan), "is not a number")
    refused(cbox, hbm, edit(dir=[[0.0, 0.0, 0.0]]), "the direction is zero")
    refused(cbox, hbm, edit(dir=[[0.0, -0.0, 1e-60]]), "the direction is zero")
    refused(cbox, hbm, edit(tnear=-1e-9), "tnear < 0")
    refused(cbox, hbm, edit(tnear=2.0, tfar=1.0), "tfar < tnear")
    # a bad ray anywhere in the array refuses the whole call
    many = np.concatenate([np.repeat(good, 300), edit(tnear=-1.0), np.repeat(good, 5)])
    refused(cbox, hbm, many, "ray 300: tnear < 0")
    # n above the cap: refused on the count alone (the arrays hold one ray; nothing is read)
    q, out = (G.GdptKatTraceQuery * 1)(), (G.GdptKatTraceResult * 1)()
    assert G.lib().gdpt_debug_kat_trace(cbox.handle, hbm, (1 << 20) + 1, q, out) != 0 and "n must be in [0, 1048576]" in G.lib().gdpt_last_error().decode()
    assert G.lib().gdpt_debug_kat_trace(None, hbm, 1, q, out) != 0 and "null scene handle" in G.lib().gdpt_last_error().decode()
    # and the good ray is taken
    assert trace(G, cbox, hbm, np.repeat(good, 3))["gid"].tolist() == [int(uploaded("cbox")[0].oracle.closest_hits(T.as_oracle(good))[0][0])] * 3
