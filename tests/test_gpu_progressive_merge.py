"""A progressive session's samples split over sessions and devices (include/gdpt.h: gdpt_progressive_create_slice,
gdpt_progressive_merge, gdpt_progressive_group_*): slice sessions against the windows they must draw, the merge against its numpy
restatement (tests/progressive_merge_ref.py) and against the one session that folded every pass, spent slices against the one-shot
render, the accumulator, refusals, determinism, the group (one slice session per device, a merged total) and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import progressive_merge_ref as M
import progressive_ref as R
from helpers import ROOT, rel_l2, scene_variant
from test_gpu_progressive import FAMILIES, read_pfm, render_window, session_planes

pytestmark = pytest.mark.gpu
BUFS = R.BUFS
CBOX = "cbox/cbox_gdpt.xml"

# measured on an MI355X: rel L2 of the merged session's M2 planes against the restatement fed the read-back states, worst buffer
# (test_merge_against_the_restatement's docstring). The restatement is the yardstick; 100 x is the margin
# test_fold_against_the_restatement uses for the same kind of FMA-only difference.
M2_MEASURED = 1.5e-16
M2_BOUND = min(100 * M2_MEASURED, 1e-9)


def cbox(G, scene_tmp, w, h, **kw):
    return G.parse_scene(scene_variant(scene_tmp, CBOX, width=w, height=h, **kw))


def state_of(ses):
    """The session's (mean, M2, W, K) as a Fold, from its read-out: M2 = var_mean x (K - 1) W. Needs K >= 2."""
    st = ses.status()
    means, var, _ = ses.read()
    norm = float(st["passes"] - 1) * float(st["spp"])
    return M.state(means, {k: var[k] * norm for k in var}, st["spp"], st["passes"])


def check_against(ses, ref, what):
    """Means, variances, assembled variances and the error estimate of `ses` against the Fold `ref` under the bounds of the fold
    test; returns the worst M2 figure."""
    st = ses.status()
    means, var, asm = ses.read()
    want_var, want_asm = ref.var_mean(), ref.assembled_var()
    assert st["passes"] == ref.K and st["spp"] == ref.W
    worst = 0.0
    for name in BUFS:
        e_mean = rel_l2(means[name], ref.mean[name])
        e_m2 = rel_l2(var[name] * ref.norm(), ref.M2[name])
        worst = max(worst, e_m2)
        print(f"{what} {name}: mean rel L2 {e_mean:.2e}, M2 rel L2 {e_m2:.2e}")
        assert e_mean < 1e-13, (what, name, e_mean)
        assert rel_l2(var[name], want_var[name]) < M2_BOUND, (what, name)
    for name in ("c", "cx", "cy"):
        assert rel_l2(asm[name], want_asm[name]) < M2_BOUND, (what, name)
    e_ref, out_ref = ref.error_estimate()
    print(f"{what}: M2 rel L2 (worst buffer) {worst:.2e}; error estimate {st['error']:.6e} against {e_ref:.6e}")
    assert worst < M2_BOUND
    assert st["pixels_left_out"] == out_ref == 0
    assert abs(st["error"] - e_ref) <= (M2_BOUND + 1e-12) * e_ref
    return worst


def test_struct_sizes_did_not_grow(G, tmp_path):
    """The feature adds entry points and an opaque handle, no struct; the two session structs keep the size the header had."""
    src = tmp_path / "sz.c"
    structs = {"GdptProgressiveConfig": 16, "GdptProgressiveStatus": 136, "GdptSampleWindow": 8}
    body = "\n".join(f'printf("{s} %zu\\n", sizeof({s}));' for s in structs)
    src.write_text(f'#include <stdio.h>\n#include "{ROOT}/include/gdpt.h"\nint main(){{{body} return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    sizes = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for s, want in structs.items():
        assert int(sizes[s]) == C.sizeof(getattr(G, s)) == want, s
    for name in ("gdpt_progressive_create_slice", "gdpt_progressive_merge", "gdpt_progressive_group_create", "gdpt_progressive_group_free",
                 "gdpt_progressive_group_run", "gdpt_progressive_group_total", "gdpt_progressive_group_member_status"):
        assert hasattr(G.lib(), name), name


def test_slice_layout(G, scene_tmp):
    """Slice (3, 4) of a block of 7: the passes are the windows {7, 3} and {7, 5}; a slice over the whole block is the plain session."""
    sc = G.Scene(cbox(G, scene_tmp, 40, 24))
    ses = G.Progressive(sc, 7, slice=(3, 4))
    assert ses.status()["budget_spp"] == 4 and ses.status()["spp"] == 0
    ses.add_pass(2)
    first, _ = render_window(G, sc, 2, (7, 3))
    means, _, _ = ses.read()
    for k in BUFS:
        assert np.array_equal(means[k], first[k]), k
    ses.add_pass(2)
    both, _ = render_window(G, sc, 4, (7, 3))
    means, _, _ = ses.read()
    for k in BUFS:
        err = rel_l2(means[k], both[k])
        print(f"slice (3, 4) of 7, {k}: rel L2 {err:.2e}")
        assert err < 1e-12, (k, err)
    st = ses.status()
    assert (st["passes"], st["spp"], st["budget_spp"]) == (2, 4, 4)
    with pytest.raises(G.GdptError, match="budget"):
        ses.add_pass(1)                              # the slice is spent, though the block is not
    assert ses.run(pass_spp=2)["stop_reason"] == "budget"
    ses.close()
    # the whole block as a slice is the plain session, bit for bit
    a, b = G.Progressive(sc, 16, slice=(0, 16)), G.Progressive(sc, 16)
    for n in (1, 3, 4, 8):
        a.add_pass(n), b.add_pass(n)
    for x, y in zip(session_planes(a), session_planes(b)):
        assert np.array_equal(x, y)
    sa, sb = a.status(), b.status()
    assert (sa["passes"], sa["spp"], sa["budget_spp"], sa["error"]) == (sb["passes"], sb["spp"], sb["budget_spp"], sb["error"]) == (4, 16, 16, sa["error"])
    a.close(), b.close()
    for sl in ((-1, 2), (0, -1), (5, 3), (8, 1), (0, 8)):       # negative start / size; [5, 8), [8, 9), [0, 8) leave [0, 7)
        with pytest.raises(G.GdptError, match="slice"):
            G.Progressive(sc, 7, slice=sl)
    empty = G.Progressive(sc, 7, slice=(7, 0))        # allowed: an accumulator
    assert empty.status()["budget_spp"] == 0
    with pytest.raises(G.GdptError, match="budget"):
        empty.add_pass(1)
    empty.close()


@pytest.fixture(scope="module")
def halves(G, scene_tmp):
    """cbox 48x32, block 16: A = slice [0, 7) in passes 1, 2, 4 and B = slice [7, 16) in passes 4, 5 on a second scene handle, with
    their states as read back, and S, the one session that folded all five passes. Shared, never changed by a test."""
    sd = cbox(G, scene_tmp, 48, 32)
    sc1, sc2 = G.Scene(sd), G.Scene(sd)

    def make():
        a, b = G.Progressive(sc1, 16, slice=(0, 7)), G.Progressive(sc2, 16, slice=(7, 9))
        sa = [a.add_pass(n) for n in (1, 2, 4)]
        sb = [b.add_pass(n) for n in (4, 5)]
        return a, b, sa + sb
    whole = G.Progressive(sc1, 16)
    for n in (1, 2, 4, 4, 5):
        whole.add_pass(n)
    return dict(sc=(sc1, sc2), make=make, whole=whole)


def test_merge_against_the_restatement(G, halves):
    """A and B are read back, B is merged into A, and tests/progressive_merge_ref.py merges the read-back states: means to 1e-13
    relative L2. For M2, the variances and the error estimate the rule of test_fold_against_the_restatement: measured on an MI355X
    (cbox 48x32, A = passes 1, 2, 4 of [0, 7), B = passes 4, 5 of [7, 16)): 0.75e-16 (img) to 1.47e-16 (cx0) relative L2 over the
    buffers, means 1.5e-17 to 5.5e-17; the worst, rounded up, is M2_MEASURED above, and the assertion is 100 x that value, never
    looser than 1e-9. (Merge, then a pass of dst's own, test_accumulator_and_passes_after_a_merge: 1.04e-16 in the worst buffer;
    the variances against the single session below: 1.0e-16 to 2.5e-16.) (The read-out divides M2 by (K-1) W and the test multiplies it back: up to an ulp per
    element on both sides of the comparison, part of the measured figure.) Against the single session that folded all five passes:
    means to 1e-12, variances under the same bound."""
    a, b, pass_stats = halves["make"]()
    fa, fb = state_of(a), state_of(b)
    b_before = session_planes(b)
    st = a.merge(b)
    ref = M.merge(fa, fb)
    check_against(a, ref, "merge")
    assert (st["passes"], st["spp"], st["budget_spp"]) == (5, 16, 16)
    for key in ("samples", "rays", "bounces"):
        assert getattr(st["totals"], key) == sum(getattr(s, key) for s in pass_stats), key
    assert st["totals"].samples == 48 * 32 * 16 and st["fold_ms"] > 0
    for x, y in zip(session_planes(b), b_before):
        assert np.array_equal(x, y)                  # src is unchanged
    assert b.status()["passes"] == 2 and b.status()["spp"] == 9
    # against the one session of all five passes
    whole = halves["whole"]
    wm, wv, wa = whole.read()
    means, var, asm = a.read()
    for k in BUFS:
        e_mean, e_var = rel_l2(means[k], wm[k]), rel_l2(var[k], wv[k])
        print(f"merged against the single session, {k}: mean rel L2 {e_mean:.2e}, variance rel L2 {e_var:.2e}")
        assert e_mean < 1e-12 and e_var < M2_BOUND, (k, e_mean, e_var)
    for k in ("c", "cx", "cy"):
        assert rel_l2(asm[k], wa[k]) < M2_BOUND, k
    ws = whole.status()
    assert abs(st["error"] - ws["error"]) <= (M2_BOUND + 1e-12) * ws["error"]
    for key in ("samples", "rays", "bounces"):
        assert getattr(st["totals"], key) == getattr(ws["totals"], key), key
    a.close(), b.close()


@pytest.mark.parametrize("family", ["lds_lambert", "reconnect", "path"])
def test_spent_slices_are_the_one_shot_render(G, scene_tmp, family):
    """Slices [0, 8) and [8, 16), both spent, merged: the means are Scene.render(16) / path_render(16) to 1e-12 relative L2 per buffer
    (the bound of test_session_that_spends_its_budget_has_drawn_the_one_shot_samples), the counters add up exactly."""
    rel, film, integ, shift_name, knobs, path, route = FAMILIES[family]
    shift = getattr(G, shift_name)
    sd = G.parse_scene(scene_variant(scene_tmp, rel, width=40, height=24, integrator=integ))
    sc1, sc2 = G.Scene(sd), G.Scene(sd)
    with G.debug_knobs(**knobs):
        if path:
            img, ost = sc1.path_render(16, G.RNG_SAMPLE)
            one = {"img": img}
        else:
            one, ost = sc1.render(16, G.RNG_SAMPLE, shift=shift)
        assert G.debug_knobs.last_route().startswith(route), G.debug_knobs.last_route()
        assert ost.nonfinite_samples == 0
        a, b = G.Progressive(sc1, 16, shift=shift, path=path, slice=(0, 8)), G.Progressive(sc2, 16, shift=shift, path=path, slice=(8, 8))
        stats = [a.add_pass(n) for n in (1, 3, 4)] + [b.add_pass(n) for n in (6, 2)]
    st = a.merge(b)
    assert (st["passes"], st["spp"], st["budget_spp"]) == (5, 16, 16)
    for key in ("samples", "rays", "bounces"):
        assert sum(getattr(s, key) for s in stats) == getattr(ost, key) == getattr(st["totals"], key), key
    means, _, _ = a.read()
    assert sorted(means) == sorted(one)
    for k in one:
        err = rel_l2(means[k], one[k])
        print(f"{family} {k}: rel L2 {err:.2e}")
        assert err < 1e-12, (family, k, err)
    a.close(), b.close()


def test_accumulator_and_passes_after_a_merge(G, halves, scene_tmp):
    sc1, sc2 = halves["sc"]
    a, b, _ = halves["make"]()
    acc = G.Progressive(sc1, 16, slice=(0, 0))
    st = acc.merge(a)
    for x, y in zip(session_planes(acc), session_planes(a)):
        assert np.array_equal(x, y)                  # into an empty accumulator: src, bit for bit
    sa = a.status()
    assert (st["passes"], st["spp"], st["budget_spp"], st["error"]) == (3, 7, 7, sa["error"])
    st = acc.merge(b)
    a.merge(b)
    for x, y in zip(session_planes(acc), session_planes(a)):
        assert np.array_equal(x, y)
    assert (st["passes"], st["spp"], st["budget_spp"], st["error"]) == (5, 16, 16, a.status()["error"])
    with pytest.raises(G.GdptError, match="budget"):
        acc.add_pass(1)                              # an accumulator draws nothing
    for s in (a, b, acc):
        s.close()
    # dst goes on with passes of its own after a merge: A = [0, 9) with 7 drawn, B = [9, 16) spent
    a, b = G.Progressive(sc1, 16, slice=(0, 9)), G.Progressive(sc2, 16, slice=(9, 7))
    for n in (1, 2, 4):
        a.add_pass(n)
    for n in (4, 3):
        b.add_pass(n)
    fa, fb = state_of(a), state_of(b)
    a.merge(b)
    a.add_pass(2)
    own, _ = render_window(G, sc1, 2, (16, 7))
    ref = M.merge(fa, fb).add(own, 2)
    check_against(a, ref, "merge, then a pass")
    st = a.status()
    assert (st["passes"], st["spp"], st["budget_spp"]) == (6, 16, 16)
    with pytest.raises(G.GdptError, match="budget"):
        a.add_pass(1)
    a.close(), b.close()


def test_merge_refusals(G, halves, scene_tmp):
    sc1, sc2 = halves["sc"]
    a, b, _ = halves["make"]()

    def refused(dst, src, match):
        before = dst.status()
        with pytest.raises(G.GdptError, match=match):
            dst.merge(src)
        after = dst.status()
        assert (after["passes"], after["spp"], after["budget_spp"]) == (before["passes"], before["spp"], before["budget_spp"])

    refused(a, a, "same session")
    a.merge(b)
    refused(a, b, "overlap")                          # the same src twice
    c = G.Progressive(sc2, 16, slice=(4, 8))
    c.add_pass(4)
    refused(c, b, "overlap")                          # B holds [7, 16), C holds [4, 8) of its slice [4, 12)
    refused(b, c, "overlap")
    d = G.Progressive(sc2, 16, slice=(0, 4))          # D = [0, 4) drawn: free of B = [7, 16), not of A (A's own [0, 7))
    d.add_pass(4)
    refused(a, d, "overlap")
    other_block = G.Progressive(sc2, 32, slice=(16, 4))
    other_block.add_pass(4)
    refused(b, other_block, "stream blocks")
    shifted = G.Progressive(sc2, 16, shift=G.SHIFT_RECONNECT, slice=(0, 4))
    shifted.add_pass(4)
    refused(b, shifted, "shift")
    deeper = G.Progressive(sc2, 16, slice=(0, 4), max_depth_override=3)
    deeper.add_pass(4)
    refused(b, deeper, "max_depth_override")
    small = G.Scene(cbox(G, scene_tmp, 40, 24))
    other_film = G.Progressive(small, 16, slice=(0, 4))
    other_film.add_pass(4)
    refused(b, other_film, "film")
    psc = G.Scene(cbox(G, scene_tmp, 48, 32, integrator="path"))
    path_ses = G.Progressive(psc, 16, path=True, slice=(0, 4))
    path_ses.add_pass(4)
    refused(b, path_ses, "mode")                      # a Path session into a GradPath session
    refused(path_ses, d, "mode")
    assert G.lib().gdpt_progressive_merge(None, b.handle) != 0 and G.lib().gdpt_progressive_merge(b.handle, None) != 0
    # a src without passes is a no-op, and D, which none of this touched, still merges into B
    idle = G.Progressive(sc2, 16, slice=(0, 4))
    st = b.merge(idle)
    assert (st["passes"], st["spp"], st["budget_spp"]) == (2, 9, 9)
    st = b.merge(d)
    assert (st["passes"], st["spp"], st["budget_spp"]) == (3, 13, 13)
    # the total of a group is rebuilt by its group alone
    grp = G.ProgressiveGroup(cbox(G, scene_tmp, 48, 32), (0, 0), 16)
    grp.run(pass_spp=4, max_rounds=1)
    for call in (lambda: grp.total.add_pass(1), lambda: grp.total.run(pass_spp=1), lambda: grp.total.merge(d)):
        with pytest.raises(G.GdptError, match="total of a group"):
            call()
    assert grp.total.status()["passes"] == 2
    grp.close()


def test_the_same_sequence_gives_the_same_bits(G, halves):
    runs = []
    for _ in range(2):
        a, b, _ = halves["make"]()
        a.merge(b)
        runs.append((a.status(), session_planes(a)))
        a.close(), b.close()
    (s0, p0), (s1, p1) = runs
    assert (s0["passes"], s0["spp"], s0["error"], s0["pixels_left_out"]) == (s1["passes"], s1["spp"], s1["error"], s1["pixels_left_out"])
    assert np.isfinite(s0["error"]) and s0["error"] > 0
    for x, y in zip(p0, p1):
        assert np.array_equal(x, y)


def group_body(G, scene_tmp, devices):
    """Budget 24 in passes of 4 over len(devices) members, cbox 40x24."""
    import torch
    if torch.cuda.device_count() <= max(devices):
        pytest.skip(f"needs {max(devices) + 1} GPUs")
    W, H, B, P, N = 40, 24, 24, 4, len(devices)
    sd = cbox(G, scene_tmp, W, H)
    rounds = -(-(B // N) // P)
    grp = G.ProgressiveGroup(sd, devices, B)
    st = grp.run(pass_spp=P, max_rounds=1)
    assert (st["stop_reason"], st["passes"], st["spp"], st["budget_spp"]) == ("max_passes", N, N * P, N * P)
    e1 = st["error"]
    assert np.isfinite(e1) and e1 > 0
    st = grp.run(pass_spp=P)
    assert (st["stop_reason"], st["passes"], st["spp"], st["budget_spp"]) == ("budget", N * rounds, B, B) and N * rounds == 6
    assert grp.total.status()["passes"] == N * rounds and grp.total.status()["stop_reason"] == "budget"
    for i in range(N):
        ms = grp.member_status(i)
        assert (ms["passes"], ms["spp"], ms["budget_spp"]) == (rounds, B // N, B // N)
    with pytest.raises(G.GdptError):
        grp.member_status(N)
    assert st["totals"].samples == W * H * B
    assert abs(st["totals"].render_ms - sum(grp.member_status(i)["totals"].render_ms for i in range(N))) <= 1e-9 * st["totals"].render_ms
    # the one-shot render
    sc = G.Scene(sd)
    one, ost = sc.render(B, G.RNG_SAMPLE)
    means, var, asm = grp.total.read()
    for k in BUFS:
        err = rel_l2(means[k], one[k])
        print(f"group {devices} {k}: rel L2 against render({B}) {err:.2e}")
        assert err < 1e-12, (k, err)
    for key in ("samples", "rays", "bounces"):
        assert getattr(st["totals"], key) == getattr(ost, key), key
    # three hand-made slice sessions merged in index order into an accumulator: the same bits
    scenes = [G.Scene(sd, device=d) for d in devices]
    acc = G.Progressive(scenes[0], B, slice=(0, 0))
    for i in range(N):
        first, end = i * B // N, (i + 1) * B // N
        s = G.Progressive(scenes[i], B, slice=(first, end - first))
        assert s.run(pass_spp=P)["stop_reason"] == "budget"
        acc.merge(s)
        s.close()
    for x, y in zip(session_planes(grp.total), session_planes(acc)):
        assert np.array_equal(x, y)
    assert acc.status()["error"] == st["error"]
    acc.close()
    # the total is a session: L2 reconstruction against fourierSolve of the one-shot assembled buffers, weighted reconstruction
    cx, cy = one["cx0"].copy(), one["cy0"].copy()
    cx[:, 1:] += one["cx1"][:, :-1]
    cy[1:, :] += one["cy1"][:-1, :]
    want = G.fourierSolve(W, H, one["img"], cx, cy, 0.04)
    got, _ = grp.total.reconstruct()
    err = rel_l2(got, want)
    print(f"group {devices}: reconstruction against fourierSolve of the one-shot buffers: rel L2 {err:.2e}")
    assert err < 1e-11
    wimg, wst = grp.total.reconstruct_weighted()
    assert np.isfinite(wimg).all() and wimg.shape == (H, W, 3)
    grp.close()
    # a target between the estimate after one round and nothing: the second group stops there
    grp2 = G.ProgressiveGroup(sd, devices, B)
    st2 = grp2.run(target_error=1.5 * e1, pass_spp=P)
    assert (st2["stop_reason"], st2["passes"], st2["spp"]) == ("target", N, N * P) and st2["error"] == e1
    grp2.close()


def test_group_on_one_gpu(G, scene_tmp):
    group_body(G, scene_tmp, (0, 0, 0))


def test_group_on_two_gpus(G, scene_tmp):
    group_body(G, scene_tmp, (0, 1))


def test_cli_sample_devices(G, tmp_path):
    exe = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")
    xml = os.path.join(ROOT, "scenes", "cbox", "cbox_gdpt.xml")
    out = tmp_path / "o.pfm"
    r = subprocess.run([exe, "--sample-devices", "0,0", "--spp", "16", "--pass-spp", "4", "--film", "48x32", "-o", str(out), xml],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    grp = G.ProgressiveGroup(G.parse_scene(xml, film=(48, 32)), (0, 0), 16)
    st = grp.run(pass_spp=4)
    assert np.array_equal(read_pfm(out, 48, 32), grp.total.reconstruct()[0].astype(np.float32))
    line = [l for l in r.stdout.splitlines() if l.startswith("[gdpt] progressive:")]
    assert len(line) == 1, r.stdout
    assert "4 passes, 16 of 16 samples per pixel" in line[0] and "stopped by budget" in line[0]
    printed = float(line[0].split("error estimate ")[1].split()[0])
    assert abs(printed - st["error"]) <= 1e-5 * st["error"]
    slices = [l for l in r.stdout.splitlines() if l.startswith("[gdpt] 2 sample slices:")]
    assert len(slices) == 1 and "[0,8)" in slices[0] and "[8,16)" in slices[0], r.stdout
    grp.close()
    for extra in (["--sample-devices", "0,0"],                                        # without --pass-spp
                  ["--sample-devices", "0,0", "--pass-spp", "4", "--gpus", "1"],
                  ["--sample-devices", "0,0", "--pass-spp", "4", "--devices", "0"]):
        r = subprocess.run([exe, "--spp", "16", *extra, "-o", str(out), xml], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
