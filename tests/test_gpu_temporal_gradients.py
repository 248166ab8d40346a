"""The gradient push on the GPU (include/gdpt.h: gdpt_temporal_push_gradients*).

The kernel against the numpy restatement (temporal_gradients_ref.py, fed the LIBRARY's matrices M) on the films, moves and planted
pixels of test_gpu_temporal.py, with random gradients beside the random colours and two more planted pixels (a NaN gradient, a
negative gradient variance), three consecutive pushes each. Every case keeps temporal_ref.MARGIN between each decision and its
threshold, the gradient decisions (cosine, side, w_k, j_max) included, so the comparison is one of rounding alone. BOUND is 100 x
the worst relative figure measured over all cases; the counts and the N', N_g' of the reset, gradient-reset,
background and left-out classes are exact.

Then: the primal and the base statistics against a second handle that is only ever pushed plainly, bit for bit; a plain push between
gradient pushes restarts every gradient; the same bits twice, on a second stream, from the host and the device entry and enqueue-only;
a film past the block cap; Temporal.frame(gradients=True) against its pieces; and the CLI: with --temporal-gradients the frame files
against Temporal.frame's reconstruction, without it against hashes recorded from the build before the flag existed."""
import ctypes as C
import functools
import hashlib
import json
import math
import os
import subprocess

import numpy as np
import pytest

import hip_rt
import temporal_gradients_ref as TG
import temporal_ref as T
from helpers import ROOT, scene_variant

pytestmark = pytest.mark.gpu

FILMS = [(1, 1), (16, 16), (17, 17), (33, 9), (40, 19)]
WORST = 5.688e-14             # measured worst figure over FILMS x MOVES x {clean, planted} x 3 pushes (40 x 19, rotation, planted): DESIGN.md 4.19
BOUND = 100 * WORST
EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")
GRADS = ("gx_out", "gx_var_out", "gy_out", "gy_var_out")


@functools.lru_cache(maxsize=None)
def frames_of(W, H, move, planted):
    """a case of temporal_gradients_ref: computed once, shared, read only"""
    return TG.case(W, H, move, planted)


def figure(got, want):
    """the worst relative difference of the six films and the two history lengths over the pixels that are not left out (those keep
    their bits: asserted), each against the largest magnitude of its array; the exact parts asserted on the way"""
    st = got["stats"]
    bad = want["masks"]["left_out"]
    for k in ("out", "var_out") + GRADS:
        assert np.array_equal(got[k][bad], want[k][bad], equal_nan=True), k
    assert (st.base.pixels_left_out, st.base.pixels_background, st.base.pixels_reset, st.pixels_gradient_reset) == \
        (want["left_out"], want["background"], want["reset"], want["gradient_reset"])
    for k in ("length", "glength"):
        for value in (0.0, 1.0):                # N', N_g' of left-out, reset and background pixels: exact, and nobody else has them
            assert np.array_equal(got[k] == value, want[k] == value), (k, value)
    inputs = want["masks"]["reset"] | want["masks"]["background"]
    for k in ("out", "var_out") + GRADS:
        assert np.array_equal(got[k][inputs], want[k][inputs]), k
    restart = want["masks"]["gradient_reset"]
    for k in GRADS:
        assert np.array_equal(got[k][restart], want[k][restart]), k
    fig = max(abs(st.base.sum_history - want["sum_history"]) / max(want["sum_history"], 1.0),
              abs(st.sum_gradient_history - want["sum_gradient_history"]) / max(want["sum_gradient_history"], 1.0))
    for k in ("out", "var_out", "length", "glength") + GRADS:
        if (~bad).any():
            fig = max(fig, float(np.abs(got[k][~bad] - want[k][~bad]).max() / np.abs(want[k][~bad]).max()))
    return fig


def run_both(G, W, H, frames, identical=False, **params):
    """the frames through the library's host entry and through the restatement with the library's M: [(got, want)]"""
    t, ref, pairs = G.Temporal(W, H), TG.TemporalGradients(W, H), []
    for frame in frames:
        cam = frame[0]
        gc = T.gdpt_camera(G, cam)
        want = ref.push(cam, G.temporal_world_to_sample(gc), *frame[1:], **params)
        assert T.margin(want["margins"], identical=identical) >= T.MARGIN, want["margins"]
        pairs.append((t.push_gradients(gc, *frame[1:], **params), want))
    t.close()
    return pairs


@pytest.mark.parametrize("planted", [False, True], ids=["clean", "planted"])
@pytest.mark.parametrize("move", T.MOVES)
@pytest.mark.parametrize("W,H", FILMS)
def test_kernel_equals_the_restatement(G, W, H, move, planted):
    worst = 0.0
    for got, want in run_both(G, W, H, frames_of(W, H, move, planted), identical=move == "identical"):
        worst = max(worst, figure(got, want))
        assert got["stats"].base.push_ms > 0
    print(f"temporal gradients {W}x{H} {move} {'planted' if planted else 'clean'}: worst figure {worst:.3e} (bound {BOUND:.1e})")
    assert worst < BOUND


def test_the_cases_exercise_every_branch(G):
    """on 40 x 19 and 17 x 17 gradients blend with a fractional N_g', the planted pixels are left out of primal and gradients alike,
    and some move meets a gradient reset that is not a primal reset"""
    fractional = blended = 0
    for W, H in ((40, 19), (17, 17)):
        for move in T.MOVES:
            pairs = run_both(G, W, H, frames_of(W, H, move, True), identical=move == "identical")
            assert pairs[1][1]["left_out"] == 5
            for got, want in pairs:
                fractional += int(((got["glength"] > 1) & (got["glength"] != np.round(got["glength"]))).sum())
                blended += int(want["masks"]["gradient_blend"].sum())
    assert fractional > 0 and blended > 1000


def test_j_max_one_restarts_gradients_and_not_the_primal(G):
    """the dolly played backwards stretches every gradient (J = I / 0.92 on the far plane): at j_max = 1 every blending pixel of the
    second push restarts its gradients while its primal blends"""
    W, H = 40, 19
    frames = frames_of(W, H, "dolly", False)[1::-1]
    (_, _), (got, want) = run_both(G, W, H, frames, j_max=1.0)
    blending = ~want["masks"]["left_out"] & ~want["masks"]["background"] & ~want["masks"]["reset"]
    assert figure(got, want) < BOUND
    assert got["stats"].pixels_gradient_reset == blending.sum() > W * H // 2
    assert (got["glength"][blending] == 1).all() and got["length"][blending].min() > 1
    for k, i in zip(GRADS, (4, 5, 6, 7)):
        assert np.array_equal(got[k], frames[1][i])


def test_primal_and_base_stats_are_the_plain_push_bit_for_bit(G):
    W, H = 40, 19
    for move in ("rotation", "quarter_pan", "behind"):
        a, b = G.Temporal(W, H), G.Temporal(W, H)
        for frame in frames_of(W, H, move, False):
            gc = T.gdpt_camera(G, frame[0])
            got = a.push_gradients(gc, *frame[1:])
            out, var_out, length, st = b.push(gc, *frame[1:4])
            assert np.array_equal(got["out"], out) and np.array_equal(got["var_out"], var_out) and np.array_equal(got["length"], length)
            base = got["stats"].base
            assert (base.pixels_left_out, base.pixels_background, base.pixels_reset, base.sum_history) == \
                (st.pixels_left_out, st.pixels_background, st.pixels_reset, st.sum_history)
        a.close(), b.close()


def test_a_plain_push_restarts_every_gradient(G):
    W, H = 33, 9
    frames = frames_of(W, H, "rotation", False)
    t, ref = G.Temporal(W, H), TG.TemporalGradients(W, H)
    cams = [T.gdpt_camera(G, f[0]) for f in frames]
    Ms = [G.temporal_world_to_sample(c) for c in cams]
    t.push_gradients(cams[0], *frames[0][1:]), ref.push(frames[0][0], Ms[0], *frames[0][1:])
    t.push(cams[1], *frames[1][1:4]), ref.push_plain(frames[1][0], Ms[1], *frames[1][1:4])
    got, want = t.push_gradients(cams[2], *frames[2][1:]), ref.push(frames[2][0], Ms[2], *frames[2][1:])
    assert figure(got, want) < BOUND
    blending = ~want["masks"]["left_out"] & ~want["masks"]["background"] & ~want["masks"]["reset"]
    assert got["stats"].pixels_gradient_reset == blending.sum() > W * H // 2
    assert (got["glength"] == 1).all() and got["length"].max() > 2 and got["stats"].sum_gradient_history == W * H
    for k, i in zip(GRADS, (4, 5, 6, 7)):
        assert np.array_equal(got[k], frames[2][i])
    got = t.push_gradients(cams[2], *frames[2][1:])                  # and the next gradient push blends again
    assert got["glength"].max() == 2
    t.reset()                                                        # reset makes both histories stale
    got = t.push_gradients(cams[2], *frames[2][1:])
    assert (got["glength"] == 1).all() and (got["length"] == 1).all() and got["stats"].pixels_gradient_reset == 0
    t.close()


def test_same_bits_twice_on_a_second_stream_and_from_both_entries(G):
    W, H = 33, 9
    frames = frames_of(W, H, "rotation", True)
    keys = ("out", "var_out", "length") + GRADS + ("glength",)
    host = [g for g, _ in run_both(G, W, H, frames)]
    again = [g for g, _ in run_both(G, W, H, frames)]
    for a, b in zip(host, again):
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)
        assert (a["stats"].sum_gradient_history, a["stats"].pixels_gradient_reset) == (b["stats"].sum_gradient_history, b["stats"].pixels_gradient_reset)
    side = hip_rt.stream(G)
    d_in = [[hip_rt.upload(G, x) for x in f[1:]] for f in frames]
    film, plane = 8 * W * H * 3, 8 * W * H
    sizes = dict(out=film, var_out=film, length=plane, glength=plane, **{k: film for k in GRADS})
    d = {k: hip_rt.alloc(G, n) for k, n in sizes.items()}
    for stream, stats in ((None, True), (side, True), (None, False), (side, False)):
        t = G.Temporal(W, H, stream=stream)
        for k, frame in enumerate(frames):
            for name, n in sizes.items():
                hip_rt.ck(hip_rt.rt(G).hipMemset(C.c_void_p(d[name]), 0, C.c_size_t(n)))
            hip_rt.ck(hip_rt.rt(G).hipDeviceSynchronize())
            u, v, feat, *grads = d_in[k]
            st = t.push_gradients_device(T.gdpt_camera(G, frame[0]), u, v, feat, grads, d["out"], d["var_out"], [d[g] for g in GRADS],
                                         len_ptr=d["length"], glen_ptr=d["glength"], stats=stats)
            assert (st is None) == (not stats)                     # enqueue-only: the read-out below synchronises
            for name in keys:
                got = hip_rt.to_host(G, d[name], (H, W, 3) if sizes[name] == film else (H, W))
                assert np.array_equal(got, host[k][name], equal_nan=True), (stream, stats, k, name)
            if stats:
                want = host[k]["stats"]
                assert (st.sum_gradient_history, st.pixels_gradient_reset, st.base.sum_history, st.base.pixels_reset, st.base.pixels_left_out) == \
                    (want.sum_gradient_history, want.pixels_gradient_reset, want.base.sum_history, want.base.pixels_reset, want.base.pixels_left_out)
        t.close()
    hip_rt.stream_destroy(G, side)
    for p in [x for row in d_in for x in row] + list(d.values()):
        hip_rt.free(G, p)


def test_a_film_past_the_block_cap(G):
    """1025 x 345: 1430 tiles of 16 x 16 on 1024 blocks, so some block takes a second trip of the tile loop and the reduction a
    second trip over the partials (asserted first). Measured 4.002e-13: q, and with it the entries of J, which are differences of
    two q, reach 1025 here, and their absolute error grows with q."""
    W, H = 1025, 345
    blocks, units = G.debug_knobs.image_grid("nlm", W, H)
    assert units > blocks > 256
    worst = 0.0
    for got, want in run_both(G, W, H, TG.case(W, H, "rotation", True)):
        worst = max(worst, figure(got, want))
    print(f"temporal gradients {W}x{H}: worst figure {worst:.3e} (bound {BOUND:.1e})")
    assert worst < BOUND


# ---- scenes ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cbox_xml(scene_tmp):
    return scene_variant(scene_tmp, "cbox/cbox_gdpt.xml", width=32, height=32, tag="temporal_gradients")


def cli_camera(G, sd, degrees):
    """the camera of frame f of `lajolla --frames N --orbit DEG` at f DEG, in the operations of the CLI: the centre of the box around
    every vertex, and T(c) R_y T(-c) cam_to_world summed term by term"""
    lo, hi = [math.inf] * 3, [-math.inf] * 3
    for s in range(sd.desc.num_shapes):
        sh = sd.desc.shapes[s]
        assert sh.positions, "a triangle mesh"
        for i in range(sh.num_vertices):
            for k in range(3):
                lo[k], hi[k] = min(lo[k], sh.positions[3 * i + k]), max(hi[k], sh.positions[3 * i + k])
    c = [0.5 * (lo[k] + hi[k]) for k in range(3)]
    a = degrees * 3.14159265358979323846 / 180.0
    cs, sn = math.cos(a), math.sin(a)
    R = [[cs, 0.0, sn, c[0] - cs * c[0] - sn * c[2]], [0.0, 1.0, 0.0, 0.0], [-sn, 0.0, cs, c[2] + sn * c[0] - cs * c[2]], [0.0, 0.0, 0.0, 1.0]]
    out = G.GdptCamera.from_buffer_copy(sd.desc.camera)
    for i in range(4):
        for j in range(4):
            v = 0.0
            for k in range(4):
                v += R[i][k] * sd.desc.camera.cam_to_world[4 * k + j]
            out.cam_to_world[4 * i + j] = v
    return out


FRAMES, SPP, PASS = 3, 8, 4


@pytest.fixture(scope="module")
def orbit(G, cbox_xml):
    """three frames of a 2 degree orbit of the 32 x 32 cbox, 8 spp in passes of 4, through Temporal.frame(gradients=True,
    reconstruct="l2"): the returned dicts, computed once and read only"""
    sd = G.parse_scene(cbox_xml)
    sc, t = G.Scene(sd), G.Temporal(32, 32)
    rs = [t.frame(sc, cli_camera(G, sd, 2.0 * f), f, FRAMES, SPP, PASS, path=False, gradients=True, reconstruct="l2") for f in range(FRAMES)]
    t.close(), sc.close()
    return rs


def test_frame_with_gradients_equals_its_pieces(G, cbox_xml, orbit):
    sd = G.parse_scene(cbox_xml)
    sc, t = G.Scene(sd), G.Temporal(32, 32)
    for f, r in enumerate(orbit):
        cam = cli_camera(G, sd, 2.0 * f)
        sc.set_camera(cam)
        ses = G.Progressive(sc, FRAMES * SPP, path=False, slice=(f * SPP, SPP))
        ses.add_pass(PASS), ses.add_pass(PASS)
        means, vars_, asm = ses.read()
        # the session's own assembly on the device: the bits of the additions frame() makes
        d_src = [hip_rt.upload(G, means[k]) for k in G.BUFFERS]
        d_dst = [hip_rt.alloc(G, 8 * 32 * 32 * 3) for _ in range(3)]
        G.assemble_device(32, 32, d_src, d_dst)
        c, cx, cy = (hip_rt.to_host(G, p, (32, 32, 3)) for p in d_dst)
        for p in d_src + d_dst:
            hip_rt.free(G, p)
        ses.close()
        feat, fvar = sc.features(SPP, window=(FRAMES * SPP, f * SPP))
        want = t.push_gradients(cam, c, asm["c"], feat, cx, asm["cx"], cy, asm["cy"])
        for name, w in (("c", c), ("cx", cx), ("cy", cy), ("mean", means["img"]), ("var", vars_["img"]), ("feat", feat), ("feat_var", fvar)):
            assert np.array_equal(r[name], w), (f, name)
        for name in ("out", "var_out", "length", "glength") + GRADS:
            assert np.array_equal(r[name], want[name]), (f, name)
        assert r["stats"].sum_gradient_history == want["stats"].sum_gradient_history
        recon, _ = G.reconstruct(32, 32, r["out"], r["gx_out"], r["gy_out"], dataCost=0.04, norm=G.RECON_L2)
        assert np.array_equal(r["reconstructed"], recon), f
        if f > 0:
            assert want["stats"].sum_gradient_history > 1.5 * 32 * 32, "most gradients keep their history through a 2 degree orbit"
            assert not np.array_equal(r["gx_out"], cx)
    t.close(), sc.close()


def test_frame_without_gradients_never_saw_one(G, cbox_xml):
    """gradients=False on a handle that also pushes gradients in between against a handle that never saw a gradient: frames 0 and 2
    of the second are plain pushes after a reset, so compare a fresh pair frame by frame from the start"""
    sd = G.parse_scene(cbox_xml)
    sc_a, sc_b = G.Scene(sd), G.Scene(sd)
    ta, tb = G.Temporal(32, 32), G.Temporal(32, 32)
    ta.frame(sc_a, cli_camera(G, sd, 0.0), 0, FRAMES, SPP, PASS, path=False, gradients=True)      # a gradient history exists ...
    ta.reset()                                                                                    # ... and is dropped
    for f in range(FRAMES):
        cam = cli_camera(G, sd, 2.0 * f)
        ra = ta.frame(sc_a, cam, f, FRAMES, SPP, PASS, path=False, atrous=dict(levels=2))
        rb = tb.frame(sc_b, cam, f, FRAMES, SPP, PASS, path=False, atrous=dict(levels=2))
        assert sorted(ra) == sorted(rb) == sorted(["out", "var_out", "length", "stats", "mean", "var", "feat", "feat_var", "denoised",
                                                   "denoised_var", "atrous_stats"])
        for k in ra:
            if k not in ("stats", "atrous_stats"):
                assert np.array_equal(ra[k], rb[k]), (f, k)
        assert ra["stats"].sum_history == rb["stats"].sum_history
    for x in (ta, tb, sc_a, sc_b):
        x.close()


# ---- the CLI --------------------------------------------------------------------------------------------------------------------

SCENE = os.path.join(ROOT, "scenes", "cbox", "cbox_gdpt.xml")
CLI_BASE = ["--film", "32x32", "--spp", str(SPP), "--pass-spp", str(PASS), "--frames", str(FRAMES), "--orbit", "2"]
# the runs whose files must stay what the build before --temporal-gradients wrote
CLI_RUNS = {"frames": [*CLI_BASE, "-o", "p.exr"],
            "temporal_atrous": [*CLI_BASE, "--temporal", "--denoised", "d.pfm", "--atrous-levels", "3", "-o", "a.pfm"]}


def cli_hashes(exe, tmp):
    """sha256 of every file each run of CLI_RUNS writes into an empty directory"""
    got = {}
    for name, args in CLI_RUNS.items():
        d = os.path.join(str(tmp), name)
        os.makedirs(d)
        subprocess.run([exe, *args, SCENE], cwd=d, check=True, capture_output=True, timeout=120)
        for f in sorted(os.listdir(d)):
            got[f"{name}/{f}"] = hashlib.sha256(open(os.path.join(d, f), "rb").read()).hexdigest()
    return got


def test_files_written_without_the_flag_are_what_they_were(tmp_path):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "temporal_gradients_cli_hashes.json")))
    assert cli_hashes(EXE, tmp_path) == want["files"]


def test_cli_frame_files_hold_the_reconstruction(G, tmp_path, orbit):
    from test_image_io import half_like_tinyexr
    r = subprocess.run([EXE, *CLI_BASE, "--temporal", "--temporal-gradients", "-o", "g.exr", SCENE], cwd=tmp_path, check=True, capture_output=True,
                       text=True, timeout=120)
    assert sorted(os.listdir(tmp_path)) == [f"g_{f:04d}.exr" for f in range(FRAMES)]
    assert "mean gradient history" in r.stdout and "gradients reset" in r.stdout
    for f in range(FRAMES):
        got = G.imread(str(tmp_path / f"g_{f:04d}.exr"), 3)
        want = half_like_tinyexr(orbit[f]["reconstructed"].astype(np.float32)).astype(np.float64)
        assert np.array_equal(got, want), f
