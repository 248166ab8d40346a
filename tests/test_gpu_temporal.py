"""Temporal reprojection and the camera setter on the GPU (include/gdpt.h: gdpt_temporal_*, gdpt_scene_set_camera).

The kernel against the numpy restatement (temporal_ref.py, fed the LIBRARY's matrices M) on the smallest films with a partial tile in
each direction and taps that land in another tile, under six camera moves, clean and with planted invalid pixels, three consecutive
pushes each so that the history length becomes fractional. Every case keeps temporal_ref.MARGIN between each of its decisions and the
decision's threshold (asserted here too), so the comparison is one of rounding alone: the kernel contracts a b + c into one fused
operation and numpy does not. BOUND is 100 x the worst relative figure measured over all cases, the project's habit
for the filters; the counts and the N' of reset, background and left-out pixels are exact.

Then the same bits twice, on a second stream, from the host and the device entry and enqueue-only followed by a synchronise; a film
past the block cap; Temporal.frame against its pieces called by hand; gdpt_scene_set_camera against fresh uploads; and the files the
CLI writes without --frames against hashes recorded from the build before --frames existed."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import hip_rt
import temporal_ref as T
from helpers import ROOT, scene_variant

pytestmark = pytest.mark.gpu

FILMS = [(1, 1), (16, 16), (17, 17), (33, 9), (40, 19)]
BOUND = 100 * 9.050e-15      # measured worst figure over FILMS x MOVES x {clean, planted} x 3 pushes (40 x 19, rotation, planted): DESIGN.md 4.18
EXE = os.path.join(ROOT, "gradient-based-path-tracing_amd", "lajolla")
CBOX_CENTRE = (278.0, 274.4, 279.6)


@functools.lru_cache(maxsize=None)
def frames_of(W, H, move, planted):
    """a case of temporal_ref: computed once, shared, read only"""
    return T.case(W, H, move, planted)


def figure(got, want):
    """the worst relative difference of out, var_out and the history length over the pixels that are not left out (those keep their
    bits: asserted), each against the largest magnitude of its array; the exact parts asserted on the way"""
    out, var_out, length, st = got
    bad = want["masks"]["left_out"]
    assert np.array_equal(out[bad], want["out"][bad], equal_nan=True) and np.array_equal(var_out[bad], want["var_out"][bad], equal_nan=True)
    assert (st.pixels_left_out, st.pixels_background, st.pixels_reset) == (want["left_out"], want["background"], want["reset"])
    for value in (0.0, 1.0):                    # N' of left-out, reset and background pixels: exact, and nobody else has them
        assert np.array_equal(length == value, want["length"] == value)
    inputs = want["masks"]["reset"] | want["masks"]["background"]
    assert np.array_equal(out[inputs], want["out"][inputs]) and np.array_equal(var_out[inputs], want["var_out"][inputs])
    fig = abs(st.sum_history - want["sum_history"]) / max(want["sum_history"], 1.0)
    for a, b in ((out, want["out"]), (var_out, want["var_out"]), (length, want["length"])):
        if (~bad).any():
            fig = max(fig, float(np.abs(a[~bad] - b[~bad]).max() / np.abs(b[~bad]).max()))
    return fig


def run_both(G, W, H, frames, identical=False, **params):
    """the frames through the library's host entry and through the restatement with the library's M: [(got, want)]"""
    t, ref, pairs = G.Temporal(W, H), T.Temporal(W, H), []
    for cam, u, v, feat in frames:
        gc = T.gdpt_camera(G, cam)
        want = ref.push(cam, G.temporal_world_to_sample(gc), u, v, feat, **params)
        assert T.margin(want["margins"], identical=identical) >= T.MARGIN, want["margins"]
        pairs.append((t.push(gc, u, v, feat, **params), want))
    t.close()
    return pairs


@pytest.mark.parametrize("planted", [False, True], ids=["clean", "planted"])
@pytest.mark.parametrize("move", T.MOVES)
@pytest.mark.parametrize("W,H", FILMS)
def test_kernel_equals_the_restatement(G, W, H, move, planted):
    worst = 0.0
    for k, (got, want) in enumerate(run_both(G, W, H, frames_of(W, H, move, planted), identical=move == "identical")):
        worst = max(worst, figure(got, want))
        assert got[3].push_ms > 0
    print(f"temporal {W}x{H} {move} {'planted' if planted else 'clean'}: worst figure {worst:.3e} (bound {BOUND:.1e})")
    assert worst < BOUND


@pytest.mark.parametrize("tau_n", [0.0, -1.0])
def test_no_normal_is_no_tap_at_any_tau_n(G, tau_n):
    """17 x 17 planted under identical cameras and a non-positive tau_n, where a stored zero normal would pass the normal test"""
    worst = 0.0
    for got, want in run_both(G, 17, 17, frames_of(17, 17, "identical", True), identical=True, tau_n=tau_n):
        worst = max(worst, figure(got, want))
    assert want["reset"] == 4 and worst < BOUND


def test_the_cases_exercise_every_branch(G):
    """over the moves on 40 x 19 and 17 x 17 the pushes blend, some with a fractional history length, reset where the pan brings in
    new surface, and under `behind` meet w <= 0: most of the film resets although the camera is where it was two pushes before"""
    fractional = 0
    for W, H in ((40, 19), (17, 17)):
        seen = {}
        for move in T.MOVES:
            pairs = run_both(G, W, H, frames_of(W, H, move, True), identical=move == "identical")
            for got, want in pairs:
                fractional += int(((got[2] > 1) & (got[2] != np.round(got[2]))).sum())
            seen[move] = pairs[2][1]
            assert pairs[1][1]["left_out"] == 3 and pairs[2][1]["length"].max() >= 2
        assert seen["quarter_pan"]["reset"] > W * H // 5 and seen["subpixel_pan"]["reset"] == 0 and seen["identical"]["reset"] == 4
        assert seen["behind"]["reset"] > W * H // 2 > seen["dolly"]["reset"] == 0
        assert seen["rotation"]["background"] > seen["identical"]["background"] > 0
    assert fractional > 0, "a fractional history length"


def test_max_history_one_and_reset_return_the_input_bits(G):
    W, H = 33, 9
    frames = frames_of(W, H, "rotation", False)
    for got, (cam, u, v, feat) in zip([g for g, _ in run_both(G, W, H, frames, max_history=1)], frames):
        assert np.array_equal(got[0], u) and np.array_equal(got[1], v) and (got[2] == 1).all()
    t = G.Temporal(W, H)
    for k, (cam, u, v, feat) in enumerate(frames):
        if k == 2:
            t.reset()
        out, var_out, length, st = t.push(T.gdpt_camera(G, cam), u, v, feat)
        if k != 1:
            assert np.array_equal(out, u) and np.array_equal(var_out, v) and (length == 1).all()
            assert st.pixels_reset == int((feat[7] > 0).sum()) and st.sum_history == W * H
        else:
            assert length.max() > 1.5
    t.close()


def test_same_bits_twice_on_a_second_stream_and_from_both_entries(G):
    W, H = 33, 9
    frames = frames_of(W, H, "rotation", True)
    host = [g for g, _ in run_both(G, W, H, frames)]
    again = [g for g, _ in run_both(G, W, H, frames)]
    for a, b in zip(host, again):
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:3], b[:3]))
        assert (a[3].sum_history, a[3].pixels_reset) == (b[3].sum_history, b[3].pixels_reset)
    side = hip_rt.stream(G)
    d_in = [[hip_rt.upload(G, x) for x in (u, v, feat)] for _, u, v, feat in frames]
    d_out, d_var, d_len = hip_rt.alloc(G, 8 * W * H * 3), hip_rt.alloc(G, 8 * W * H * 3), hip_rt.alloc(G, 8 * W * H)
    for stream, stats in ((None, True), (side, True), (None, False), (side, False)):
        t = G.Temporal(W, H, stream=stream)
        for k, (cam, *_) in enumerate(frames):
            for p, nbytes in ((d_out, 8 * W * H * 3), (d_var, 8 * W * H * 3), (d_len, 8 * W * H)):
                hip_rt.ck(hip_rt.rt(G).hipMemset(C.c_void_p(p), 0, C.c_size_t(nbytes)))
            hip_rt.ck(hip_rt.rt(G).hipDeviceSynchronize())
            st = t.push_device(T.gdpt_camera(G, cam), *d_in[k], d_out, d_var, d_len, stats=stats)
            assert (st is None) == (not stats)                     # enqueue-only: the read-out below synchronises
            got = (hip_rt.to_host(G, d_out, (H, W, 3)), hip_rt.to_host(G, d_var, (H, W, 3)), hip_rt.to_host(G, d_len, (H, W)))
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, host[k][:3])), (stream, stats, k)
            if stats:
                assert (st.sum_history, st.pixels_left_out, st.pixels_background, st.pixels_reset) == \
                    (host[k][3].sum_history, host[k][3].pixels_left_out, host[k][3].pixels_background, host[k][3].pixels_reset)
        t.close()
    hip_rt.stream_destroy(G, side)
    for p in [x for trio in d_in for x in trio] + [d_out, d_var, d_len]:
        hip_rt.free(G, p)


def test_a_film_past_the_block_cap(G):
    """1025 x 345, the WIDE film of test_gpu_films_past_the_block_cap.py: 1430 tiles of 16 x 16 on 1024 blocks, so some block takes a
    second trip of the tile loop and the reduction a second trip over the partials (asserted first). Measured 1.188e-13: q reaches 1025
    here, and the absolute error of its fraction f, which the weights are made of, grows with q."""
    W, H = 1025, 345
    blocks, units = G.debug_knobs.image_grid("nlm", W, H)
    assert units > blocks > 256
    worst = 0.0
    for got, want in run_both(G, W, H, T.case(W, H, "rotation", True)):
        worst = max(worst, figure(got, want))
    print(f"temporal {W}x{H}: worst figure {worst:.3e} (bound {BOUND:.1e})")
    assert worst < BOUND


# ---- scenes ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cbox_xml(scene_tmp):
    return scene_variant(scene_tmp, "cbox/cbox_gdpt.xml", width=32, height=32, tag="temporal")


def copy_of(G, camera):
    return G.GdptCamera.from_buffer_copy(camera)


def test_frame_equals_its_pieces_called_by_hand(G, cbox_xml):
    """three frames of a 2 degree orbit of the 32 x 32 cbox at 4 spp in two passes, with the a-trous filter: bit for bit the pieces"""
    sd = G.parse_scene(cbox_xml)
    sc_a, sc_b = G.Scene(sd), G.Scene(sd)
    ta, tb = G.Temporal(32, 32), G.Temporal(32, 32)
    frames, spp = 3, 4
    for f in range(frames):
        cam = G.orbit_camera(sd.desc.camera, CBOX_CENTRE, 2.0 * f)
        r = ta.frame(sc_a, cam, f, frames, spp, 2, path=True, atrous=dict(levels=3), feature_spp=2)
        sc_b.set_camera(cam)
        ses = G.Progressive(sc_b, frames * spp, path=True, slice=(f * spp, spp))
        ses.add_pass(2), ses.add_pass(2)
        means, vars_, _ = ses.read()
        ses.close()
        feat, fvar = sc_b.features(2, window=(frames * spp, f * spp))
        out, var_out, length, st = tb.push(cam, means["img"], vars_["img"], feat)
        den, den_var, _ = G.denoise_atrous(out, var_out, feat, fvar, guide=G.nlm_guide(), levels=3)
        for name, want in (("mean", means["img"]), ("var", vars_["img"]), ("feat", feat), ("feat_var", fvar), ("out", out), ("var_out", var_out),
                           ("length", length), ("denoised", den), ("denoised_var", den_var)):
            assert np.array_equal(r[name], want), (f, name)
        assert r["stats"].sum_history == st.sum_history
        if f > 0:
            assert st.sum_history > 1.5 * 32 * 32, "most of the film keeps its history through a 2 degree orbit"
            assert not np.array_equal(out, means["img"])
    with pytest.raises(G.GdptError, match="at least two passes"):
        ta.frame(sc_a, sd.desc.camera, 0, 1, 4, 3)
    for x in (ta, tb, sc_a, sc_b):
        x.close()


def renders(G, sc, spp=4):
    """(Path image, the five GradPath buffers, feature means and variances) of the handle as it stands"""
    img, _ = sc.path_render(spp=spp)
    bufs, _ = sc.render(spp=spp)
    feat, fvar = sc.features(spp)
    return [img] + [bufs[k] for k in ("img", "cx0", "cy0", "cx1", "cy1")] + [feat, fvar]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("rel,film,centre", [("cbox/cbox_gdpt.xml", (32, 32), CBOX_CENTRE), ("sponza/sponza.xml", (33, 17), None)], ids=["cbox", "sponza_hbm"])
def test_set_camera_equals_a_fresh_upload(G, scene_tmp, rel, film, centre):
    """centre None: the camera turns about its own position (sponza's stands inside the scene)"""
    xml = scene_variant(scene_tmp, rel, width=film[0], height=film[1], tag="setcam")
    sd, sd_moved = G.parse_scene(xml), G.parse_scene(xml)
    first_cam = copy_of(G, sd.desc.camera)
    c2w = np.array(list(first_cam.cam_to_world)).reshape(4, 4)
    moved = G.orbit_camera(first_cam, centre if centre is not None else c2w[:3, 3] / c2w[3, 3], 2.0)
    sc = G.Scene(sd)
    first = renders(G, sc)
    sc.set_camera(moved)
    after = renders(G, sc)
    C.memmove(C.byref(sd_moved.desc.camera), C.byref(moved), C.sizeof(G.GdptCamera))
    fresh_scene = G.Scene(sd_moved)
    fresh = renders(G, fresh_scene)
    assert same(after, fresh), "after the setter: the bits of a fresh upload with the camera replaced"
    assert not np.array_equal(after[0], first[0]) and not np.array_equal(after[6], first[6])
    sc.set_camera(first_cam)
    assert same(renders(G, sc), first), "set back: the bits of the first render"
    # a render enqueued before the setter keeps the old camera
    W, H = film
    side = hip_rt.stream(G)
    d_img = hip_rt.alloc(G, 8 * W * H * 3)
    sc.path_render_device(d_img, spp=4, stream=side)
    sc.set_camera(moved)
    assert np.array_equal(hip_rt.to_host(G, d_img, (H, W, 3)), first[0])
    sc.path_render_device(d_img, spp=4, stream=side)
    assert np.array_equal(hip_rt.to_host(G, d_img, (H, W, 3)), after[0])
    hip_rt.stream_destroy(G, side)
    hip_rt.free(G, d_img)
    # refusals leave the handle as it is
    sc.set_camera(first_cam)
    far = copy_of(G, first_cam)
    far.cam_to_world[3] = 1e7
    cases = [(far, "outside the extent")]
    for field, value, match in (("width", W + 1, "width"), ("height", H + 1, "height"), ("filter_type", first_cam.filter_type + 1, "filter_type"),
                                ("filter_param", first_cam.filter_param + 0.5, "filter_param")):
        bad = copy_of(G, first_cam)
        setattr(bad, field, value)
        cases.append((bad, match))
    for field in ("sample_to_cam", "cam_to_world"):
        bad = copy_of(G, first_cam)
        getattr(bad, field)[6] = np.nan
        cases.append((bad, field + " has a non-finite"))
    for bad, match in cases:
        with pytest.raises(G.GdptError, match=match):
            sc.set_camera(bad)
    with pytest.raises(G.GdptError, match="camera is null"):
        sc.set_camera(None)
    assert same(renders(G, sc), first), "a refused camera leaves the handle rendering as before"
    for x in (sc, fresh_scene):
        x.close()


# ---- the CLI --------------------------------------------------------------------------------------------------------------------

CLI_RUNS = {"gradpath": ["--film", "32x32", "--spp", "4", "-o", "a.exr"],
            "session_atrous": ["--film", "32x32", "--spp", "4", "--pass-spp", "2", "--denoised", "d.pfm", "--atrous-levels", "3", "-o", "b.pfm"]}


def cli_hashes(exe, tmp):
    """sha256 of every file each run of CLI_RUNS writes into an empty directory"""
    got = {}
    for name, args in CLI_RUNS.items():
        d = os.path.join(str(tmp), name)
        os.makedirs(d)
        subprocess.run([exe, *args, os.path.join(ROOT, "scenes", "cbox", "cbox_gdpt.xml")], cwd=d, check=True, capture_output=True, timeout=120)
        for f in sorted(os.listdir(d)):
            got[f"{name}/{f}"] = hashlib.sha256(open(os.path.join(d, f), "rb").read()).hexdigest()
    return got


def test_files_written_without_frames_are_what_they_were(tmp_path):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "temporal_cli_hashes.json")))
    assert cli_hashes(EXE, tmp_path) == want["files"]


def test_cli_frames_write_numbered_files(tmp_path):
    """three frames of a 2 degree orbit, plain and with --temporal and the a-trous filter: the numbered files and nothing else"""
    scene = os.path.join(ROOT, "scenes", "cbox", "cbox_gdpt.xml")
    base = [EXE, "--film", "32x32", "--spp", "4", "--pass-spp", "2", "--frames", "3", "--orbit", "2"]
    subprocess.run([*base, "-o", "plain.pfm", scene], cwd=tmp_path, check=True, capture_output=True, timeout=120)
    r = subprocess.run([*base, "--temporal", "--temporal-max-history", "8", "--denoised", "den.pfm", "--atrous-levels", "3", "-o", "acc.pfm", scene],
                       cwd=tmp_path, check=True, capture_output=True, text=True, timeout=120)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(f"{n}_{f:04d}.pfm" for n in ("plain", "acc", "den") for f in range(3)), names
    assert "mean history" in r.stdout and "frame 2" in r.stdout
