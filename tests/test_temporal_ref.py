"""The numpy restatement of temporal reprojection (temporal_ref.py; include/gdpt.h: gdpt_temporal_*) on the CPU: against a plain
triple loop that reads the definition pixel by pixel, its exact identities, disocclusion against a set computed from the geometry
alone, planted invalid pixels, and the condition every case of the GPU test must meet: no decision within MARGIN of its threshold."""
import math

import numpy as np
import pytest

import temporal_ref as T

FILMS = [(1, 1), (5, 3), (9, 7), (21, 13)]
GPU_FILMS = [(1, 1), (16, 16), (17, 17), (33, 9), (40, 19)]       # of test_gpu_temporal.py


def run(W, H, frames, **params):
    """the restatement over the frames of a case: the list of push results"""
    t = T.Temporal(W, H)
    return [t.push(cam, T.world_to_sample(cam), u, v, feat, **params) for cam, u, v, feat in frames]


# ---- the plain loop -------------------------------------------------------------------------------------------------------------

def ray(cam, x, y):
    s, c = cam["s2c"], cam["c2w"]
    rx, ry = (x + 0.5) / cam["W"], (y + 0.5) / cam["H"]
    t = [s[k, 0] * rx + s[k, 1] * ry + s[k, 2] * 0.0 + s[k, 3] for k in range(4)]
    pt = [t[k] * (1.0 / t[3]) for k in range(3)]
    il = 1.0 / math.sqrt(pt[0] * pt[0] + pt[1] * pt[1] + pt[2] * pt[2])
    pt = [a * il for a in pt]
    d = [c[k, 0] * pt[0] + c[k, 1] * pt[1] + c[k, 2] * pt[2] for k in range(3)]
    il = 1.0 / math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return [c[k, 3] * (1.0 / c[3, 3]) for k in range(3)], [a * il for a in d]


def plain(W, H, frames, tau_z=0.05, tau_n=0.9, s_min=1e-3, max_history=32):
    """The definition, one pixel, one tap and one channel at a time. Returns [(out, var_out, length, (left_out, background, reset))]."""
    hist, results = None, []
    for cam, u, v, feat in frames:
        out, var_out, length = u.copy(), v.copy(), np.zeros((H, W))
        new = dict(U=out, V=var_out, N=length, n=np.zeros((H, W, 3)), d=np.zeros((H, W)), cov=np.zeros((H, W)))
        counts = [0, 0, 0]
        for y in range(H):
            for x in range(W):
                if not all(math.isfinite(u[y, x, c]) and math.isfinite(v[y, x, c]) and v[y, x, c] >= 0 for c in range(3)):
                    counts[0] += 1
                    continue
                length[y, x] = 1.0
                cov = feat[7, y, x]
                if not cov > 0:
                    counts[1] += 1
                    continue
                d = feat[6, y, x] / cov
                n = [feat[3 + c, y, x] for c in range(3)]
                ln = math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
                n = [a * (1.0 / ln) for a in n] if ln > 0 else [0.0, 0.0, 0.0]
                new["n"][y, x], new["d"][y, x], new["cov"][y, x] = n, d, cov
                taps = []
                if hist is not None and any(a != 0 for a in n):
                    org, dr = ray(cam, x, y)
                    X = [org[k] + d * dr[k] for k in range(3)]
                    M = hist["M"]
                    sx, sy, _, w = [M[k, 0] * X[0] + M[k, 1] * X[1] + M[k, 2] * X[2] + M[k, 3] for k in range(4)]
                    if w > 0:
                        qx, qy = sx / w * W - 0.5, sy / w * H - 0.5
                        if -1.0 <= qx <= W and -1.0 <= qy <= H:
                            i0, j0 = math.floor(qx), math.floor(qy)
                            fx, fy = qx - i0, qy - j0
                            dX = [X[k] - hist["org"][k] for k in range(3)]
                            e = math.sqrt(dX[0] * dX[0] + dX[1] * dX[1] + dX[2] * dX[2])
                            for b in (0, 1):
                                for a in (0, 1):
                                    tx, ty = i0 + a, j0 + b
                                    if not (0 <= tx < W and 0 <= ty < H):
                                        continue
                                    if not (hist["N"][ty, tx] >= 1 and hist["cov"][ty, tx] > 0):
                                        continue
                                    if not abs(hist["d"][ty, tx] - e) <= tau_z * e:
                                        continue
                                    nq = hist["n"][ty, tx]
                                    if not any(a_ != 0 for a_ in nq):
                                        continue
                                    if not n[0] * nq[0] + n[1] * nq[1] + n[2] * nq[2] >= tau_n:
                                        continue
                                    taps.append(((fx if a else 1.0 - fx) * (fy if b else 1.0 - fy), tx, ty))
                S = 0.0
                for bt, _, _ in taps:
                    S += bt
                if not taps or S < s_min:
                    counts[2] += 1
                    continue
                N = 0.0
                for bt, tx, ty in taps:
                    N += bt * hist["N"][ty, tx]
                Np = min(N / S + 1.0, float(max_history))
                length[y, x] = Np
                if not Np > 1.0:
                    continue
                alpha = 1.0 / Np
                keep = 1.0 - alpha
                for c in range(3):
                    U = V = 0.0
                    for bt, tx, ty in taps:
                        U += bt * hist["U"][ty, tx, c]
                        V += (bt * bt) * hist["V"][ty, tx, c]
                    U, V = U / S, V / (S * S)
                    out[y, x, c] = U + alpha * (u[y, x, c] - U)
                    var_out[y, x, c] = (keep * keep) * V + (alpha * alpha) * v[y, x, c]
        new["M"], new["org"] = T.world_to_sample(cam), T.origin(cam)
        hist = new
        results.append((out, var_out, length.copy(), tuple(counts)))
    return results


@pytest.mark.parametrize("planted", [False, True], ids=["clean", "planted"])
@pytest.mark.parametrize("move", T.MOVES)
@pytest.mark.parametrize("W,H", FILMS)
def test_restatement_equals_the_plain_loop(W, H, move, planted):
    frames = T.case(W, H, move, planted)
    got, want = run(W, H, frames), plain(W, H, frames)
    for k, (g, (out, var_out, length, counts)) in enumerate(zip(got, want)):
        assert T.margin(g["margins"], identical=move == "identical") >= T.MARGIN, (k, g["margins"])
        assert (g["left_out"], g["background"], g["reset"]) == counts, k
        assert np.array_equal(g["length"] == 0, length == 0) and np.array_equal(g["length"] == 1, length == 1)
        bad = g["masks"]["left_out"]
        assert np.array_equal(g["out"][bad], out[bad], equal_nan=True) and np.array_equal(g["var_out"][bad], var_out[bad], equal_nan=True)
        for a, b in ((g["out"], out), (g["var_out"], var_out), (g["length"], length)):
            assert np.allclose(a[~bad], b[~bad], rtol=1e-14, atol=0), k


@pytest.mark.parametrize("planted", [False, True], ids=["clean", "planted"])
@pytest.mark.parametrize("move", T.MOVES)
@pytest.mark.parametrize("W,H", GPU_FILMS)
def test_every_case_of_the_gpu_test_keeps_its_margin(W, H, move, planted):
    """The condition on the inputs: no decision of any push within MARGIN of its threshold (with numpy's M; the GPU test asserts it
    again with the library's)."""
    for k, g in enumerate(run(W, H, T.case(W, H, move, planted))):
        assert T.margin(g["margins"], identical=move == "identical") >= T.MARGIN, (k, g["margins"])


# ---- identities -----------------------------------------------------------------------------------------------------------------

def all_surface(W, H, k, seed=3):
    """k frames of one camera in front of an unbounded far plane: every pixel a surface pixel"""
    rng = np.random.default_rng(seed)
    cam = T.camera(W, H, T.look_at((0, 0, 0), (0, 0, 1)), T.FOV)
    feat, which = T.features(cam, [T.plane((0, 0, T.Z_FAR), (0, 0, -1))])
    assert (which == 0).all()
    return [(cam, rng.uniform(0.5, 1.5, (H, W, 3)), rng.uniform(0.01, 0.02, (H, W, 3)), feat) for _ in range(k)]


@pytest.mark.parametrize("W,H", [(5, 3), (21, 13)])
def test_identical_cameras_give_the_running_mean(W, H):
    k = 6
    frames = all_surface(W, H, k)
    got = run(W, H, frames, max_history=k)
    for i, g in enumerate(got):
        mean = sum(f[1] for f in frames[:i + 1]) / (i + 1)
        var = sum(f[2] for f in frames[:i + 1]) / (i + 1) ** 2
        assert np.abs(g["out"] - mean).max() <= 1e-13 * np.abs(mean).max()
        assert np.abs(g["var_out"] - var).max() <= 1e-13 * np.abs(var).max()
        assert np.abs(g["length"] - (i + 1)).max() <= 1e-13 * (i + 1)
        assert (g["left_out"], g["background"], g["reset"]) == (0, 0, W * H if i == 0 else 0)


def test_first_push_and_push_after_reset_return_the_input_bits():
    W, H = 9, 7
    frames = T.case(W, H, "subpixel_pan", False)
    t = T.Temporal(W, H)
    for k, (cam, u, v, feat) in enumerate(frames):
        if k == 2:
            t.reset()
        g = t.push(cam, T.world_to_sample(cam), u, v, feat)
        if k != 1:
            assert np.array_equal(g["out"], u) and np.array_equal(g["var_out"], v) and (g["length"] == 1).all()
            assert g["reset"] == int((feat[7] > 0).sum()) and g["background"] == int((feat[7] == 0).sum())
        else:
            assert not np.array_equal(g["out"], u) and g["length"].max() > 1.5


@pytest.mark.parametrize("move", T.MOVES)
def test_max_history_one_returns_the_input_bits_always(move):
    W, H = 9, 7
    frames = T.case(W, H, move, False)
    for g, (cam, u, v, feat) in zip(run(W, H, frames, max_history=1), frames):
        assert np.array_equal(g["out"], u) and np.array_equal(g["var_out"], v) and (g["length"] == 1).all()


# ---- disocclusion ---------------------------------------------------------------------------------------------------------------

def test_disocclusion_resets_exactly_the_uncovered_pixels():
    """A fronto-parallel near plane in front of a far one, the camera panned by 2.37 far-plane pixels across and 0.29 down: a pixel
    of the second frame keeps its history exactly when one of the four previous pixels around its reprojected position saw the
    SAME plane. That set is computed here from the geometry (which plane each pixel centre sees, and a pinhole projection written out
    by hand), not from the code under test."""
    W, H = 21, 13
    planes = T.step_scene(tilted=False)
    px = T.far_pixel(W)
    pos = [(0.0, 0.0, 0.0), (2.37 * px, 0.29 * px, 0.0)]
    cams = [T.camera(W, H, T.look_at(p, (p[0], p[1], 1.0)), T.FOV) for p in pos]
    rng = np.random.default_rng(5)
    frames, which = [], []
    for cam in cams:
        feat, wh = T.features(cam, planes)
        frames.append((cam, rng.uniform(0.5, 1.5, (H, W, 3)), rng.uniform(0.01, 0.02, (H, W, 3)), feat))
        which.append(wh)
    t = math.tan(math.radians(T.FOV) / 2)
    expected = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            k = which[1][y, x]
            if k < 0:
                continue
            z = (T.Z_FAR, T.Z_NEAR)[k]
            # the point the pixel centre sees, by similar triangles from the second camera; then the first camera's pixel position
            X = (pos[1][0] + ((x + 0.5) / W * 2 - 1) * t * z, pos[1][1] + (1 - (y + 0.5) / H * 2) * t * H / W * z)
            qx = (X[0] / (t * z) + 1) / 2 * W - 0.5
            qy = (1 - X[1] / (t * H / W * z)) / 2 * H - 0.5
            same = [0 <= math.floor(qx) + a < W and 0 <= math.floor(qy) + b < H and which[0][math.floor(qy) + b, math.floor(qx) + a] == k
                    for b in (0, 1) for a in (0, 1)]
            expected[y, x] = not any(same)
    got = run(W, H, frames)[1]
    assert T.margin(got["margins"]) >= T.MARGIN
    assert np.array_equal(got["masks"]["reset"], expected)
    assert 0 < expected.sum() < (which[1] >= 0).sum()                      # some are uncovered, most are not
    near_edge = expected & (which[1] == 0)
    assert near_edge.any(), "far-plane pixels uncovered by the near plane's move"


# ---- planted pixels -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tau_n", [0.9, 0.0, -1.0])
def test_planted_pixels_are_counted_and_never_a_tap(tau_n):
    """Each kind in its own count; in the next push (identical cameras, so every pixel's taps are itself and weightless neighbours) the
    pixel that was left out, background or without a normal has no history: it is reset, while its neighbours blend."""
    W, H = 9, 7
    frames = all_surface(W, H, 2)
    cam, u, v, feat = frames[0]
    u, v, feat = u.copy(), v.copy(), feat.copy()
    u[1, 1, 0] = np.nan
    v[1, 3, 1] = np.inf
    v[1, 5, 2] = -1e-6
    feat[3:8, 3, 1] = 0.0            # no coverage
    feat[3:6, 3, 3] = 0.0            # no normal
    frames[0] = (cam, u, v, feat)
    a, b = run(W, H, frames, tau_n=tau_n)             # (at tau_n <= 0 a zero normal would pass the normal test: it is no tap by itself)
    assert (a["left_out"], a["background"], a["reset"]) == (3, 1, W * H - 4)
    assert a["length"][1, 1] == a["length"][1, 3] == a["length"][1, 5] == 0 and a["length"][3, 1] == a["length"][3, 3] == 1
    assert np.isnan(a["out"][1, 1, 0]) and np.isinf(a["var_out"][1, 3, 1]) and a["var_out"][1, 5, 2] == -1e-6
    spots = np.zeros((H, W), dtype=bool)
    for y, x in ((1, 1), (1, 3), (1, 5), (3, 1), (3, 3)):
        spots[y, x] = True
    assert T.margin(b["margins"], identical=True) >= T.MARGIN
    assert np.array_equal(b["masks"]["reset"], spots)
    assert (b["length"][spots] == 1).all() and np.allclose(b["length"][~spots], 2.0, rtol=1e-13)
    assert np.array_equal(b["out"][spots], frames[1][1][spots]) and np.isfinite(b["out"]).all() and np.isfinite(b["var_out"]).all()
