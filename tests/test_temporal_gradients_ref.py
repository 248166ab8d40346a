"""The numpy restatement of the gradient push (temporal_gradients_ref.py) on the CPU: against a plain per-pixel loop that follows
include/gdpt.h line by line; its identities; the primal against temporal_ref bit for bit; the analytic Jacobian of a fronto-parallel
plane; and the experiment the feature rests on, rebuilt from the restatement: on a textured plane the reprojected gradient with the
Jacobian is several times closer to the new frame's exact differences than the same gather without it."""
import functools
import math

import numpy as np
import pytest

import temporal_gradients_ref as TG
import temporal_ref as T

FILMS = [(1, 1), (5, 3), (9, 7), (21, 13)]


@functools.lru_cache(maxsize=None)
def frames_of(W, H, move, planted):
    return TG.case(W, H, move, planted)


# ---- the plain loop -------------------------------------------------------------------------------------------------------------

def ray_dir(cam, rx, ry):
    s, c = cam["s2c"], cam["c2w"]
    row = lambda k: s[k, 0] * rx + s[k, 1] * ry + s[k, 2] * 0.0 + s[k, 3]      # noqa: E731
    iw = 1.0 / row(3)
    pt = [row(0) * iw, row(1) * iw, row(2) * iw]
    il = 1.0 / math.sqrt(pt[0] * pt[0] + pt[1] * pt[1] + pt[2] * pt[2])
    pt = [a * il for a in pt]
    d = [c[k, 0] * pt[0] + c[k, 1] * pt[1] + c[k, 2] * pt[2] for k in range(3)]
    il = 1.0 / math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return [a * il for a in d]


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def loop_push(W, H, cam, prev, gprev, frame, tau_z, tau_n, s_min, max_history, j_max, cos_min):
    """one gradient push pixel by pixel, tap by tap, channel by channel. prev: the primal history of temporal_ref (or None), gprev:
    the gradient history (or None: stale). Returns out, var_out, length, gx_out, gx_var_out, gy_out, gy_var_out, glength and the five counts."""
    _, u, v, feat, gx, gxv, gy, gyv = frame
    g, gv = (gx, gy), (gxv, gyv)
    res = dict(out=u.copy(), var_out=v.copy(), length=np.zeros((H, W)), glength=np.zeros((H, W)),
               g_out=[gx.copy(), gy.copy()], gv_out=[gxv.copy(), gyv.copy()], left_out=0, background=0, reset=0, gradient_reset=0)
    org = [float(a) for a in T.origin(cam)]
    for y in range(H):
        for x in range(W):
            vals = [a[y, x, c] for a in (u, v, gx, gxv, gy, gyv) for c in range(3)]
            variances = [a[y, x, c] for a in (v, gxv, gyv) for c in range(3)]
            if not all(math.isfinite(a) for a in vals) or any(a < 0 for a in variances):
                res["left_out"] += 1
                continue
            res["length"][y, x] = res["glength"][y, x] = 1.0
            cov = feat[7, y, x]
            if not cov > 0:
                res["background"] += 1
                continue
            d = feat[6, y, x] / cov
            n = [feat[3 + k, y, x] for k in range(3)]
            ln = math.sqrt(dot(n, n))
            if not ln > 0 or prev is None:
                res["reset"] += 1
                continue
            n = [a * (1.0 / ln) for a in n]
            dr = ray_dir(cam, (x + 0.5) / W, (y + 0.5) / H)
            X = [org[k] + d * dr[k] for k in range(3)]
            Mp = prev["M"]
            hom = lambda P, i: Mp[i, 0] * P[0] + Mp[i, 1] * P[1] + Mp[i, 2] * P[2] + Mp[i, 3]      # noqa: E731
            w = hom(X, 3)
            if not w > 0:
                res["reset"] += 1
                continue
            qx, qy = hom(X, 0) / w * W - 0.5, hom(X, 1) / w * H - 0.5
            if not (-1.0 <= qx <= W and -1.0 <= qy <= H):
                res["reset"] += 1
                continue
            i0, j0 = math.floor(qx), math.floor(qy)
            fx, fy = qx - i0, qy - j0
            dX = [X[k] - prev["org"][k] for k in range(3)]
            e = math.sqrt(dot(dX, dX))
            S = N = Ng = 0.0
            U, V = [0.0] * 3, [0.0] * 3
            G, VG = [[0.0] * 3, [0.0] * 3], [[0.0] * 3, [0.0] * 3]
            for b in (0, 1):
                for a in (0, 1):
                    tx, ty = i0 + a, j0 + b
                    if tx < 0 or ty < 0 or tx >= W or ty >= H:
                        continue
                    nq = prev["n"][ty, tx]
                    if not prev["N"][ty, tx] >= 1 or not prev["cov"][ty, tx] > 0 or not abs(prev["d"][ty, tx] - e) <= tau_z * e:
                        continue
                    if not (nq != 0).any() or not dot(n, nq) >= tau_n:
                        continue
                    bt = (fx if a else 1.0 - fx) * (fy if b else 1.0 - fy)
                    S += bt
                    N += bt * prev["N"][ty, tx]
                    for c in range(3):
                        U[c] += bt * prev["U"][ty, tx, c]
                        V[c] += (bt * bt) * prev["V"][ty, tx, c]
                    if gprev is not None:
                        Ng += bt * gprev["N"][ty, tx]
                        for k in range(2):
                            for c in range(3):
                                G[k][c] += bt * gprev["G"][k][ty, tx, c]
                                VG[k][c] += (bt * bt) * gprev["VG"][k][ty, tx, c]
            if not S >= s_min:
                res["reset"] += 1
                continue
            Np = min(N / S + 1.0, float(max_history))
            res["length"][y, x] = Np
            if Np > 1:
                al = 1.0 / Np
                for c in range(3):
                    Uc, Vc = U[c] / S, V[c] / (S * S)
                    res["out"][y, x, c] = Uc + al * (u[y, x, c] - Uc)
                    res["var_out"][y, x, c] = ((1.0 - al) * (1.0 - al)) * Vc + (al * al) * v[y, x, c]
            # the gradients of a blending pixel
            J, fine = [0.0] * 4, gprev is not None
            c0 = dot(n, dr)
            for k, (ox, oy) in enumerate(((-0.5, 0.5), (0.5, -0.5))):
                if not fine:
                    break
                dk = ray_dir(cam, (x + ox) / W, (y + oy) / H)
                ck = dot(n, dk)
                if abs(ck) < cos_min or not c0 / ck > 0:
                    fine = False
                    break
                tk = d * (c0 / ck)
                Xk = [org[i] + tk * dk[i] for i in range(3)]
                wk = hom(Xk, 3)
                if not wk > 0:
                    fine = False
                    break
                J[2 * k], J[2 * k + 1] = qx - (hom(Xk, 0) / wk * W - 0.5), qy - (hom(Xk, 1) / wk * H - 0.5)
                if not (abs(J[2 * k]) <= j_max and abs(J[2 * k + 1]) <= j_max):
                    fine = False
            if not fine:
                res["gradient_reset"] += 1
                continue
            Ngp = min(Ng / S + 1.0, float(max_history))
            res["glength"][y, x] = Ngp
            if Ngp > 1:
                al = 1.0 / Ngp
                for k in range(2):
                    for c in range(3):
                        Gx, Gy, VGx, VGy = G[0][c] / S, G[1][c] / S, VG[0][c] / (S * S), VG[1][c] / (S * S)
                        Hk = J[2 * k] * Gx + J[2 * k + 1] * Gy
                        VHk = (J[2 * k] * J[2 * k]) * VGx + (J[2 * k + 1] * J[2 * k + 1]) * VGy
                        res["g_out"][k][y, x, c] = Hk + al * (g[k][y, x, c] - Hk)
                        res["gv_out"][k][y, x, c] = ((1.0 - al) * (1.0 - al)) * VHk + (al * al) * gv[k][y, x, c]
    return res


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("planted", [False, True], ids=["clean", "planted"])
@pytest.mark.parametrize("move", T.MOVES)
@pytest.mark.parametrize("W,H", FILMS)
def test_restatement_equals_the_plain_loop(W, H, move, planted):
    ref = TG.TemporalGradients(W, H)
    for k, frame in enumerate(frames_of(W, H, move, planted)):
        cam = frame[0]
        prev, gprev = ref.primal.hist, ref.ghist
        want = loop_push(W, H, cam, prev, gprev, frame, j_max=4.0, cos_min=0.02, **T.DEFAULTS)
        got = ref.push(cam, T.world_to_sample(cam), *frame[1:])
        assert T.margin(got["margins"], identical=move == "identical") >= T.MARGIN, got["margins"]
        for name in ("out", "var_out", "length", "glength"):
            assert same(got[name], want[name]), (k, name)
        for i, name in enumerate(("gx", "gy")):
            assert same(got[name + "_out"], want["g_out"][i]) and same(got[name + "_var_out"], want["gv_out"][i]), (k, name)
        for name in ("left_out", "background", "reset", "gradient_reset"):
            assert got[name] == want[name], (k, name)
        assert got["sum_gradient_history"] == float(want["glength"].sum())
        if planted and W * H >= 8 and k < 2:
            assert got["left_out"] == 3 + 2                      # temporal_ref's three and the two invalid gradients
            assert (got["glength"] == 0).sum() == 5 and same(got["glength"] == 0, got["length"] == 0)


@pytest.mark.parametrize("move", T.MOVES)
def test_primal_is_temporal_ref_bit_for_bit_on_clean_inputs(move):
    W, H = 21, 13
    ref, plain = TG.TemporalGradients(W, H), T.Temporal(W, H)
    for frame in frames_of(W, H, move, False):
        cam, u, v, feat = frame[:4]
        M = T.world_to_sample(cam)
        got, want = ref.push(cam, M, *frame[1:]), plain.push(cam, M, u, v, feat)
        for name in ("out", "var_out", "length"):
            assert np.array_equal(got[name], want[name]), name
        assert all(got[k] == want[k] for k in ("left_out", "background", "reset", "sum_history"))


def test_identical_cameras_give_the_running_mean():
    W, H = 9, 7
    frames = frames_of(W, H, "identical", False)
    ref = TG.TemporalGradients(W, H)
    for k, frame in enumerate(frames):
        r = ref.push(frame[0], T.world_to_sample(frame[0]), *frame[1:])
    m = r["masks"]["gradient_blend"]
    assert m.sum() > W * H // 2 and (r["glength"][m] == 3).all()
    for name, i, iv in (("gx", 4, 5), ("gy", 6, 7)):
        mean = sum(f[i] for f in frames) / 3.0
        var = sum(f[iv] for f in frames) / 9.0
        assert np.abs(r[name + "_out"][m] - mean[m]).max() < 1e-12 and np.abs(r[name + "_var_out"][m] - var[m]).max() < 1e-12


def test_pushes_that_return_the_gradient_inputs_bits():
    W, H = 21, 13
    frames = frames_of(W, H, "rotation", False)
    grads = lambda r: [r[k] for k in ("gx_out", "gx_var_out", "gy_out", "gy_var_out")]      # noqa: E731
    inputs = lambda f: [f[4], f[5], f[6], f[7]]      # noqa: E731
    M = [T.world_to_sample(f[0]) for f in frames]
    ref = TG.TemporalGradients(W, H)
    r = ref.push(frames[0][0], M[0], *frames[0][1:])                       # the first push
    assert all(same(a, b) for a, b in zip(grads(r), inputs(frames[0]))) and (r["glength"] == 1).all() and r["gradient_reset"] == 0
    r = ref.push(frames[1][0], M[1], *frames[1][1:])
    assert r["masks"]["gradient_blend"].sum() > W * H // 2 and not same(r["gx_out"], frames[1][4])
    ref.reset()                                                              # the push after reset
    r = ref.push(frames[2][0], M[2], *frames[2][1:])
    assert all(same(a, b) for a, b in zip(grads(r), inputs(frames[2]))) and (r["glength"] == 1).all()
    ref = TG.TemporalGradients(W, H)                                         # a push after a plain push: the primal blends, every gradient restarts
    ref.push(frames[0][0], M[0], *frames[0][1:])
    ref.push_plain(frames[1][0], M[1], *frames[1][1:4])
    r = ref.push(frames[2][0], M[2], *frames[2][1:])
    blending = ~r["masks"]["left_out"] & ~r["masks"]["background"] & ~r["masks"]["reset"]
    assert all(same(a, b) for a, b in zip(grads(r), inputs(frames[2]))) and (r["glength"] == 1).all()
    assert r["gradient_reset"] == blending.sum() > W * H // 2 and r["length"].max() > 2
    ref = TG.TemporalGradients(W, H)                                         # max_history = 1
    for f, m in zip(frames, M):
        r = ref.push(f[0], m, *f[1:], max_history=1)
        assert all(same(a, b) for a, b in zip(grads(r), inputs(f))) and (r["glength"] == 1).all() and same(r["out"], f[1])


# ---- the Jacobian on planes -----------------------------------------------------------------------------------------------------

PW, PH = 64, 48
FRONTO = T.plane((0, 0, 10), (0, 0, -1))
TILTED = T.plane((0, 0, 8), (0.6, 0.1, -1))


def texture(X):
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    return np.stack([np.sin(0.9 * x + 0.4 * y), np.cos(0.5 * x - 0.8 * y + 0.3 * z), 0.3 * x * y], axis=-1)


def plane_frame(cam, pl):
    """(u, feat, exact backward differences gx, gy) of the textured plane seen by `cam`; column 0 of gx and row 0 of gy are 0"""
    feat, which = T.features(cam, [pl])
    assert (which == 0).all()
    org, d = T.rays(cam)
    img = texture(org[None, None, :] + feat[6][..., None] * d)
    gx, gy = np.zeros_like(img), np.zeros_like(img)
    gx[:, 1:], gy[1:, :] = img[:, 1:] - img[:, :-1], img[1:, :] - img[:-1, :]
    return img, feat, gx, gy


def two_pushes(pl, cams, **kw):
    """frame 0 pushed with its exact differences, then frame 1: the second push's dict and frame 1's exact differences"""
    ref = TG.TemporalGradients(PW, PH)
    var = np.full((PH, PW, 3), 1e-4)
    for cam in cams[:2]:
        img, feat, gx, gy = plane_frame(cam, pl)
        r = ref.push(cam, T.world_to_sample(cam), img, var, feat, gx, var, gy, var, **kw)
    assert T.margin(r["margins"]) >= T.MARGIN, r["margins"]
    return r, gx, gy


def inner(r):
    """the gradient-blending pixels that have four taps in the film, all of them and the pixel itself with x >= 1, y >= 1 (where the
    exact differences exist). A pixel at the film's edge that gathers from fewer than four taps is not a bilinear interpolation: its
    error is the gather's, with or without J (the figures of the experiment are reproduced to three digits with this mask alone)."""
    m = r["masks"]["gradient_blend"].copy()
    m[0, :] = m[:, 0] = False
    i0, j0 = np.floor(r["q"][0]), np.floor(r["q"][1])
    return m & (i0 >= 1) & (j0 >= 1) & (i0 + 1 <= PW - 1) & (j0 + 1 <= PH - 1)


def rms(a):
    return float(np.sqrt(np.mean(a * a)))


@pytest.mark.parametrize("name,pl,move", [("fronto", FRONTO, "dolly"), ("fronto", FRONTO, "rotation"), ("tilted", TILTED, "quarter_pan"),
                                          ("tilted", TILTED, "dolly"), ("tilted", TILTED, "rotation")],
                         ids=["fronto-dolly", "fronto-rotation", "tilted-quarter_pan", "tilted-dolly", "tilted-rotation"])
def test_the_jacobian_brings_the_history_gradient_to_the_new_frame(name, pl, move):
    cams = T.move_cameras(PW, PH, move)
    with_j, gx, gy = two_pushes(pl, cams)
    without, _, _ = two_pushes(pl, cams, force_identity=True)
    m = inner(with_j)
    assert np.array_equal(m, inner(without)) and m.sum() > PW * PH // 2
    for k, exact in (("Hx", gx), ("Hy", gy)):
        a, b = rms(with_j[k][m] - exact[m]), rms(without[k][m] - exact[m])
        print(f"{name} {move} {k}: {b:.3e} -> {a:.3e} (x{a / b:.3f}), gradient rms {rms(exact[m]):.3e}")
        assert a < 0.25 * b


@pytest.mark.parametrize("move", ["subpixel_pan", "quarter_pan"])
def test_a_pan_over_a_fronto_plane_needs_no_jacobian(move):
    cams = T.move_cameras(PW, PH, move)
    with_j, gx, gy = two_pushes(FRONTO, cams)
    without, _, _ = two_pushes(FRONTO, cams, force_identity=True)
    m = inner(with_j)
    assert m.sum() > PW * PH // 2
    for k, exact in (("Hx", gx), ("Hy", gy)):
        a, b = rms(with_j[k][m] - exact[m]), rms(without[k][m] - exact[m])
        assert abs(a - b) <= 1e-9 * b
    Jxx, Jyx, Jxy, Jyy = (j[m] for j in with_j["J"])
    assert max(np.abs(Jxx - 1).max(), np.abs(Jyy - 1).max(), np.abs(Jyx).max(), np.abs(Jxy).max()) < 1e-10


def test_a_dolly_towards_a_fronto_plane_scales_by_the_depth_ratio():
    cams = T.move_cameras(PW, PH, "dolly")
    r, _, _ = two_pushes(FRONTO, cams)
    m = r["masks"]["gradient_blend"]
    s = (10.0 - 0.8) / 10.0           # the depth of the plane along the axis, now over before
    Jxx, Jyx, Jxy, Jyy = (j[m] for j in r["J"])
    assert m.sum() > PW * PH // 2
    assert max(np.abs(Jxx - s).max(), np.abs(Jyy - s).max(), np.abs(Jyx).max(), np.abs(Jxy).max()) < 1e-10


def test_j_max_one_restarts_what_is_stretched_and_nothing_else():
    """towards the plane J = 0.92 I: nothing restarts at j_max = 1; away from it J = I / 0.92: every blending pixel does"""
    cams = T.move_cameras(PW, PH, "dolly")
    forward, _, _ = two_pushes(FRONTO, cams, j_max=1.0)
    back, _, _ = two_pushes(FRONTO, cams[1::-1], j_max=1.0)
    for r, stretched in ((forward, False), (back, True)):
        blending = ~r["masks"]["left_out"] & ~r["masks"]["background"] & ~r["masks"]["reset"]
        assert blending.sum() > PW * PH // 2
        assert np.array_equal(r["masks"]["gradient_reset"], blending if stretched else np.zeros_like(blending))
        assert r["gradient_reset"] == (blending.sum() if stretched else 0)


def test_a_grazing_plane_restarts_where_the_cosine_is_small():
    """a floor y = -1 under a pan: n^ = (0, 1, 0), so c_k is the y component of the neighbour ray, written down here from the pinhole
    alone: the ray through the sample (sx, sy) of a camera looking along +z is (t (2 sx - 1), t (H / W) (1 - 2 sy), 1), normalised"""
    cos_min = 0.1
    floor = T.plane((0, -1, 0), (0, 1, 0))
    cams = T.move_cameras(PW, PH, "subpixel_pan")
    ref = TG.TemporalGradients(PW, PH)
    rng = np.random.default_rng(5)
    for cam in cams[:2]:
        feat, _ = T.features(cam, [floor])
        a = [rng.uniform(0.5, 1.5, (PH, PW, 3)) for _ in range(3)]
        var = np.full((PH, PW, 3), 1e-3)
        r = ref.push(cam, T.world_to_sample(cam), a[0], var, feat, a[1], var, a[2], var, cos_min=cos_min)
    assert T.margin(r["margins"]) >= T.MARGIN, r["margins"]
    t = np.tan(np.radians(T.FOV) / 2)
    ys, xs = np.mgrid[0:PH, 0:PW]

    def cosine(sx, sy):
        d = np.stack([t * (2 * sx - 1), t * PH / PW * (1 - 2 * sy), np.ones_like(sx)], axis=-1)
        return d[..., 1] / np.sqrt((d * d).sum(axis=-1))
    small = (np.abs(cosine((xs - 0.5) / PW, (ys + 0.5) / PH)) < cos_min) | (np.abs(cosine((xs + 0.5) / PW, (ys - 0.5) / PH)) < cos_min)
    blending = ~r["masks"]["left_out"] & ~r["masks"]["background"] & ~r["masks"]["reset"]
    assert (blending & small).sum() > PW and (blending & ~small).sum() > PW
    assert np.array_equal(r["masks"]["gradient_reset"], blending & small)
