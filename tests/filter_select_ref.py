"""numpy restatement of the per-pixel filter selection of include/gdpt.h (gdpt_filter_select*), on the helpers of tests/nlm_ref.py
(shifted, box): the two-half error estimate of every candidate, its box mean over the valid pixels of a (2s+1)^2 window, and the
lowest-index argmin. Not collected by pytest; tests/test_filter_select_ref.py pins it, tests/test_gpu_filter_select.py holds the
kernel against it.

    select(FA, FB, T, uA, vA, uB, vB, radius) -> dict(out, sel, mse, E (n, H, W), e (n, H, W), left_out, chosen, sum_e, sum_mse, sum_sq_out)
    brute_force(...)       the same pixel by pixel, candidate by candidate, tap by tap, for small films
    valid_mask(...)        HxW
    FA, FB, T: sequences of n HxWx3 arrays; uA, vA, uB, vB: HxWx3"""
import numpy as np

from nlm_ref import box

MAX_CANDIDATES = 8
MAX_RADIUS = 8
DEFAULT_RADIUS = 4


def valid_mask(FA, FB, T, uA, vA, uB, vB):
    """HxW: every triple finite, the two variances >= 0."""
    ok = np.ones(np.shape(uA)[:2], dtype=bool)
    for a in list(FA) + list(FB) + list(T) + [uA, vA, uB, vB]:
        ok &= np.isfinite(a).all(axis=2)
    with np.errstate(invalid="ignore"):
        return ok & (np.asarray(vA) >= 0).all(axis=2) & (np.asarray(vB) >= 0).all(axis=2)


def error_terms(FA, FB, uA, vA, uB, vB, ok):
    """(n, H, W): e_j in the operations of the header, 0.0 on the invalid pixels."""
    e = []
    with np.errstate(all="ignore"):
        for fa, fb in zip(FA, FB):
            dA, dB = fa - uB, fb - uA
            t = 0.5 * ((dA * dA - vB) + (dB * dB - vA))
            e.append(np.where(ok, ((t[..., 0] + t[..., 1]) + t[..., 2]) / 3.0, 0.0))
    return np.stack(e)


def select(FA, FB, T, uA, vA, uB, vB, radius=DEFAULT_RADIUS):
    f64 = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    FA, FB, T = [f64(a) for a in FA], [f64(a) for a in FB], [f64(a) for a in T]
    uA, vA, uB, vB = f64(uA), f64(vA), f64(uB), f64(vB)
    n = len(T)
    ok = valid_mask(FA, FB, T, uA, vA, uB, vB)
    e = error_terms(FA, FB, uA, vA, uB, vB, ok)
    C = np.maximum(box(ok.astype(np.int64), radius), 1)
    E = np.stack([np.where(ok, box(e[j], radius) / C, np.nan) for j in range(n)])
    best, best_e = np.zeros(ok.shape, dtype=np.int32), E[0].copy()
    for j in range(1, n):
        with np.errstate(invalid="ignore"):
            less = E[j] < best_e
        best, best_e = np.where(less, j, best), np.where(less, E[j], best_e)
    sel = np.where(ok, best, -1).astype(np.int32)
    out = T[0].copy()
    for j in range(1, n):
        out[sel == j] = T[j][sel == j]
    d = dict(out=out, sel=sel, mse=np.where(ok, best_e, np.nan), E=E, e=e, left_out=int((~ok).sum()))
    d["chosen"] = [int((sel == j).sum()) for j in range(n)]
    d["sum_e"] = [float(e[j][ok].sum()) for j in range(n)]
    d["sum_mse"] = float(best_e[ok].sum())
    d["sum_sq_out"] = float((out * out)[ok].sum())
    return d


def brute_force(FA, FB, T, uA, vA, uB, vB, radius=DEFAULT_RADIUS):
    """The definition read literally, pixel by pixel: validity per pixel, the window tap by tap in row-major order (not separable:
    the last places of E may differ from select())."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    FA, FB, T = [f64(a) for a in FA], [f64(a) for a in FB], [f64(a) for a in T]
    uA, vA, uB, vB = f64(uA), f64(vA), f64(uB), f64(vB)
    n = len(T)
    h, w = uA.shape[:2]
    fin = lambda x: bool(np.isfinite(x))      # noqa: E731
    ok = np.zeros((h, w), dtype=bool)
    e = np.zeros((n, h, w))
    for y in range(h):
        for x in range(w):
            good = all(fin(a[y, x, c]) for a in FA + FB + T + [uA, vA, uB, vB] for c in range(3))
            good = good and all(v[y, x, c] >= 0 for v in (vA, vB) for c in range(3))
            ok[y, x] = good
            if not good:
                continue
            for j in range(n):
                dA, dB = FA[j][y, x] - uB[y, x], FB[j][y, x] - uA[y, x]
                t = [0.5 * ((dA[c] * dA[c] - vB[y, x, c]) + (dB[c] * dB[c] - vA[y, x, c])) for c in range(3)]
                e[j, y, x] = ((t[0] + t[1]) + t[2]) / 3.0
    out, sel = T[0].copy(), np.full((h, w), -1, dtype=np.int32)
    mse, E = np.full((h, w), np.nan), np.full((n, h, w), np.nan)
    for y in range(h):
        for x in range(w):
            if not ok[y, x]:
                continue
            for j in range(n):
                S, C = 0.0, 0
                for qy in range(max(0, y - radius), min(h, y + radius + 1)):
                    for qx in range(max(0, x - radius), min(w, x + radius + 1)):
                        if ok[qy, qx]:
                            S += e[j, qy, qx]
                            C += 1
                E[j, y, x] = S / C
                if j == 0 or E[j, y, x] < mse[y, x]:
                    mse[y, x], sel[y, x] = E[j, y, x], j
            out[y, x] = T[sel[y, x]][y, x]
    d = dict(out=out, sel=sel, mse=mse, E=E, e=e, left_out=int((~ok).sum()))
    d["chosen"] = [int((sel == j).sum()) for j in range(n)]
    d["sum_e"] = [float(e[j][ok].sum()) for j in range(n)]
    d["sum_mse"] = float(mse[ok].sum())
    d["sum_sq_out"] = float((out * out)[ok].sum())
    return d


def fields(w, h, n, seed, noise=0.05):
    """Test inputs: continuous noise around a few smooth "filtered" fields. The truth is a smooth film; half means are truth plus
    noise of a variance that varies over the film; candidate j is a blend of the half mean and a smooth field whose bias grows
    towards another corner per candidate, so that the best candidate changes over the film. Returns (FA, FB, T, uA, vA, uB, vB)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    fx, fy = x / max(1, w - 1), y / max(1, h - 1)
    truth = np.stack([0.6 + 0.3 * np.sin(3.0 * fx + c) * np.cos(2.0 * fy - c) for c in range(3)], axis=2)
    sigma = noise * (0.5 + fx + 0.5 * fy)[..., None] * np.ones(3)
    uA, uB = truth + sigma * rng.standard_normal(truth.shape), truth + sigma * rng.standard_normal(truth.shape)
    vA = sigma ** 2 * (0.7 + 0.6 * rng.random(truth.shape))
    vB = sigma ** 2 * (0.7 + 0.6 * rng.random(truth.shape))
    FA, FB, T = [], [], []
    for j in range(n):
        keep = j / max(1, n)                                 # the share of the noisy mean the candidate keeps
        ang = 2.0 * np.pi * j / max(1, n)
        bias = 0.06 * (0.5 + 0.5 * (np.cos(ang) * (2 * fx - 1) + np.sin(ang) * (2 * fy - 1)))[..., None] * np.array([1.0, -0.5, 0.7])
        jit = lambda: 0.003 * rng.standard_normal(truth.shape)      # noqa: E731
        FA.append(keep * uA + (1 - keep) * (truth + bias) + jit())
        FB.append(keep * uB + (1 - keep) * (truth + bias) + jit())
        T.append(keep * 0.5 * (uA + uB) + (1 - keep) * (truth + bias) + jit())
    return FA, FB, T, uA, vA, uB, vB


KINDS = ("uA", "vA", "uB", "vB", "FA", "FB", "T")


def plant(inputs, kind, seed, count=3):
    """A copy of fields()'s tuple with non-finite values (and, in a variance, a negative one) in `count` pixels of one kind of input;
    for FA, FB, T in the last candidate."""
    FA, FB, T, uA, vA, uB, vB = inputs
    FA, FB, T = [a.copy() for a in FA], [a.copy() for a in FB], [a.copy() for a in T]
    uA, vA, uB, vB = uA.copy(), vA.copy(), uB.copy(), vB.copy()
    target = dict(uA=uA, vA=vA, uB=uB, vB=vB, FA=FA[-1], FB=FB[-1], T=T[-1])[kind]
    h, w = uA.shape[:2]
    rng = np.random.default_rng(seed)
    values = [np.nan, np.inf, -1e-3 if kind in ("vA", "vB") else -np.inf]
    for i in range(count):
        target[int(rng.integers(h)), int(rng.integers(w)), int(rng.integers(3))] = values[i % 3]
    return FA, FB, T, uA, vA, uB, vB
