"""CPU restatement of the variance-weighted reconstruction (include/gdpt.h, gdpt_reconstruct_weighted): per-row confidences from
variance planes, then recon_l1_ref's IRLS with a direct sparse inner solve and the confidences multiplied into the row weights;
and the heteroscedastic synthetic input its tests use. Not collected by pytest. Shapes: H x W x 3 float64."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from recon_l1_ref import clean_image, diff_ops, exact_gradients


def row_variances(u, gx, gy, vc, vgx, vgy):
    """(v_d, v_x, v_y), H x W each: the sum of a row's three channel variances; -1 where the row is invalid (a variance that is
    not finite or negative, a sum that is not finite, a non-finite c / gx / gy triple) or the film has no such row (x = 0, y = 0)."""
    def rows(val, var):
        with np.errstate(invalid="ignore", over="ignore"):
            v = (var[..., 0] + var[..., 1]) + var[..., 2]
            ok = np.isfinite(val).all(axis=2) & (var >= 0).all(axis=2) & np.isfinite(v)
        return np.where(ok, v, -1.0)
    vd, vx, vy = rows(u, vc), rows(gx, vgx), rows(gy, vgy)
    vx[:, 0] = -1.0
    vy[0] = -1.0
    return vd, vx, vy


def geometric_mean(v):
    pos = v[v > 0]
    return float(np.exp(np.mean(np.log(pos)))) if pos.size else 1.0


def confidences(u, gx, gy, vc, vgx, vgy, delta=0.05):
    """dict: kd, kx, ky (H x W; 0 for invalid and absent rows), scale_data, scale_grad, rows_dropped, pixels_isolated."""
    vd, vx, vy = row_variances(u, gx, gy, vc, vgx, vgy)
    s_d, s_g = geometric_mean(vd), geometric_mean(np.r_[vx.ravel(), vy.ravel()])

    def kappa(v, s):
        return np.where(v < 0, 0.0, s / (np.where(v < 0, 1.0, v) + delta * s))
    kd, kx, ky = kappa(vd, s_d), kappa(vx, s_g), kappa(vy, s_g)
    touch = kd.copy()                              # sum of the confidences of every row a pixel takes part in
    touch += kx + ky
    touch[:, :-1] += kx[:, 1:]
    touch[:-1] += ky[1:]
    return dict(kd=kd, kx=kx, ky=ky, scale_data=s_d, scale_grad=s_g,
                rows_dropped=int((vd < 0).sum() + (vx[:, 1:] < 0).sum() + (vy[1:] < 0).sum()), pixels_isolated=int((touch == 0).sum()))


def system(u, gx, gy, conf, alpha, wd=None, wx=None, wy=None):
    """(A, b, parts) of one round: row weights kappa * w (w = None: 1). Rows with kappa = 0 are taken out (their values are
    replaced by 0 before anything is multiplied); an isolated pixel gets diagonal 1."""
    h, w, _ = u.shape
    n = w * h
    Dx, Dy = diff_ops(w, h)
    kd, kx, ky = conf["kd"].reshape(n), conf["kx"][:, 1:].reshape(-1), conf["ky"][1:].reshape(-1)
    U = np.where(kd[:, None] > 0, u.reshape(n, 3), 0.0)
    bx = np.where(kx[:, None] > 0, gx[:, 1:].reshape(-1, 3), 0.0)
    by = np.where(ky[:, None] > 0, gy[1:].reshape(-1, 3), 0.0)
    od = kd * (1.0 if wd is None else wd)
    ox = kx * (1.0 if wx is None else wx)
    oy = ky * (1.0 if wy is None else wy)
    A = (alpha * sp.diags(od) + Dx.T @ sp.diags(ox) @ Dx + Dy.T @ sp.diags(oy) @ Dy).tocsr()
    A = A + sp.diags((A.diagonal() == 0).astype(np.float64))
    b = alpha * od[:, None] * U + Dx.T @ (ox[:, None] * bx) + Dy.T @ (oy[:, None] * by)
    return A, b, (Dx, Dy, U, bx, by, kd, kx, ky)


def weighted(u, gx, gy, vc, vgx, vgy, alpha, K, delta=0.05, eps_init=0.05, eps_decay=0.5, eps_floor=1e-3):
    """Returns (f_K, energies, iterates, conf): round 0 = weighted least squares; energies[k] = sum of kappa |r|_2 at f_k."""
    h, w, _ = u.shape
    conf = confidences(u, gx, gy, vc, vgx, vgy, delta)
    A, b, (Dx, Dy, U, bx, by, kd, kx, ky) = system(u, gx, gy, conf, alpha)

    def row_norms(f):
        rd = np.where(kd[:, None] > 0, np.sqrt(alpha) * (f - U), 0.0)
        rx = np.where(kx[:, None] > 0, Dx @ f - bx, 0.0)
        ry = np.where(ky[:, None] > 0, Dy @ f - by, 0.0)
        return [np.linalg.norm(r, axis=1) for r in (rd, rx, ry)]
    energies, iterates = [], []
    for k in range(K + 1):
        if k > 0:
            eps = max(eps_init * eps_decay ** (k - 1), eps_floor)
            A, b, _ = system(u, gx, gy, conf, alpha, *[1.0 / (eps + r) for r in row_norms(f)])
        f = spla.splu(A.tocsc()).solve(b)
        energies.append(float(sum((kap * r).sum() for kap, r in zip((kd, kx, ky), row_norms(f)))))
        iterates.append(f.reshape(h, w, 3).copy())
    return iterates[-1], energies, iterates, conf


def heteroscedastic(w, h, seed, passes=16, outliers=True):
    """(clean, u, gx, gy, vc, vgx, vgy): means and variances of the mean (var(ddof=1) / passes, channel-wise) of `passes` passes of
    clean + 0.3 m N(0,1) and gradient + 0.03 m N(0,1), noise level m = 0.25 or 2.5 per 16x16 block as a checkerboard; each gradient
    pass-sample is hit with probability 0.0025 by 20 N(0,1), added to all three channels."""
    clean = clean_image(w, h)
    ex, ey = exact_gradients(clean)
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    m = np.where(((x // 16) + (y // 16)) % 2 == 0, 0.25, 2.5)[None, :, :, None]
    rng = np.random.default_rng(seed)
    shape = (passes,) + clean.shape
    pu = clean[None] + 0.3 * m * rng.standard_normal(shape)
    px = ex[None] + 0.03 * m * rng.standard_normal(shape)
    py = ey[None] + 0.03 * m * rng.standard_normal(shape)
    hx, hy = rng.random(shape[:3]) < 0.0025, rng.random(shape[:3]) < 0.0025
    ox, oy = 20.0 * rng.standard_normal(shape[:3]), 20.0 * rng.standard_normal(shape[:3])
    if outliers:
        px += (hx * ox)[..., None]
        py += (hy * oy)[..., None]
    stats = [(p.mean(axis=0), p.var(axis=0, ddof=1) / passes) for p in (pu, px, py)]
    return (clean,) + tuple(s[0] for s in stats) + tuple(s[1] for s in stats)


def spoil(u, gx, gy, vc, vgx, vgy):
    """Copies of the inputs with every kind of row the definition names: zero variances (a data row and an edge row), a NaN
    variance, a negative variance, a NaN gradient triple, a NaN primal, and one pixel all of whose rows are invalid. Needs a
    film of at least 12 x 8."""
    u, gx, gy, vc, vgx, vgy = [np.array(a, copy=True) for a in (u, gx, gy, vc, vgx, vgy)]
    vc[1, 2] = 0.0
    vgx[2, 3] = 0.0
    vgy[3, 1, 1] = np.nan
    vgx[4, 5, 0] = -1e-3
    gx[2, 6, 2] = np.nan
    u[5, 4, 0] = np.nan
    vc[6, 9] = np.inf                  # pixel (x = 9, y = 6): data row and its four edge rows
    vgx[6, 9, 1] = np.nan
    gx[6, 10] = np.nan
    gy[6, 9, 0] = np.inf
    vgy[7, 9, 2] = np.nan
    return u, gx, gy, vc, vgx, vgy
