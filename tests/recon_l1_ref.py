"""CPU restatement of the L1 reconstruction (include/gdpt.h, gdpt_reconstruct): IRLS with a direct sparse inner solve, and the
synthetic inputs its tests use. Not collected by pytest. Shapes: H x W x 3 float64."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def diff_ops(w, h):
    """Dx, Dy on the row-major flattened film: one row per edge inside the film, f(x,y) - f(x-1,y) and f(x,y) - f(x,y-1)."""
    idx = np.arange(w * h).reshape(h, w)

    def D(a, b):
        n = a.size
        rows = np.r_[np.arange(n), np.arange(n)]
        return sp.csr_matrix((np.r_[np.ones(n), -np.ones(n)], (rows, np.r_[a.ravel(), b.ravel()])), shape=(n, w * h))
    return D(idx[:, 1:], idx[:, :-1]), D(idx[1:, :], idx[:-1, :])


def irls(u, gx, gy, alpha, K, eps_init=0.05, eps_decay=0.5, eps_floor=1e-3):
    """Returns (f_K, energies, iterates): energies[k] = E(f_k) = sum over rows of |r|_2, iterates[k] = f_k, k = 0..K."""
    h, w, _ = u.shape
    n = w * h
    Dx, Dy = diff_ops(w, h)
    U, bx, by = u.reshape(n, 3), gx[:, 1:].reshape(-1, 3), gy[1:].reshape(-1, 3)     # gx(0,.) and gy(.,0) are not used

    def row_norms(f):
        return [np.linalg.norm(r, axis=1) for r in (np.sqrt(alpha) * (f - U), Dx @ f - bx, Dy @ f - by)]
    f, energies, iterates = U.copy(), [], []
    for k in range(K + 1):
        if k == 0:
            wd, wx, wy = np.ones(n), np.ones(Dx.shape[0]), np.ones(Dy.shape[0])
        else:
            eps = max(eps_init * eps_decay ** (k - 1), eps_floor)
            wd, wx, wy = [1.0 / (eps + r) for r in row_norms(f)]
        A = alpha * sp.diags(wd) + Dx.T @ sp.diags(wx) @ Dx + Dy.T @ sp.diags(wy) @ Dy
        b = alpha * wd[:, None] * U + Dx.T @ (wx[:, None] * bx) + Dy.T @ (wy[:, None] * by)
        f = spla.splu(A.tocsc()).solve(b)
        energies.append(float(sum(r.sum() for r in row_norms(f))))
        iterates.append(f.reshape(h, w, 3).copy())
    return iterates[-1], energies, iterates


def clean_image(w, h):
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    base = 0.5 + 0.4 * np.sin(x / 7.0) * np.cos(y / 5.0)
    return np.stack([base, 0.8 * base + 0.1, base * np.where(x > w // 2, 1.0, 0.2)], axis=2)


def exact_gradients(img):
    gx, gy = np.zeros_like(img), np.zeros_like(img)
    gx[:, 1:] = img[:, 1:] - img[:, :-1]
    gy[1:] = img[1:] - img[:-1]
    return gx, gy


def synthetic(w, h, seed):
    """(clean, u, gx, gy): smooth image with a step; primal noise 0.3, gradient noise 0.03, 1 % of the gradient samples hit by
    outliers of sigma 20 (one draw per hit pixel, added to all three channels)."""
    clean = clean_image(w, h)
    gx, gy = exact_gradients(clean)
    rng = np.random.default_rng(seed)
    u = clean + 0.3 * rng.standard_normal(clean.shape)
    gx += 0.03 * rng.standard_normal(clean.shape)
    gy += 0.03 * rng.standard_normal(clean.shape)
    mx, my = rng.random((h, w)) < 0.01, rng.random((h, w)) < 0.01
    gx[mx] += 20.0 * rng.standard_normal(int(mx.sum()))[:, None]
    gy[my] += 20.0 * rng.standard_normal(int(my.sum()))[:, None]
    return clean, u, gx, gy
