"""The CPU restatement of the variance-weighted reconstruction (tests/recon_weighted_ref.py) pinned by its defining properties, so
that the yardstick the GPU is compared against (tests/test_gpu_recon_weighted.py) is not arbitrary; and the C structs against their
ctypes mirrors."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import recon_l1_ref as R
import recon_weighted_ref as RW
from helpers import ROOT, rel_l2

ALPHA = 0.04


@pytest.mark.parametrize("K", [0, 5])
@pytest.mark.parametrize("w,h", [(33, 20), (64, 48)])
def test_uniform_variances_reproduce_the_unweighted_irls(w, h, K):
    """v = s in both families: kappa = 1 / (1 + delta) for every row, the system is the unweighted one times a constant."""
    _, u, gx, gy = R.synthetic(w, h, seed=1)
    one = np.ones_like(u)
    f, e, _, conf = RW.weighted(u, gx, gy, 0.37 * one, 0.011 * one, 0.011 * one, ALPHA, K)
    ref, e_ref, _ = R.irls(u, gx, gy, ALPHA, K)
    k0 = 1.0 / 1.05
    assert np.allclose(conf["kd"], k0, rtol=1e-14, atol=0) and np.allclose(conf["kx"][:, 1:], k0, rtol=1e-14, atol=0)
    assert np.allclose(conf["ky"][1:], k0, rtol=1e-14, atol=0) and (conf["kx"][:, 0] == 0).all() and (conf["ky"][0] == 0).all()
    assert abs(conf["scale_data"] - 3 * 0.37) < 1e-14 and abs(conf["scale_grad"] - 3 * 0.011) < 1e-15
    assert conf["rows_dropped"] == 0 and conf["pixels_isolated"] == 0
    assert rel_l2(f, ref) < 1e-10
    assert abs(e[-1] - k0 * e_ref[-1]) <= 1e-9 * e_ref[-1]


@pytest.mark.parametrize("w,h", [(17, 9), (64, 48)])
def test_round_zero_satisfies_the_weighted_normal_equations(w, h):
    """A built here from the definition, row by row, not by the restatement's own system()."""
    _, u, gx, gy, vc, vgx, vgy = RW.heteroscedastic(w, h, seed=1)
    delta = 0.05
    f, _, _, conf = RW.weighted(u, gx, gy, vc, vgx, vgy, ALPHA, 0, delta)
    vd, vx, vy = vc.sum(axis=2), vgx[:, 1:].sum(axis=2), vgy[1:].sum(axis=2)
    s_d = np.exp(np.log(vd).mean())
    s_g = np.exp(np.r_[np.log(vx).ravel(), np.log(vy).ravel()].mean())
    assert abs(conf["scale_data"] - s_d) <= 1e-13 * s_d and abs(conf["scale_grad"] - s_g) <= 1e-13 * s_g
    kd, kx, ky = s_d / (vd + delta * s_d), s_g / (vx + delta * s_g), s_g / (vy + delta * s_g)
    Dx, Dy = R.diff_ops(w, h)
    A = ALPHA * sp.diags(kd.ravel()) + Dx.T @ sp.diags(kx.ravel()) @ Dx + Dy.T @ sp.diags(ky.ravel()) @ Dy
    b = ALPHA * kd.reshape(-1, 1) * u.reshape(-1, 3) + Dx.T @ (kx.reshape(-1, 1) * gx[:, 1:].reshape(-1, 3)) + Dy.T @ (ky.reshape(-1, 1) * gy[1:].reshape(-1, 3))
    res = A @ f.reshape(-1, 3) - b
    assert np.linalg.norm(res) <= 1e-10 * np.linalg.norm(b)


def test_invalid_rows_leave_the_system_and_the_image_stays_finite():
    w, h = 33, 20
    _, u, gx, gy, vc, vgx, vgy = RW.heteroscedastic(w, h, seed=2)
    bad = RW.spoil(u, gx, gy, vc, vgx, vgy)
    for K in (0, 3):
        f, e, _, conf = RW.weighted(*bad, ALPHA, K)
        assert np.isfinite(f).all() and np.isfinite(e).all()
        # data rows (2,1)... : zero variance is valid; NaN u, inf variance are not. edges: NaN / negative variance, NaN / inf triples
        assert conf["rows_dropped"] == 2 + 4 + 3
        assert conf["pixels_isolated"] == 1 and (f[6, 9] == 0).all()
        assert abs(conf["kd"][1, 2] - 20.0) < 1e-13 and abs(conf["kx"][2, 3] - 20.0) < 1e-13        # v = 0: 1 / delta
        for plane, (y, x) in (("kd", (5, 4)), ("kd", (6, 9)), ("kx", (4, 5)), ("kx", (2, 6)), ("kx", (6, 9)), ("kx", (6, 10)), ("ky", (3, 1)), ("ky", (6, 9)), ("ky", (7, 9))):
            assert conf[plane][y, x] == 0, (plane, y, x)
        # what a dropped row holds does not matter
        other = [np.array(a, copy=True) for a in bad]
        other[1][2, 6] = 1e6
        other[4][2, 6, 0] = np.nan
        other[0][5, 4] = -7.0
        other[3][5, 4, 1] = np.nan
        g, _, _, _ = RW.weighted(*other, ALPHA, K)
        assert np.array_equal(f, g)
    # a family without a row of positive variance has scale 1
    z = np.zeros_like(u)
    conf = RW.confidences(u, gx, gy, z, z, z)
    assert conf["scale_data"] == 1.0 and conf["scale_grad"] == 1.0 and (conf["kd"] == 20.0).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_one_weighted_solve_beats_l1_and_l2_on_heteroscedastic_data(seed):
    w, h = 64, 48
    clean, u, gx, gy, vc, vgx, vgy = RW.heteroscedastic(w, h, seed)
    wl2 = RW.weighted(u, gx, gy, vc, vgx, vgy, ALPHA, 0)[0]
    _, _, iterates = R.irls(u, gx, gy, ALPHA, 10)
    e_w, e_l1, e_l2, e_p = rel_l2(wl2, clean), rel_l2(iterates[-1], clean), rel_l2(iterates[0], clean), rel_l2(u, clean)
    print(f"seed {seed}: primal {e_p:.4f}  L2 {e_l2:.4f}  L1 {e_l1:.4f}  weighted L2 {e_w:.4f}")
    assert e_w < e_l1 and e_w < 0.25 * e_l2


def test_weighted_struct_layouts_match_the_header(G, tmp_path):
    src = tmp_path / "sz.c"
    structs = ["GdptWeightedReconParams", "GdptWeightedReconStats", "GdptReconParams", "GdptReconStats"]
    body = "\n".join(f'printf("{s} %zu\\n", sizeof({s}));' for s in structs)
    body += 'printf("floor %zu\\nscale %zu\\n", offsetof(GdptWeightedReconParams, conf_floor), offsetof(GdptWeightedReconStats, scale_data));'
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/gdpt.h"\nint main(){{{body} return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for s in structs:
        assert int(got[s]) == C.sizeof(getattr(G, s)), s
    assert int(got["floor"]) == G.GdptWeightedReconParams.conf_floor.offset and int(got["scale"]) == G.GdptWeightedReconStats.scale_data.offset
    p = G.weighted_recon_params(G.RECON_L1, 0.1, irls_iters=7)
    assert (p.recon.norm, p.recon.irls_iters, p.conf_floor) == (G.RECON_L1, 7, 0.1)
    assert G.weighted_recon_params().recon.norm == G.RECON_L2


def test_weighted_entry_refuses_bad_arguments_and_fails_loudly_without_a_gpu(G):
    import torch
    z = np.zeros((4, 4, 3))
    for kw in (dict(conf_floor=-0.1), dict(conf_floor=float("nan")), dict(conf_floor=float("inf")), dict(dataCost=0.0), dict(dataCost=float("nan")),
               dict(norm=5), dict(eps_decay=1.5)):
        with pytest.raises(G.GdptError):
            G.reconstruct_weighted(4, 4, z, z, z, z, z, z, **kw)
    with pytest.raises(G.GdptError):
        G.reconstruct_weighted(4, 1, z[:1], z[:1], z[:1], z[:1], z[:1], z[:1])
    if not torch.cuda.is_available():
        with pytest.raises(G.GdptError):
            G.reconstruct_weighted(4, 4, z, z, z, z, z, z)
