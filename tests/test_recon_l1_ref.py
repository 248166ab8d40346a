"""The CPU restatement of the L1 reconstruction (tests/recon_l1_ref.py) pinned by its defining properties, so that the yardstick
the GPU is compared against (tests/test_gpu_recon_l1.py) is not arbitrary; and the C structs against their ctypes mirrors."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import recon_l1_ref as R
from helpers import ROOT, rel_l2

ALPHA = 0.04
EXTENTS = [(64, 48), (33, 20), (128, 96)]


@pytest.mark.parametrize("w,h", EXTENTS + [(2, 2), (17, 9)])
def test_round_zero_is_the_unweighted_least_squares_solution(w, h):
    _, u, gx, gy = R.synthetic(w, h, seed=1)
    f, _, _ = R.irls(u, gx, gy, ALPHA, 0)
    Dx, Dy = R.diff_ops(w, h)
    A = ALPHA * sp.identity(w * h) + Dx.T @ Dx + Dy.T @ Dy
    b = ALPHA * u.reshape(-1, 3) + Dx.T @ gx[:, 1:].reshape(-1, 3) + Dy.T @ gy[1:].reshape(-1, 3)
    ref = np.stack([spla.spsolve(A.tocsc(), b[:, c]) for c in range(3)], axis=1).reshape(h, w, 3)
    assert rel_l2(f, ref) < 1e-12
    # the first column of gx and the first row of gy are not read
    gx2, gy2 = gx.copy(), gy.copy()
    gx2[:, 0] = 1e6
    gy2[0] = -1e6
    assert np.array_equal(R.irls(u, gx2, gy2, ALPHA, 2)[0], R.irls(u, gx, gy, ALPHA, 2)[0])


@pytest.mark.parametrize("w,h", EXTENTS)
def test_energy_never_rises_and_halves_within_ten_rounds(w, h):
    _, u, gx, gy = R.synthetic(w, h, seed=1)
    _, e, _ = R.irls(u, gx, gy, ALPHA, 10)
    assert len(e) == 11
    for a, b in zip(e, e[1:]):
        assert b <= a * (1 + 1e-12), e
    assert e[10] < 0.5 * e[0], e


@pytest.mark.parametrize("w,h", EXTENTS)
def test_consistent_inputs_are_a_fixed_point(w, h):
    clean = R.clean_image(w, h)
    gx, gy = R.exact_gradients(clean)
    _, e, iterates = R.irls(clean, gx, gy, ALPHA, 5)
    for f in iterates:
        assert rel_l2(f, clean) < 1e-12
    assert max(e) < 1e-9


@pytest.mark.parametrize("w,h", EXTENTS)
def test_l1_is_robust_to_gradient_outliers_where_l2_is_not(w, h):
    clean, u, gx, gy = R.synthetic(w, h, seed=1)
    _, _, iterates = R.irls(u, gx, gy, ALPHA, 20)
    e_l1, e_l2, e_primal = rel_l2(iterates[-1], clean), rel_l2(iterates[0], clean), rel_l2(u, clean)
    print(f"{w}x{h}: L1 {e_l1:.3f} primal {e_primal:.3f} L2 {e_l2:.3f}")
    assert e_l1 < e_primal and e_l1 < 0.25 * e_l2


def test_recon_struct_layouts_match_the_header(G, tmp_path):
    src = tmp_path / "sz.c"
    structs = ["GdptReconParams", "GdptReconStats"]
    body = "\n".join(f'printf("{s} %zu\\n", sizeof({s}));' for s in structs)
    body += 'printf("L2 %d\\nL1 %d\\n", (int)GDPT_RECON_L2, (int)GDPT_RECON_L1);'
    src.write_text(f'#include <stdio.h>\n#include "{ROOT}/include/gdpt.h"\nint main(){{{body} return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for s in structs:
        assert int(got[s]) == C.sizeof(getattr(G, s)), s
    assert (int(got["L2"]), int(got["L1"])) == (G.RECON_L2, G.RECON_L1)
    # the mirror's parameter helper: None = the library's default count, 0 = no reweighted round (a negative count in C)
    assert G.recon_params().irls_iters == 0 and G.recon_params(irls_iters=0).irls_iters < 0 and G.recon_params(irls_iters=7).irls_iters == 7


def test_reconstruct_fails_loudly_without_a_gpu_and_refuses_bad_arguments(G):
    import torch
    z = np.zeros((4, 4, 3))
    for kw in (dict(eps_decay=1.5), dict(eps_decay=-0.1), dict(eps_init=float("nan")), dict(cg_tol=float("nan")), dict(eps_floor=-1.0)):
        with pytest.raises(G.GdptError):
            G.reconstruct(4, 4, z, z, z, 0.04, **kw)
    with pytest.raises(G.GdptError):
        G.reconstruct(4, 1, z[:1], z[:1], z[:1], 0.04)
    with pytest.raises(G.GdptError):
        G.reconstruct(4, 4, z, z, z, 0.04, norm=7)
    if not torch.cuda.is_available():
        for norm in (G.RECON_L1, G.RECON_L2):
            with pytest.raises(G.GdptError):
                G.reconstruct(4, 4, z, z, z, 0.04, norm=norm)
