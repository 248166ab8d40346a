"""The small-footprint shape of dct_fold_gemm_f64 (32 x 32 tile, K step 16, 256 threads, one LDS buffer: the shape a solve takes while
a render kernel is resident beside it, csrc/hip/poisson_kernels.hip) against each of the three shapes the solver had: every output
element is accumulated by the same MFMA sequence with k ascending in all of them, so the result must not depend on the shape by a
single bit — a shape choice that depends on what is in flight must not change the image. Films: 37x21 (inside one tile, odd: the
self-paired middle sample, the scalar staging path), 64x64, 130x66 and 65x129 (across the 32- and 64-row tile edges, ragged tiles,
odd and even extents). Against the CPU solve: the tolerance of tests/test_gpu_poisson_and_pipeline.py."""
import numpy as np
import pytest

from helpers import rel_l2
from test_poisson_oracle import lcg_fields

pytestmark = pytest.mark.gpu

SMALL = ({"dct_bm": 32, "dct_bk": 16}, "32x32x16")
PRESENT = [({"dct_bm": 32}, "32x64x32"), ({"dct_bm": 64, "dct_bk": 32}, "64x64x32"), ({"dct_bm": 64, "dct_bk": 16}, "64x64x16")]


def solve(G, w, h, fields, knobs, shape):
    with G.debug_knobs(**knobs):
        out = G.fourierSolve(w, h, *fields, 0.04, solver=G.SOLVER_DCT_MFMA)
        assert G.debug_knobs.last_dct_shape() == shape, (knobs, G.debug_knobs.last_dct_shape())
    return out


@pytest.mark.parametrize("w,h", [(37, 21), (64, 64), (130, 66), (65, 129)])
def test_small_shape_bit_equal_to_every_present_shape(G, O, w, h):
    fields = lcg_fields(w, h, seed=w * 1000 + h)
    small = solve(G, w, h, fields, *SMALL)
    assert np.isfinite(small).all() and np.any(small)
    err = rel_l2(small, O.fourier_solve(*fields, 0.04))
    print(f"{w}x{h}: small-footprint shape against the CPU solve, rel L2 {err:.3e}")
    assert err < 1e-11
    for knobs, shape in PRESENT:
        other = solve(G, w, h, fields, knobs, shape)
        assert np.array_equal(small, other), f"{w}x{h}: {shape} differs from the small-footprint shape in {np.count_nonzero(small != other)} values"

