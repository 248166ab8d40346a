"""numpy restatement of the merge of two progressive sessions (csrc/hip/progressive.hip: merge_kernel; include/gdpt.h:
gdpt_progressive_merge), on the Fold of tests/progressive_ref.py. The pairwise update of Chan, Golub and LeVeque (1979), per
component, written from the formula in the order the kernel evaluates it:
    W = Wa + Wb;  d = mean_b - mean_a;  mean = mean_a + (Wb / W) d;  M2 = (M2a + M2b) + (d d) (Wa Wb / W);  K = Ka + Kb
so the only differences to the GPU are FMA contractions (and the order of the two film-wide sums of the error estimate, which
Fold.error_estimate takes)."""
import numpy as np

from progressive_ref import Fold


def state(means, m2, W, K):
    """A Fold holding the given planes (dicts name -> array): e.g. a session's state read back from the GPU."""
    f = Fold()
    f.W, f.K = float(W), int(K)
    f.mean = {k: np.array(v, dtype=np.float64) for k, v in means.items()}
    f.M2 = {k: np.array(v, dtype=np.float64) for k, v in m2.items()}
    return f


def merge(dst, src):
    """`dst` takes in `src` (Folds); `src` is unchanged; returns `dst`. Into a dst that holds nothing, src's planes are copied; a src
    that holds nothing is a no-op."""
    if src.K == 0:
        return dst
    if dst.K == 0:
        dst.W, dst.K = src.W, src.K
        dst.mean = {k: v.copy() for k, v in src.mean.items()}
        dst.M2 = {k: v.copy() for k, v in src.M2.items()}
        return dst
    assert sorted(dst.mean) == sorted(src.mean)
    wa, wb = dst.W, src.W
    w = wa + wb
    f, g = wb / w, wa * wb / w
    with np.errstate(invalid="ignore", over="ignore"):
        for k in dst.mean:
            d = src.mean[k] - dst.mean[k]
            dst.M2[k] = (dst.M2[k] + src.M2[k]) + (d * d) * g
            dst.mean[k] = dst.mean[k] + f * d
    dst.W, dst.K = w, dst.K + src.K
    return dst


def merged(folds):
    """The merge of `folds`, in order, into an empty accumulator."""
    acc = Fold()
    for f in folds:
        merge(acc, f)
    return acc
