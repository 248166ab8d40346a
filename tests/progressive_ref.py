"""numpy restatement of the progressive session's arithmetic (csrc/hip/progressive.hip, include/gdpt.h: gdpt_progressive_*):
the fold of passes into running means and sums of weighted squared deviations, the variance read-out, the variances of
the assembled c / cx / cy and the error estimate. Written from the definitions, element-wise, in the order the kernel
evaluates them, so the only differences to the GPU are FMA contractions (and the order of the two film-wide sums)."""
import numpy as np

BUFS = ("img", "cx0", "cy0", "cx1", "cy1")


class Fold:
    """West's weighted update (1979), per component: W += n; d = m - mean; mean += (n/W) d; M2 += n d (m - mean_new)."""

    def __init__(self):
        self.W = 0.0         # samples so far
        self.K = 0           # passes so far
        self.mean = None     # dict name -> array
        self.M2 = None

    def add(self, passes, n):
        """`passes`: dict name -> array (the pass's means over its n samples)."""
        n = float(n)
        if self.mean is None:
            self.mean = {k: np.zeros_like(np.asarray(v, dtype=np.float64)) for k, v in passes.items()}
            self.M2 = {k: np.zeros_like(self.mean[k]) for k in passes}
        self.W += n
        self.K += 1
        f = n / self.W
        with np.errstate(invalid="ignore", over="ignore"):
            for k, m in passes.items():
                m = np.asarray(m, dtype=np.float64)
                d = m - self.mean[k]
                new = self.mean[k] + f * d
                self.M2[k] = self.M2[k] + n * d * (m - new)
                self.mean[k] = new
        return self

    def norm(self):
        return float(self.K - 1) * self.W

    def var_mean(self):
        """Variance of the running mean per buffer: M2 / ((K-1) W); defined from K >= 2."""
        assert self.K >= 2
        with np.errstate(invalid="ignore"):
            return {k: v / self.norm() for k, v in self.M2.items()}

    def assembled_var(self):
        """Variances of c = img, cx = cx0(x,y) + cx1(x-1,y), cy = cy0(x,y) + cy1(x,y-1): the two terms come from different
        pixels' streams and are independent, so their variances add; the second term is absent at x = 0 / y = 0."""
        v = self.var_mean()
        vcx = v["cx0"].copy()
        vcx[:, 1:] = v["cx0"][:, 1:] + v["cx1"][:, :-1]
        vcy = v["cy0"].copy()
        vcy[1:, :] = v["cy0"][1:, :] + v["cy1"][:-1, :]
        return {"c": v["img"], "cx": vcx, "cy": vcy}

    def error_estimate(self):
        """(sqrt(sum var_mean(img) / sum mean(img)^2), pixels left out): over pixels and channels; a pixel whose img mean or
        M2 has a non-finite channel is left out of both sums and counted. NaN before the second pass."""
        if self.K < 2:
            return float("nan"), 0
        mean, m2 = self.mean["img"], self.M2["img"]
        ok = np.isfinite(mean).all(axis=-1) & np.isfinite(m2).all(axis=-1)
        var = m2[ok] / self.norm()
        return float(np.sqrt(var.sum() / (mean[ok] ** 2).sum())), int(ok.size - ok.sum())


def fold(pass_list, sizes):
    """Fold of `pass_list` (dicts, or bare arrays taken as the img plane) with `sizes` samples each."""
    f = Fold()
    for p, n in zip(pass_list, sizes):
        f.add(p if isinstance(p, dict) else {"img": p}, n)
    return f
