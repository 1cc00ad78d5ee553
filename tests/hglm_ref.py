"""The hierarchical GLM target of include/mivi.h (mivi_set_target_hglm) restated in numpy: float64, or every array and sum in `dtype` (the
same-precision restatement the GPU tests measure rounding against).  The oracle targets' interface; pinned to torch.autograd in
tests/test_gpu_hglm.py."""
import math

import numpy as np

LOG2PI = float(np.log(2.0 * np.pi))


class HierGLMRef:
    def __init__(self, X, y, groups, J, likelihood="bernoulli", offset=None, prior_std=1.0, tau_scale=1.0, likeadj=1.0, dtype=np.float64):
        as_t = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)   # noqa: E731
        self.X, self.y, self.groups, self.J = as_t(X), as_t(y), np.asarray(groups, dtype=np.int64), int(J)
        self.offset = as_t(np.zeros(len(self.y)) if offset is None else offset)
        self.likelihood, self.prior_std, self.tau_scale, self.likeadj, self.dtype = likelihood, prior_std, tau_scale, likeadj, np.dtype(dtype).type
        self.lgam = sum(math.lgamma(v + 1.0) for v in self.y.astype(np.float64)) if likelihood == "poisson" else 0.0

    def dimension(self):
        return self.X.shape[1] + self.J + 1

    def logdensity_and_gradient(self, z):
        T, p, J = self.dtype, self.X.shape[1], self.J
        z = np.asarray(z, dtype=np.float64).astype(T)
        beta, u, s = z[:p], z[p:p + J], z[p + J]
        eta = self.X @ beta + u[self.groups] + self.offset
        if self.likelihood == "bernoulli":
            e = np.exp(-np.abs(eta))
            ll = (self.y * eta - (np.maximum(eta, T(0)) + np.log1p(e))).sum(dtype=T)
            res = self.y - np.where(eta >= 0, T(1), e) / (T(1) + e)
        else:
            e = np.exp(eta)
            ll = (self.y * eta - e).sum(dtype=T) - T(self.lgam)
            res = self.y - e
        ip2, it2, e2, em2 = T(1.0 / self.prior_std ** 2), T(1.0 / self.tau_scale ** 2), np.exp(T(2) * s), np.exp(T(-2) * s)
        gsum = np.zeros(J, dtype=T)
        np.add.at(gsum, self.groups, res)
        g = np.empty(p + J + 1, dtype=T)
        g[:p] = T(self.likeadj) * (self.X.T @ res) - beta * ip2
        g[p:p + J] = T(self.likeadj) * gsum - u * em2
        uu = (u * u).sum(dtype=T)
        g[p + J] = T(-J) + uu * em2 - e2 * it2 + T(1)
        lp = (T(-0.5) * (beta * beta).sum(dtype=T) * ip2 - T(p * (np.log(self.prior_std) + 0.5 * LOG2PI))
              - T(0.5) * uu * em2 - T(J) * (s + T(0.5 * LOG2PI))
              + T(np.log(2.0) - 0.5 * LOG2PI - np.log(self.tau_scale)) - T(0.5) * e2 * it2 + s)
        return float(T(self.likeadj) * ll + lp), g.astype(np.float64)

    def logdensity(self, z):
        return self.logdensity_and_gradient(z)[0]
