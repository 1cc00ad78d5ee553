"""The softmax regression target of include/mivi.h (mivi_set_target_softmax) restated in numpy: float64, or every array and sum in `dtype`
(the same-precision restatement the GPU tests measure rounding against).  The oracle targets' interface; pinned to torch.autograd in tests/test_gpu_softmax.py."""
import numpy as np

LOG2PI = float(np.log(2.0 * np.pi))


class SoftmaxRef:
    def __init__(self, X, y, n_classes, variant="logsigma_normal", likeadj=1.0, dtype=np.float64):
        self.X, self.y, self.C = np.asarray(X, dtype=np.float64).astype(dtype), np.asarray(y, dtype=np.int64), int(n_classes)
        self.variant, self.likeadj, self.dtype = variant, float(likeadj), np.dtype(dtype).type

    def dimension(self):
        return self.X.shape[1] * self.C + 1

    def logdensity_and_gradient(self, z):
        T, (n, p), C = self.dtype, self.X.shape, self.C
        z = np.asarray(z, dtype=np.float64).astype(T)
        B, s, rows = z[:p * C].reshape(p, C, order="F"), z[p * C], np.arange(n)
        L = self.X @ B
        mx = L.max(axis=1, keepdims=True)
        E = np.exp(L - mx)
        se = E.sum(axis=1, keepdims=True, dtype=T)
        loglike = (L[rows, self.y] - mx[:, 0] - np.log(se[:, 0])).sum(dtype=T)
        R = -E / se
        R[rows, self.y] += T(1)
        is2, bb, npc = np.exp(T(-2) * s), (B * B).sum(dtype=T), T(p * C)
        g = np.empty(p * C + 1, dtype=T)
        g[:p * C] = (T(self.likeadj) * (self.X.T @ R) - B * is2).reshape(-1, order="F")
        lp, gs = T(-0.5 * LOG2PI) * npc - npc * s - T(0.5) * bb * is2, -npc + bb * is2
        if self.variant == "logsigma_normal":
            s2 = np.exp(T(2) * s)
            lp, gs = lp + T(-0.5 * np.log(2.0 * np.pi * 9.0)) - s2 / T(18), gs - s2 / T(9)
        else:   # "lognormal_exp_bijector"
            lp, gs = lp - s - T(np.log(3.0) + 0.5 * LOG2PI) - s * s / T(18) + s, gs - T(1) - s / T(9) + T(1)
        g[p * C] = gs
        return float(T(self.likeadj) * loglike + lp), g.astype(np.float64)

    def logdensity(self, z):
        return self.logdensity_and_gradient(z)[0]

