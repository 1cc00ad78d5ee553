"""The probabilistic PCA target of include/mivi.h (mivi_set_target_ppca) restated in numpy: float64, or every array and sum in `dtype`.  The oracle
targets' interface; `rows` evaluates a selection (z_r keeps its row id, the other rows get a zero gradient).  Pinned to torch.autograd in tests/test_gpu_ppca.py."""
import numpy as np

LOG2PI = float(np.log(2.0 * np.pi))


class PPCARef:
    def __init__(self, Y, k, mask=None, ard=False, prior_std=1.0, mean_std=10.0, noise_scale=1.0, likeadj=1.0, rows=None, dtype=np.float64):
        self.Y = np.asarray(Y, dtype=np.float64).astype(dtype)
        self.N, self.D = self.Y.shape
        self.m = np.ones(self.Y.shape, dtype=dtype) if mask is None else np.asarray(mask).astype(dtype)
        self.Y = np.where(self.m > 0, self.Y, dtype(0))   # (an unobserved entry may hold anything)
        self.k, self.ard, self.rows = int(k), bool(ard), np.arange(self.N) if rows is None else np.asarray(rows, dtype=np.int64)
        self.prior_std, self.mean_std, self.noise_scale, self.likeadj, self.dtype = prior_std, mean_std, noise_scale, likeadj, np.dtype(dtype).type

    def dimension(self):
        return self.D * self.k + self.N * self.k + self.D + (self.k if self.ard else 0) + 1

    def logdensity_and_gradient(self, theta):
        T, D, N, k, R = self.dtype, self.D, self.N, self.k, self.rows
        th = np.asarray(theta, dtype=np.float64).astype(T)
        oz, om = D * k, D * k + N * k
        W, Z, mu, a, s = th[:oz].reshape(k, D).T, th[oz:om].reshape(N, k), th[om:om + D], th[om + D:-1], th[-1]   # (a: empty without ARD)
        la, em2, e2 = T(self.likeadj), np.exp(T(-2) * s), np.exp(T(2) * s)
        ip2, im2, in2 = T(1.0 / self.prior_std ** 2), T(1.0 / self.mean_std ** 2), T(1.0 / self.noise_scale ** 2)
        hn, Zs, m = np.log(2.0) - 0.5 * LOG2PI, Z[R], self.m[R]   # hn: log of the half-normal's constant, before the scale
        res = m * (self.Y[R] - (mu + Zs @ W.T))
        ss, cnt, zz = (res * res).sum(dtype=T), m.sum(dtype=T), (Zs * Zs).sum(dtype=T)
        val = la * (T(-0.5) * ss * em2 - cnt * (s + T(0.5 * LOG2PI)) - T(0.5) * zz - T(len(R) * 0.5 * k * LOG2PI))
        val += T(-0.5) * (mu * mu).sum(dtype=T) * im2 - T(D * (np.log(self.mean_std) + 0.5 * LOG2PI))
        val += T(hn - np.log(self.noise_scale)) - T(0.5) * e2 * in2 + s
        g = np.zeros(th.size, dtype=T)
        e = res * em2
        gW = la * (e.T @ Zs)
        g[oz:om].reshape(N, k)[R] = la * (e @ W - Zs)
        g[om:om + D] = la * e.sum(axis=0, dtype=T) - mu * im2
        g[-1] = la * (ss * em2 - cnt) - e2 * in2 + T(1)
        if self.ard:
            w2, ea2, eam2 = (W * W).sum(axis=0, dtype=T), np.exp(T(2) * a), np.exp(T(-2) * a)
            val += (T(-0.5) * w2 * eam2 - T(D) * (a + T(0.5 * LOG2PI)) + T(hn - np.log(self.prior_std)) - T(0.5) * ea2 * ip2 + a).sum(dtype=T)
            gW = gW - W * eam2
            g[om + D:om + D + k] = T(-D) + w2 * eam2 - ea2 * ip2 + T(1)
        else:
            val += T(-0.5) * (W * W).sum(dtype=T) * ip2 - T(D * k * (np.log(self.prior_std) + 0.5 * LOG2PI))
            gW = gW - W * ip2
        g[:oz] = gW.T.reshape(-1)
        return float(val), g.astype(np.float64)

    def logdensity(self, theta):
        return self.logdensity_and_gradient(theta)[0]
