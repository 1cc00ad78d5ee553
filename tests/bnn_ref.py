"""The Bayesian neural network target of include/mivi.h (mivi_set_target_bnn) restated in numpy: float64, or every array and sum in `dtype`
(the same-precision restatement the GPU tests measure rounding against).  The oracle targets' interface; pinned to torch.autograd in
tests/test_bnn_ref_host.py."""
import numpy as np

LOG2PI = float(np.log(2.0 * np.pi))


class BNNRef:
    def __init__(self, X, y, hidden, likelihood="bernoulli", noise=1.0, prior_std=1.0, likeadj=1.0, dtype=np.float64):
        self.X, self.y = np.asarray(X, dtype=np.float64).astype(dtype), np.asarray(y, dtype=np.float64).astype(dtype)
        self.widths = (self.X.shape[1],) + tuple(hidden) + (1,)
        self.likelihood, self.noise, self.prior_std, self.likeadj, self.dtype = likelihood, noise, prior_std, likeadj, np.dtype(dtype).type

    def dimension(self):
        return sum(o * (i + 1) for i, o in zip(self.widths, self.widths[1:]))

    def unpack(self, z):
        out, off = [], 0
        for i, o in zip(self.widths, self.widths[1:]):
            out.append((z[off:off + o * i].reshape(o, i, order="F"), z[off + o * i:off + o * (i + 1)]))
            off += o * (i + 1)
        return out

    def forward(self, z, X=None):
        """(f, [a_0 .. a_H]) on the rows of X (default: the data)"""
        T = self.dtype
        layers = self.unpack(np.asarray(z, dtype=np.float64).astype(T))
        acts = [self.X if X is None else np.asarray(X, dtype=np.float64).astype(T)]
        for W, b in layers[:-1]:
            acts.append(np.tanh(acts[-1] @ W.T + b))
        return acts[-1] @ layers[-1][0][0] + layers[-1][1][0], acts

    def logdensity_and_gradient(self, z):
        T, n, d = self.dtype, self.X.shape[0], self.dimension()
        z = np.asarray(z, dtype=np.float64).astype(T)
        f, acts = self.forward(z)
        if self.likelihood == "bernoulli":
            e = np.exp(-np.abs(f))
            ll = (self.y * f - (np.maximum(f, T(0)) + np.log1p(e))).sum(dtype=T)
            res = self.y - np.where(f >= 0, T(1), e) / (T(1) + e)
        else:
            u, in2 = self.y - f, T(1.0 / self.noise ** 2)
            ll = T(-0.5) * (u * u).sum(dtype=T) * in2 - T(n * (np.log(self.noise) + 0.5 * LOG2PI))
            res = u * in2
        ip2, g, delta, off = T(1.0 / self.prior_std ** 2), np.empty(d, dtype=T), res[:, None], d
        for (W, b), a in zip(reversed(self.unpack(z)), reversed(acts)):
            off -= W.size + b.size
            g[off:off + W.size] = (T(self.likeadj) * (delta.T @ a) - W * ip2).reshape(-1, order="F")
            g[off + W.size:off + W.size + b.size] = T(self.likeadj) * delta.sum(axis=0, dtype=T) - b * ip2
            delta = (delta @ W) * (T(1) - a * a)   # tanh' from the saved activation (unused past the first layer)
        lp = T(-0.5) * (z * z).sum(dtype=T) * ip2 - T(d * (np.log(self.prior_std) + 0.5 * LOG2PI))
        return float(T(self.likeadj) * ll + lp), g.astype(np.float64)

    def logdensity(self, z):
        return self.logdensity_and_gradient(z)[0]
