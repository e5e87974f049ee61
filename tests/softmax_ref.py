"""NumPy restatement of gpflow.likelihoods.Softmax [ext] (GPflow 2.2.1: a ``MonteCarloLikelihood`` with
``num_monte_carlo_points = 100``) and of the project's normal generator (include/tsvgp_hip.h, "The normal generator":
Philox4x32-10 and Box-Muller), for the parity tests of the Softmax likelihood (reference docs/notebooks/mnist.py).

``oracle.t_SVGP`` is duck-typed on its likelihood: with an instance of ``Softmax`` below it runs the reference's E-step op for op
(g0, g1 are [N, C], Y is [N, 1]).  Every evaluation without an explicit ``epsilon`` takes the draws of the current
``(seed, draw)`` for the global rows ``row_offset .. row_offset + N`` and then advances ``draw`` by one, as the product does.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SHIFT = np.uint64(32)
TWO_PI = 6.283185307179586


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11): ctr = four uint32 arrays (or scalars), key = two uint32 scalars or arrays."""
    c = [np.asarray(x, np.uint64) & MASK for x in ctr]
    k = [np.asarray(key[0], np.uint64) & MASK, np.asarray(key[1], np.uint64) & MASK]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> SHIFT) ^ c[1] ^ k[0], p1 & MASK, (p0 >> SHIFT) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return c


def _box_muller(xa, xb):
    u1 = (xa.astype(np.float64) + 0.5) * 2.0 ** -32
    u2 = (xb.astype(np.float64) + 0.5) * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u1))
    th = TWO_PI * u2
    return r * np.cos(th), r * np.sin(th)


def normals(seed, draw, rows, S, C):
    """[S, len(rows), C] fp64: the draw of (seed, draw, global row n, sample s, class c).  ``rows``: global row numbers."""
    rows = np.asarray(rows, np.int64).astype(np.uint64)
    seed = np.uint64(np.int64(seed).astype(np.uint64))
    Q4 = (C + 3) // 4
    s = np.arange(S, dtype=np.uint64)[:, None, None]
    n = rows[None, :, None]
    q = np.arange(Q4, dtype=np.uint64)[None, None, :]
    shape = (S, len(rows), Q4)
    bc = lambda a: np.broadcast_to(a, shape)
    x = philox4x32_10((bc(n & MASK), bc(n >> SHIFT), bc(s * np.uint64(8) + q), bc(np.uint64(int(draw) & 0xFFFFFFFF))),
                      (seed & MASK, seed >> SHIFT))
    z0, z1 = _box_muller(x[0], x[1])
    z2, z3 = _box_muller(x[2], x[3])
    return np.stack([z0, z1, z2, z3], axis=-1).reshape(S, len(rows), 4 * Q4)[:, :, :C]


class Softmax:
    def __init__(self, num_classes, seed=0):
        self.num_classes = self.latent_dim = int(num_classes)
        self.num_monte_carlo_points = 100
        self.seed, self.draw, self.row_offset = int(seed), 0, 0

    def _eps(self, N, epsilon, offset=None):
        if epsilon is not None:
            return np.asarray(epsilon, np.float64)
        offset = self.row_offset if offset is None else offset
        eps = normals(self.seed, self.draw, offset + np.arange(N), self.num_monte_carlo_points, self.num_classes)
        self.draw += 1
        return eps

    def _samples(self, Fmu, Fvar, epsilon, offset=None):
        Fmu, Fvar = np.asarray(Fmu, np.float64), np.asarray(Fvar, np.float64)
        eps = self._eps(Fmu.shape[0], epsilon, offset)
        return Fmu[None] + np.sqrt(Fvar[None]) * eps, eps  # [S, N, C]

    @staticmethod
    def _lse(f):
        mx = f.max(axis=-1, keepdims=True)
        return mx + np.log(np.sum(np.exp(f - mx), axis=-1, keepdims=True))

    def _onehot(self, Y):
        y = np.asarray(Y, np.float64).reshape(-1)
        return (y[:, None] == np.arange(self.num_classes)[None, :]).astype(np.float64)  # [N, C]

    def log_prob_samples(self, Fmu, Fvar, Y, epsilon=None, offset=None):
        """log p(y | f^s) [S, N]."""
        f, _ = self._samples(Fmu, Fvar, epsilon, offset)
        return np.sum(self._onehot(Y)[None] * f, axis=-1) - self._lse(f)[..., 0]

    def variational_expectations(self, Fmu, Fvar, Y, epsilon=None):
        return self.log_prob_samples(Fmu, Fvar, Y, epsilon).mean(axis=0)

    def variational_expectations_grads(self, Fmu, Fvar, Y, epsilon=None):
        """d ve / d(mean, var) of the estimator through f = m + sqrt(v) eps (what GradientTape returns at reference
        src/models/tsvgp.py:256-259).  [N, C] each."""
        f, eps = self._samples(Fmu, Fvar, epsilon)
        d = self._onehot(Y)[None] - np.exp(f - self._lse(f))
        sd = np.sqrt(np.asarray(Fvar, np.float64))
        return d.mean(axis=0), (d * eps).mean(axis=0) / (2.0 * sd)

    def predict_mean_and_var(self, Fmu, Fvar, epsilon=None):
        f, _ = self._samples(Fmu, Fvar, epsilon, 0)  # test points are numbered from 0, whatever the training shard's offset
        p = np.exp(f - self._lse(f))
        ey = p.mean(axis=0)
        return ey, ((p - p * p) + p * p).mean(axis=0) - ey ** 2

    def predict_log_density(self, Fmu, Fvar, Y, epsilon=None):
        lp = self.log_prob_samples(Fmu, Fvar, Y, epsilon, 0)
        mx = lp.max(axis=0)
        return mx + np.log(np.sum(np.exp(lp - mx), axis=0)) - np.log(lp.shape[0])
