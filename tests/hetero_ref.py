"""NumPy restatement of gpflow.likelihoods.HeteroskedasticTFPConditional [ext] with its defaults (Normal(loc=f0, scale=exp(f1)),
GPflow 2.2.1: MultiLatentTFPConditional -> QuadratureLikelihood, ``NDiagGHQuadrature(dim=2, n_gh=20)``), for the parity tests of
the heteroskedastic likelihood (reference docs/notebooks/heteroskedastic.py:58-76).

Everything here sums the LITERAL 20 x 20 product grid, point by point, so that the separated form the HIP map uses is itself
under test.  ``oracle.t_SVGP`` is duck-typed on its likelihood: with an instance of this class it runs the reference's E-step
op for op (g0, g1 are [N, 2], Y is [N, 1]).
"""
import numpy as np

from oracle import tsvgp_oracle as O

LOG_2PI = np.log(2.0 * np.pi)


class HeteroskedasticTFPConditional:
    latent_dim = 2
    n_gh = 20

    def _grid(self, Fmu, Fvar):
        """f0 [N, 20, 1], f1 [N, 1, 20], w_i w_j [20, 20], z [20], sd [N, 2]."""
        z, w = O.gh_points_and_weights(self.n_gh)
        Fmu, Fvar = np.asarray(Fmu, np.float64), np.asarray(Fvar, np.float64)
        sd = np.sqrt(Fvar)
        f0 = (Fmu[:, 0:1] + sd[:, 0:1] * z)[:, :, None]
        f1 = (Fmu[:, 1:2] + sd[:, 1:2] * z)[:, None, :]
        return f0, f1, w[:, None] * w[None, :], z, sd

    @staticmethod
    def log_prob(f0, f1, y):
        return -0.5 * LOG_2PI - f1 - 0.5 * (y - f0) ** 2 * np.exp(-2.0 * f1)

    def variational_expectations(self, Fmu, Fvar, Y):
        f0, f1, W, _, _ = self._grid(Fmu, Fvar)
        y = np.asarray(Y, np.float64)[:, :, None]
        return np.sum(W * self.log_prob(f0, f1, y), axis=(1, 2))

    def variational_expectations_grads(self, Fmu, Fvar, Y):
        """d ve / d(mean, var) of the grid sum by the chain rule through f_p = m_p + sqrt(v_p) z (what GradientTape returns
        at reference src/models/tsvgp.py:256-259).  [N, 2] each."""
        f0, f1, W, z, sd = self._grid(Fmu, Fvar)
        y = np.asarray(Y, np.float64)[:, :, None]
        e = np.exp(-2.0 * f1)
        d0 = W * (y - f0) * e  # d log p / d f0 at every grid point
        d1 = W * (-1.0 + (y - f0) ** 2 * e)  # d log p / d f1
        g0 = np.stack([d0.sum(axis=(1, 2)), d1.sum(axis=(1, 2))], axis=1)
        g1 = np.stack([(d0 * z[None, :, None]).sum(axis=(1, 2)) / (2.0 * sd[:, 0]),
                       (d1 * z[None, None, :]).sum(axis=(1, 2)) / (2.0 * sd[:, 1])], axis=1)
        return g0, g1

    def separated(self, Fmu, Fvar, Y):
        """(g0, g1 [N, 2], ve [N]) from the separated form of the same grid sum: with S0 = sum_i w_i (y - f0_i)^2 = W0 r^2 + Q2 v0
        (r = y - m0; the odd sums vanish node pair by node pair), S1 = sum_j w_j exp(-2 f1_j), T1 = sum_j w_j z_j exp(-2 f1_j),
            ve = -1/2 log 2 pi W0^2 - W0^2 m1 - 1/2 S0 S1,   d/dm0 = W0 r S1,   d/dv0 = -1/2 Q2 S1,
            d/dm1 = S0 S1 - W0^2,   d/dv1 = S0 T1 / (2 s1).
        The literal grid above adds summands of size |r| S1 that cancel to d/dm0 = 0 at r = 0 and to d/dv0 = O(sd0) at any r: its
        rounding error is u |r| S1 / sd0 there.  Against mpmath (tests/test_likmap_range_cpu.py's fixture) it returns d/dm0 = 1.2e25
        where the sum is 0 (r = 0, v1 = 100) and d/dv0 to 1.7e-8 relative at |r| = 1e7, sd0 = 2.7e-3.  This form has no such sum;
        it is the one the range tests compare the HIP map with."""
        z, w = O.gh_points_and_weights(self.n_gh)
        Fmu, Fvar = np.asarray(Fmu, np.float64), np.asarray(Fvar, np.float64)
        m0, m1, v0, s1 = Fmu[:, 0], Fmu[:, 1], Fvar[:, 0], np.sqrt(Fvar[:, 1])
        r = np.asarray(Y, np.float64).reshape(-1) - m0
        e = w * np.exp(-2.0 * (m1[:, None] + s1[:, None] * z))
        W0, Q2, S1, T1 = w.sum(), np.sum(w * z * z), e.sum(axis=1), (e * z).sum(axis=1)
        S0 = W0 * r * r + Q2 * v0
        ve = -0.5 * LOG_2PI * W0 * W0 - W0 * W0 * m1 - 0.5 * S0 * S1
        return np.stack([W0 * r * S1, S0 * S1 - W0 * W0], axis=1), np.stack([-0.5 * Q2 * S1, S0 * T1 / (2.0 * s1)], axis=1), ve

    def predict_mean_and_var(self, Fmu, Fvar):
        f0, f1, W, _, _ = self._grid(Fmu, Fvar)
        ey = np.sum(W * f0 * np.ones_like(f1), axis=(1, 2))
        ey2 = np.sum(W * (np.exp(2.0 * f1) + f0 ** 2), axis=(1, 2))
        return ey[:, None], (ey2 - ey ** 2)[:, None]

    def predict_log_density(self, Fmu, Fvar, Y):
        f0, f1, W, _, _ = self._grid(Fmu, Fvar)
        y = np.asarray(Y, np.float64)[:, :, None]
        a = (self.log_prob(f0, f1, y) + np.log(W)).reshape(f0.shape[0], -1)
        amax = a.max(axis=1, keepdims=True)
        return (amax + np.log(np.sum(np.exp(a - amax), axis=1, keepdims=True)))[:, 0]
