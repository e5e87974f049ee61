"""NumPy restatement of gpflow.likelihoods.MultiClass(num_classes) with the RobustMax inverse link [ext] (GPflow 2.2.1), for the
parity tests of the MultiClass likelihood.

``oracle.t_SVGP`` is duck-typed on its likelihood: with an instance of ``MultiClass`` below it runs the reference's E-step op for
op (g0, g1 are [N, C], Y is [N, 1]).  The value is written from ``RobustMax.prob_is_largest``, array op for array op as GPflow
writes it; the gradients are written on their own from the closed form of the derivative of that quadrature sum (what
tf.GradientTape returns at reference src/models/tsvgp.py:256-259), node by node, so that the two check each other through
difference quotients (tests/test_robustmax_cpu.py).  The derivative through an active clip is zero, as under tf.clip_by_value.
"""
import numpy as np
from scipy.special import erf

NGH = 20
CLIP = 1e-10
JIT = 1e-4  # the jitter of prob_is_largest's normal cdf: cdf * (1 - 2e-4) + 1e-4


class MultiClass:
    def __init__(self, num_classes, epsilon=1e-3):
        self.num_classes = self.latent_dim = int(num_classes)
        self.epsilon = float(epsilon)
        self.num_gauss_hermite_points = NGH

    @property
    def eps_k1(self):
        return self.epsilon / (self.num_classes - 1.0)

    # ------------------------------------------------------------------ the value: RobustMax.prob_is_largest
    def _onehot(self, Y):
        y = np.asarray(Y, np.float64).reshape(-1)
        return y[:, None] == np.arange(self.num_classes)[None, :]  # [N, C] bool

    def prob_is_largest(self, Y, mu, var):
        mu, var = np.asarray(mu, np.float64), np.asarray(var, np.float64)
        gh_x, gh_w = np.polynomial.hermite.hermgauss(NGH)
        oh_on = self._onehot(Y).astype(np.float64)
        mu_selected = np.sum(oh_on * mu, axis=1).reshape(-1, 1)
        var_selected = np.sum(oh_on * var, axis=1).reshape(-1, 1)
        X = mu_selected + gh_x * np.sqrt(np.clip(2.0 * var_selected, CLIP, np.inf))  # [N, 20]
        dist = (X[:, None, :] - mu[:, :, None]) / np.sqrt(np.clip(var, CLIP, np.inf))[:, :, None]  # [N, C, 20]
        cdfs = 0.5 * (1.0 + erf(dist / np.sqrt(2.0)))
        cdfs = cdfs * (1.0 - 2.0 * JIT) + JIT
        oh_off = 1.0 - oh_on
        cdfs = cdfs * oh_off[:, :, None] + oh_on[:, :, None]  # the labelled class leaves the product
        return np.prod(cdfs, axis=1) @ (gh_w / np.sqrt(np.pi)).reshape(-1, 1)  # [N, 1]

    def variational_expectations(self, Fmu, Fvar, Y):
        p = self.prob_is_largest(Y, Fmu, Fvar)[:, 0]
        return p * np.log(1.0 - self.epsilon) + (1.0 - p) * np.log(self.eps_k1)

    def _density(self, Fmu, Fvar, Y):
        p = self.prob_is_largest(Y, Fmu, Fvar)[:, 0]
        return p * (1.0 - self.epsilon) + (1.0 - p) * self.eps_k1

    def predict_log_density(self, Fmu, Fvar, Y):
        return np.log(self._density(Fmu, Fvar, Y))

    def predict_mean_and_var(self, Fmu, Fvar):
        n = np.asarray(Fmu).shape[0]
        ps = np.stack([self._density(Fmu, Fvar, np.full((n, 1), float(k))) for k in range(self.num_classes)], axis=1)
        return ps, ps - ps ** 2

    def log_prob(self, F, Y):
        hit = np.argmax(np.asarray(F), axis=1) == np.asarray(Y).reshape(-1)
        return np.where(hit, np.log(1.0 - self.epsilon), np.log(self.eps_k1))

    # ------------------------------------------------------------------ the gradients: closed form, node by node
    def variational_expectations_grads(self, Fmu, Fvar, Y):
        """(g0, g1) [N, C] = d ve / d (mean, var), uncropped: the closed form of the derivative of the quadrature sum, one node at
        a time over all rows (none of the array expressions of ``prob_is_largest``: the labelled class is masked, not one-hot
        weighted, and the products are taken per node)."""
        mu, var = np.asarray(Fmu, np.float64), np.asarray(Fvar, np.float64)
        N, C = mu.shape
        rows, k = np.arange(N), np.asarray(Y, np.float64).reshape(-1).astype(np.int64)
        x, w = np.polynomial.hermite.hermgauss(NGH)
        z, om = np.sqrt(2.0) * x, w / np.sqrt(np.pi)
        kappa = np.log(1.0 - self.epsilon) - np.log(self.eps_k1)
        other = np.arange(C)[None, :] != k[:, None]  # [N, C]: the classes the labelled latent is compared with
        mu_y, v_y = mu[rows, k], var[rows, k]
        with np.errstate(invalid="ignore"):
            clip_y, clip_c = 2.0 * v_y < CLIP, var < CLIP  # a NaN compares false and stays NaN below
            s_y = np.sqrt(np.where(clip_y, CLIP / 2.0, v_y))
            v_c = np.where(clip_c, CLIP, var)
            s_c = np.sqrt(v_c)
            g0, g1 = np.zeros((N, C)), np.zeros((N, C))
            for i in range(NGH):
                # (m_y - m_c) + z_i s_y, not (m_y + z_i s_y) - m_c: with |m| = 12 and s_c = 1e-5 the second form's rounding, u |m| / s_c
                # in d, is 4.6e-10 relative in r at d = 3.5 (tests/test_likmap_range_cpu.py measures it against mpmath)
                d = ((mu_y[:, None] - mu) + (z[i] * s_y)[:, None]) / s_c
                cdf = 0.5 * (1.0 + erf(d / np.sqrt(2.0))) * (1.0 - 2.0 * JIT) + JIT
                r = (1.0 - 2.0 * JIT) * np.exp(-0.5 * d * d) / np.sqrt(2.0 * np.pi) / cdf
                wP = om[i] * np.prod(np.where(other, cdf, 1.0), axis=1)  # w_i P_i
                g0 += np.where(other, -kappa * wP[:, None] * r / s_c, 0.0)
                g1 += np.where(other & ~clip_c, -kappa * wP[:, None] * r * d / (2.0 * v_c), 0.0)
                t = kappa * wP * np.sum(np.where(other, r / s_c, 0.0), axis=1)
                g0[rows, k] += t
                g1[rows, k] += np.where(clip_y, 0.0, t * z[i] / (2.0 * s_y))
        return g0, g1
