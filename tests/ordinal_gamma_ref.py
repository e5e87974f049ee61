"""NumPy fp64 restatement of gpflow.likelihoods.Ordinal, gpflow.likelihoods.Gamma and gpflow.likelihoods.Exponential (exp link)
[ext], GPflow 2.2.1, for the parity tests of ``tsvgp_lik_map_ordinal_*``, of the Gamma arm of ``tsvgp_lik_map_scalar_*`` and of
the models on top of them, in the style of tests/scalar_lik_ref.py.

Ordinal sums the LITERAL 20 Gauss-Hermite nodes point by point (the HIP map pairs the nodes +-z); Gamma and Exponential take the
closed form GPflow takes under the exp link.  ``oracle.t_SVGP`` / ``oracle.t_SVGP_white`` are duck-typed on their likelihood:
with an instance of one of these classes they run the reference's E-step op for op (Y [N, P], g0, g1 [N, P]).

Ordinal's bin probability Phi~(a) - Phi~(b), Phi~(x) = Phi(x) (1 - 2e-3) + 1e-3, equals (1 - 2e-3) (Phi(a) - Phi(b)): the two
jitters cancel.  ``log_prob(..., literal=True)`` forms it as GPflow writes it, from two erf values near 1 in the upper tail; the
default forms it from erfc on the side where both tail masses are small, which keeps every digit of a far-tail bin.  The two
differ by the rounding of the literal form, at most a few 1e-16 in phi and so a few 1e-10 in log(phi + 1e-6)
(tests/test_ordinal_gamma_cpu.py bounds it).
"""
import math

import numpy as np
from scipy.special import digamma, erf, erfc, gammaln

from tests.scalar_lik_ref import _logsumexp, _nodes

JIT = 1e-3  # gpflow.likelihoods.utils.inv_probit
FLOOR = 1e-6  # gpflow.likelihoods.Ordinal._scalar_log_prob
_RSQRT2PI = 1.0 / math.sqrt(2.0 * math.pi)


def _density(x):
    """N(x); 0 at an infinite edge."""
    with np.errstate(over="ignore"):
        return _RSQRT2PI * np.exp(-0.5 * x * x)


def _times_density(x):
    """x N(x); 0 at an infinite edge."""
    fin = np.isfinite(x)
    return np.where(fin, np.where(fin, x, 0.0) * _density(np.where(fin, x, 0.0)), 0.0)


class Ordinal:
    latent_dim = 1

    def __init__(self, bin_edges, sigma=1.0):
        self.bin_edges = np.asarray(bin_edges, np.float64)
        self.num_bins = self.bin_edges.size + 1
        self.sigma = float(sigma)
        self._up = np.concatenate([self.bin_edges, [np.inf]])
        self._lo = np.concatenate([[-np.inf], self.bin_edges])

    def _ab(self, F, Y, sigma=None):
        s = self.sigma if sigma is None else sigma
        k = np.broadcast_to(np.asarray(Y, np.float64), np.shape(F)).astype(np.int64)
        return (self._up[k] - F) / s, (self._lo[k] - F) / s, s

    @staticmethod
    def _phi(a, b, literal=False):
        if literal:
            inv_probit = lambda x: 0.5 * (1.0 + erf(x / np.sqrt(2.0))) * (1 - 2 * JIT) + JIT
            return inv_probit(a) - inv_probit(b)
        flip = b > 0.0
        hi, lw = np.where(flip, -b, a), np.where(flip, -a, b)
        return 0.5 * (1 - 2 * JIT) * (erfc(-hi / np.sqrt(2.0)) - erfc(-lw / np.sqrt(2.0)))

    def log_prob(self, F, Y, sigma=None, literal=False):
        a, b, _ = self._ab(np.asarray(F, np.float64), Y, sigma)
        return np.log(self._phi(a, b, literal) + FLOOR)

    def dlog_prob_df(self, F, Y):
        a, b, s = self._ab(np.asarray(F, np.float64), Y)
        return -(1 - 2 * JIT) * (_density(a) - _density(b)) / (s * (self._phi(a, b) + FLOOR))

    def dlog_prob_dsigma(self, F, Y):
        a, b, s = self._ab(np.asarray(F, np.float64), Y)
        return -(1 - 2 * JIT) * (_times_density(a) - _times_density(b)) / (s * (self._phi(a, b) + FLOOR))

    def variational_expectations(self, Fmu, Fvar, Y, sigma=None, literal=False):
        f, w, _, _ = _nodes(Fmu, Fvar)
        return np.sum(w * self.log_prob(f, np.asarray(Y, np.float64)[..., None], sigma, literal), axis=-1)

    def variational_expectations_grads(self, Fmu, Fvar, Y):
        """d ve / d (mean, var) of the quadrature sum through f_i = m + sqrt(v) z_i, uncropped."""
        f, w, z, sd = _nodes(Fmu, Fvar)
        d = w * self.dlog_prob_df(f, np.asarray(Y, np.float64)[..., None])
        return d.sum(axis=-1), (d * z).sum(axis=-1) / (2.0 * sd)

    def variational_expectations_dsigma(self, Fmu, Fvar, Y):
        """d ve / d sigma, per entry."""
        f, w, _, _ = _nodes(Fmu, Fvar)
        return np.sum(w * self.dlog_prob_dsigma(f, np.asarray(Y, np.float64)[..., None]), axis=-1)

    def _bin_probs(self, F):
        """[..., K]: GPflow's _make_phi, the probability of every bin without the 1e-6."""
        F = np.asarray(F, np.float64)[..., None]
        return self._phi((self._up - F) / self.sigma, (self._lo - F) / self.sigma, literal=True)

    def predict_mean_and_var(self, Fmu, Fvar):
        f, w, _, _ = _nodes(Fmu, Fvar)
        ks = np.arange(self.num_bins, dtype=np.float64)
        phi = self._bin_probs(f)
        cm = phi @ ks
        cv = phi @ (ks * ks) - cm * cm
        ey = np.sum(w * cm, axis=-1)
        return ey, np.sum(w * (cv + cm * cm), axis=-1) - ey * ey

    def predict_log_density(self, Fmu, Fvar, Y):
        f, w, _, _ = _nodes(Fmu, Fvar)
        a = self.log_prob(f, np.asarray(Y, np.float64)[..., None]) + np.log(w)
        return np.sum(_logsumexp(a, -1), axis=-1)


class Gamma:
    """Gamma(shape a) with scale exp(f): log p = -a f - lgamma(a) + (a - 1) log y - y exp(-f); the power of y is skipped at
    a == 1 exactly."""

    latent_dim = 1

    def __init__(self, shape=1.0):
        self.shape = float(shape)

    def log_prob(self, F, Y, shape=None):
        a = self.shape if shape is None else shape
        F, Y = np.asarray(F, np.float64), np.asarray(Y, np.float64)
        out = -a * F - gammaln(a) - Y * np.exp(-F)
        return out if a == 1.0 else out + (a - 1.0) * np.log(Y)

    def variational_expectations(self, Fmu, Fvar, Y, shape=None):
        a = self.shape if shape is None else shape
        Fmu, Fvar, Y = (np.asarray(x, np.float64) for x in (Fmu, Fvar, Y))
        out = -a * Fmu - gammaln(a) - Y * np.exp(-Fmu + 0.5 * Fvar)
        return out if a == 1.0 else out + (a - 1.0) * np.log(Y)

    def variational_expectations_quadrature(self, Fmu, Fvar, Y):
        """The same expectation by 20-point Gauss-Hermite: a cross-check."""
        f, w, _, _ = _nodes(Fmu, Fvar)
        return np.sum(w * self.log_prob(f, np.asarray(Y, np.float64)[..., None]), axis=-1)

    def variational_expectations_grads(self, Fmu, Fvar, Y):
        Fmu, Fvar, Y = (np.asarray(x, np.float64) for x in (Fmu, Fvar, Y))
        e = Y * np.exp(-Fmu + 0.5 * Fvar)
        return -self.shape + e, -0.5 * e

    def variational_expectations_dshape(self, Fmu, Fvar, Y):
        """d ve / d shape, per entry."""
        Fmu, Y = np.asarray(Fmu, np.float64), np.asarray(Y, np.float64)
        return -Fmu - digamma(self.shape) + np.log(Y)

    def conditional_mean(self, F):
        return self.shape * np.exp(F)

    def conditional_variance(self, F):
        return self.shape * np.exp(2.0 * F)

    def predict_mean_and_var(self, Fmu, Fvar):
        f, w, _, _ = _nodes(Fmu, Fvar)
        cm = self.conditional_mean(f)
        ey = np.sum(w * cm, axis=-1)
        return ey, np.sum(w * (self.conditional_variance(f) + cm * cm), axis=-1) - ey * ey

    def predict_log_density(self, Fmu, Fvar, Y):
        f, w, _, _ = _nodes(Fmu, Fvar)
        a = self.log_prob(f, np.asarray(Y, np.float64)[..., None]) + np.log(w)
        return np.sum(_logsumexp(a, -1), axis=-1)


class Exponential:
    """log p = -f - y exp(-f), written out on its own (not through Gamma): the two must agree bit for bit at shape 1."""

    latent_dim = 1

    def log_prob(self, F, Y):
        F, Y = np.asarray(F, np.float64), np.asarray(Y, np.float64)
        return -F - Y * np.exp(-F)

    def variational_expectations(self, Fmu, Fvar, Y):
        Fmu, Fvar, Y = (np.asarray(x, np.float64) for x in (Fmu, Fvar, Y))
        return -Fmu - Y * np.exp(-Fmu + 0.5 * Fvar)

    def variational_expectations_grads(self, Fmu, Fvar, Y):
        Fmu, Fvar, Y = (np.asarray(x, np.float64) for x in (Fmu, Fvar, Y))
        e = Y * np.exp(-Fmu + 0.5 * Fvar)
        return -1.0 + e, -0.5 * e

    def predict_mean_and_var(self, Fmu, Fvar):
        f, w, _, _ = _nodes(Fmu, Fvar)
        cm = np.exp(f)
        ey = np.sum(w * cm, axis=-1)
        return ey, np.sum(w * (np.exp(2.0 * f) + cm * cm), axis=-1) - ey * ey

    def predict_log_density(self, Fmu, Fvar, Y):
        f, w, _, _ = _nodes(Fmu, Fvar)
        a = self.log_prob(f, np.asarray(Y, np.float64)[..., None]) + np.log(w)
        return np.sum(_logsumexp(a, -1), axis=-1)
