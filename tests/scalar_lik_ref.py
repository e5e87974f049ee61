"""NumPy fp64 restatement of gpflow.likelihoods.StudentT and gpflow.likelihoods.Poisson (exp link) [ext], GPflow 2.2.1, for the
parity tests of ``tsvgp_lik_map_scalar_*`` and of the models on top of it.

StudentT sums the LITERAL 20 Gauss-Hermite nodes point by point (the HIP map pairs the nodes +-z); Poisson takes the closed form
GPflow takes under the exp link.  ``oracle.t_SVGP`` / ``oracle.t_SVGP_white`` are duck-typed on their likelihood: with an
instance of one of these classes they run the reference's E-step op for op (Y [N, P], g0, g1 [N, P]) -- the host-side step the
GPU tests compare with.
"""
import math

import numpy as np
from scipy.special import gammaln

from oracle import tsvgp_oracle as O

N_GH = 20


def _nodes(Fmu, Fvar):
    """f [..., 20], w [20], z [20], sd [...]."""
    z, w = O.gh_points_and_weights(N_GH)
    Fmu, Fvar = np.asarray(Fmu, np.float64), np.asarray(Fvar, np.float64)
    sd = np.sqrt(Fvar)
    return Fmu[..., None] + sd[..., None] * z, w, z, sd


def _logsumexp(a, axis):
    amax = a.max(axis=axis, keepdims=True)
    return np.squeeze(amax, axis) + np.log(np.sum(np.exp(a - amax), axis=axis))


class StudentT:
    latent_dim = 1

    def __init__(self, scale=1.0, df=3.0):
        self.scale, self.df = float(scale), float(df)

    def log_prob(self, F, Y, scale=None):
        s, nu = self.scale if scale is None else scale, self.df
        const = math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi) - np.log(s)
        return const - 0.5 * (nu + 1.0) * np.log1p(((np.asarray(Y, np.float64) - F) / s) ** 2 / nu)

    def dlog_prob_df(self, F, Y):
        s, nu = self.scale, self.df
        r = (np.asarray(Y, np.float64) - F) / s
        return (nu + 1.0) * r / (s * nu * (1.0 + r * r / nu))

    def variational_expectations(self, Fmu, Fvar, Y, scale=None):
        f, w, _, _ = _nodes(Fmu, Fvar)
        return np.sum(w * self.log_prob(f, np.asarray(Y, np.float64)[..., None], scale), axis=-1)

    def variational_expectations_grads(self, Fmu, Fvar, Y):
        """d ve / d (mean, var) of the quadrature sum through f_i = m + sqrt(v) z_i (what GradientTape returns at reference
        src/models/tsvgp.py:256-259)."""
        f, w, z, sd = _nodes(Fmu, Fvar)
        d = w * self.dlog_prob_df(f, np.asarray(Y, np.float64)[..., None])
        return d.sum(axis=-1), (d * z).sum(axis=-1) / (2.0 * sd)

    def variational_expectations_dscale(self, Fmu, Fvar, Y):
        """d ve / d scale, per entry."""
        f, w, _, _ = _nodes(Fmu, Fvar)
        s, nu = self.scale, self.df
        u = ((np.asarray(Y, np.float64)[..., None] - f) / s) ** 2 / nu
        return np.sum(w * ((nu + 1.0) * u / (1.0 + u) - 1.0), axis=-1) / s

    def predict_mean_and_var(self, Fmu, Fvar):
        if self.df <= 2.0:
            raise ValueError("df <= 2")
        return np.asarray(Fmu, np.float64), np.asarray(Fvar, np.float64) + self.scale ** 2 * self.df / (self.df - 2.0)

    def predict_log_density(self, Fmu, Fvar, Y):
        f, w, _, _ = _nodes(Fmu, Fvar)
        a = self.log_prob(f, np.asarray(Y, np.float64)[..., None]) + np.log(w)
        return np.sum(_logsumexp(a, -1), axis=-1)


class Poisson:
    latent_dim = 1

    def __init__(self, binsize=1.0):
        self.binsize = float(binsize)

    def log_prob(self, F, Y):
        Y = np.asarray(Y, np.float64)
        return Y * (F + math.log(self.binsize)) - self.binsize * np.exp(F) - gammaln(Y + 1.0)

    def variational_expectations(self, Fmu, Fvar, Y):
        Fmu, Fvar, Y = (np.asarray(a, np.float64) for a in (Fmu, Fvar, Y))
        return Y * Fmu + Y * math.log(self.binsize) - self.binsize * np.exp(Fmu + 0.5 * Fvar) - gammaln(Y + 1.0)

    def variational_expectations_quadrature(self, Fmu, Fvar, Y):
        """The same expectation by 20-point Gauss-Hermite (what GPflow falls back to under another link): a cross-check."""
        f, w, _, _ = _nodes(Fmu, Fvar)
        return np.sum(w * self.log_prob(f, np.asarray(Y, np.float64)[..., None]), axis=-1)

    def variational_expectations_grads(self, Fmu, Fvar, Y):
        Fmu, Fvar, Y = (np.asarray(a, np.float64) for a in (Fmu, Fvar, Y))
        e = self.binsize * np.exp(Fmu + 0.5 * Fvar)
        return Y - e, -0.5 * e

    def predict_mean_and_var(self, Fmu, Fvar):
        f, w, _, _ = _nodes(Fmu, Fvar)
        rate = self.binsize * np.exp(f)
        ey = np.sum(w * rate, axis=-1)
        return ey, np.sum(w * (rate + rate * rate), axis=-1) - ey * ey

    def predict_log_density(self, Fmu, Fvar, Y):
        f, w, _, _ = _nodes(Fmu, Fvar)
        a = self.log_prob(f, np.asarray(Y, np.float64)[..., None]) + np.log(w)
        return np.sum(_logsumexp(a, -1), axis=-1)
