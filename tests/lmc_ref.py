"""NumPy fp64 restatement of the linear model of coregionalization (gpflow.kernels.LinearCoregionalization and
gpflow.conditionals.util.mix_latent_gp [ext], GPflow 2.2.1, restated from the public API): P outputs f = W g mixed from L
independent latent GPs, W [P, L].

``mix`` / ``unmix`` / ``dW`` are what ``tsvgp_lmc_mix_*`` / ``tsvgp_lmc_unmix_*`` compute, in plain matrix products.  ``Mixed(W,
base)`` wraps a likelihood with one latent per output column (the oracle's Gaussian / Bernoulli, tests/scalar_lik_ref.py's
Poisson) into one over the LATENT moments: ``oracle.t_SVGP`` is duck-typed on its likelihood, so with ``SeparateIndependent``
kernels and an instance of this class it runs the reference's E-step (src/models/tsvgp.py:234-304) op for op, its crop of g1
applied to the latents' gradient as the issue states (g0, g1 are [N, L], Y is [N, P]).
"""
import numpy as np


def mix(W, mean_g, var_g):
    """(Fmu, Fvar) [N, P]: Fmu = mean_g W^T, Fvar = var_g (W * W)^T."""
    W = np.asarray(W, np.float64)
    return np.asarray(mean_g, np.float64) @ W.T, np.asarray(var_g, np.float64) @ (W * W).T


def unmix(W, g0_f, g1_f, crop=True):
    """(g0_g, g1_g) [N, L]: g0_g = g0_f W, g1_g = g1_f (W * W), the latter cropped at -1e-8 (tsvgp.py:262-263) with ``crop``."""
    W = np.asarray(W, np.float64)
    g0 = np.asarray(g0_f, np.float64) @ W
    g1 = np.asarray(g1_f, np.float64) @ (W * W)
    if crop:
        g1 = np.minimum(g1, -1e-8 * np.ones_like(g1))
    return g0, g1


def dW(W, g0_f, g1_f, mean_g, var_g):
    """sum_n d ve_n / d W [P, L] = g0_f^T mean_g + 2 W * (g1_f^T var_g)."""
    W = np.asarray(W, np.float64)
    return (np.asarray(g0_f, np.float64).T @ np.asarray(mean_g, np.float64)
            + 2.0 * W * (np.asarray(g1_f, np.float64).T @ np.asarray(var_g, np.float64)))


def full_output_cov(W, var_g):
    """W diag(var_g[n]) W^T, [N, P, P]."""
    W = np.asarray(W, np.float64)
    return np.einsum("pl,nl,ql->npq", W, np.asarray(var_g, np.float64), W)


class Mixed:
    """``base`` applied to the mixed moments, as a likelihood over the L latent moments."""

    def __init__(self, W, base):
        self.W = np.asarray(W, np.float64)
        self.base = base
        self.latent_dim = self.W.shape[1]

    def _per_row(self, ve):
        ve = np.asarray(ve, np.float64)
        return ve if ve.ndim == 1 else np.sum(ve, axis=-1)  # (the oracle's likelihoods sum over the columns, Poisson does not)

    def variational_expectations(self, mean_g, var_g, Y):
        Fmu, Fvar = mix(self.W, mean_g, var_g)
        return self._per_row(self.base.variational_expectations(Fmu, Fvar, np.asarray(Y, np.float64)))

    def output_grads(self, mean_g, var_g, Y):
        """(g0_f, g1_f) [N, P] of the base likelihood at the mixed moments."""
        Fmu, Fvar = mix(self.W, mean_g, var_g)
        return self.base.variational_expectations_grads(Fmu, Fvar, np.asarray(Y, np.float64))

    def variational_expectations_grads(self, mean_g, var_g, Y):
        """d ve / d (mean_g, var_g) [N, L], uncropped (the oracle's natgrad_step crops what this returns)."""
        g0_f, g1_f = self.output_grads(mean_g, var_g, Y)
        return unmix(self.W, g0_f, g1_f, crop=False)

    def predict_mean_and_var(self, mean_g, var_g):
        return self.base.predict_mean_and_var(*mix(self.W, mean_g, var_g))

    def predict_log_density(self, mean_g, var_g, Y):
        return self.base.predict_log_density(*mix(self.W, mean_g, var_g), np.asarray(Y, np.float64))
