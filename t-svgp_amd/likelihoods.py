"""Likelihood objects of the hot path: ``Gaussian``, ``Bernoulli`` (probit, 20-point Gauss-Hermite) and
``HeteroskedasticTFPConditional`` (Normal with an Exp scale over two latents, 20 x 20 Gauss-Hermite).

Their N-sized maps -- variational expectations and the (mean, var) gradients the E-step needs
(reference src/models/tsvgp.py:256-263) -- run inside the fused HIP moments kernel
(``tsvgp_moments_*`` with ``lik`` = GAUSSIAN / BERNOULLI) or, for the likelihood that couples two latents, in
``tsvgp_lik_map_hetero_*`` behind the moments; the classes here only carry parameters and
the small predictive helpers drivers call on test points (experiments/uci_regression.py:157).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _backend as B
from .base import Parameter


class Gaussian:
    """gpflow.likelihoods.Gaussian [ext]."""

    lik_id = B.LIK_GAUSSIAN

    def __init__(self, variance=1.0):
        self.variance = Parameter(variance)

    @property
    def lik_param(self) -> float:
        return self.variance.item()

    def predict_mean_and_var(self, Fmu, Fvar):
        return Fmu, Fvar + self.variance.value

    def predict_log_density(self, Fmu, Fvar, Y):
        v = Fvar + self.variance.value
        return torch.sum(-0.5 * (math.log(2 * math.pi) + torch.log(v) + (Y - Fmu) ** 2 / v), dim=-1)


class Bernoulli:
    """gpflow.likelihoods.Bernoulli with the default probit link (1e-3 jitter) [ext]."""

    lik_id = B.LIK_BERNOULLI
    lik_param = 0.0
    num_gauss_hermite_points = 20

    @staticmethod
    def invlink(F):
        return 0.5 * (1.0 + torch.erf(F / math.sqrt(2.0))) * (1 - 2e-3) + 1e-3

    def predict_mean_and_var(self, Fmu, Fvar):
        p = self.invlink(Fmu / torch.sqrt(1 + Fvar))
        return p, p - torch.square(p)

    def predict_log_density(self, Fmu, Fvar, Y):
        p = self.invlink(Fmu / torch.sqrt(1 + Fvar))
        return torch.sum(torch.log(torch.where(Y == 1, p, 1 - p)), dim=-1)


def _named(obj, name: str) -> bool:
    """``obj`` is a class called ``name`` or an instance of one (tfp.distributions.Normal, tfp.bijectors.Exp())."""
    return getattr(obj, "__name__", type(obj).__name__) == name


class HeteroskedasticTFPConditional:
    """gpflow.likelihoods.HeteroskedasticTFPConditional [ext] with its defaults: Normal(loc=f0, scale=exp(f1)), two latent GPs
    per output (``latent_dim = 2``), Y [N, 1] (reference docs/notebooks/heteroskedastic.py:58-60).  The variational expectations
    and their gradients run on the GPU (``tsvgp_lik_map_hetero_*``); the predictive helpers here take the same 20 x 20
    Gauss-Hermite grid as GPflow's ``NDiagGHQuadrature(2, 20)``.  Only the Normal distribution and the Exp scale transform are
    implemented; ``distribution_class`` / ``scale_transform`` may be the tfp objects of those names or None (the defaults)."""

    lik_id = B.LIK_HETERO
    lik_param = 0.0
    latent_dim = 2
    num_gauss_hermite_points = 20
    _CHUNK = 1 << 15  # rows per [rows, 20, 20] grid evaluation of the predictive helpers

    def __init__(self, distribution_class=None, scale_transform=None, **kwargs):
        if distribution_class is not None and not _named(distribution_class, "Normal"):
            raise NotImplementedError(f"HeteroskedasticTFPConditional: only the Normal distribution is implemented, got "
                                      f"{distribution_class!r}")
        if scale_transform is not None and not _named(scale_transform, "Exp"):
            raise NotImplementedError(f"HeteroskedasticTFPConditional: only the Exp scale transform is implemented, got "
                                      f"{scale_transform!r}")
        if kwargs:
            raise NotImplementedError(f"HeteroskedasticTFPConditional: unsupported arguments {sorted(kwargs)}")

    def _grid(self, Fmu, Fvar):
        """(f0 [N, 20, 1], f1 [N, 1, 20], log w_i + log w_j [20, 20]) of the product grid."""
        z, w = np.polynomial.hermite.hermgauss(self.num_gauss_hermite_points)
        z = torch.as_tensor(z * math.sqrt(2.0), dtype=Fmu.dtype, device=Fmu.device)
        logw = torch.as_tensor(np.log(w / math.sqrt(math.pi)), dtype=Fmu.dtype, device=Fmu.device)
        sd = torch.sqrt(Fvar)
        f0 = (Fmu[:, 0:1] + sd[:, 0:1] * z)[:, :, None]
        f1 = (Fmu[:, 1:2] + sd[:, 1:2] * z)[:, None, :]
        return f0, f1, logw[:, None] + logw[None, :]

    def _chunks(self, *arrays):
        n = arrays[0].shape[0]
        for lo in range(0, max(n, 1), self._CHUNK):
            yield tuple(a[lo:lo + self._CHUNK] for a in arrays)

    def predict_mean_and_var(self, Fmu, Fvar):
        """E[y] = E_q[f0], Var[y] = E_q[exp(2 f1) + f0^2] - E[y]^2 over the 400-point grid; [N, 1] each."""
        means, variances = [], []
        for mu, var in self._chunks(Fmu, Fvar):
            f0, f1, logw = self._grid(mu, var)
            w = torch.exp(logw)
            ey = torch.sum(w * f0, dim=(1, 2))
            ey2 = torch.sum(w * (torch.exp(2.0 * f1) + f0 * f0), dim=(1, 2))
            means.append(ey[:, None])
            variances.append((ey2 - ey * ey)[:, None])
        return torch.cat(means), torch.cat(variances)

    def predict_log_density(self, Fmu, Fvar, Y):
        """log sum_ij w_i w_j p(y | f0_i, f1_j), summed in log space over the 400-point grid; [N]."""
        out = []
        for mu, var, y in self._chunks(Fmu, Fvar, Y):
            f0, f1, logw = self._grid(mu, var)
            logp = -0.5 * math.log(2 * math.pi) - f1 - 0.5 * (y[:, :, None] - f0) ** 2 * torch.exp(-2.0 * f1)
            out.append(torch.logsumexp((logp + logw).reshape(mu.shape[0], -1), dim=1))
        return torch.cat(out)
