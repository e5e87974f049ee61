"""Gaussian exponential-family site containers (mirror of reference src/sites.py).

``DenseSites`` is the state the E-step mutates: lambda_1 [M, P] and the Cholesky-like factor of Lambda_2,
``lambda_2_sqrt`` [P, M, M], kept lower-triangular (the reference stores it under GPflow's ``triangular()``
transform, src/sites.py:63).  Note the reference's sign convention: the factor has a NEGATIVE diagonal
(src/models/tsvgp.py:176-179,300).
"""
from __future__ import annotations

import torch

from .base import Parameter, to_tensor


class Sites:
    """The base sites class (reference src/sites.py:14-23)."""

    def __init__(self, name=None):
        self.name = name


class DenseSites(Sites):
    """Sites with dense lambda_2 saved as a Cholesky factor (reference src/sites.py:43-80)."""

    def __init__(self, lambda_1, lambda_2_sqrt=None, lambda_2=None, name=None):
        super().__init__(name=name)
        self.lambda_1 = Parameter(lambda_1, trainable=False)  # [M, P]
        self.num_latent_gps = self.lambda_1.shape[0]  # sic, as reference src/sites.py:57
        assert (lambda_2_sqrt is not None) or (lambda_2 is not None)
        if lambda_2_sqrt is not None:
            self.factor = True
            self._lambda_2_sqrt = Parameter(torch.tril(to_tensor(lambda_2_sqrt)), trainable=False)  # [P, M, M]
        else:
            self.factor = False
            self._lambda_2 = Parameter(lambda_2, trainable=False)  # [P, M, M]

    @property
    def lambda_2(self) -> torch.Tensor:
        """second natural parameter"""
        if self.factor:
            L = self._lambda_2_sqrt.value
            return L @ L.transpose(-1, -2)
        return self._lambda_2.value

    @property
    def lambda_2_sqrt(self):
        """Cholesky factor of the second natural parameter (a Parameter when stored as a factor)."""
        if self.factor:
            return self._lambda_2_sqrt
        return Parameter(torch.linalg.cholesky(self._lambda_2.value), trainable=False)

    def assign_lambda_2(self, value):
        """Full second natural parameter (the whitened model's state, reference src/models/tsvgp_white.py:248)."""
        if self.factor:
            raise ValueError("sites are stored as a Cholesky factor")
        self._lambda_2.assign(value)

    def assign_lambda_2_sqrt(self, value, lower_and_owned: bool = False):
        """triangular() transform: only the lower triangle is kept (reference src/sites.py:63).
        ``lower_and_owned``: ``value`` is a fresh tensor with exact zeros above the diagonal (a factor straight out of the
        factorisation): adopted without the triangle pass and the copy."""
        if not self.factor:
            raise ValueError("sites are stored as a full lambda_2")
        if lower_and_owned and isinstance(value, torch.Tensor):
            self._lambda_2_sqrt.assign_owned(value)
        else:
            self._lambda_2_sqrt.assign(torch.tril(to_tensor(value, device=self._lambda_2_sqrt.device)))


class DiagSites(Sites):
    """Sites with diagonal lambda_2 (reference src/sites.py:25-40): one pair lambda_1, lambda_2 [N, P] per datum, the state of
    ``t_SVGP_sites``.  Deviation: the reference keeps lambda_2 under GPflow's ``positive()`` (softplus) transform; the value
    itself is stored here, as ``DenseSites`` does (the softplus round trip moves it by about one ulp).

    Both parameters are views of one zero-padded fp64 buffer [2, Np, P] (Np = N rounded up to 128) that the HIP site step
    updates in place and the projection reads as its weights; ``padded()`` hands it out, re-binding a parameter that was
    replaced through ``assign`` first."""

    def __init__(self, lambda_1, lambda_2, name=None, device=None, pad=128):
        super().__init__(name=name)
        self.lambda_1 = Parameter(lambda_1, trainable=False, device=device)  # [N, P]
        self.lambda_2 = Parameter(lambda_2, trainable=False, device=device)  # [N, P]
        if self.lambda_1.shape != self.lambda_2.shape or len(self.lambda_1.shape) != 2:
            raise ValueError(f"lambda_1, lambda_2 must both be [N, P], got {self.lambda_1.shape} and {self.lambda_2.shape}")
        N, P = self.lambda_1.shape
        self._store = torch.zeros((2, -(-N // pad) * pad, P), dtype=torch.float64, device=self.lambda_1.device)
        self._bind()

    def _bind(self):
        N = self.lambda_1.shape[0]
        for k, par in enumerate((self.lambda_1, self.lambda_2)):
            if par.value.data_ptr() != self._store[k].data_ptr():
                self._store[k, :N].copy_(par.value)
                par.assign_owned(self._store[k, :N])

    def padded(self):
        """(lambda_1, lambda_2) as [Np, P] fp64 views of the padded buffer (rows >= N zero)."""
        self._bind()
        return self._store[0], self._store[1]
