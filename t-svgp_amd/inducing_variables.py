"""``gpflow.inducing_variables.InducingPoints`` / ``inducingpoint_wrapper`` mirror (reference tsvgp.py:22,150)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .base import Parameter, to_tensor
from .estep import MAX_INPUT_DIM, EStepEngine
from .kernels import SeparateIndependent


class InducingPoints:
    def __init__(self, Z, name=None):
        self.Z = Parameter(Z)
        if self.Z.value.dim() != 2:
            raise ValueError("InducingPoints expects Z of shape [M, D]")
        self.name = name

    @property
    def num_inducing(self) -> int:
        return self.Z.shape[0]

    def __len__(self):
        return self.num_inducing


class SharedIndependentInducingVariables:
    """``gpflow.inducing_variables.SharedIndependentInducingVariables`` [ext]: one set of inducing points shared by
    all latent GPs (reference docs/notebooks/heteroskedastic.py:72-74; special-cased at tsvgp.py:249-252)."""

    def __init__(self, inducing_variable, name=None):
        self.inducing_variable = inducingpoint_wrapper(inducing_variable)
        self.inducing_variables = [self.inducing_variable]  # the attribute tsvgp.py:252 reads
        self.name = name

    @property
    def Z(self):
        return self.inducing_variable.Z

    @property
    def num_inducing(self) -> int:
        return self.inducing_variable.num_inducing

    def __len__(self):
        return self.num_inducing


def inducingpoint_wrapper(inducing_variable):
    """Accepts an InducingPoints (or shared multi-output wrapper) or a raw [M, D] array
    (reference docs/notebooks/regression_1D.py:79-84)."""
    if isinstance(inducing_variable, (InducingPoints, SharedIndependentInducingVariables)):
        return inducing_variable
    return InducingPoints(inducing_variable)


@dataclass
class InducingSelection:
    """What ``select_inducing_points`` returns (tensors on the device the selection ran on)."""

    Z: torch.Tensor  # [count, D] the chosen rows of X, in the order they were taken: feeds the model constructors and InducingPoints
    indices: torch.Tensor  # [count] int64 row numbers into X
    pivots: torch.Tensor  # [count] residual variance of each row when it was taken = squared diagonal of chol K(Z, Z), non-increasing
    residual: torch.Tensor  # [N] diag(K_ff - K_fZ K_ZZ^-1 K_Zf), exactly 0 at the chosen rows
    trace: torch.Tensor  # 0-dim: residual.sum() = tr(K_ff - Q_ff), the gap the sparse bound can lose to the exact one
    count: int  # rows taken: < num_inducing when the residual fell to the threshold first (or X ran out of distinct rows)


def select_inducing_points(X, kernel, num_inducing, *, threshold=0.0, device=None) -> InducingSelection:
    """Greedy conditional-variance choice of ``num_inducing`` rows of X as inducing points (Burt, Rasmussen, van der Wilk 2020,
    "ConditionalVariance"): pivoted Cholesky of K(X, X) that always takes the row with the largest remaining prior variance
    given the rows taken so far.  Deterministic: no seed, the lowest row number wins ties (so row 0 is always first).

    It stops early, with ``count < num_inducing`` and a shorter Z, once no residual variance exceeds
    ``max(threshold, 1e-12 * variance)`` -- duplicates of a taken row are never taken.  The pivots bound the conditioning of
    K(Z, Z) the route gates of t_SVGP_white / t_SVGP_sites look at (cond >= pivots[0] / pivots[-1]); ``trace`` bounds what the
    sparse ELBO can lose to the exact one.

    Runs on the ROCm device (X is moved there; ``device`` picks one) through ``EStepEngine.greedy_select``; there is no CPU
    fallback.  The factor it builds takes 8 * num_inducing * N bytes of device memory for the length of the call.
    Out of scope: fp32 arithmetic (the selection is fp64 whatever X is), more than 32 input columns, and a row-sharded X -- a
    global argmax would cost one collective per step; a sharded caller selects on one rank from its shard or from a subsample.
    ``SeparateIndependent`` is refused: one kernel defines one conditional variance, so pass the latent's kernel you mean."""
    if isinstance(kernel, SeparateIndependent):
        raise ValueError("select_inducing_points: SeparateIndependent holds one kernel per latent and one kernel defines one "
                         "conditional variance; pass the kernel of the latent you mean")
    if not hasattr(X, "shape"):
        X = np.asarray(X, dtype=np.float64)
    shape = tuple(X.shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"select_inducing_points: X must be a non-empty [N, D] array, got shape {shape}")
    if shape[1] > MAX_INPUT_DIM:
        raise ValueError(f"select_inducing_points: at most {MAX_INPUT_DIM} input columns, got {shape[1]}")
    if int(num_inducing) != num_inducing or int(num_inducing) < 1:
        raise ValueError(f"select_inducing_points: num_inducing must be an integer >= 1, got {num_inducing}")
    threshold = float(threshold)
    if not threshold >= 0.0 or threshold == float("inf"):
        raise ValueError(f"select_inducing_points: threshold must be finite and >= 0, got {threshold}")
    engine = EStepEngine(torch.float64, device)
    if isinstance(X, Parameter):
        X = X.value
    Xd = X.to(engine.device) if isinstance(X, torch.Tensor) else to_tensor(X, device=engine.device)
    indices, pivots, residual, count = engine.greedy_select(Xd, kernel, int(num_inducing), threshold)
    return InducingSelection(Z=Xd[indices], indices=indices, pivots=pivots, residual=residual, trace=residual.sum(), count=count)
