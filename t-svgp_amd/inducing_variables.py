"""``gpflow.inducing_variables.InducingPoints`` / ``inducingpoint_wrapper`` mirror (reference tsvgp.py:22,150)."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from ._backend import KMEANSPP_MAX_TRIALS
from .base import Parameter, to_tensor
from .estep import MAX_INPUT_DIM, EStepEngine
from .kernels import LinearCoregionalization, SeparateIndependent, refuse_sum


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
    refuse_sum(kernel, "select_inducing_points")
    if isinstance(kernel, LinearCoregionalization):
        raise NotImplementedError("select_inducing_points does not take LinearCoregionalization: one kernel defines one conditional "
                                  "variance; pass the kernel of the latent you mean")
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


def _rows_and_count(name, X, num_inducing, lengthscales):
    """The checks of X and num_inducing the k-means functions share: (X, N, D, M)."""
    if isinstance(lengthscales, SeparateIndependent):
        raise ValueError(f"{name}: SeparateIndependent holds one kernel per latent; pass the lengthscales of the latent you mean")
    if isinstance(X, Parameter):
        X = X.value
    if not hasattr(X, "shape"):
        X = np.asarray(X, dtype=np.float64)
    shape = tuple(X.shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{name}: X must be a non-empty [N, D] array, got shape {shape}")
    N, D = shape
    if D > MAX_INPUT_DIM:
        raise ValueError(f"{name}: at most {MAX_INPUT_DIM} input columns, got {D}")
    if isinstance(num_inducing, bool) or int(num_inducing) != num_inducing or not 1 <= int(num_inducing) <= N:
        raise ValueError(f"{name}: num_inducing must be an integer in [1, N = {N}], got {num_inducing}")
    return X, N, D, int(num_inducing)


def _lengthscales(name, lengthscales, D):
    """None, a scalar or [D], finite and > 0, as a NumPy [D]."""
    if lengthscales is None:
        return np.ones(D)
    if isinstance(lengthscales, Parameter):
        lengthscales = lengthscales.value
    if isinstance(lengthscales, torch.Tensor):
        lengthscales = lengthscales.detach().cpu().numpy()
    ls = np.asarray(lengthscales, dtype=np.float64)
    if ls.ndim == 0:
        ls = np.full(D, float(ls))
    if ls.shape != (D,):
        raise ValueError(f"{name}: lengthscales must be None, a scalar or [{D}], got shape {ls.shape}")
    if not np.all(np.isfinite(ls)) or not np.all(ls > 0.0):
        raise ValueError(f"{name}: lengthscales must be finite and > 0, got {ls}")
    return ls


def _trials(name, n_local_trials, M):
    """n_local_trials: None = scikit-learn's 2 + floor(ln M), else an integer in [1, KMEANSPP_MAX_TRIALS]."""
    if n_local_trials is None:
        return min(2 + int(math.log(M)), KMEANSPP_MAX_TRIALS)
    if isinstance(n_local_trials, bool) or int(n_local_trials) != n_local_trials or not 1 <= int(n_local_trials) <= KMEANSPP_MAX_TRIALS:
        raise ValueError(f"{name}: n_local_trials must be None or an integer in [1, {KMEANSPP_MAX_TRIALS}], got {n_local_trials}")
    return int(n_local_trials)


def _seed(name, seed):
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 63:
        raise ValueError(f"{name}: seed must be an integer in [0, 2^63), got {seed}")
    return int(seed)


@dataclass
class KMeansSeeding:
    """What ``kmeanspp_seeds`` returns (tensors on the device the seeding ran on)."""

    Z: torch.Tensor  # [M, D] = X[indices]: feeds kmeans_inducing_points(init=...), the model constructors and InducingPoints
    indices: torch.Tensor  # [M] int64 row numbers into X, in the order chosen
    dist: torch.Tensor  # [N] scaled squared distance of each row to the nearest seed (0 at the seeds and their duplicates)
    potential: torch.Tensor  # 0-dim: the sum of ``dist`` = potential_history[-1]
    potential_history: torch.Tensor  # [M] the potential after each centre, non-increasing
    candidates: torch.Tensor  # [M, L] int64: the rows each round drew (row 0: the first centre in column 0; -1 where unused)
    trial_potentials: torch.Tensor  # [M, L] the potential each candidate would leave (+inf where unused); the lowest won
    uniforms: torch.Tensor  # [M, L] the uniform behind each candidate (0 where unused)
    seed: int
    n_local_trials: int


def kmeanspp_seeds(X, num_inducing, *, lengthscales=None, seed=0, n_local_trials=None, device=None) -> KMeansSeeding:
    """k-means++ seeding (Arthur and Vassilvitskii 2007) as scikit-learn's ``KMeans`` runs it by default: ``num_inducing`` rows
    of X, the first uniform, every later one drawn with probability proportional to its scaled squared distance to the nearest
    row already taken, the best of ``n_local_trials`` draws kept (None = 2 + floor(ln M), at most 16).  It needs no kernel and
    no N x M array, and it is the start ``kmeans_inducing_points(init="k-means++")`` runs Lloyd's iterations from.

    Random, but a pure function of (X, lengthscales, seed, n_local_trials): the uniforms come from the package's counter-based
    generator (Philox4x32-10), every sum has a fixed order, and two calls agree bit for bit.  ``lengthscales`` as in
    ``kmeans_inducing_points``.  With fewer than M distinct rows the call still returns M rows (duplicates, the potential 0).

    Runs on the ROCm device through ``EStepEngine.kmeanspp`` (one call, two launches per centre, X read once per centre);
    there is no CPU fallback.  X must be finite: that is checked once on the device (the one host read of the call)."""
    name = "kmeanspp_seeds"
    X, N, D, M = _rows_and_count(name, X, num_inducing, lengthscales)
    ls = _lengthscales(name, lengthscales, D)
    seed, L = _seed(name, seed), _trials(name, n_local_trials, M)
    engine = EStepEngine(torch.float64, device)
    dev = engine.device
    Xd = (X.to(dev) if isinstance(X, torch.Tensor) else to_tensor(X, device=dev)).to(torch.float64).contiguous()
    return _kmeanspp(name, engine, Xd, 1.0 / to_tensor(ls, device=dev).to(torch.float64), M, L, seed)


def _kmeanspp(name, engine, Xd, il, M, L, seed) -> KMeansSeeding:
    if not bool(torch.isfinite(Xd).all()):
        raise ValueError(f"{name}: X must be finite for k-means++ seeding (a NaN or an infinite entry has no distance)")
    indices, dist, pot_hist, cand, cand_pot, unif = engine.kmeanspp(Xd, il, M, L, seed)
    return KMeansSeeding(Z=Xd[indices], indices=indices, dist=dist, potential=pot_hist[M - 1].clone(), potential_history=pot_hist,
                         candidates=cand, trial_potentials=cand_pot, uniforms=unif, seed=seed, n_local_trials=L)


@dataclass
class KMeansInducing:
    """What ``kmeans_inducing_points`` returns (tensors on the device the clustering ran on)."""

    Z: torch.Tensor  # [M, D] fp64 cluster centres in the original coordinates: feeds the model constructors and InducingPoints
    labels: torch.Tensor  # [N] int64: the centre of Z nearest to each row (the lowest index on equal distances)
    counts: torch.Tensor  # [M] int64 rows per centre; 0 for a centre that lost all its rows (it stays where it was)
    inertia: torch.Tensor  # 0-dim: sum of the scaled squared distances of ``labels`` to ``Z``
    inertia_history: torch.Tensor  # [n_iter] the inertia each iteration's assignment found, non-increasing
    n_iter: int  # iterations run
    converged: bool  # the labels stopped changing (or the centres moved by at most ``tol``) within ``max_iter``
    # the KMeansSeeding the run started from (init="k-means++" or a KMeansSeeding), else None.  A plain attribute, set on the
    # result, not a dataclass field: the seven fields above, their order and the positional constructor stay what they were
    seeding = None


def kmeans_inducing_points(X, num_inducing, *, init="first", lengthscales=None, max_iter=25, tol=0.0, seed=None,
                           n_local_trials=None, device=None) -> KMeansInducing:
    """Lloyd's k-means cluster centres of X as inducing points -- the usual initialisation of sparse GPs, the reference drivers'
    ``KMeans(n_clusters=M).fit(X).cluster_centers_``.  It needs no kernel, returns centres that are not rows of X, and minimises
    the quantisation error the Nystrom residual grows from; ``select_inducing_points`` is the other standard choice, and its
    result is a good start for this one.

    Two calls agree bit for bit.  ``init`` is ``"first"`` (X[:M], the reference's own initialisation), an [M, D] array of
    starting centres, an ``InducingSelection`` (its Z; ``count`` must be M), ``"k-means++"`` (``kmeanspp_seeds`` with ``seed``,
    default 0, and ``n_local_trials``: scikit-learn's default start, and the one that needs no kernel) or a ``KMeansSeeding``
    made for this M; the last two leave the seeding in the result's ``seeding``.  ``seed`` and ``n_local_trials`` with any
    other ``init`` are an error; without them nothing is drawn.  ``lengthscales`` (None = ones, a scalar or [D]) are the
    kernel's: distances are taken in the coordinates it sees, x / l, and the centres are returned in the original ones.  With il = 1 / l and s(x, c) = sum_q ((x_q il_q) - (c_q il_q))^2:

        C = init
        for it = 1 .. max_iter:
            labels[n] = the lowest m with s(x_n, c_m) minimal;  inertia_it = sum_n min_m s
            if it > 1 and labels == previous labels: converged, stop        (C is already their mean)
            C_new[m] = mean of the rows labelled m, or C[m] unchanged if none        (an empty cluster keeps its centre)
            shift = max_m s(C_new[m], C[m]);  C = C_new
            if tol > 0 and shift <= tol^2: converged, stop
        if the loop did not end on unchanged labels: one more assignment, so labels / counts / inertia belong to the returned Z

    Runs on the ROCm device (X is moved there; ``device`` picks one) through ``EStepEngine.kmeans_assign`` and
    ``kmeans_update``; there is no CPU fallback.  The arithmetic is fp64 whatever X is.  One scalar goes to the host per
    iteration (did any label change); no N x M array exists at any point.  Out of scope: more than 32 input columns, fp32
    arithmetic, relocating empty clusters, mini-batches, and a row-sharded X -- a sharded caller clusters on one rank or on a
    subsample."""
    name = "kmeans_inducing_points"
    X, N, D, M = _rows_and_count(name, X, num_inducing, lengthscales)
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError(f"{name}: max_iter must be an integer >= 1, got {max_iter}")
    tol = float(tol)
    if not tol >= 0.0 or tol == float("inf"):
        raise ValueError(f"{name}: tol must be finite and >= 0, got {tol}")
    ls = _lengthscales(name, lengthscales, D)
    plusplus = isinstance(init, str) and init == "k-means++"
    if not plusplus and (seed is not None or n_local_trials is not None):
        raise ValueError(f"{name}: seed and n_local_trials belong to init='k-means++', not to the init given")
    if plusplus:
        seed, trials = _seed(name, 0 if seed is None else seed), _trials(name, n_local_trials, M)
    start, seeding = None, None
    if isinstance(init, KMeansSeeding):
        if tuple(init.indices.shape) != (M,) or tuple(init.Z.shape) != (M, D):
            raise ValueError(f"{name}: init holds {tuple(init.indices.shape)[0]} rows of shape {tuple(init.Z.shape)}, num_inducing = "
                             f"{M} rows of {D} columns are needed (the seeding was made for another M)")
        start, seeding = init.Z, init
    elif isinstance(init, InducingSelection):
        if init.count != M or tuple(init.Z.shape) != (M, D):
            raise ValueError(f"{name}: init holds {init.count} rows of shape {tuple(init.Z.shape)}, num_inducing = {M} rows of "
                             f"{D} columns are needed (the selection stopped early, or it was made for another M)")
        start = init.Z
    elif isinstance(init, str):
        if init != "first" and not plusplus:
            raise ValueError(f"{name}: init must be 'first', 'k-means++', an [M, D] array, an InducingSelection or a "
                             f"KMeansSeeding, got {init!r}")
    else:
        start = init.value if isinstance(init, Parameter) else init
        if not hasattr(start, "shape"):
            start = np.asarray(start, dtype=np.float64)
        if tuple(start.shape) != (M, D):
            raise ValueError(f"{name}: init must have shape ({M}, {D}), got {tuple(start.shape)}")
    engine = EStepEngine(torch.float64, device)
    dev = engine.device
    Xd = (X.to(dev) if isinstance(X, torch.Tensor) else to_tensor(X, device=dev)).to(torch.float64).contiguous()
    il = 1.0 / to_tensor(ls, device=dev).to(torch.float64)
    if plusplus:
        seeding = _kmeanspp(name, engine, Xd, il, M, trials, seed)
        start = seeding.Z
    if start is None:
        C = Xd[:M].clone()
    else:
        C = (start.detach().to(dev) if isinstance(start, torch.Tensor) else to_tensor(start, device=dev)).to(torch.float64).contiguous()
    history, prev, counts = [], None, None
    converged, on_labels = False, False
    for it in range(1, int(max_iter) + 1):
        labels, dist, inertia = engine.kmeans_assign(Xd, C, il)
        history.append(inertia)
        if prev is not None and torch.equal(labels, prev):  # the iteration's one host read
            converged = on_labels = True
            break
        prev = labels
        C_new, counts = engine.kmeans_update(Xd, labels, C)
        if tol > 0.0:
            dd = C_new * il - C * il
            shift = float((dd * dd).sum(dim=1).max())
        C = C_new
        if tol > 0.0 and shift <= tol * tol:
            converged = True
            break
    if not on_labels:
        labels, dist, inertia = engine.kmeans_assign(Xd, C, il)
        counts = torch.bincount(labels, minlength=M)
    res = KMeansInducing(Z=C, labels=labels.to(torch.int64), counts=counts.to(torch.int64), inertia=inertia,
                         inertia_history=torch.stack(history), n_iter=it, converged=converged)
    res.seeding = seeding
    return res
