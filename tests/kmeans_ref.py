"""NumPy fp64 restatement of Lloyd's k-means as ``kmeans_inducing_points`` runs it (include/tsvgp_hip.h (12)), with the rounding
bound its distances are compared under.  Test infrastructure only: the package never imports it.

    il = 1 / lengthscales;   s(x, c) = sum_{q = 0 .. D-1} dd_q^2,   a = x_q il_q,  b = c_q il_q,  dd = a - b
    C = init
    for it = 1 .. max_iter:
        labels[n] = the lowest m with s(x_n, c_m) minimal;  inertia_it = sum_n min_m s
        if it > 1 and labels == previous labels: converged, stop        (C is already their mean)
        C_new[m] = mean of the rows labelled m (in original coordinates), or C[m] unchanged if none
        shift = max_m s(C_new[m], C[m]);  C = C_new
        if tol > 0 and shift <= tol^2: converged, stop
    if the loop did not end on unchanged labels: one more assignment, so labels / counts / inertia belong to the returned Z

The device adds the D squares with fused multiply-adds, NumPy rounds the square first: both stay within ``E`` of the exact s.
"""
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -53


def dist2(X, C, il):
    """s [N, M] and the rounding bound E [N, M] = 4 u ((D + 2) s + 2 sum_q |dd_q| (|a_q| + |b_q|)): the roundings of a, b and dd
    (each at most u (|a| + |b|) off in dd, carried through the square as 2 |dd| times that) plus the D accumulations."""
    X, C, il = (np.asarray(v, dtype=np.float64) for v in (X, C, il))
    N, D = X.shape
    A, Bc = X * il, C * il
    s = np.zeros((N, C.shape[0]))
    cross = np.zeros_like(s)
    for q in range(D):
        a, b = A[:, q:q + 1], Bc[None, :, q]
        dd = a - b
        s += dd * dd
        cross += np.abs(dd) * (np.abs(a) + np.abs(b))
    return s, 4.0 * U * ((D + 2) * s + 2.0 * cross)


def assign(X, C, il):
    """(labels [N] int64 -- the first, i.e. lowest, index of the minimum --, minimal s [N], second-best s [N] (+inf when M = 1),
    E [N, M])."""
    s, E = dist2(X, C, il)
    labels = np.argmin(s, axis=1)
    rows = np.arange(s.shape[0])
    best = s[rows, labels]
    rest = s.copy()
    rest[rows, labels] = np.inf
    return labels.astype(np.int64), best, rest.min(axis=1), E


def update(X, labels, C):
    """(C_new [M, D], counts [M]): the mean of each cluster's rows, in increasing row number; an empty one keeps its centre."""
    M = C.shape[0]
    counts = np.bincount(labels, minlength=M).astype(np.int64)
    C_new = np.array(C, dtype=np.float64, copy=True)
    for m in np.nonzero(counts)[0]:
        C_new[m] = X[labels == m].sum(axis=0) / counts[m]
    return C_new, counts


@dataclass
class Result:
    Z: np.ndarray
    labels: np.ndarray
    counts: np.ndarray
    inertia: float
    inertia_history: np.ndarray
    n_iter: int
    converged: bool
    min_gap: float  # the smallest (second best - best) / best any row saw in any assignment of the run


def lloyd(X, num_inducing, init="first", lengthscales=None, max_iter=25, tol=0.0):
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    M = int(num_inducing)
    il = 1.0 / (np.ones(D) if lengthscales is None else np.broadcast_to(np.asarray(lengthscales, dtype=np.float64), (D,)))
    C = X[:M].copy() if isinstance(init, str) else np.array(init, dtype=np.float64, copy=True)
    assert C.shape == (M, D)
    history, prev, counts, gap = [], None, None, np.inf
    converged = on_labels = False

    def step(C):
        nonlocal gap
        labels, best, second, _ = assign(X, C, il)
        ok = best > 0
        if M > 1 and ok.any():
            gap = min(gap, float(np.min((second[ok] - best[ok]) / best[ok])))
        return labels, float(best.sum())

    for it in range(1, int(max_iter) + 1):
        labels, inertia = step(C)
        history.append(inertia)
        if prev is not None and np.array_equal(labels, prev):
            converged = on_labels = True
            break
        prev = labels
        C_new, counts = update(X, labels, C)
        shift = float(dist2(C_new, C, il)[0].diagonal().max())
        C = C_new
        if tol > 0.0 and shift <= tol * tol:
            converged = True
            break
    if not on_labels:
        labels, inertia = step(C)
        counts = np.bincount(labels, minlength=M).astype(np.int64)
    return Result(C, labels, counts, inertia, np.asarray(history), it, converged, gap)


def blobs(seed, N=3000, K=6, D=3, sigma=0.5, spread=4.0):
    """Clustered data: K centres randn(K, D) * spread, N rows at sigma around centres drawn uniformly.  Returns (X, centres, which).
    With M = 12, init "first" and lengthscales (1.0, 0.7, 1.6), seeds 0 / 1 / 2 stop on unchanged labels in iteration
    15 / 21 / 11 (after 14 / 20 / 10 centre updates); the smallest relative gap between best and second best over a run is
    1.4e-5, the smallest final count 102."""
    rng = np.random.RandomState(seed)
    centres = rng.randn(K, D) * spread
    which = rng.randint(K, size=N)
    X = centres[which] + sigma * rng.randn(N, D)
    return X, centres, which
