"""NumPy fp64 restatement of the k-means++ seeding ``kmeanspp_seeds`` runs (include/tsvgp_hip.h (13)), on top of
``kmeans_ref.dist2`` and ``softmax_ref.philox4x32_10``, with the rounding bounds the device is compared under.  Test
infrastructure only: the package never imports it.

    L = n_local_trials, default 2 + floor(ln M)
    u(r, j) = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53,  (x0, x1, ., .) = Philox4x32-10((r, j, 0x6B2B2B, 0), (seed lo, seed hi))
    round 0:  i_0 = min(floor(u(0, 0) N), N - 1);  mind[n] = s(x_n, x_{i_0});  pot_0 = sum_n mind[n]
    round r:  for j < L:  t_j = u(r, j) pot_{r-1};  cand_j = the lowest n whose running sum of mind through n exceeds t_j;
                          newpot_j = sum_n min(mind[n], s(x_n, x_{cand_j}))
              j* = the lowest j of the minimum;  i_r = cand_{j*};  mind = min(mind, s(., x_{i_r}));  pot_r = newpot_{j*}

The inverse CDF is taken as "the HIGHEST n of positive mass whose running sum BEFORE n is <= t": with exact sums that is the
rule above; in floating point it can never return a row of zero mass, a t at or above the top of the sum falls to the last row
of positive mass, and with no mass at all the answer is N - 1.

Summation order.  The device adds mind per workgroup of ``rows`` consecutive rows (a lane's rows, a 64-lane butterfly, four
waves), adds the workgroups in 16 interleaved slots and a pairwise tree, and forms the running sum hierarchically (256 chunks
of consecutive workgroups scanned by Hillis-Steele, the workgroups of one chunk in order, the rows of one workgroup R per lane
and the same scan).  This file does not imitate that order: ``seed`` below adds with ``math.fsum`` and a sequential
``np.cumsum``, and the comparison is made under a bound that holds for ANY order.

The bound delta_r (``Forced.delta``).  Write mind_d for the device's values and mind for this file's.
  (a) Every computed s is within ``kmeans_ref.dist2``'s E of the exact s, on the device (fused multiply-adds) and here (rounded
      squares) alike, so two computed values of one s differ by at most 2 E, and because min is 1-Lipschitz in the sup norm,
      |mind_d[n] - mind[n]| <= e_n := 2 max_{i chosen} E[n, i].  (A row equal to a chosen row has a == b bit for bit on both
      sides: s = 0 = E exactly, so zero mass here is zero mass there.)
  (b) Every running sum the device compares with t is a floating-point sum, in some tree, of mind_d over a prefix of the rows
      (plus zeros).  A term passes at most N - 1 additions, so the computed value is within gamma_N * (sum of the prefix) of the
      exact sum of mind_d, gamma_k = k u / (1 - k u)  (Higham, Accuracy and Stability, section 4.2: any order).
  (c) So each such value is within  delta = sum_n e_n + gamma_N (sum_n mind[n] + sum_n e_n) + 2 u sum_n mind[n]  of the exact
      running sum ``cum`` of this file's mind at the same row (the last term: ``cum`` is exact, then rounded to fp64 once,
      and t = u(r, j) * pot is one rounded product of reported numbers, which the test repeats bit for bit).
  The device takes row n only if its sum before n is <= t (so cum[n-1] - delta <= t), and the next position of positive mass
  had a sum before it that is > t, or there was none and t <= pot_{r-1}, itself such a sum (so t <= cum[n] + delta).
  Trial potentials: |newpot_d - exact sum_n min(mind[n], s(x_n, x_cand))| <= sum_n eb_n + gamma_N (exact + sum_n eb_n),
  eb_n = max(e_n, 2 E[n, cand]), by (a) and (b).
"""
import math
from dataclasses import dataclass
from fractions import Fraction
from itertools import accumulate

import numpy as np

from tests import kmeans_ref as K
from tests import softmax_ref as S

U = 2.0 ** -53
STREAM = 0x6B2B2B
MAX_TRIALS = 16


def default_trials(M):
    return 2 + int(math.log(M))


def uniforms(seed, M, L):
    """u [M, L] fp64 in [0, 1): u[r, j] of the contract, every (r, j) -- also those no round uses."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = np.arange(M, dtype=np.uint64)[:, None] + np.zeros((1, L), np.uint64)
    j = np.arange(L, dtype=np.uint64)[None, :] + np.zeros((M, 1), np.uint64)
    x = S.philox4x32_10((r, j, np.full((M, L), STREAM, np.uint64), np.zeros((M, L), np.uint64)), (seed & 0xFFFFFFFF, seed >> 32))
    hi, lo = (x[0] >> np.uint64(5)).astype(np.float64), (x[1] >> np.uint64(6)).astype(np.float64)
    return (hi * 2.0 ** 26 + lo) * 2.0 ** -53


def inv_ls(D, lengthscales=None):
    return 1.0 / (np.ones(D) if lengthscales is None else np.broadcast_to(np.asarray(lengthscales, dtype=np.float64), (D,)))


def pick(mind, t):
    """The highest n of positive mass whose (sequential) running sum before n is <= t; N - 1 when there is no mass."""
    before = np.concatenate([[0.0], np.cumsum(mind)[:-1]])
    ok = np.nonzero((mind > 0.0) & (before <= t))[0]
    return int(ok[-1]) if ok.size else len(mind) - 1


@dataclass
class Seeding:
    indices: np.ndarray  # [M] int64
    dist: np.ndarray  # [N] final mind
    potential_history: np.ndarray  # [M]
    candidates: np.ndarray  # [M, L] int64, -1 where unused
    trial_potentials: np.ndarray  # [M, L], +inf where unused
    uniforms: np.ndarray  # [M, L], 0 where unused


def seed(X, num_inducing, lengthscales=None, seed=0, n_local_trials=None, uniform=None):
    """Free-running mode.  ``uniform``: an [M, L] array that replaces the generator's (for tests of the sampling rule alone)."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    M = int(num_inducing)
    L = default_trials(M) if n_local_trials is None else int(n_local_trials)
    assert 1 <= M <= N and 1 <= L <= MAX_TRIALS
    il = inv_ls(D, lengthscales)
    u = uniforms(seed, M, L) if uniform is None else np.asarray(uniform, dtype=np.float64)
    cand = np.full((M, L), -1, np.int64)
    cpot = np.full((M, L), np.inf)
    used = np.zeros((M, L))
    indices, hist = np.zeros(M, np.int64), np.zeros(M)
    i0 = min(int(math.floor(u[0, 0] * N)), N - 1)
    mind = K.dist2(X, X[i0:i0 + 1], il)[0][:, 0]
    indices[0], hist[0] = i0, math.fsum(mind)
    cand[0, 0], cpot[0, 0], used[0, 0] = i0, hist[0], u[0, 0]
    for r in range(1, M):
        used[r] = u[r]
        for j in range(L):
            cand[r, j] = pick(mind, u[r, j] * hist[r - 1])
        trial = np.minimum(mind[:, None], K.dist2(X, X[cand[r]], il)[0])  # [N, L]
        cpot[r] = [math.fsum(trial[:, j]) for j in range(L)]
        js = int(np.argmin(cpot[r]))  # the first, i.e. lowest, index of the minimum
        indices[r], hist[r], mind = cand[r, js], cpot[r, js], trial[:, js]
    return Seeding(indices, mind, hist, cand, cpot, used)


def gamma(k):
    return k * U / (1.0 - k * U)


@dataclass
class Forced:
    mind: np.ndarray  # [N] this file's mind after the chosen rows
    e: np.ndarray  # [N] the bound (a) on |device mind - mind|
    cum: np.ndarray  # [N] the exact running sum of mind, rounded to fp64 once
    pot: float  # math.fsum(mind)
    delta: float  # the bound (c)
    trial: np.ndarray  # [len(cands)] exact sum_n min(mind[n], s(x_n, x_cand)); empty without cands
    trial_bound: np.ndarray  # its bound


def forced(X, lengthscales, chosen, cands=()):
    """Teacher-forced mode: the state after the rows ``chosen`` (the device's indices[:r], r >= 0; none: mind = +inf) and, for
    each row in ``cands``, the potential it would leave with its bound."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    il = inv_ls(D, lengthscales)
    chosen = np.asarray(chosen, np.int64)
    if chosen.size:
        s, E = K.dist2(X, X[chosen], il)
        mind, e = s.min(axis=1), 2.0 * E.max(axis=1)
        exact = list(accumulate(map(Fraction, mind.tolist())))
        cum = np.array([float(c) for c in exact])
        pot = float(exact[-1])
        se = math.fsum(e)
        delta = se + gamma(N) * (pot + se) + 2.0 * U * pot
    else:
        mind, e = np.full(N, np.inf), np.zeros(N)
        cum, pot, delta = np.full(N, np.inf), np.inf, np.inf
    cands = np.asarray(cands, np.int64)
    trial, bound = np.zeros(len(cands)), np.zeros(len(cands))
    if cands.size:
        s, E = K.dist2(X, X[cands], il)
        for j in range(len(cands)):
            trial[j] = math.fsum(np.minimum(mind, s[:, j]))
            eb = math.fsum(np.maximum(e, 2.0 * E[:, j]))
            bound[j] = eb + gamma(N) * (trial[j] + eb)
    return Forced(mind, e, cum, pot, delta, trial, bound)


def sorted_blobs(seed):
    """``kmeans_ref.blobs(seed)`` with the first row's blob moved to the front (a stable sort), so X[:12] sits in one cluster
    and Lloyd's iterations from init "first" end far from the optimum."""
    X, _, which = K.blobs(seed)
    order = np.argsort(which != which[0], kind="stable")
    return X[order]
