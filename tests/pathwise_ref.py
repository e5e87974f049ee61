"""NumPy fp64 restatement of the pathwise function draws (t-svgp_amd/pathwise.py, ``tsvgp_pathwise_f64``): the spectral draws,
the random features, the evaluation and the sampler that turns q(u) = N(m, S) into the operands of the evaluation, with the
random numbers laid out as the product lays them out (``tests/softmax_ref.py::normals`` restates the generator).

    g_s(x) = sqrt(variance / L) sum_l (w_s[l] cos(Omega_l . x~) + w_s[L + l] sin(Omega_l . x~)),    x~ = x * inv_ls
    f_s(x) = g_s(x) + sum_m k(x, z_m) V[s, m],    V_s = K6^-1 (u_s - g_s(Z)),    u_s = m + chol(S) eps_s

Generator draw 4 * draw + j: j = 0 the normals E [L, D] behind Omega (sample 0, rows p L + l), j = 1 the chi-square normals of the
Matern kernels (same rows, columns 0 .. 2 nu - 1), j = 2 the weights w [S, 2 L, P], j = 3 eps [S, M, P].
"""
import functools

import numpy as np

from tests import softmax_ref

SE, MATERN32, MATERN52 = 0, 2, 3
CHI2_NORMALS = {MATERN32: 3, MATERN52: 5}  # 2 nu


@functools.lru_cache(maxsize=2)
def normals(seed, gdraw, nrows, S, C):
    """``softmax_ref.normals`` for rows 0 .. nrows - 1, [S, nrows, C], taken in blocks of rows (the restated generator works on
    whole uint64 arrays: S = 4096 samples of 8192 rows at once would need gigabytes) and kept for the tests that share a draw.
    Read-only."""
    step = max(1, (1 << 20) // max(1, S * ((C + 3) // 4)))
    out = np.concatenate([softmax_ref.normals(seed, gdraw, np.arange(r, min(r + step, nrows)), S, C)
                          for r in range(0, nrows, step)], axis=1)
    out.setflags(write=False)
    return out


def profile(kind, s):
    """k(s) / variance as a function of the scaled squared distance (GPflow [ext]: Matern kernels take r = sqrt(max(s, 1e-36)))."""
    if kind == SE:
        return np.exp(-0.5 * s)
    r = np.sqrt(np.maximum(s, 1e-36))
    if kind == MATERN32:
        a = np.sqrt(3.0) * r
        return (1.0 + a) * np.exp(-a)
    if kind == MATERN52:
        a = np.sqrt(5.0) * r
        return (1.0 + a + 5.0 / 3.0 * r * r) * np.exp(-a)
    raise ValueError(f"kind {kind}")


def kernel_matrix(kind, X, Z, inv_ls, variance):
    """variance * k(r(x_n, z_m)), r^2 in the difference form on the scaled inputs (the form of the HIP fill)."""
    d = (np.asarray(X, np.float64) * inv_ls)[:, None, :] - (np.asarray(Z, np.float64) * inv_ls)[None, :, :]
    return variance * profile(kind, np.sum(d * d, axis=-1))


def spectral(kind, seed, draw, L, D, p=0):
    """Omega [L, D] of latent kernel p: E for the squared exponential, E_l sqrt(2 nu / chi2_l) for Matern-nu."""
    rows = p * L + np.arange(L)
    E = softmax_ref.normals(seed, 4 * draw, rows, 1, D)[0]
    if kind == SE:
        return E
    nu2 = CHI2_NORMALS[kind]
    c = softmax_ref.normals(seed, 4 * draw + 1, rows, 1, nu2)[0]
    return E * np.sqrt(nu2 / np.sum(c * c, axis=1))[:, None]


def features(X, inv_ls, Omega):
    """[N, 2 L]: cos(Omega_l . x~_n) in the first L columns, sin in the last L."""
    arg = (np.asarray(X, np.float64) * inv_ls) @ np.asarray(Omega, np.float64).T
    return np.concatenate([np.cos(arg), np.sin(arg)], axis=1)


def evaluate(kind, X, Z, inv_ls, variance, Omega, W, V):
    """out [S, N] of ``tsvgp_pathwise_f64``: W [S, 2 L] already scaled by sqrt(variance / L); V [S, M] or None (M = 0)."""
    out = np.asarray(W, np.float64) @ features(X, inv_ls, Omega).T
    if V is not None and np.shape(V)[1] > 0:
        out = out + np.asarray(V, np.float64) @ kernel_matrix(kind, X, Z, inv_ls, variance).T
    return out


def magnitude(kind, X, Z, inv_ls, variance, Omega, W, V):
    """A [S, N] = sum_l (|W[s, l]| + |W[s, L + l]|)(1 + sum_d |Omega_ld x~_nd|) + sum_m |V[s, m]| k(x_n, z_m): what the rounding
    errors of ``evaluate``'s summands scale with (the argument's rounding moves a sine or cosine by eps sum_d |Omega_ld x~_nd|)."""
    L = np.shape(Omega)[0]
    W = np.abs(np.asarray(W, np.float64))
    amp = 1.0 + np.abs(np.asarray(X, np.float64) * inv_ls) @ np.abs(np.asarray(Omega, np.float64)).T  # [N, L]
    A = (W[:, :L] + W[:, L:]) @ amp.T
    if V is not None and np.shape(V)[1] > 0:
        A = A + np.abs(np.asarray(V, np.float64)) @ kernel_matrix(kind, X, Z, inv_ls, variance).T
    return A


def sampler(m, cholS, K6, kinds, Z, inv_ls, variances, seed, draw, L, S, shared=True):
    """The operands of S draws of P latent functions from q(u) = N(m, S): m [M, P], cholS [P, M, M], K6 [M, M] (one kernel for
    every latent, ``shared``) or [P, M, M]; kinds, inv_ls ([D] each), variances: one entry per latent (P equal entries when shared).
    Returns dict(Omega [P, L, D], W [P, S, 2 L] (scaled), V [P, S, M], u [S, M, P], w, eps): latent p evaluates as
    ``evaluate(kinds[p], X, Z, inv_ls[p], variances[p], Omega[p], W[p], V[p])``."""
    m, cholS, K6 = np.asarray(m, np.float64), np.asarray(cholS, np.float64), np.asarray(K6, np.float64)
    M, P = m.shape
    D = np.shape(Z)[1]
    w = normals(seed, 4 * draw + 2, 2 * L, S, P)  # [S, 2 L, P]
    eps = normals(seed, 4 * draw + 3, M, S, P)  # [S, M, P]
    u = m[None] + np.einsum("pmk,skp->smp", cholS, eps)
    Omega, W, V = [], [], []
    for p in range(P):
        Omega.append(spectral(kinds[p], seed, draw, L, D, 0 if shared else p))
        W.append(w[:, :, p] * np.sqrt(variances[p] / L))
        gZ = evaluate(kinds[p], Z, None, inv_ls[p], variances[p], Omega[p], W[p], None)  # [S, M]
        V.append(np.linalg.solve(K6 if K6.ndim == 2 else K6[p], (u[:, :, p] - gZ).T).T)
    return dict(Omega=np.stack(Omega), W=np.stack(W), V=np.stack(V), u=u, w=w, eps=eps)


def sample(ops, kinds, X, Z, inv_ls, variances):
    """[S, N, P]: the draws of ``sampler`` at the rows of X."""
    return np.stack([evaluate(kinds[p], X, Z, inv_ls[p], variances[p], ops["Omega"][p], ops["W"][p], ops["V"][p])
                     for p in range(len(kinds))], axis=2)
