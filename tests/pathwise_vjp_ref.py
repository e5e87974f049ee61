"""NumPy restatement of the vector-Jacobian product of the pathwise function draws (``tsvgp_pathwise_vjp_f64``,
``FunctionSamples.vjp``), on top of tests/pathwise_ref.py.  With cotangents C [S, N] on ``pathwise_ref.evaluate``'s output,

    dX[n, d] = sum_s C[s, n] d f_s(x_n) / d x_nd
             = inv_ls_d (  sum_l Omega[l, d] ( cos(a_nl) sum_s C[s, n] W[s, L + l] - sin(a_nl) sum_s C[s, n] W[s, l] )
                         + sum_m 2 (x~_nd - z~_md) variance f'(s2_nm) sum_s C[s, n] V[s, m] ),
    a_nl = Omega_l . x~_n,    x~ = x * inv_ls,    z~ = z * inv_ls,    s2_nm = |x~_n - z~_m|^2,

f' the derivative of ``pathwise_ref.profile`` with respect to s2 (the Matern kernels with r = sqrt(max(s2, 1e-36)), as the
product's device function has it).  ``dtype=np.longdouble`` runs the same arithmetic in extended precision: what the fp64
restatement itself is held to.
"""
import functools

import numpy as np

from tests import pathwise_ref as R


def profile_grad(kind, s, dtype=np.float64):
    """d profile / d s2."""
    T = dtype
    s = np.asarray(s, T)
    if kind == R.SE:
        return T(-0.5) * np.exp(T(-0.5) * s)
    r = np.sqrt(np.maximum(s, T(1e-36)))
    if kind == R.MATERN32:
        return T(-1.5) * np.exp(-np.sqrt(T(3)) * r)
    if kind == R.MATERN52:
        a = np.sqrt(T(5)) * r
        return -T(5) / T(6) * (T(1) + a) * np.exp(-a)
    raise ValueError(f"kind {kind}")


def _parts(kind, X, Z, inv_ls, V, dtype):
    """x~ [N, D], and for M > 0 the differences [N, M, D], f'(s2) [N, M] and V; None, None, None for M = 0."""
    xt = np.asarray(X, dtype) * np.asarray(inv_ls, dtype)
    if V is None or np.shape(V)[1] == 0:
        return xt, None, None, None
    zt = np.asarray(Z, dtype) * np.asarray(inv_ls, dtype)
    diff = xt[:, None, :] - zt[None, :, :]
    return xt, diff, profile_grad(kind, np.sum(diff * diff, axis=-1), dtype), np.asarray(V, dtype)


def vjp(kind, X, Z, inv_ls, variance, Omega, W, V, C, dtype=np.float64):
    """dX [N, D] of ``tsvgp_pathwise_vjp_f64``: the operands of ``pathwise_ref.evaluate`` and the cotangents C [S, N]."""
    T = dtype
    Omega, W, C = np.asarray(Omega, T), np.asarray(W, T), np.asarray(C, T)
    L = Omega.shape[0]
    xt, diff, df, V = _parts(kind, X, Z, inv_ls, V, T)
    arg = xt @ Omega.T  # [N, L]
    wc, ws = C.T @ W[:, :L], C.T @ W[:, L:]  # [N, L]: the cotangent's weight on the cosine and on the sine of a frequency
    acc = (np.cos(arg) * ws - np.sin(arg) * wc) @ Omega  # [N, D]
    if diff is not None:
        g = T(2) * T(variance) * df * (C.T @ V)  # [N, M]
        acc = acc + np.einsum("nm,nmd->nd", g, diff)
    return acc * np.asarray(inv_ls, T)


def magnitude_vjp(kind, X, Z, inv_ls, variance, Omega, W, V, C):
    """A [N, D]: the size of ``vjp``'s summands,

        A[n, d] = inv_ls_d (  sum_l |Omega_ld| (sum_s |C_sn| (|W_sl| + |W_s,L+l|)) (1 + sum_d' |Omega_ld' x~_nd'|)
                            + sum_m 2 (|x~_nd| + |z~_md|) variance |f'(s2_nm)| (sum_s |C_sn| |V_sm|) ),

    with |x~| + |z~| and not |x~ - z~|: the difference cancels, and its rounding error is that of its terms."""
    T = np.float64
    Omega, W, C = np.abs(np.asarray(Omega, T)), np.abs(np.asarray(W, T)), np.abs(np.asarray(C, T))
    L = Omega.shape[0]
    xt, diff, df, V = _parts(kind, X, Z, inv_ls, V, T)
    amp = 1.0 + np.abs(xt) @ Omega.T  # [N, L]
    A = ((C.T @ (W[:, :L] + W[:, L:])) * amp) @ Omega
    if diff is not None:
        zt = np.abs(np.asarray(Z, T) * np.asarray(inv_ls, T))
        g = 2.0 * variance * np.abs(df) * (C.T @ np.abs(V))  # [N, M]
        A = A + np.abs(xt) * np.sum(g, axis=1)[:, None] + g @ zt
    return A * np.asarray(inv_ls, T)


@functools.lru_cache(maxsize=None)
def problem(kind, N, L, M, D, S, seed):
    """(X, Z, inv_ls, variance, Omega, W, V, C), read-only: ARD lengthscales; with M > 0 every second row within 0.4 (scaled) of
    an inducing point and every fourth of those exactly on it (the Matern clamp, the factor x~ - z~ = 0); the other rows with
    |x~| up to 20; V = None for M = 0; C standard normal."""
    rng = np.random.RandomState(seed)
    ls = rng.uniform(0.5, 2.0, D)
    inv_ls, variance = 1.0 / ls, 1.7
    Zt = rng.uniform(-3.0, 3.0, (max(M, 1), D))
    Xt = rng.uniform(-20.0, 20.0, (N, D))
    if M > 0:
        near = np.flatnonzero(np.arange(N) % 2 == 0)
        pick = rng.randint(0, M, near.size)
        Xt[near] = Zt[pick] + 0.4 * rng.randn(near.size, D)
        Xt[near[::4]] = Zt[pick[::4]]
    X, Z = Xt * ls, Zt[:M] * ls  # (the same product on both sides: a row on an inducing point scales to x~ == z~ exactly)
    Omega = R.spectral(kind, seed, 1, L, D)
    W = rng.randn(S, 2 * L) * np.sqrt(variance / L)
    V = 3.0 * rng.randn(S, M) if M > 0 else None
    C = rng.randn(S, N)
    for a in (X, Z, inv_ls, Omega, W, V, C):
        if a is not None:
            a.setflags(write=False)
    return X, Z, inv_ls, variance, Omega, W, V, C


@functools.lru_cache(maxsize=None)
def problem_vjp(kind, N, L, M, D, S, seed):
    """(vjp, magnitude_vjp) of ``problem`` in fp64, computed once for the tests that share it.  Read-only."""
    args = problem(kind, N, L, M, D, S, seed)
    out = vjp(kind, *args), magnitude_vjp(kind, *args)
    for a in out:
        a.setflags(write=False)
    return out
