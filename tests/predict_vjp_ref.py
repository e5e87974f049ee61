"""NumPy fp64 restatement of the input gradient of the marginal moments (``tsvgp_moments_vjp_*``), written from the formulas
alone (include/tsvgp_hip.h (11)), not from the kernel's loops.

With x~ = X * inv_ls, z~ = Z * inv_ls, s_d = x~_nd - z~_md, s = sum_d s_d^2, K = variance * f(s), mean = K beta and
var = variance - rowsum((K Q) * K) with Q symmetric, U = K Q:
    V[n, m]  = cm[n] beta[m] - 2 cv[n] U[n, m]
    dX[n, d] = sum_m V variance f'(s) 2 s_d inv_ls_d
Next to the result stands A, the sum of the absolute values of each entry's terms with the cancellation inside s_d opened up
(|x~| + |z~| for |s_d|), as in tests/kgrad_ref.py: the quantity a rounding bound ``c * u * A`` is taken against.  Every operand is
used as given (the caller passes what the kernel sees: values already rounded to the array type) and promoted to fp64.  No GPU, no
torch."""
import numpy as np

from tests.kgrad_ref import KINDS, profile_grad  # noqa: F401  (KINDS: the names the callers iterate over)


def vjp(kind, X, Z, inv_ls, variance, U, cm, cv, beta, rows=128):
    """X [N, D], Z [M, D], inv_ls [D], U [N, M], cm, cv [N], beta [M]: one latent.  Returns (dX [N, D], A [N, D]).  Rows are taken
    ``rows`` at a time only to bound the [rows, M, D] temporaries."""
    X, Z, inv_ls, U, cm, cv, beta = [np.asarray(a, dtype=np.float64) for a in (X, Z, inv_ls, U, cm, cv, beta)]
    variance = float(variance)
    N, D = X.shape
    M = Z.shape[0]
    assert Z.shape == (M, D) and inv_ls.shape == (D,) and U.shape == (N, M) and cm.shape == cv.shape == (N,) and beta.shape == (M,)
    xt, zt = X * inv_ls, Z * inv_ls
    dX, A = np.empty((N, D)), np.empty((N, D))
    for a in range(0, N, rows):
        b = min(a + rows, N)
        sd = xt[a:b, None, :] - zt[None, :, :]  # [n, M, D]
        _, df = profile_grad(kind, np.sum(sd * sd, axis=-1))
        V = cm[a:b, None] * beta[None, :] - 2.0 * cv[a:b, None] * U[a:b]
        absV = np.abs(cm[a:b, None]) * np.abs(beta[None, :]) + 2.0 * np.abs(cv[a:b, None]) * np.abs(U[a:b])
        w = 2.0 * variance * V * df
        absw = 2.0 * abs(variance) * absV * np.abs(df)
        spread = np.abs(xt[a:b, None, :]) + np.abs(zt)[None, :, :]
        dX[a:b] = np.einsum("nm,nmd->nd", w, sd)
        A[a:b] = np.einsum("nm,nmd->nd", absw, spread)
    return dX * inv_ls, A * np.abs(inv_ls)


def predict_vjp(kind, X, Z, inv_ls, variance, beta, Q, cm, cv):
    """The sum over the latents: beta [M, P], Q [P, M, M] symmetric, cm, cv [N, P]; K(X, Z) and U_p = K Q_p are formed here in
    fp64.  Returns (dX, A)."""
    X, Z, inv_ls, beta, Q, cm, cv = [np.asarray(a, dtype=np.float64) for a in (X, Z, inv_ls, beta, Q, cm, cv)]
    sd = (X * inv_ls)[:, None, :] - (Z * inv_ls)[None, :, :]
    K = float(variance) * profile_grad(kind, np.sum(sd * sd, axis=-1))[0]
    dX, A = np.zeros(X.shape), np.zeros(X.shape)
    for p in range(beta.shape[1]):
        g, a = vjp(kind, X, Z, inv_ls, variance, K @ Q[p], cm[:, p], cv[:, p], beta[:, p])
        dX += g
        A += a
    return dX, A
