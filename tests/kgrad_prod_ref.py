"""NumPy fp64 restatement of the M-step gradient contraction of a PRODUCT of stationary kernels (``tsvgp_kernel_grad_prod_*``),
written from the formulas alone (include/tsvgp_hip.h (8p)), not from the kernel's loops.

With s_cd = (X_nd - Z_md) inv_ls[c, d], s_c = sum_d s_cd^2, K = variance prod_c f_c(s_c), variance = prod_c variance_c:
    V[n, m]   = g0[n] beta[m] - 2 g1[n] U[n, m]
    P_c       = prod_{c' != c} f_c'(s_c')
    w_c       = -2 variance V P_c f_c'(s_c)
    dvar[c]   = (variance / variance_c) sum_nm V prod_c f_c
    dls[c, d] = sum_nm w_c s_cd^2 inv_ls[c, d]
    dZ[m, d]  = sum_n sum_c w_c s_cd inv_ls[c, d]
Next to each result stands the sum of the absolute values of its terms, |V|, |f'| and P_c taken as in ``kgrad_ref.fused`` and
|x~| + |z~| (x~ = X inv_ls[c], z~ = Z inv_ls[c]) standing for |s_cd|: the quantity a rounding bound ``c * u * A`` is taken against.
Every operand is used as given and promoted to fp64.  No GPU, no torch."""
import numpy as np

from tests.kgrad_ref import profile_grad


def fused(kinds, X, Z, inv_ls, variances, U, g0, g1, beta, rows=128):
    """kinds [C] (names of ``kgrad_ref.KINDS``), X [N, D], Z [M, D], inv_ls [C, D], variances [C], U [N, M], g0, g1 [N], beta [M].
    Returns a dict with dvar [C], dls [C, D], dZ [M, D], vsum (the launch's own sum of V prod f) and A_var [C], A_ls [C, D],
    A_Z [M, D], A_vsum."""
    X, Z, inv_ls, U, g0, g1, beta = [np.asarray(a, dtype=np.float64) for a in (X, Z, inv_ls, U, g0, g1, beta)]
    variances = [float(v) for v in variances]
    C = len(kinds)
    N, D = X.shape
    M = Z.shape[0]
    assert Z.shape == (M, D) and inv_ls.shape == (C, D) and U.shape == (N, M) and g0.shape == g1.shape == (N,) and beta.shape == (M,)
    variance = float(np.prod(variances))
    vsum = A_vsum = 0.0
    dls, A_ls = np.zeros((C, D)), np.zeros((C, D))
    dZ, A_Z = np.zeros((M, D)), np.zeros((M, D))
    for a in range(0, N, rows):
        b = min(a + rows, N)
        V = g0[a:b, None] * beta[None, :] - 2.0 * g1[a:b, None] * U[a:b]
        absV = np.abs(g0[a:b, None]) * np.abs(beta[None, :]) + 2.0 * np.abs(g1[a:b, None]) * np.abs(U[a:b])
        sd, spread, f, df = [], [], [], []
        for c in range(C):
            xt, zt = X[a:b] * inv_ls[c], Z * inv_ls[c]
            sd.append(xt[:, None, :] - zt[None, :, :])  # [n, M, D]
            spread.append(np.abs(xt)[:, None, :] + np.abs(zt)[None, :, :])
            fc, dfc = profile_grad(kinds[c], np.sum(sd[c] * sd[c], axis=-1))
            f.append(fc)
            df.append(dfc)
        full = np.ones_like(V)
        for c in range(C):
            full = full * f[c]
        vsum += np.sum(V * full)
        A_vsum += np.sum(absV * full)
        for c in range(C):
            P = np.ones_like(V)
            for c2 in range(C):
                if c2 != c:
                    P = P * f[c2]
            w = -2.0 * variance * V * P * df[c]
            absw = 2.0 * abs(variance) * absV * P * np.abs(df[c])
            il, ail = inv_ls[c], np.abs(inv_ls[c])
            dZ += np.einsum("nm,nmd->md", w, sd[c]) * il
            A_Z += np.einsum("nm,nmd->md", absw, spread[c]) * ail
            dls[c] += np.einsum("nm,nmd->d", w, sd[c] * sd[c]) * il
            A_ls[c] += np.einsum("nm,nmd->d", absw, spread[c] * spread[c]) * ail
    others = np.array([np.prod([v for c2, v in enumerate(variances) if c2 != c]) for c in range(C)])
    return dict(dvar=others * vsum, dls=dls, dZ=dZ, vsum=vsum, A_var=np.abs(others) * A_vsum, A_ls=A_ls, A_Z=A_Z, A_vsum=A_vsum)


def objective(kinds, X, Z, lengthscales, variances, V):
    """sum_nm V[n, m] K[n, m] of the product kernel with V held fixed: what ``fused`` differentiates (its self-check)."""
    X, Z, V = [np.asarray(a, dtype=np.float64) for a in (X, Z, V)]
    K = np.full(V.shape, float(np.prod(variances)))
    for c, kind in enumerate(kinds):
        sd = (X[:, None, :] - Z[None, :, :]) / np.asarray(lengthscales[c], dtype=np.float64)
        K = K * profile_grad(kind, np.sum(sd * sd, axis=-1))[0]
    return float(np.sum(V * K))
