"""NumPy fp64 restatement of the M-step gradient contraction (``tsvgp_kernel_grad_*``, ``tsvgp_gram_to_gradw_*``), written from
the formulas alone (the comment block above ``kgrad_kernel`` in t-svgp_amd/csrc/tsvgp_grad.hip), not from the kernels' loops.

With x~ = X * inv_ls, z~ = Z * inv_ls, s_d = x~_nd - z~_md, s = sum_d s_d^2, K = variance * f(s):
    V[n, m]  = g0[n] beta[m] - 2 g1[n] U[n, m]
    w[n, m]  = -2 variance V f'(s)
    dvar     = sum_nm V f(s)
    dZ[m, d] = sum_n  w s_d   inv_ls_d
    dls[d]   = sum_nm w s_d^2 inv_ls_d
Next to each result stands the sum of the absolute values of its terms, with the cancellation inside s_d opened up
(|x~| + |z~| for |s_d|): the quantity a rounding bound ``c * u * A`` is taken against.  Every operand is used as given (the caller
passes what the kernel sees: values already rounded to the array type) and promoted to fp64.  No GPU, no torch."""
import numpy as np

KINDS = ("se", "matern32", "matern52")
SQRT3, SQRT5 = np.sqrt(3.0), np.sqrt(5.0)


def profile_grad(kind, s):
    """(f(s), f'(s)) with K = variance * f(s), s the scaled squared distance.  The Matern profiles take
    r = sqrt(max(s, 1e-36)) as GPflow's IsotropicStationary and the kernels do."""
    s = np.asarray(s, dtype=np.float64)
    if kind == "se":
        f = np.exp(-0.5 * s)
        return f, -0.5 * f
    r = np.sqrt(np.maximum(s, 1e-36))
    if kind == "matern32":
        a = SQRT3 * r
        e = np.exp(-a)
        return (1.0 + a) * e, -1.5 * e
    if kind == "matern52":
        a = SQRT5 * r
        e = np.exp(-a)
        return (1.0 + a + 5.0 / 3.0 * r * r) * e, -5.0 / 6.0 * (1.0 + a) * e
    raise ValueError(kind)


def _f64(*arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


def fused(kind, X, Z, inv_ls, variance, U, g0, g1, beta, rows=128):
    """X [N, D], Z [M, D], inv_ls [D], U [N, M], g0, g1 [N], beta [M].  Returns a dict with dvar (scalar), dls [D], dZ [M, D] and
    A_var, A_ls [D], A_Z [M, D].  Rows are taken ``rows`` at a time only to bound the [rows, M, D] temporaries."""
    X, Z, inv_ls, U, g0, g1, beta = _f64(X, Z, inv_ls, U, g0, g1, beta)
    variance = float(variance)
    N, D = X.shape
    M = Z.shape[0]
    assert Z.shape == (M, D) and inv_ls.shape == (D,) and U.shape == (N, M) and g0.shape == g1.shape == (N,) and beta.shape == (M,)
    xt, zt = X * inv_ls, Z * inv_ls
    azt = np.abs(zt)
    dvar = A_var = 0.0
    dls, A_ls = np.zeros(D), np.zeros(D)
    dZ, A_Z = np.zeros((M, D)), np.zeros((M, D))
    for a in range(0, N, rows):
        b = min(a + rows, N)
        sd = xt[a:b, None, :] - zt[None, :, :]  # [n, M, D]
        f, df = profile_grad(kind, np.sum(sd * sd, axis=-1))
        V = g0[a:b, None] * beta[None, :] - 2.0 * g1[a:b, None] * U[a:b]
        absV = np.abs(g0[a:b, None]) * np.abs(beta[None, :]) + 2.0 * np.abs(g1[a:b, None]) * np.abs(U[a:b])
        w = -2.0 * variance * V * df
        absw = 2.0 * abs(variance) * absV * np.abs(df)
        spread = np.abs(xt[a:b, None, :]) + azt[None, :, :]  # |x~_nd| + |z~_md|
        dvar += np.sum(V * f)
        A_var += np.sum(absV * f)
        dZ += np.einsum("nm,nmd->md", w, sd)
        A_Z += np.einsum("nm,nmd->md", absw, spread)
        dls += np.einsum("nm,nmd->d", w, sd * sd)
        A_ls += np.einsum("nm,nmd->d", absw, spread * spread)
    return dict(dvar=dvar, dls=dls * inv_ls, dZ=dZ * inv_ls, A_var=A_var, A_ls=A_ls * np.abs(inv_ls), A_Z=A_Z * np.abs(inv_ls))


def gemm_form(kind, G, xx, zz, variance, U, g0, g1, beta, N, M, u=2.0 ** -53, c=512.0, rows=1024):
    """The GEMM form: s = xx[n] + zz[m] - 2 G[n, m] with G = x~ z~^T, xx = |x~|^2, zz = |z~|^2 given (the leading [N, M] block of
    G and U is used).  Returns (W [N, M], dvar, W_bound [N, M], dvar_bound) with W = -2 variance V f'(s), dvar = sum V f(s).

    The bounds are for a kernel that forms s in arrays of unit roundoff ``u``: s is a difference of terms far larger than itself
    when x~ is close to z~, so an absolute error ds = 4 u (|xx| + |zz| + 2 |G|) on s (two additions, twice over) is carried through
    the profile -- which is monotone in s, so the two ends of [s - ds, s + ds] bound what lies between -- and every other
    rounding goes into c * u * |W~| with W~ = W with |V| for V:
        W_bound = c u |W~| + max(|W(s + ds) - W(s)|, |W(s - ds) - W(s)|),
    and the same, term by term and summed, for dvar."""
    G, xx, zz, U, g0, g1, beta = _f64(G, xx, zz, U, g0, g1, beta)
    variance = float(variance)
    G, U = G[:N, :M], U[:N, :M]
    assert G.shape == (N, M) and U.shape == (N, M) and xx.shape == (N,) and zz.shape == (M,) and g0.shape == g1.shape == (N,)
    assert beta.shape == (M,)
    W, W_bound = np.empty((N, M)), np.empty((N, M))
    dvar = dvar_bound = 0.0
    for a in range(0, N, rows):  # row blocks only to keep the temporaries in cache
        b = min(a + rows, N)
        s = xx[a:b, None] + zz[None, :] - 2.0 * G[a:b]
        ds = 4.0 * u * (np.abs(xx[a:b])[:, None] + np.abs(zz)[None, :] + 2.0 * np.abs(G[a:b]))
        V = g0[a:b, None] * beta[None, :] - 2.0 * g1[a:b, None] * U[a:b]
        absV = np.abs(g0[a:b, None]) * np.abs(beta[None, :]) + 2.0 * np.abs(g1[a:b, None]) * np.abs(U[a:b])
        f, df = profile_grad(kind, s)
        f_up, df_up = profile_grad(kind, s + ds)
        f_dn, df_dn = profile_grad(kind, s - ds)
        W[a:b] = -2.0 * variance * V * df
        W_bound[a:b] = c * u * 2.0 * abs(variance) * absV * np.abs(df) \
            + 2.0 * abs(variance) * np.abs(V) * np.maximum(np.abs(df_up - df), np.abs(df_dn - df))
        dvar += float(np.sum(V * f))
        dvar_bound += float(np.sum(c * u * absV * f + np.abs(V) * np.maximum(np.abs(f_up - f), np.abs(f_dn - f))))
    return W, dvar, W_bound, dvar_bound


def gemm_finish(W, xt, zt, inv_ls):
    """What is left of the GEMM form in M x D (``EStepEngine._kernel_grad_gemm`` after the kernel; include/tsvgp_hip.h (1c)):
    dZ = (W^T x~ - z~ colsum W) inv_ls,  dls_d = (sum_n x~_nd^2 rowsum_n - 2 sum_m z~_md (W^T x~)_md + sum_m z~_md^2 colsum_m) inv_ls_d."""
    W, xt, zt, inv_ls = _f64(W, xt, zt, inv_ls)
    colsum, rowsum = W.sum(axis=0), W.sum(axis=1)
    WtX = W.T @ xt
    dZ = (WtX - zt * colsum[:, None]) * inv_ls
    dls = (np.einsum("nd,n->d", xt * xt, rowsum) - 2.0 * np.sum(zt * WtX, axis=0) + np.einsum("md,m->d", zt * zt, colsum)) * inv_ls
    return dls, dZ
