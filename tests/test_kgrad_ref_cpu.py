"""tests/kgrad_ref.py checked on its own, without a GPU: it is what tests/test_gpu_kgrad.py holds the HIP gradient kernels to.

With V held fixed, F(theta) = sum_nm V[n, m] K_theta(x_n, z_m) is linear in K, so ``kgrad_ref.fused`` must equal the central
differences of F taken through the ORACLE's kernels (h = 1e-6: truncation ~h^2, rounding ~1e-16 |F| / h ~ 1e-9 of the largest
entry; asserted at 1e-7 of the largest entry, the sibling tests' reasoning in tests/test_gpu_mstep.py).  ``gemm_form`` plus the
host finish must then equal ``fused`` to 1e-10 when G, xx, zz are formed in fp64 from the same X, Z."""
import numpy as np
import pytest

from oracle import tsvgp_oracle as O
from tests import kgrad_ref as R

ORACLE = {"se": O.SquaredExponential, "matern32": O.Matern32, "matern52": O.Matern52}
N, M = 50, 7


def _problem(kind, D):
    rng = np.random.RandomState(100 * D + R.KINDS.index(kind))
    X, Z = rng.randn(N, D), rng.randn(M, D)
    Z[:2] = X[:2]  # inducing points taken from the data: s = 0, the Matern clamp
    ls = (0.7 + rng.rand(D)) * np.sqrt(D)
    U, g0, g1, beta = rng.randn(N, M), rng.randn(N), rng.randn(N), rng.randn(M)
    return X, Z, ls, 1.3, U, g0, g1, beta


@pytest.mark.parametrize("D", [1, 3, 16])
@pytest.mark.parametrize("kind", R.KINDS)
def test_fused_equals_central_differences_of_the_oracle_kernels(kind, D):
    X, Z, ls, var, U, g0, g1, beta = _problem(kind, D)
    V = g0[:, None] * beta[None, :] - 2.0 * g1[:, None] * U
    F = lambda var_=var, ls_=ls, Z_=Z: float(np.sum(V * ORACLE[kind](var_, ls_).K(X, Z_)))
    ref = R.fused(kind, X, Z, 1.0 / ls, var, U, g0, g1, beta)
    h = 1e-6
    fd_var = (F(var_=var + h) - F(var_=var - h)) / (2 * h)
    fd_ls, fd_Z = np.zeros(D), np.zeros((M, D))
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        fd_ls[d] = (F(ls_=ls + e) - F(ls_=ls - e)) / (2 * h)
        for m in range(M):
            E = np.zeros((M, D))
            E[m, d] = h
            fd_Z[m, d] = (F(Z_=Z + E) - F(Z_=Z - E)) / (2 * h)
    for name, got, fd in (("dvar", ref["dvar"], fd_var), ("dls", ref["dls"], fd_ls), ("dZ", ref["dZ"], fd_Z)):
        err, scale = np.max(np.abs(got - fd)), np.max(np.abs(fd))
        print(f"{kind} D={D} {name}: max abs err {err:.3e}, largest entry {scale:.3e}")
        assert scale > 0 and np.all(np.abs(got - fd) <= 1e-7 * scale), (name, err, scale)
    # the absolute-value sums dominate what they bound
    assert ref["A_var"] >= abs(ref["dvar"]) and np.all(ref["A_ls"] >= np.abs(ref["dls"])) and np.all(ref["A_Z"] >= np.abs(ref["dZ"]))


@pytest.mark.parametrize("D", [1, 3, 16])
@pytest.mark.parametrize("kind", R.KINDS)
def test_gemm_form_with_the_host_finish_equals_fused(kind, D):
    X, Z, ls, var, U, g0, g1, beta = _problem(kind, D)
    il = 1.0 / ls
    xt, zt = X * il, Z * il
    ref = R.fused(kind, X, Z, il, var, U, g0, g1, beta)
    W, dvar, W_bound, dvar_bound = R.gemm_form(kind, xt @ zt.T, np.sum(xt * xt, 1), np.sum(zt * zt, 1), var, U, g0, g1, beta, N, M)
    dls, dZ = R.gemm_finish(W, xt, zt, il)
    for name, got, want in (("dvar", dvar, ref["dvar"]), ("dls", dls, ref["dls"]), ("dZ", dZ, ref["dZ"])):
        err, scale = np.max(np.abs(got - want)), np.max(np.abs(want))
        print(f"{kind} D={D} {name}: gemm form vs fused {err / scale:.3e}")
        assert err <= 1e-10 * scale, (name, err, scale)
    assert W.shape == W_bound.shape == (N, M) and np.all(W_bound >= 0) and np.all(np.isfinite(W_bound)) and dvar_bound > 0


@pytest.mark.parametrize("kind", R.KINDS)
def test_profile_grad_is_the_derivative_of_the_profile(kind):
    s = np.array([0.0, 1e-3, 0.5, 2.0, 17.0, 60.0])
    f, df = R.profile_grad(kind, s)
    K = ORACLE[kind](1.0, 1.0).K(np.sqrt(s)[:, None], np.zeros((1, 1)))[:, 0]
    assert np.max(np.abs(f - K)) <= 1e-15
    h = 1e-6 * np.maximum(s[2:], 1.0)
    fd = (R.profile_grad(kind, s[2:] + h)[0] - R.profile_grad(kind, s[2:] - h)[0]) / (2 * h)
    assert np.all(np.abs(df[2:] - fd) <= 1e-8 * np.abs(df[2]))
    # s = 0 and below: the clamp, finite values
    f0, df0 = R.profile_grad(kind, np.array([0.0, -1e-7]))
    assert np.all(np.isfinite(f0)) and np.all(np.isfinite(df0)) and abs(f0[0] - 1.0) <= 1e-15
    assert kind == "se" or (f0[1] == f0[0] and df0[1] == df0[0])
