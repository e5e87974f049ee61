"""CPU checks of the pathwise function draws (no GPU): ``tsvgp_pathwise_f64`` is in the built library, declared, bound and
validating, and the NumPy restatement tests/pathwise_ref.py -- what the GPU tests hold the kernel and the models to -- has the law
it claims (mean and covariance of ``predict_f(full_cov=True)`` up to the random-feature error) and interpolates the inducing
values."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import pathwise_ref as R
from tests.helpers import pkg

KINDS = [R.SE, R.MATERN32, R.MATERN52]


def _declared(header, name):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in {header}"
    return [a.strip() for a in m.group(1).split(",")]


def test_pathwise_symbol_built_declared_and_bound(repo_root):
    p = pkg()
    B = p._backend
    p.build_library()
    lib = B.lib()
    assert lib.tsvgp_abi_version() == 5 and B.ABI_VERSION == 5  # a new symbol only: the calling conventions did not move
    header = os.path.join(repo_root, "include", "tsvgp_hip.h")
    name = "tsvgp_pathwise_f64"
    assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert name in B.exported_symbols()
    args = _declared(header, name)
    restype, argtypes = B._PROTOTYPES[name]
    assert restype is ctypes.c_int and len(args) == len(argtypes) == 16
    for decl, ct in zip(args, argtypes):  # pointers, 64-bit sizes, ints and scalars line up with the header
        want = (ctypes.c_void_p if "*" in decl else ctypes.c_int64 if decl.startswith("int64_t") else
                ctypes.c_int if decl.startswith("int ") else ctypes.c_double)
        assert ct is want, f"{name}: `{decl}` is bound as {ct.__name__}"
    assert B.PATHWISE_MAX_S >= 1 and f"#define TSVGP_PATHWISE_MAX_S {B.PATHWISE_MAX_S}\n" in open(header).read()
    assert "FunctionSamples" in p.__all__ and isinstance(p.FunctionSamples, type)
    assert hasattr(p.base_SVGP, "sample_functions") and not hasattr(p.t_VGP, "sample_functions")


def test_pathwise_argument_validation_needs_no_gpu():
    """Every refusal of the header, from a call that differs from an accepted one in that single argument.  Fake, aligned, non-null
    pointers that are never dereferenced: none of these calls gets as far as a launch."""
    B = pkg()._backend
    fn = B.lib().tsvgp_pathwise_f64
    fake = 4096
    good = dict(kind=B.KERNEL_SE, X=fake, Z=fake, inv_ls=fake, variance=1.0, Omega=fake, W=fake, V=fake, out=fake, N=100, M=8, L=16,
                D=2, S=3, ldo=100)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["kind"], a["X"], a["Z"], a["inv_ls"], a["variance"], a["Omega"], a["W"], a["V"], a["out"], a["N"], a["M"], a["L"],
                  a["D"], a["S"], a["ldo"], None)

    for bad in (dict(X=None), dict(inv_ls=None), dict(Omega=None), dict(W=None), dict(out=None),  # each required pointer on its own
                dict(V=None), dict(Z=None),  # required with M > 0
                dict(N=0), dict(N=-1), dict(L=0), dict(L=-1), dict(M=-1),
                dict(D=0), dict(D=33), dict(D=-1),
                dict(S=0), dict(S=-1), dict(S=B.PATHWISE_MAX_S + 1),
                dict(ldo=99), dict(ldo=0),
                dict(variance=0.0), dict(variance=-1.0), dict(variance=float("nan")), dict(variance=float("inf")),
                dict(kind=1), dict(kind=4), dict(kind=-1), dict(kind=7)):  # 1 is the reserved Matern-1/2
        assert call(**bad) == 1, bad
    # M = 0 makes V and Z optional, and nothing else: the call with them absent gets as far as the other checks
    assert call(M=0, V=None, Z=None, S=0) == 1 and call(M=0, V=None, Z=None, X=None) == 1 and call(M=0, V=None, Z=None, D=33) == 1


# ---------------------------------------------------------------------------------------------------------------
# The law of the restatement.  One latent GP in one dimension, M = 8 inducing points a lengthscale apart (cond(K6) <= 1e3: V is
# of moderate size and the random-feature error is not amplified), a hand-made definite S, L = 4096 features, S = 4096 draws, 12
# test points inside and outside the inducing points.  With A = K(x, Z) K6^-1 the exact moments of predict_f(full_cov=True) are
#     mean = A m,     C = K(x, x) - A K(Z, x) + A S A^T.
# Sample mean: each entry has standard deviation sqrt(C_ii / S).  Sample covariance: each entry has standard deviation
# sqrt((C_ii C_jj + C_ij^2) / S) (Wishart), and the draws' own covariance differs from C by the random-feature error of the prior
# term, variance / sqrt(L) per entry of K(., .), which enters through (I, -A) on both sides: (1 + |A|_inf)^2 variance / sqrt(L).
# Five of each, at every point and every entry.  (SEED, DRAW) was picked on the CPU as one for which all three kernels pass with
# no entry left out; the generator is counter based, so the draws are the same on every machine.
# ---------------------------------------------------------------------------------------------------------------
SEED, DRAW = 2020, 0
LAW_L, LAW_S = 4096, 4096


def _law_problem(kind):
    rng = np.random.RandomState(7)
    M = 8
    inv_ls, variance = np.array([1.0 / 0.8]), 1.3
    Z = np.linspace(-3.0, 3.0, M)[:, None]
    m = rng.randn(M, 1)
    cholS = np.tril(0.1 * rng.randn(M, M), -1) + np.diag(0.3 + 0.2 * rng.rand(M))
    Xs = np.linspace(-4.0, 4.0, 12)[:, None]
    K6 = R.kernel_matrix(kind, Z, Z, inv_ls, variance) + pkg().default_jitter() * np.eye(M)
    return Z, m, cholS, Xs, K6, inv_ls, variance


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_has_the_law_of_predict_f_full_cov(kind):
    Z, m, cholS, Xs, K6, inv_ls, variance = _law_problem(kind)
    assert np.linalg.cond(K6) <= 1e3
    ops = R.sampler(m, cholS[None], K6, [kind], Z, [inv_ls], [variance], SEED, DRAW, LAW_L, LAW_S)
    f = R.sample(ops, [kind], Xs, Z, [inv_ls], [variance])[:, :, 0]  # [S, 12]
    A = np.linalg.solve(K6, R.kernel_matrix(kind, Z, Xs, inv_ls, variance)).T  # [12, M]
    mean = (A @ m)[:, 0]
    C = R.kernel_matrix(kind, Xs, Xs, inv_ls, variance) - A @ R.kernel_matrix(kind, Z, Xs, inv_ls, variance) + A @ cholS @ cholS.T @ A.T
    d = np.diagonal(C)
    assert np.all(d > 0)
    mean_err, mean_bound = np.abs(f.mean(axis=0) - mean), 5.0 * np.sqrt(d / LAW_S)
    cov_err = np.abs(np.cov(f.T) - C)
    amp = (1.0 + np.max(np.sum(np.abs(A), axis=1))) ** 2
    cov_bound = 5.0 * (np.sqrt((np.outer(d, d) + C * C) / LAW_S) + amp * variance / np.sqrt(LAW_L))
    print(f"kind {kind}: mean err / bound max {np.max(mean_err / mean_bound):.3f}, cov err / bound max {np.max(cov_err / cov_bound):.3f}, "
          f"|A|_inf {np.sqrt(amp) - 1:.2f}")
    assert np.all(mean_err <= mean_bound)
    assert np.all(cov_err <= cov_bound)


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_interpolates_the_inducing_values(kind):
    """f_s(Z) = g_s(Z) + (K6 - jitter I) V_s = u_s - jitter V_s: exact algebra, whatever L is."""
    Z, m, cholS, _, K6, inv_ls, variance = _law_problem(kind)
    ops = R.sampler(m, cholS[None], K6, [kind], Z, [inv_ls], [variance], SEED, 3, 64, 8)
    fZ = R.sample(ops, [kind], Z, Z, [inv_ls], [variance])  # [S, M, 1]
    V = ops["V"].transpose(1, 2, 0)  # [S, M, P]
    gap = np.max(np.abs(fZ - ops["u"] + pkg().default_jitter() * V))
    print(f"kind {kind}: interpolation gap {gap:.2e}, max |u| {np.max(np.abs(ops['u'])):.2f}, max |V| {np.max(np.abs(V)):.1f}")
    assert gap <= 1e-12 * (1.0 + np.max(np.abs(ops["u"])))


def test_sample_functions_fails_loudly_without_gpu():
    """No CPU fallback: without a ROCm device ``sample_functions`` raises as the other entry points do (tests/test_cabi.py)."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = pkg()
    Z = np.zeros((4, 2)) + np.arange(4)[:, None]
    data = (np.zeros((5, 2)), np.zeros((5, 1)))
    for m in (p.t_SVGP(p.SquaredExponential(), p.Gaussian(0.1), Z), p.t_SVGP_white(p.SquaredExponential(), p.Gaussian(0.1), Z),
              p.t_SVGP_sites(data, p.SquaredExponential(), p.Gaussian(0.1), Z)):
        with pytest.raises(p.HipExtensionError):
            m.sample_functions(2, 16)
        assert m._function_draw == 0


def test_spectral_draws_follow_the_layout():
    """Rows p L + l of generator draw 4 draw (+ 1 for the chi-square normals): latent kernel p's frequencies are rows of one
    stream, and a Matern frequency is its normal row scaled by sqrt(2 nu / chi2)."""
    from tests import softmax_ref

    L, D = 5, 3
    both = softmax_ref.normals(11, 4 * 2, np.arange(2 * L), 1, D)[0]
    np.testing.assert_array_equal(R.spectral(R.SE, 11, 2, L, D, 0), both[:L])
    np.testing.assert_array_equal(R.spectral(R.SE, 11, 2, L, D, 1), both[L:])
    c = softmax_ref.normals(11, 4 * 2 + 1, L + np.arange(L), 1, 5)[0]
    np.testing.assert_allclose(R.spectral(R.MATERN52, 11, 2, L, D, 1), both[L:] * np.sqrt(5.0 / np.sum(c * c, axis=1))[:, None],
                               rtol=1e-15, atol=0)
    c3 = softmax_ref.normals(11, 4 * 2 + 1, np.arange(L), 1, 3)[0]
    np.testing.assert_allclose(R.spectral(R.MATERN32, 11, 2, L, D, 0), both[:L] * np.sqrt(3.0 / np.sum(c3 * c3, axis=1))[:, None],
                               rtol=1e-15, atol=0)
