"""CPU checks of the joint-prediction feature (no GPU): the NumPy restatement tests/fullcov_ref.py is pinned by the reference's own
relational check, and the new C-ABI entry points ``tsvgp_cov_*`` are in the built library, declared, bound and validating."""
import ctypes
import os
import re

import numpy as np

from oracle import tsvgp_oracle as O
from tests import fullcov_ref as R
from tests.helpers import pkg

LENGTH_SCALE, VARIANCE, NUM_DATA, NOISE_VARIANCE = 2.0, 2.25, 8, 0.3


def _gpr_setup():
    """reference tests/models/test_tsvgp.py:19-43, 91-103 (N = M = 8, Z = X; 10 steps at lr 0.9)."""
    rng = np.random.RandomState(123)
    func = lambda x: np.sin(x * 3 * 3.14) + 0.3 * np.cos(x * 9 * 3.14) + 0.5 * np.sin(x * 7 * 3.14)
    X = rng.rand(NUM_DATA, 1) * 2 - 1
    Y = func(X) + 0.2 * rng.randn(NUM_DATA, 1)
    kernel = O.SquaredExponential(lengthscales=LENGTH_SCALE, variance=VARIANCE)
    model = O.t_SVGP(kernel=kernel, likelihood=O.Gaussian(variance=NOISE_VARIANCE), inducing_variable=O.InducingPoints(X))
    for _ in range(10):
        model.natgrad_step((X, Y), lr=0.9)
    return model, X, Y, kernel, rng


def test_restatement_matches_the_exact_gp_posterior():
    """The reference's relational check (tests/models/test_tsvgp.py:113-120) extended to the joint covariance: with Z = X at the
    optimum q(f*) is the exact GP posterior, mean and FULL covariance, to the reference's decimal=4."""
    model, X, Y, kernel, rng = _gpr_setup()
    Xs = np.concatenate([X + 1.0, rng.rand(40, 1) * 4 - 2])
    mean, cov = R.predict_f_full_cov(model, Xs)
    assert mean.shape == (48, 1) and cov.shape == (1, 48, 48)
    Ky = kernel.K(X) + NOISE_VARIANCE * np.eye(NUM_DATA)
    Ksx = kernel.K(Xs, X)
    mean_gpr = Ksx @ np.linalg.solve(Ky, Y)
    cov_gpr = kernel.K(Xs) - Ksx @ np.linalg.solve(Ky, Ksx.T)
    print("gap cov", np.max(np.abs(cov[0] - cov_gpr)), "gap mean", np.max(np.abs(mean - mean_gpr)))
    np.testing.assert_array_almost_equal(cov[0], cov_gpr, decimal=4)
    np.testing.assert_array_almost_equal(mean, mean_gpr, decimal=4)
    # its diagonal and its mean are the oracle's predict_f
    mu, var = model.predict_f(Xs)
    assert np.max(np.abs(np.diagonal(cov[0]) - var[:, 0])) <= 1e-12 * np.max(np.abs(var))
    assert np.max(np.abs(mean - mu)) <= 1e-12 * np.max(np.abs(mu))
    np.testing.assert_allclose(cov[0], cov[0].T, rtol=0, atol=1e-14)  # (BLAS products: symmetric to rounding only)


def test_sample_formula_restated():
    """sample_mvn [ext]: f = mean + chol(cov + jitter I) eps, per latent; the marginal form f = mean + sqrt(var) eps."""
    model, X, _, _, rng = _gpr_setup()
    Xs = rng.rand(12, 1) * 2 - 1
    mean, cov = R.predict_f_full_cov(model, Xs)
    eps = rng.randn(5, 12, 1)
    f = R.sample_mvn_full_cov(mean, cov, eps)
    assert f.shape == (5, 12, 1)
    L = np.linalg.cholesky(cov[0] + 1e-6 * np.eye(12))
    np.testing.assert_allclose(f[3, :, 0], mean[:, 0] + L @ eps[3, :, 0], rtol=0, atol=1e-14)
    var = np.diagonal(cov[0])[:, None]
    np.testing.assert_allclose(R.sample_mvn_diag(mean, var, eps)[2], mean + np.sqrt(var) * eps[2], rtol=0, atol=0)


def _declared(header, name):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in {header}"
    return [a.strip() for a in m.group(1).split(",")]


def test_cov_symbols_built_declared_and_bound(repo_root):
    B = pkg()._backend
    pkg().build_library()
    lib = B.lib()
    assert lib.tsvgp_abi_version() == 5 and B.ABI_VERSION == 5  # new symbols only: the calling conventions did not move
    header = os.path.join(repo_root, "include", "tsvgp_hip.h")
    for name in ("tsvgp_cov_f64", "tsvgp_cov_f32"):
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in B.exported_symbols()
        args = _declared(header, name)
        restype, argtypes = B._PROTOTYPES[name]
        assert len(args) == len(argtypes) == 14
        for decl, ct in zip(args, argtypes):  # pointers, 64-bit sizes, ints and scalars line up with the header
            want = (ctypes.c_void_p if "*" in decl else ctypes.c_int64 if decl.startswith("int64_t") else
                    ctypes.c_int if decl.startswith("int ") else ctypes.c_double if decl.startswith("double") else ctypes.c_float)
            assert ct is want, f"{name}: `{decl}` is bound as {ct.__name__}"
    assert B.COV_ACCUMULATE == 1 and "#define TSVGP_COV_ACCUMULATE 1" in open(header).read()


def test_cov_argument_validation_needs_no_gpu():
    """tsvgp_cov_* reject bad arguments before any launch.  Fake, aligned, non-null pointers (never dereferenced: every call below
    has exactly one bad argument and none is valid) so that only the argument under test can be what is refused; one all-NULL
    call for the pointer check itself."""
    B = pkg()._backend
    lib = B.lib()
    fake = 4096
    for sfx in ("f64", "f32"):
        fn = getattr(lib, f"tsvgp_cov_{sfx}")
        good = dict(kind=B.KERNEL_SE, T=fake, X=fake, inv_ls=fake, C=fake, D=2, sign=-1.0, N=100, Np=128, Mp=128, ldc=128, flags=0)

        def call(**kw):
            a = dict(good, **kw)
            return fn(a["kind"], a["T"], a["X"], a["inv_ls"], 1.0, a["sign"], a["C"], a["N"], a["Np"], a["Mp"], a["D"], a["ldc"],
                      a["flags"], None)

        assert call(T=None, X=None, inv_ls=None, C=None) == 1
        for bad in (dict(T=None), dict(C=None), dict(X=None), dict(inv_ls=None)):  # each pointer on its own
            assert call(**bad) == 1, bad
        for bad in (dict(kind=7), dict(kind=1), dict(kind=-1),  # not a kernel (1 is the reserved Matern-1/2)
                    dict(D=33), dict(D=0), dict(sign=0.5), dict(sign=0.0), dict(sign=float("nan")),
                    dict(ldc=120), dict(ldc=127), dict(ldc=129),  # below Np; rows off the 16-byte grid
                    dict(Np=100), dict(Np=256), dict(Np=0), dict(N=0), dict(N=129),  # Np is N rounded up to 128
                    dict(Mp=100), dict(Mp=0), dict(flags=2), dict(flags=-1),
                    dict(T=fake + 8), dict(C=fake + 8), dict(C=fake + 4)):  # 16-byte boundaries
            assert call(**bad) == 1, (sfx, bad)
        # ACCUMULATE ignores kind / X / inv_ls / D: with those absent or nonsensical the call gets as far as the checks on T and C
        acc = dict(flags=B.COV_ACCUMULATE, X=None, inv_ls=None, kind=7, D=99)
        assert call(C=None, **acc) == 1 and call(T=None, **acc) == 1 and call(C=fake + 8, **acc) == 1
        assert call(sign=0.5, **acc) == 1 and call(ldc=120, **acc) == 1 and call(Np=100, **acc) == 1
