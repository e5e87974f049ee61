"""t_VGP without a GPU: the reference's own pins (reference tests/models/test_tvgp.py) on the NumPy restatement
(tests/tvgp_ref.py), the conditioning of the problems the GPU tests use, the constructor's errors and the argument checks of
the two new entry points."""
import numpy as np
import pytest

from oracle import tsvgp_oracle as O
from tests import tvgp_ref as R
from tests.helpers import pkg, relerr

# the shapes of tests/test_gpu_tvgp.py's model test: (N, D, kernel)
MODEL_CASES = [(8, 1, "SquaredExponential"), (128, 3, "Matern52"), (129, 8, "SquaredExponential"), (300, 1, "Matern52"),
               (300, 3, "SquaredExponential")]


def reference_setup():
    """reference tests/models/test_tvgp.py:81-93 (its module-level RandomState(123), first use)."""
    rng = np.random.RandomState(123)

    def func(x):
        return np.sin(x * 3 * 3.14) + 0.3 * np.cos(x * 9 * 3.14) + 0.5 * np.sin(x * 7 * 3.14)

    X = rng.rand(8, 1) * 2 - 1
    Y = func(X) + 0.2 * rng.randn(8, 1)
    return X, Y, dict(variance=2.25, lengthscales=2.0), 0.3


@pytest.fixture(scope="module")
def gpr_pair():
    X, Y, kern, s2 = reference_setup()
    kernel = O.SquaredExponential(**kern)
    m = R.TVGPRef(X, Y, kernel, O.Gaussian(variance=s2))
    m.update(beta=1.0)
    return m, O.gpr_log_marginal_likelihood(kernel, X, Y, s2), s2


def test_optimal_sites(gpr_pair):
    """test_tvgp.py:115-129: one beta = 1 step under a Gaussian likelihood lands on the exact sites."""
    m, _, s2 = gpr_pair
    np.testing.assert_allclose(m.lambda_1, m.Y / s2)
    np.testing.assert_allclose(m.lambda_2, np.ones_like(m.lambda_2) / s2)


def test_elbo_is_the_gpr_log_marginal_likelihood(gpr_pair):
    """test_tvgp.py:96-99."""
    m, lml, _ = gpr_pair
    np.testing.assert_almost_equal(m.elbo(), lml, decimal=4)


def test_unchanged_at_optimum(gpr_pair):
    """test_tvgp.py:102-112."""
    m, _, _ = gpr_pair
    m2 = R.TVGPRef(m.X, m.Y, m.kernel, m.likelihood)
    m2.lambda_1, m2.lambda_2 = m.lambda_1.copy(), m.lambda_2.copy()
    before = m2.elbo()
    m2.update(beta=1.0)
    np.testing.assert_almost_equal(before, m2.elbo(), decimal=4)


@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
@pytest.mark.parametrize("N,D,kernel", MODEL_CASES)
def test_solve_form_and_inverse_form_agree(N, D, kernel, lik):
    """The restatement in the reference's own operations against explicit inverses, after the five beta = 0.5 updates of the GPU
    test: an order of magnitude inside the GPU test's bounds (1e-8 on the sites and predictions, 1e-9 on the ELBO), so those
    bounds measure the HIP path and not the conditioning of the problem."""
    X, Y, k, l, Xnew = R.problem(N, D, lik, kernel)
    a, b = R.TVGPRef(X, Y, k, l, "solve"), R.TVGPRef(X, Y, k, l, "inv")
    for _ in range(5):
        a.update(0.5)
        b.update(0.5)
    assert relerr(a.lambda_1, b.lambda_1) < 1e-9 and relerr(a.lambda_2, b.lambda_2) < 1e-9
    ea, eb = a.elbo(), b.elbo()
    assert abs(ea - eb) <= 1e-10 * abs(eb)
    (ma, va), (mb, vb) = a.predict_f(Xnew), b.predict_f(Xnew)
    assert relerr(ma, mb) < 1e-9 and relerr(va, vb) < 1e-9
    ca, cb = a.predict_f(Xnew, full_cov=True)[1], b.predict_f(Xnew, full_cov=True)[1]
    assert relerr(ca, cb) < 1e-9
    assert np.all(va > 0) and np.all(a.lambda_2 > 0)


def test_constructor_errors():
    p = pkg()
    X, Y = np.linspace(0, 1, 6)[:, None], np.zeros((6, 1))
    k = p.SquaredExponential()
    with pytest.raises(ValueError):
        p.t_VGP((X, np.zeros((6, 2))), k, p.Gaussian(0.1), num_latent=2)
    with pytest.raises(ValueError):
        p.t_VGP((X, np.zeros((6, 2))), k, p.Gaussian(0.1), num_latent=None)
    with pytest.raises(ValueError):
        p.t_VGP((X, Y), k, p.HeteroskedasticTFPConditional())
    with pytest.raises(ValueError):
        p.t_VGP((X, Y), k, p.Softmax(3))
    with pytest.raises(ValueError):
        p.t_VGP((X, Y), k, p.Gaussian(0.1), mean_function=lambda x: x)
    with pytest.raises(ValueError):
        p.t_VGP((np.zeros((6, 33)), Y), k, p.Gaussian(0.1))
    m = p.t_VGP((X, Y), k, p.Gaussian(0.1))
    assert m.lambda_1.shape == (6, 1) and m.lambda_2.shape == (6, 1) and m.sites is not None
    assert np.all(m.lambda_1.numpy() == 0) and np.all(m.lambda_2.numpy() == 1e-6)
    with pytest.raises(ValueError):
        m.update_variational_parameters(beta=1.5)


def test_entry_points_reject_null_and_unpadded_arguments():
    lib = pkg()._backend.lib()
    sys_ = lib.tsvgp_vgp_system_f64
    assert sys_(0, None, None, 1.0, 1e-6, None, None, None, 8, 128, 1, 128, 0, None) == 1
    one = 16  # a non-null, 16-byte aligned address that is never dereferenced: the checks below fail before any launch
    assert sys_(0, one, one, 1.0, 1e-6, one, one, one, 8, 100, 1, 128, 0, None) == 1  # Np not a multiple of 128
    assert sys_(0, one, one, 1.0, 1e-6, one, one, one, 200, 128, 1, 128, 0, None) == 1  # Np < N
    assert sys_(0, one, one, 1.0, 1e-6, one, one, one, 8, 128, 1, 127, 0, None) == 1  # lds < Np
    assert sys_(0, one, one, 1.0, 1e-6, one, one, one, 8, 128, 33, 128, 0, None) == 1  # D > 32
    assert sys_(1, one, one, 1.0, 1e-6, one, one, one, 8, 128, 1, 128, 0, None) == 1  # kind
    assert sys_(0, one, one, 1.0, 1e-6, one, one, one, 8, 128, 1, 128, 2, None) == 1  # flags
    rows = lib.tsvgp_vgp_rows_f64
    assert rows(None, 128, None, None, None, None, 1.0, 0, 0.0, 0.0, None, None, None, None, None, 8, 128, 128, None) == 1
    assert rows(one, 128, None, None, None, None, 1.0, 0, 0.0, 0.0, one, one, None, None, one, 8, 100, 128, None) == 1  # Np
    assert rows(one, 128, None, None, None, None, 1.0, 0, 0.0, 0.0, one, one, None, None, one, 8, 128, 127, None) == 1  # K odd
    assert rows(one, 126, None, None, None, None, 1.0, 0, 0.0, 0.0, one, one, None, None, one, 8, 128, 128, None) == 1  # ldc < K
    assert rows(one, 128, None, None, None, None, 1.0, 0, 0.0, 0.0, None, None, None, None, one, 8, 128, 128, None) == 1  # no output
    assert rows(one, 128, None, one, one, one, 1.0, 1, 0.3, 0.5, None, None, one, one, one, 8, 128, 128, None) == 1  # lik without z
    assert rows(one, 128, one, one, one, one, 1.0, 1, 0.3, 1.5, None, None, one, one, one, 8, 128, 128, None) == 1  # beta
    assert rows(one, 128, one, one, one, one, 1.0, 3, 0.3, 0.5, None, None, one, one, one, 8, 128, 128, None) == 1  # coupled lik


def test_product_path_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = pkg()
    m = p.t_VGP((np.linspace(0, 1, 6)[:, None], np.zeros((6, 1))), p.SquaredExponential(), p.Gaussian(0.1))
    for call in (m.elbo, m.update_variational_parameters, lambda: m.predict_f(np.zeros((3, 1))), lambda: m.q_alpha,
                 m.maximum_log_likelihood_objective):
        with pytest.raises(p.HipExtensionError):
            call()
