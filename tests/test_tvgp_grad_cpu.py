"""The hyperparameter gradient of t_VGP without a GPU: the NumPy restatement of its algebra (tests/tvgp_grad_ref.py) against torch
autograd through the reference's own op sequence, against difference quotients of the restated ELBO and against the closed-form
gradient of the GPR log marginal likelihood (the stand-in for reference tests/models/test_tvgp.py::
test_gradient_wrt_hyperparameters, which needs GPflow's VGP); the conditioning of the problems the GPU test uses; the training
plumbing for a model without an inducing variable; the argument checks of the new entry point.

Every bound is stated against S_theta = sum_ij |G_ij dK_ij / d theta|, the absolute sum of the terms of the gradient
(tvgp_grad_ref.contract)."""
import contextlib
import types

import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests import tvgp_grad_ref as GR
from tests import tvgp_ref as R
from tests.helpers import pkg
from tests.test_tvgp_cpu import MODEL_CASES, reference_setup

LIKS = ["gaussian", "bernoulli"]
NEGATIVE_CASE = (128, 3, "Matern52", "gaussian")  # the case of the GPU model test that gets negative lambda_2 written by hand
TRAINING_CASE = (129, 1, "SquaredExponential", "gaussian")


def stepped_model(N, D, kernel, lik, form="solve", negative=False):
    """The restatement after the two beta = 0.5 updates of the gradient tests (h0, h1 != 0: not a fixed point of the sites);
    ``negative``: lambda_2 of every 7th datum is then replaced by -0.3 times itself (the formula uses |lambda_2| only in s)."""
    X, Y, k, l, _ = R.problem(N, D, lik, kernel)
    m = R.TVGPRef(X, Y, k, l, "solve")
    for _ in range(2):
        m.update(0.5)
    m.form = form  # both forms are compared at the SAME sites, moved by the reference's own operations
    if negative:
        m.lambda_2[::7] *= -0.3
    return m


# -- 1. torch autograd through the reference's op sequence -------------------------------------------------------------
def _torch_kernel(name, X, variance, ls):
    d = (X[:, None, :] - X[None, :, :]) / ls
    r2 = (d * d).sum(-1)
    if name == "SquaredExponential":
        return variance * torch.exp(-0.5 * r2)
    r = torch.sqrt(torch.clamp(r2, min=1e-36))
    if name == "Matern32":
        return variance * (1.0 + np.sqrt(3.0) * r) * torch.exp(-np.sqrt(3.0) * r)
    return variance * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * torch.exp(-np.sqrt(5.0) * r)


def _torch_elbo(name, X, Y, lam1, lam2, variance, ls, s2):
    """reference src/models/tvgp.py:77-111 op for op, Gaussian likelihood; the sites are constants."""
    N = X.shape[0]
    eye = torch.eye(N, dtype=torch.float64)
    pseudo_y = lam1 / lam2
    sW = torch.sqrt(torch.abs(lam2))
    K = _torch_kernel(name, X, variance, ls) + eye * R.DEFAULT_JITTER
    L = torch.linalg.cholesky(eye + (sW @ sW.T) * K)
    T = torch.linalg.solve_triangular(L, sW.repeat(1, N) * K, upper=False)
    post_v = (torch.diagonal(K) - (T * T).sum(0)).reshape(N, 1)
    alpha = sW * torch.linalg.solve_triangular(L.T, torch.linalg.solve_triangular(L, sW * pseudo_y, upper=False), upper=True)
    post_m = K @ alpha
    ve = torch.sum(-0.5 * np.log(2.0 * np.pi) - 0.5 * torch.log(s2) - 0.5 * ((Y - post_m) ** 2 + post_v) / s2)
    eqt = -torch.sum(0.5 * lam2 * ((pseudo_y - post_m) ** 2 + post_v))
    log_Z = -(pseudo_y.T @ alpha).reshape(()) / 2.0 - torch.sum(torch.log(torch.diagonal(L)))
    return log_Z - eqt + ve


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("N,D,kernel", MODEL_CASES)
def test_restatement_against_autograd(N, D, kernel, negative):
    """Bound 1e-12 S_theta: both sides are fp64 evaluations of the same quantity whose terms sum to S_theta in absolute value; the
    factorisation behind them is conditioned below 1e3 (tests/test_gpu_tvgp.py), leaving three orders of magnitude above 2^-53."""
    m = stepped_model(N, D, kernel, "gaussian", negative=negative)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    variance = t(m.kernel.variance).requires_grad_()
    ls = t(m.kernel.lengthscales).requires_grad_()
    s2 = t(m.likelihood.variance).requires_grad_()
    elbo = _torch_elbo(kernel, t(m.X), t(m.Y), t(m.lambda_1), t(m.lambda_2), variance, ls, s2)
    elbo.backward()
    assert abs(elbo.item() - m.elbo()) <= 1e-12 * abs(m.elbo())
    ref = GR.elbo_grads(m)
    for name, auto in (("variance", variance.grad), ("lengthscales", ls.grad), ("likelihood_variance", s2.grad)):
        g, S = ref[name]
        err = np.abs(np.asarray(g) - auto.numpy())
        print(f"{name}: worst |ref - autograd| / S = {np.max(err / S):.2e}")
        assert np.all(err <= 1e-12 * S)
    assert np.all(np.abs(GR.parts(m)[0] - GR.parts(m)[0].T) <= 1e-12 * np.max(np.abs(GR.parts(m)[0])))


# -- 2. difference quotients of the restated ELBO --------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["SquaredExponential", "Matern32", "Matern52"])
def test_restatement_against_difference_quotients(kernel):
    """Bernoulli likelihood (g0, g1 from the quadrature), N = 40, D = 2, ARD.  Central quotient with step h = 1e-5 theta: its
    truncation error is h^2 / 6 |ELBO'''| ~ 1e-10 theta^2 |ELBO'''|, its rounding error 2^-53 |ELBO| k / h with k ~ 10 roundings
    that do not cancel ~ 1e-15 * 30 / 1e-5 = 3e-9; the gradients are of order 1 to 10 and S_theta >= |gradient|, so the quotient
    supports 1e-6 S_theta with two orders of magnitude to spare."""
    m = stepped_model(40, 2, kernel, "bernoulli")
    ref = GR.elbo_grads(m)
    assert set(ref) == {"variance", "lengthscales"}
    base = (m.kernel.variance, m.kernel.lengthscales.copy())

    def elbo_at(variance, ls):
        m.kernel = getattr(O, kernel)(variance=variance, lengthscales=ls)
        return m.elbo()

    def quotient(make):
        theta, at = make
        h = 1e-5 * theta
        return (at(theta + h) - at(theta - h)) / (2.0 * h)

    g, S = ref["variance"]
    q = quotient((base[0], lambda v: elbo_at(v, base[1])))
    print(f"variance: {g:.10f} quotient {q:.10f} S {S:.3e}")
    assert abs(q - g) <= 1e-6 * S
    for d in range(2):
        def at(x, d=d):
            ls = base[1].copy()
            ls[d] = x
            return elbo_at(base[0], ls)

        g, S = ref["lengthscales"][0][d], ref["lengthscales"][1][d]
        q = quotient((base[1][d], at))
        print(f"lengthscale {d}: {g:.10f} quotient {q:.10f} S {S:.3e}")
        assert abs(q - g) <= 1e-6 * S


# -- 3. the reference's pin -----------------------------------------------------------------------------------------
def gpr_gradients(X, Y, kern, s2):
    """1/2 tr((alpha alpha^T - K_y^-1) dK_y / d theta) of log N(Y | 0, K_y), K_y = K + jitter I + s2 I, for theta = variance,
    lengthscale, s2 (Rasmussen & Williams [ext], eq. 5.9)."""
    k = O.SquaredExponential(**kern)
    N = X.shape[0]
    Ky = k.K(X) + (R.DEFAULT_JITTER + s2) * np.eye(N)
    Kinv = np.linalg.inv(Ky)
    a = Kinv @ Y
    Gm = 0.5 * (a @ a.T - Kinv)
    dvar, dls, _, _ = GR.contract(k, X, Gm)
    return {"variance": dvar, "lengthscales": dls, "likelihood_variance": np.trace(Gm)}


def test_gradient_wrt_hyperparameters_at_the_optimal_sites():
    """Stands in for reference tests/models/test_tvgp.py::test_gradient_wrt_hyperparameters: on its setup, after one beta = 1
    step under a Gaussian likelihood the bound is tight (the ELBO is the GPR log marginal likelihood), so the tangents agree."""
    X, Y, kern, s2 = reference_setup()
    m = R.TVGPRef(X, Y, O.SquaredExponential(**kern), O.Gaussian(variance=s2))
    m.update(beta=1.0)
    ref, gpr = GR.elbo_grads(m), gpr_gradients(X, Y, kern, s2)
    for name in ("variance", "lengthscales", "likelihood_variance"):
        np.testing.assert_almost_equal(ref[name][0], gpr[name], decimal=4)


# -- 4. conditioning ------------------------------------------------------------------------------------------------
def grad_cases():
    """Every (N, D, kernel, lik, negative) the GPU model test runs."""
    out = [(N, D, k, lik, False) for (N, D, k) in MODEL_CASES for lik in LIKS]
    return out + [NEGATIVE_CASE + (True,), TRAINING_CASE + (False,)]


@pytest.mark.parametrize("N,D,kernel,lik,negative", grad_cases())
def test_solve_form_and_inverse_form_agree(N, D, kernel, lik, negative):
    """The gradient from triangular solves against the gradient from an explicit inverse, at the same sites: 1e-9 S_theta, an
    order of magnitude inside the GPU test's 1e-8 S_theta, so that bound measures the HIP path and not the conditioning."""
    a = stepped_model(N, D, kernel, lik, "solve", negative)
    b = stepped_model(N, D, kernel, lik, "inv", negative)
    assert np.array_equal(a.lambda_1, b.lambda_1) and np.array_equal(a.lambda_2, b.lambda_2)
    ga, gb = GR.elbo_grads(a), GR.elbo_grads(b)
    assert set(ga) == set(gb)
    for name in ga:
        err = np.abs(np.asarray(ga[name][0]) - np.asarray(gb[name][0]))
        print(f"{name}: worst |solve - inv| / S = {np.max(err / ga[name][1]):.2e}")
        assert np.all(err <= 1e-9 * ga[name][1])


def test_pin_setup_is_conditioned():
    X, Y, kern, s2 = reference_setup()
    out = []
    for form in ("solve", "inv"):
        m = R.TVGPRef(X, Y, O.SquaredExponential(**kern), O.Gaussian(variance=s2), "solve")
        m.update(beta=1.0)
        m.form = form
        out.append(GR.elbo_grads(m))
    for name in out[0]:
        assert abs(out[0][name][0] - out[1][name][0]) <= 1e-9 * out[0][name][1]


# -- 5. training plumbing -------------------------------------------------------------------------------------------
def test_trainable_parameters_of_a_model_without_inducing_variable():
    p = pkg()
    from importlib import import_module

    training = import_module("t-svgp_amd.training")
    stub = types.SimpleNamespace(kernel=p.SquaredExponential(variance=1.0, lengthscales=[1.0, 2.0]), likelihood=p.Gaussian(0.1))
    names = training.trainable_parameters(stub)
    assert set(names) == {"variance", "lengthscales", "likelihood_variance"}
    stub.likelihood = p.Bernoulli()
    assert set(training.trainable_parameters(stub)) == {"variance", "lengthscales"}
    m = p.t_VGP((np.linspace(0, 1, 6)[:, None], np.zeros((6, 1))), p.SquaredExponential(), p.Gaussian(0.1))
    assert set(training.trainable_parameters(m)) == {"variance", "lengthscales", "likelihood_variance"}
    assert len(m.trainable_parameters) == 3 and callable(m.training_loss_closure())
    assert "not implemented" not in import_module("t-svgp_amd.models.tvgp").__doc__
    with (contextlib.nullcontext() if torch.cuda.is_available() else pytest.raises(p.HipExtensionError)):
        m.elbo_and_grads()


# -- 6. the entry point's argument checks ---------------------------------------------------------------------------
def test_entry_point_rejects_null_and_unpadded_arguments():
    lib = pkg()._backend.lib()
    fn = lib.tsvgp_vgp_kernel_grad_f64
    one = 16  # a non-null, 16-byte aligned address that is never dereferenced: the checks below fail before any launch
    assert fn(0, None, None, 1.0, None, 128, None, None, 8, 128, 1, None, None) == 1
    assert fn(0, one, one, 1.0, one, 128, one, one, 8, 100, 1, one, None) == 1  # Np not a multiple of 128
    assert fn(0, one, one, 1.0, one, 128, one, one, 200, 128, 1, one, None) == 1  # Np < N
    assert fn(0, one, one, 1.0, one, 256, one, one, 8, 256, 1, one, None) == 1  # Np beyond N rounded up
    assert fn(0, one, one, 1.0, one, 126, one, one, 8, 128, 1, one, None) == 1  # ldw < Np
    assert fn(0, one, one, 1.0, one, 129, one, one, 8, 128, 1, one, None) == 1  # ldw odd
    assert fn(0, one, one, 1.0, 8, 128, one, one, 8, 128, 1, one, None) == 1  # W off the 16-byte boundary
    assert fn(0, one, one, 1.0, one, 128, one, one, 8, 128, 33, one, None) == 1  # D > 32
    assert fn(0, one, one, 1.0, one, 128, one, one, 8, 128, 0, one, None) == 1  # D = 0
    assert fn(1, one, one, 1.0, one, 128, one, one, 8, 128, 1, one, None) == 1  # kind
    assert fn(0, one, one, 1.0, one, 128, None, one, 8, 128, 1, one, None) == 1  # a
    assert fn(0, one, one, 1.0, one, 128, one, one, 8, 128, 1, None, None) == 1  # part
    parts = lib.tsvgp_vgp_kernel_grad_parts
    assert parts(128, 1) == 2 * 2 and parts(384, 3) == 7 * 5 and parts(384, 32) == 7 * 33 and parts(256, 9) == 4 * 17
    assert parts(100, 1) == -1 and parts(128, 33) == -1 and parts(128, 0) == -1
