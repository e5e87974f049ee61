"""CPU checks of the heteroskedastic likelihood: the NumPy restatement (tests/hetero_ref.py) pinned against closed forms,
finite differences and a brute-force integral; the package's likelihood class (its torch predictive helpers, its argument
handling) against the restatement; the model's shape errors and the C-ABI map's argument validation (no GPU needed)."""
import math

import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests.hetero_ref import LOG_2PI, HeteroskedasticTFPConditional as RefHetero
from tests.helpers import pkg


def _moments(n=40, seed=0, v1max=1.0):
    rng = np.random.RandomState(seed)
    mu = np.stack([rng.randn(n), 0.5 * rng.randn(n)], axis=1)
    var = np.stack([rng.uniform(0.05, 2.0, n), rng.uniform(0.01, v1max, n)], axis=1)
    y = (mu[:, :1] + rng.randn(n, 1))
    return mu, var, y


def test_variational_expectations_match_the_closed_form():
    mu, var, y = _moments()
    ve = RefHetero().variational_expectations(mu, var, y)
    closed = (-0.5 * LOG_2PI - mu[:, 1] - 0.5 * ((y[:, 0] - mu[:, 0]) ** 2 + var[:, 0]) * np.exp(-2 * mu[:, 1] + 2 * var[:, 1]))
    np.testing.assert_allclose(ve, closed, rtol=1e-10, atol=1e-12)


def test_gradients_are_the_derivative_of_the_quadrature_sum():
    mu, var, y = _moments(n=12, seed=1)
    lik = RefHetero()
    g0, g1 = lik.variational_expectations_grads(mu, var, y)
    for p in range(2):
        h = 1e-6
        up, dn = mu.copy(), mu.copy()
        up[:, p] += h
        dn[:, p] -= h
        fd0 = (lik.variational_expectations(up, var, y) - lik.variational_expectations(dn, var, y)) / (2 * h)
        np.testing.assert_allclose(g0[:, p], fd0, rtol=1e-6, atol=1e-8)
        hv = 1e-7
        up, dn = var.copy(), var.copy()
        up[:, p] += hv
        dn[:, p] -= hv
        fd1 = (lik.variational_expectations(mu, up, y) - lik.variational_expectations(mu, dn, y)) / (2 * hv)
        np.testing.assert_allclose(g1[:, p], fd1, rtol=1e-5, atol=1e-7)


def test_predictive_moments_match_the_closed_form():
    mu, var, _ = _moments(seed=2)
    ey, vy = RefHetero().predict_mean_and_var(mu, var)
    np.testing.assert_allclose(ey[:, 0], mu[:, 0], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(vy[:, 0], var[:, 0] + np.exp(2 * mu[:, 1] + 2 * var[:, 1]), rtol=1e-10)


def test_log_density_matches_a_brute_force_integral():
    mu = np.array([[0.3, -0.2], [-1.0, 0.4], [0.0, 0.0]])
    var = np.array([[0.4, 0.05], [0.2, 0.1], [1.0, 0.02]])
    y = np.array([[0.8], [-1.5], [0.1]])
    got = RefHetero().predict_log_density(mu, var, y)
    for n in range(3):
        s0, s1 = np.sqrt(var[n])
        f0 = np.linspace(mu[n, 0] - 10 * s0, mu[n, 0] + 10 * s0, 2001)
        f1 = np.linspace(mu[n, 1] - 10 * s1, mu[n, 1] + 10 * s1, 2001)
        F0, F1 = np.meshgrid(f0, f1, indexing="ij")
        q = (np.exp(-0.5 * (F0 - mu[n, 0]) ** 2 / var[n, 0]) / np.sqrt(2 * np.pi * var[n, 0])
             * np.exp(-0.5 * (F1 - mu[n, 1]) ** 2 / var[n, 1]) / np.sqrt(2 * np.pi * var[n, 1]))
        dens = q * np.exp(RefHetero.log_prob(F0, F1, y[n, 0]))
        brute = np.log(np.trapezoid(np.trapezoid(dens, f1, axis=1), f0))
        assert abs(got[n] - brute) < 1e-6, (n, got[n], brute)


def test_first_latent_reduces_to_the_gaussian_likelihood_at_zero_log_scale_variance():
    mu, var, y = _moments(seed=3)
    var[:, 1] = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        g0, g1 = RefHetero().variational_expectations_grads(mu, var, y)
    for n in range(0, 40, 7):
        gauss = O.Gaussian(variance=np.exp(2 * mu[n, 1]))
        r0, r1 = gauss.variational_expectations_grads(mu[n:n + 1, :1], var[n:n + 1, :1], y[n:n + 1])
        np.testing.assert_allclose(g0[n, 0], r0[0, 0], rtol=1e-12)
        np.testing.assert_allclose(g1[n, 0], r1[0, 0], rtol=1e-12)


def test_likelihood_class_predictions_match_the_restatement():
    p = pkg()
    mu, var, y = _moments(seed=4)
    lik = p.HeteroskedasticTFPConditional()
    assert lik.latent_dim == 2 and lik.lik_id == p._backend.LIK_HETERO
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    ey, vy = lik.predict_mean_and_var(t(mu), t(var))
    ey_r, vy_r = RefHetero().predict_mean_and_var(mu, var)
    np.testing.assert_allclose(ey.numpy(), ey_r, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(vy.numpy(), vy_r, rtol=1e-13)
    lpd = lik.predict_log_density(t(mu), t(var), t(y))
    assert lpd.shape == (40,)
    np.testing.assert_allclose(lpd.numpy(), RefHetero().predict_log_density(mu, var, y), rtol=1e-12)


def test_likelihood_class_accepts_the_notebook_arguments_only():
    p = pkg()

    class Normal:  # stand-ins for tfp.distributions.Normal / tfp.bijectors.Exp (tfp is not a dependency)
        pass

    class Exp:
        pass

    class StudentT:
        pass

    class Softplus:
        pass

    p.HeteroskedasticTFPConditional()
    p.HeteroskedasticTFPConditional(distribution_class=Normal, scale_transform=Exp())
    p.HeteroskedasticTFPConditional(Normal, Exp)
    with pytest.raises(NotImplementedError):
        p.HeteroskedasticTFPConditional(distribution_class=StudentT)
    with pytest.raises(NotImplementedError):
        p.HeteroskedasticTFPConditional(scale_transform=Softplus())


def test_model_shape_errors():
    p = pkg()
    Z = np.linspace(0, 1, 6)[:, None]
    lik = p.HeteroskedasticTFPConditional()
    for P in (1, 3):
        with pytest.raises(ValueError):
            p.t_SVGP(p.SquaredExponential(), lik, Z, num_latent_gps=P)
    with pytest.raises(ValueError):
        p.t_SVGP(p.SeparateIndependent([p.SquaredExponential(), p.SquaredExponential(), p.SquaredExponential()]), lik,
                 p.SharedIndependentInducingVariables(Z), num_latent_gps=3)
    m = p.t_SVGP(p.SeparateIndependent([p.SquaredExponential(), p.SquaredExponential()]), lik,
                 p.SharedIndependentInducingVariables(Z), num_latent_gps=2)
    X = np.linspace(0, 1, 10)[:, None]
    for Y in (np.zeros((10, 2)), np.zeros(10), np.zeros((9, 1))):
        for call in (m.natgrad_step, m.elbo, m.elbo_and_grads, m.moments_and_gradients, m.predict_log_density):
            with pytest.raises(ValueError):
                call((X, Y))
    with pytest.raises(NotImplementedError):
        p.t_SVGP_white(p.SquaredExponential(), lik, Z)
    with pytest.raises(NotImplementedError):
        p.t_SVGP_white(p.SquaredExponential(), lik, Z, num_latent_gps=2)


def test_map_argument_validation_needs_no_gpu():
    lib = pkg()._backend.lib()
    B = pkg()._backend
    for fn in (lib.tsvgp_lik_map_hetero_f64, lib.tsvgp_lik_map_hetero_f32):
        assert fn(None, None, None, B.LIK_HETERO, None, None, None, None, 10, 128, None) == 1
        fake = 4096  # never dereferenced: every call below is rejected before a launch
        for flags in (B.LIK_GAUSSIAN, B.LIK_BERNOULLI, B.LIK_NONE, B.LIK_HETERO | B.LIK_MEANONLY, B.LIK_HETERO | 0x1000):
            assert fn(fake, fake, fake, flags, fake, fake, fake, fake, 10, 128, None) == 1
        assert fn(fake, fake, fake, B.LIK_HETERO, fake, fake, fake, fake, 10, 100, None) == 1  # Np not a multiple of 128
        assert fn(fake, fake, fake, B.LIK_HETERO, fake, fake, fake, fake, 200, 128, None) == 1  # Np < N
        assert fn(fake, fake, fake, B.LIK_HETERO, fake, fake, fake, fake, 0, 128, None) == 1
    # the other maps keep rejecting the coupled selector
    assert lib.tsvgp_lik_map_f64(4096, 4096, 4096, B.LIK_HETERO, 0.0, 4096, 4096, 4096, 4096, 10, 128, 2, None) == 1
    assert lib.tsvgp_moments_f64(4096, 4096, 4096, 4096, 1.0, B.LIK_HETERO, 0.0, 4096, 4096, 4096, 4096, 4096, 4096, 10, 128,
                                 128, 2, 1, None) == 1
    assert math.isfinite(float(B.ABI_VERSION)) and lib.tsvgp_abi_version() == B.ABI_VERSION == 5
