"""LinearCoregionalization without a GPU: the NumPy restatement the GPU tests compare with (tests/lmc_ref.py) checked on its own
-- the gradients of ``Mixed`` over the latent moments against central difference quotients of its own variational
expectations -- and the host logic of the package around the new kernel class: validation, exports, the refusals, the trainable
W, the two new C entries' symbols, prototypes and argument checks, and the loud failure of the product path without a device.
"""
import ctypes
import importlib
import re

import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests import lmc_ref
from tests.helpers import pkg
from tests.scalar_lik_ref import Poisson as RefPoisson

W23 = np.array([[0.9, -0.4], [0.0, 1.3], [-0.7, 0.5]])  # P = 3, L = 2, mixed signs


def _latent_moments(N=60, L=2, seed=0):
    rng = np.random.RandomState(seed)
    return rng.uniform(-1.5, 1.5, (N, L)), rng.uniform(0.05, 1.5, (N, L))


def _targets(base, N, P, seed=1):
    rng = np.random.RandomState(seed)
    if base == "gaussian":
        return O.Gaussian(0.3), rng.randn(N, P)
    if base == "bernoulli":
        return O.Bernoulli(), (rng.rand(N, P) > 0.5).astype(np.float64)
    return RefPoisson(), rng.poisson(2.0, (N, P)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("base", ["gaussian", "bernoulli", "poisson"])
def test_mixed_grads_match_central_differences_of_its_own_ve(base):
    """h = 1e-6; 1e-7 relative to the largest gradient entry (truncation ~h^2 |ve'''| / 6 ~ 1e-12, rounding ~eps |ve| / h ~ 1e-8
    of a ve of a few tens: both well inside).  ve is a sum over rows of per-row terms, so one perturbed column moves every
    row's own term only: the quotient of the per-row ve is the row's derivative."""
    m, v = _latent_moments()
    lik_base, Y = _targets(base, m.shape[0], W23.shape[0])
    lik = lmc_ref.Mixed(W23, lik_base)
    g0, g1 = lik.variational_expectations_grads(m, v, Y)
    assert g0.shape == m.shape and g1.shape == v.shape
    h = 1e-6
    for l in range(m.shape[1]):
        e = np.zeros_like(m)
        e[:, l] = h
        d0 = (lik.variational_expectations(m + e, v, Y) - lik.variational_expectations(m - e, v, Y)) / (2 * h)
        d1 = (lik.variational_expectations(m, v + e, Y) - lik.variational_expectations(m, v - e, Y)) / (2 * h)
        r0 = np.max(np.abs(d0 - g0[:, l])) / max(np.max(np.abs(g0)), 1.0)
        r1 = np.max(np.abs(d1 - g1[:, l])) / max(np.max(np.abs(g1)), 1.0)
        print(f"{base} latent {l}: g0 rel {r0:.2e}, g1 rel {r1:.2e}")
        assert r0 < 1e-7 and r1 < 1e-7


def test_dW_matches_central_differences_of_the_summed_ve():
    m, v = _latent_moments(seed=3)
    lik_base, Y = _targets("bernoulli", m.shape[0], W23.shape[0])
    g0_f, g1_f = lmc_ref.Mixed(W23, lik_base).output_grads(m, v, Y)
    got = lmc_ref.dW(W23, g0_f, g1_f, m, v)
    h = 1e-6
    for p in range(W23.shape[0]):
        for l in range(W23.shape[1]):
            e = np.zeros_like(W23)
            e[p, l] = h
            d = (np.sum(lmc_ref.Mixed(W23 + e, lik_base).variational_expectations(m, v, Y))
                 - np.sum(lmc_ref.Mixed(W23 - e, lik_base).variational_expectations(m, v, Y))) / (2 * h)
            assert abs(d - got[p, l]) < 1e-7 * max(np.max(np.abs(got)), 1.0)


def test_mix_and_unmix_are_adjoint_and_identity_is_exact():
    m, v = _latent_moments(seed=5)
    Fmu, Fvar = lmc_ref.mix(np.eye(2), m, v)
    assert np.array_equal(Fmu, m) and np.array_equal(Fvar, v)
    rng = np.random.RandomState(7)
    a, b = rng.randn(m.shape[0], 3), rng.randn(m.shape[0], 3)
    Fmu, Fvar = lmc_ref.mix(W23, m, v)
    g0, g1 = lmc_ref.unmix(W23, a, b, crop=False)
    np.testing.assert_allclose(np.sum(a * Fmu) + np.sum(b * Fvar), np.sum(g0 * m) + np.sum(g1 * v), rtol=1e-13)
    cov = lmc_ref.full_output_cov(W23, v)
    np.testing.assert_allclose(np.einsum("npp->np", cov), Fvar, rtol=1e-14)
    _, g1c = lmc_ref.unmix(W23, a, b)
    assert np.all(g1c <= -1e-8) and np.array_equal(g1c[g1 <= -1e-8], g1[g1 <= -1e-8])


# ------------------------------------------------------------------------------------------------------- the kernel class
def _kernels(p, L):
    return [p.SquaredExponential(variance=1.0 + 0.1 * l, lengthscales=0.8 + 0.1 * l) for l in range(L)]


def test_class_shape_and_prior_variances():
    p = pkg()
    assert "LinearCoregionalization" in p.__all__
    k = p.LinearCoregionalization(_kernels(p, 2), W23)
    assert isinstance(k, p.SeparateIndependent)
    assert k.num_latent_gps == 2 and k.num_outputs == 3
    assert k.W.shape == (3, 2) and k.W.trainable
    X = np.zeros((5, 2))
    want = np.tile(((W23 * W23) @ np.array([1.0, 1.1]))[None, :], (5, 1))
    np.testing.assert_allclose(k.K_diag(X).cpu().numpy(), want, rtol=1e-14)
    assert k.device_W("cpu") is k.device_W("cpu") and k.device_W("cpu").dtype == torch.float64
    before = k.device_W("cpu")
    k.W.assign(2.0 * W23)
    after = k.device_W("cpu")
    assert after is not before and np.array_equal(after.numpy(), 2.0 * W23)


def test_class_validation():
    p = pkg()
    with pytest.raises(ValueError, match="W must be"):
        p.LinearCoregionalization(_kernels(p, 3), W23)  # three kernels, two columns
    with pytest.raises(ValueError, match="W must be"):
        p.LinearCoregionalization(_kernels(p, 2), np.ones(2))
    for bad in (float("nan"), float("inf")):
        Wb = W23.copy()
        Wb[1, 0] = bad
        with pytest.raises(ValueError, match="finite"):
            p.LinearCoregionalization(_kernels(p, 2), Wb)
    with pytest.raises(ValueError, match="at most 32"):
        p.LinearCoregionalization(_kernels(p, 2), np.ones((33, 2)))
    with pytest.raises(ValueError, match="at most 32"):
        p.LinearCoregionalization(_kernels(p, 33), np.ones((2, 33)))
    with pytest.raises(ValueError):
        p.LinearCoregionalization([], np.ones((2, 0)))
    p.LinearCoregionalization(_kernels(p, 32), np.ones((32, 32)))
    k = p.LinearCoregionalization(_kernels(p, 2), W23)
    k.W.value[0, 0] = float("nan")  # an edit behind the class's back is caught where the value is next handed to a kernel
    with pytest.raises(ValueError, match="finite"):
        k.device_W("cpu")


def _model(p, **kw):
    return p.t_SVGP(p.LinearCoregionalization(_kernels(p, 2), W23), kw.pop("lik", None) or p.Gaussian(0.1), np.zeros((4, 2)) + np.arange(4)[:, None],
                    num_latent_gps=2, **kw)


def test_model_refusals_are_by_name():
    p = pkg()
    Z = np.zeros((4, 2)) + np.arange(4)[:, None]
    X, Y = np.zeros((5, 2)), np.zeros((5, 3))
    kern = lambda: p.LinearCoregionalization(_kernels(p, 2), W23)
    with pytest.raises(ValueError, match="num_latent_gps must be 2"):
        p.t_SVGP(kern(), p.Gaussian(0.1), Z, num_latent_gps=3)
    with pytest.raises(NotImplementedError, match="LinearCoregionalization"):
        p.t_SVGP_white(kern(), p.Gaussian(0.1), Z)
    with pytest.raises(NotImplementedError, match="LinearCoregionalization"):
        p.t_SVGP_sites((X, Y), kern(), p.Gaussian(0.1), Z)
    with pytest.raises(NotImplementedError, match="LinearCoregionalization"):
        p.t_VGP((X, Y), kern(), p.Gaussian(0.1))
    with pytest.raises(NotImplementedError, match="LinearCoregionalization"):
        p.select_inducing_points(X, kern(), 2)
    with pytest.raises(NotImplementedError, match="latent_split"):
        _model(p, latent_split=True)
    for lik in (p.HeteroskedasticTFPConditional(), p.Softmax(2), p.MultiClass(2)):
        with pytest.raises(NotImplementedError, match="LinearCoregionalization"):
            _model(p, lik=lik)
    m = _model(p)
    Xg = torch.zeros((5, 2), dtype=torch.float64, requires_grad=True)
    calls = {
        "full_cov": lambda: m.predict_f(X, full_cov=True),
        "new_predict_f": lambda: m.new_predict_f(X),
        "predict_f_samples": lambda: m.predict_f_samples(X, 2),
        "predict_f_samples marginal": lambda: m.predict_f_samples(X, 2, full_cov=False),
        "sample_functions": lambda: m.sample_functions(2),
        "predict_f_vjp": lambda: m.predict_f_vjp(X, np.zeros((5, 3))),
        "autograd": lambda: m.predict_f(Xg),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match="LinearCoregionalization"):
            call()
    # the other models' refusals of SeparateIndependent stand as they were
    sep = p.SeparateIndependent(_kernels(p, 2))
    with pytest.raises(NotImplementedError, match="one shared kernel"):
        p.t_SVGP_white(sep, p.Gaussian(0.1), Z)
    with pytest.raises(ValueError, match="one kernel"):
        p.t_VGP((X, Y[:, :1]), sep, p.Gaussian(0.1))


def test_W_is_trainable_and_unconstrained():
    p = pkg()
    training = importlib.import_module("t-svgp_amd.training")
    m = _model(p)
    named = training.trainable_parameters(m)
    assert named["W"][0] is m.kernel.W and named["W"][1] is None
    assert {"kernels.0.variance", "kernels.1.lengthscales", "Z", "likelihood_variance"} <= set(named)
    assert any(par is m.kernel.W for par in m.trainable_parameters)
    sep = p.t_SVGP(p.SeparateIndependent(_kernels(p, 2)), p.Gaussian(0.1), np.zeros((4, 2)), num_latent_gps=2)
    assert "W" not in training.trainable_parameters(sep)


# ------------------------------------------------------------------------------------------------------- the C entries
NAMES = ("tsvgp_lmc_mix_f64", "tsvgp_lmc_mix_f32", "tsvgp_lmc_unmix_f64", "tsvgp_lmc_unmix_f32")


def test_new_symbols_prototypes_and_abi_version():
    B = pkg()._backend
    lib = B.lib()
    assert lib.tsvgp_abi_version() == 5 == B.ABI_VERSION  # new symbols only
    header = open(B.HEADER_PATH).read()
    assert "#define TSVGP_ABI_VERSION 5" in header
    for name in NAMES:
        assert hasattr(lib, name) and name in B.exported_symbols()
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto is not None, name
        args = [a.strip() for a in proto.group(1).replace("\n", " ").split(",")]
        assert len(args) == len(B._PROTOTYPES[name][1]), name
        assert args[-1] == "void *stream" and "const double *W" in args
    mix_args = re.search(r"\bint tsvgp_lmc_mix_f32\(([^;]*)\);", header).group(1)
    assert "const float *mean_g" in mix_args and "int32_t *nonpos_partial" in mix_args
    unmix_args = re.search(r"\bint tsvgp_lmc_unmix_f32\(([^;]*)\);", header).group(1)
    assert "double *dW_partial" in unmix_args and "int flags" in unmix_args


def test_cabi_rejects_bad_arguments_without_a_gpu():
    """Argument validation comes before any device call: every line below returns TSVGP_EINVAL on a machine with no GPU."""
    B = pkg()._backend
    lib = B.lib()
    buf = (ctypes.c_double * 2048)()
    ibuf = (ctypes.c_int32 * 2)()
    a, ia = ctypes.addressof(buf), ctypes.addressof(ibuf)

    def mix(fn, mean=a, var=a, W=a, Fmu=a, Fvar=a, nonpos=ia, N=100, Np=128, L=2, P=3):
        return fn(mean, var, W, Fmu, Fvar, nonpos, N, Np, L, P, None)

    shape_errors = (dict(N=0), dict(N=-1), dict(N=129), dict(Np=100), dict(Np=192), dict(N=100, Np=256), dict(N=1, Np=256),
                    dict(L=0), dict(L=33), dict(L=-1), dict(P=0), dict(P=33), dict(P=-1))
    for fn in (lib.tsvgp_lmc_mix_f64, lib.tsvgp_lmc_mix_f32):
        for bad in (dict(mean=None), dict(var=None), dict(W=None), dict(Fmu=None), dict(Fvar=None)) + shape_errors:
            assert mix(fn, **bad) == 1, bad

    def unmix(fn, g0f=a, g1f=a, W=a, flags=0, g0g=a, g1g=a, mean=None, var=None, dW=None, N=100, Np=128, L=2, P=3):
        return fn(g0f, g1f, W, flags, g0g, g1g, mean, var, dW, N, Np, L, P, None)

    for fn in (lib.tsvgp_lmc_unmix_f64, lib.tsvgp_lmc_unmix_f32):
        for bad in (dict(g0f=None), dict(g1f=None), dict(W=None), dict(g0g=None), dict(g1g=None), dict(dW=a), dict(dW=a, mean=a),
                    dict(dW=a, var=a), dict(flags=B.LIK_GAUSSIAN), dict(flags=B.LIK_NOCROP | B.LIK_MEANONLY),
                    dict(flags=B.LIK_NOCROP | 1)) + shape_errors:
            assert unmix(fn, **bad) == 1, bad


def test_product_path_fails_loudly_without_gpu():
    """No CPU fallback: with no ROCm device the mixed-output model refuses to run (it never routes through the reference)."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = pkg()
    m = _model(p)
    data = (np.zeros((5, 2)), np.zeros((5, 3)))
    for call in (lambda: m.natgrad_step(data), lambda: m.elbo(data), lambda: m.predict_f(data[0]), lambda: m.predict_y(data[0]),
                 lambda: m.predict_log_density(data), lambda: m.elbo_and_grads(data),
                 lambda: m.predict_f(data[0], full_output_cov=True)):
        with pytest.raises(p.HipExtensionError):
            call()
