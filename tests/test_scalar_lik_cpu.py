"""The StudentT and Poisson likelihoods without a GPU: the NumPy restatement the GPU tests compare with (tests/scalar_lik_ref.py)
checked on its own -- against SciPy's densities, against difference quotients of its own variational expectations, the Poisson
closed form against 20-point Gauss-Hermite, StudentT at df = 1e8 against the Gaussian map -- the host-side step built on it (the
oracle's t_SVGP with the restated likelihood) at its fixed point, and the host logic of the package around the new likelihoods.

Every tolerance below is computed in the test from the step size / the quadrature remainder and printed (run with -s).
"""
import ctypes
import math

import numpy as np
import pytest
import scipy.stats
import torch

from oracle import tsvgp_oracle as O
from tests.helpers import pkg
from tests.scalar_lik_ref import Poisson as RefPoisson
from tests.scalar_lik_ref import StudentT as RefStudentT

EPS = np.finfo(np.float64).eps


def _student_inputs(N=200, seed=0, scale=0.7):
    rng = np.random.RandomState(seed)
    m = rng.randn(N, 1)
    v = rng.uniform(0.05, 3.0, (N, 1))
    y = m + scale * rng.standard_t(3.0, (N, 1))
    y[::17] += 50.0 * scale  # gross outliers
    return m, v, y


def _poisson_inputs(N=200, seed=1, vmax=4.0):
    rng = np.random.RandomState(seed)
    m = rng.uniform(-5.0, 5.0, (N, 1))
    v = rng.uniform(1e-6, vmax, (N, 1))
    y = rng.choice([0.0, 1.0, 7.0, 1000.0], (N, 1))
    return m, v, y


# ------------------------------------------------------------------------------------------------------- log densities
@pytest.mark.parametrize("df", [2.5, 3.0, 30.0])
def test_student_log_prob_matches_scipy(df):
    rng = np.random.RandomState(0)
    f, y = rng.randn(500), rng.randn(500) * 5.0
    y[::10] *= 200.0  # residuals up to ~1e3 scale
    lik = RefStudentT(scale=0.7, df=df)
    ref = scipy.stats.t.logpdf(y, df, loc=f, scale=0.7)
    tol = 64 * EPS * np.max(np.abs(ref))  # both sides: a handful of fp64 operations on values of this size
    print(f"student logp df={df}: max |diff| {np.max(np.abs(lik.log_prob(f, y) - ref)):.2e}, tol {tol:.2e}")
    assert np.max(np.abs(lik.log_prob(f, y) - ref)) <= tol


@pytest.mark.parametrize("binsize", [1.0, 0.25])
def test_poisson_log_prob_matches_scipy(binsize):
    rng = np.random.RandomState(0)
    f = rng.uniform(-5.0, 5.0, 400)
    y = rng.choice([0.0, 1.0, 7.0, 1000.0], 400)
    ref = scipy.stats.poisson.logpmf(y, binsize * np.exp(f))
    got = RefPoisson(binsize).log_prob(f, y)
    tol = 64 * EPS * np.max(np.abs(ref))
    print(f"poisson logp b={binsize}: max |diff| {np.max(np.abs(got - ref)):.2e}, tol {tol:.2e}")
    assert np.max(np.abs(got - ref)) <= tol


# ------------------------------------------------------------------------------------------------------- gradients
def _central(fun, x, h):
    """Central difference quotients of fun at x with steps h and h / 2 and the a-posteriori bound of the finer one: the scheme
    is O(h^2), so its truncation error at h / 2 is |D_h - D_{h/2}| / 3 to leading order (doubled here), and each quotient carries
    2 eps |fun| / step of rounding."""
    d1 = (fun(x + h) - fun(x - h)) / (2.0 * h)
    d2 = (fun(x + 0.5 * h) - fun(x - 0.5 * h)) / h
    tol = 2.0 * np.abs(d1 - d2) / 3.0 + 8.0 * EPS * np.max(np.abs(fun(x))) / h + 1e-300
    return d2, tol


def _assert_within(name, got, ref, tol):
    err = np.abs(got - ref)
    worst = np.argmax(err / tol)
    print(f"{name}: max |diff| {err.max():.3e}, max tol {tol.max():.3e}, worst ratio {float((err / tol).flat[worst]):.3f}")
    assert np.all(err <= tol)


@pytest.mark.parametrize("df", [2.5, 3.0, 30.0])
def test_student_grads_match_difference_quotients(df):
    m, v, y = _student_inputs()
    lik = RefStudentT(scale=0.7, df=df)
    g0, g1 = lik.variational_expectations_grads(m, v, y)
    h = 1e-4
    d0, t0 = _central(lambda mm: lik.variational_expectations(mm, v, y), m, h)
    d1, t1 = _central(lambda vv: lik.variational_expectations(m, vv, y), v, h * v)  # a relative step: v goes down to 0.05
    _assert_within(f"student g0 df={df}", g0, d0, t0)
    _assert_within(f"student g1 df={df}", g1, d1, t1)
    ds = lik.variational_expectations_dscale(m, v, y)
    dd, ts = _central(lambda s: lik.variational_expectations(m, v, y, scale=s), np.full_like(m, 0.7), h)
    _assert_within(f"student d/dscale df={df}", ds, dd, ts)
    assert (g1 > 0).any(), "the Student-t is not log-concave: some d ve / d var are positive at the outliers"


def test_poisson_grads_match_difference_quotients():
    m, v, y = _poisson_inputs()
    lik = RefPoisson(binsize=0.5)
    g0, g1 = lik.variational_expectations_grads(m, v, y)
    h = 1e-4
    d0, t0 = _central(lambda mm: lik.variational_expectations(mm, v, y), m, h)
    d1, t1 = _central(lambda vv: lik.variational_expectations(m, vv, y), v, h * v)
    _assert_within("poisson g0", g0, d0, t0)
    _assert_within("poisson g1", g1, d1, t1)


# ------------------------------------------------------------------------------------------------------- cross-checks
def _gh_exp_remainder(s):
    """Bound on |E[exp(s z)] - sum_i w_i exp(s z_i)|, z ~ N(0, 1), for the 20-point rule: it is exact for polynomials up to degree
    39, so only the terms k >= 40 of the exponential series are left, each at most s^k / k! (E|z|^k + max_i |z_i|^k)."""
    if s <= 0:
        return 0.0
    zmax = np.max(np.abs(O.gh_points_and_weights(20)[0]))
    total = 0.0
    for k in range(40, 400):  # E|z|^k = 2^(k/2) Gamma((k+1)/2) / sqrt(pi); every term in log space
        log_abs_moment = 0.5 * k * math.log(2.0) + math.lgamma(0.5 * (k + 1)) - 0.5 * math.log(math.pi)
        log_coef = k * math.log(s) - math.lgamma(k + 1)
        total += math.exp(log_coef + log_abs_moment) + math.exp(log_coef + k * math.log(zmax))
    return total


def test_poisson_closed_form_matches_gauss_hermite_for_small_variances():
    m, v, y = _poisson_inputs(vmax=1.0)
    lik = RefPoisson(binsize=2.0)
    closed = lik.variational_expectations(m, v, y)
    quad = lik.variational_expectations_quadrature(m, v, y)
    # the linear term y f and the constants are integrated exactly; what is left is b e^m times the remainder of E[e^(s z)]
    rem = np.array([_gh_exp_remainder(s) for s in np.sqrt(v[:, 0])])[:, None]
    tol = lik.binsize * np.exp(m) * rem + 64 * EPS * np.maximum(np.abs(closed), 1.0)
    _assert_within("poisson closed form vs 20-point Gauss-Hermite", quad, closed, tol)
    assert rem.max() < 1e-11  # v <= 1: the rule resolves the exponential far below the project's 1e-8


def test_student_with_huge_df_is_the_gaussian_map():
    m, v, y = _student_inputs(scale=0.7)
    y = m + 0.7 * np.random.RandomState(3).randn(*m.shape)  # no outliers: r^4 / nu stays small
    nu, s = 1e8, 0.7
    lik, gauss = RefStudentT(scale=s, df=nu), O.Gaussian(variance=s * s)
    z = np.max(np.abs(O.gh_points_and_weights(20)[0]))
    R = (np.abs(y - m) + z * np.sqrt(v)) / s  # the largest standardised residual any node sees
    # (nu+1)/2 log1p(r^2/nu) = r^2/2 + O(r^2/(2 nu) + r^4/(4 nu)); the normalising constants differ by O(1/nu) and by the
    # rounding of lgamma(nu/2) ~ 8e8, two ulps of which is the larger term
    ulp = np.spacing(math.lgamma(0.5 * nu))
    tol_ve = (R ** 2 / (2 * nu) + R ** 4 / (4 * nu)) + 1.0 / nu + 4 * ulp
    ve_g = -0.5 * np.log(2 * np.pi) - 0.5 * np.log(s * s) - 0.5 * ((y - m) ** 2 + v) / (s * s)
    _assert_within("student(df=1e8) ve vs gaussian", lik.variational_expectations(m, v, y), ve_g, tol_ve)
    g0, g1 = lik.variational_expectations_grads(m, v, y)
    r0, r1 = gauss.variational_expectations_grads(m, v, y)
    # l' = (r / s) (1 + 1/nu) / (1 + r^2/nu): relative deviation <= (1 + R^2) / nu at every node
    tol0 = (R / s) * (1 + R ** 2) / nu + 64 * EPS * np.abs(r0).max()
    tol1 = z * (R / s) * (1 + R ** 2) / nu / (2 * np.sqrt(v)) + 64 * EPS / np.sqrt(v) * (R / s).max()
    _assert_within("student(df=1e8) g0 vs gaussian", g0, r0, tol0)
    _assert_within("student(df=1e8) g1 vs gaussian", g1, r1, tol1)


# ------------------------------------------------------------------------------------------------------- predictive helpers
def test_package_helpers_match_restatement():
    p = pkg()
    m, v, y = _student_inputs(50)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    lik, ref = p.StudentT(scale=0.7, df=3.0), RefStudentT(0.7, 3.0)
    np.testing.assert_allclose(lik.predict_log_density(t(m), t(v), t(y)).numpy(), ref.predict_log_density(m, v, y), rtol=1e-12)
    mu, var = lik.predict_mean_and_var(t(m), t(v))
    np.testing.assert_allclose(var.numpy(), ref.predict_mean_and_var(m, v)[1], rtol=1e-14)
    np.testing.assert_array_equal(mu.numpy(), m)
    np.testing.assert_allclose(lik.log_prob(t(m), t(y)).numpy(), ref.log_prob(m, y), rtol=1e-12, atol=1e-13)
    m, v, y = _poisson_inputs(50)
    lik, ref = p.Poisson(binsize=0.5), RefPoisson(0.5)
    np.testing.assert_allclose(lik.predict_log_density(t(m), t(v), t(y)).numpy(), ref.predict_log_density(m, v, y), rtol=1e-12)
    for a, b in zip(lik.predict_mean_and_var(t(m), t(v)), ref.predict_mean_and_var(m, v)):
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-12)
    # 20 nodes against the closed form of the log-normal mean at a small variance
    mu, _ = ref.predict_mean_and_var(np.zeros((1, 1)), np.full((1, 1), 0.25))
    np.testing.assert_allclose(mu, 0.5 * math.exp(0.125), rtol=1e-12)


# ------------------------------------------------------------------------------------------------------- host-side step
def test_poisson_fit_is_stationary_at_convergence():
    """The reference's own fixed-point pin (its tests assert the ELBO to decimal=4 across a further step at convergence), with
    the restated likelihood plugged into the oracle's t_SVGP."""
    rng = np.random.RandomState(0)
    N, M = 100, 10
    X = np.sort(rng.rand(N, 1) * 4 - 2, axis=0)
    Y = rng.poisson(np.exp(1.0 + np.sin(2 * X))).astype(np.float64)
    Z = np.linspace(-2, 2, M)[:, None]
    model = O.t_SVGP(O.SquaredExponential(variance=1.0, lengthscales=0.8), RefPoisson(), Z)
    for _ in range(40):
        model.natgrad_step((X, Y), lr=0.8)
    e0 = model.elbo((X, Y))
    model.natgrad_step((X, Y), lr=0.8)
    e1 = model.elbo((X, Y))
    print(f"poisson fixed point: elbo {e0:.8f} -> {e1:.8f}")
    np.testing.assert_almost_equal(e1, e0, decimal=4)
    mu, _ = model.predict_y(X)
    assert np.corrcoef(mu[:, 0], np.exp(1.0 + np.sin(2 * X))[:, 0])[0, 1] > 0.9


# ------------------------------------------------------------------------------------------------------- host logic
def test_package_exports_the_new_likelihoods():
    p = pkg()
    assert {"StudentT", "Poisson"} <= set(p.__all__)
    B = p._backend
    assert p.StudentT.lik_id == B.LIK_STUDENT_T and p.Poisson.lik_id == B.LIK_POISSON
    assert p.StudentT.latent_dim == 1 and p.Poisson.latent_dim == 1
    assert p.StudentT(2.0, 4.0).lik_param == (2.0, 4.0) and p.Poisson(0.5).lik_param == (0.5, 0.0)
    assert {B.LIK_STUDENT_T, B.LIK_POISSON}.isdisjoint(B.COUPLED_LIKS) and set(B.SCALAR_MAP_LIKS) <= set(B.MAPPED_LIKS)


def test_constructor_and_helper_errors():
    p = pkg()
    for df in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError):
            p.StudentT(df=df)
    with pytest.raises(ValueError):
        p.StudentT(scale=0.0)
    one = torch.ones(2, 1, dtype=torch.float64)
    for df in (2.0, 1.5):  # a valid density, but no predictive variance
        with pytest.raises(ValueError, match="df <= 2"):
            p.StudentT(df=df).predict_mean_and_var(one, one)
    with pytest.raises(NotImplementedError, match="exp inverse link"):
        p.Poisson(invlink=torch.square)
    with pytest.raises(NotImplementedError):
        p.Poisson(foo=1)
    with pytest.raises(ValueError):
        p.Poisson(binsize=0.0)
    p.Poisson(invlink=torch.exp)
    p.Poisson(invlink=np.exp)


@pytest.mark.parametrize("name", ["StudentT", "Poisson"])
def test_fused_models_refuse_the_new_likelihoods(name):
    p = pkg()
    lik = getattr(p, name)()
    X, Y, Z = np.zeros((4, 1)), np.ones((4, 1)), np.zeros((2, 1))
    with pytest.raises(NotImplementedError, match=name):
        p.t_VGP((X, Y), p.SquaredExponential(), lik)
    with pytest.raises(NotImplementedError, match=name):
        p.t_SVGP_sites((X, Y), p.SquaredExponential(), lik, Z)


def test_trainable_parameters_list_the_scale():
    p = pkg()
    training = __import__("importlib").import_module("t-svgp_amd.training")
    lik = p.StudentT(scale=0.5, df=4.0)
    model = p.t_SVGP(p.SquaredExponential(), lik, np.zeros((3, 1)))
    assert any(par is lik.scale for par in model.trainable_parameters)
    named = training.trainable_parameters(model)
    assert named["likelihood_scale"][0] is lik.scale and named["likelihood_scale"][1] == 0.0
    assert "likelihood_variance" not in named
    assert "likelihood_scale" not in training.trainable_parameters(p.t_SVGP(p.SquaredExponential(), p.Poisson(), np.zeros((3, 1))))
    assert lik.graph_key() == (4.0,)  # df is no Parameter: a captured step is keyed on it through this


def test_cabi_rejects_bad_arguments_without_a_gpu():
    """Argument validation comes before any device call: every line below returns TSVGP_EINVAL on a machine with no GPU."""
    B = pkg()._backend
    lib = B.lib()
    buf = (ctypes.c_double * 256)()
    ibuf = (ctypes.c_int32 * 2)()
    a = ctypes.addressof(buf)
    ia = ctypes.addressof(ibuf)
    S, Pn = B.LIK_STUDENT_T, B.LIK_POISSON

    def call(fn=lib.tsvgp_lik_map_scalar_f64, mean=a, var=a, Y=a, istride=1, lik=S, p0=1.0, p1=3.0, g0=a, g1=a, ostride=1, ve=a,
             dpar=None, nonpos=ia, N=100, Np=128):
        return fn(mean, var, Y, istride, lik, p0, p1, g0, g1, ostride, ve, dpar, nonpos, N, Np, None)

    for fn in (lib.tsvgp_lik_map_scalar_f64, lib.tsvgp_lik_map_scalar_f32):
        for bad in (dict(mean=None), dict(var=None), dict(Y=None), dict(g0=None), dict(g1=None), dict(ve=None), dict(nonpos=None),
                    dict(N=0), dict(N=129), dict(Np=100), dict(istride=0), dict(ostride=0), dict(ostride=-2),
                    dict(lik=B.LIK_GAUSSIAN), dict(lik=B.LIK_BERNOULLI), dict(lik=B.LIK_HETERO), dict(lik=S | B.LIK_MEANONLY),
                    dict(p0=0.0), dict(p0=-1.0), dict(p0=float("nan")), dict(p1=0.0), dict(p1=float("inf")),
                    dict(lik=Pn, p0=0.0), dict(lik=Pn, p0=float("inf")), dict(lik=Pn, dpar=a)):
            assert call(fn=fn, **bad) == 1, bad
