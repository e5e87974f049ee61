"""``Product`` kernels on the models, on the GPU: t_SVGP and t_SVGP_white with Matern52(active_dims=[0]) *
SquaredExponential(active_dims=[1, 2]) against the CPU oracle on the duck-typed NumPy ``Product`` of tests/product_kernel_ref.py.
N = 300, M = 24, D = 3 unless said.

Tolerances (tests/test_gpu_sum_kernel.py): fp64 relerr < 1e-8 on lambda_1, Lambda_2 and the predictions,
|dELBO| < 1e-9 |ELBO|; fp32 compute: mean, var atol 1e-4 + rtol 1e-3, ELBO 1e-4 relative.  Gradients: central differences of the
oracle's ELBO at 2e-6 max(|ref|, scale) (tests/test_gpu_mstep.py)."""
import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests import fullcov_ref
from tests import product_kernel_ref as R
from tests.helpers import pkg, relerr, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, M, D = 300, 24, 3
SPEC = [("Matern52", 1.3, 0.9, [0]), ("SquaredExponential", 0.7, [1.2, 1.5], [1, 2])]


def _lik(mod, lik, noise=0.2):
    return mod.Gaussian(noise) if lik == "gaussian" else mod.Bernoulli()


def _pair(model, lik, Z, spec=SPEC, num_data=None, noise=0.2, **kw):
    """(HIP model, oracle model) of one description."""
    p = pkg()
    hip = getattr(p, model)(R.build_pkg(p, spec), _lik(p, lik, noise), Z.copy(), num_data=num_data, **kw)
    ora = getattr(O, model)(R.build(spec), _lik(O, lik, noise), Z.copy(), num_data=num_data)
    return hip, ora


def _lambda_2(m):
    v = m.lambda_2
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else (v.numpy() if hasattr(v, "numpy") else np.asarray(v))


def _state_close(hip, ora, tol=1e-8):
    assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < tol
    assert relerr(_lambda_2(hip), ora.lambda_2) < tol


def _problem(lik, seed=7):
    X, Y, _ = synthetic(N=N, M=M, D=D, P=1, lik=lik, seed=seed)
    Z = np.random.RandomState(41).randn(M, D) * 1.2
    return X, Y, Z


@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
@pytest.mark.parametrize("model", ["t_SVGP", "t_SVGP_white"])
def test_steps_match_oracle_fp64(model, lik):
    X, Y, Z = _problem(lik)
    hip, ora = _pair(model, lik, Z, num_data=N)
    assert isinstance(hip.kernel, pkg().Product)
    for _ in range(5):
        hip.natgrad_step((X, Y), lr=0.8)
        ora.natgrad_step((X, Y), lr=0.8)
        _state_close(hip, ora)
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    assert abs(e_h - e_o) < 1e-9 * abs(e_o)
    assert abs(float(hip.prior_kl()) - ora.prior_kl()) < 1e-8 * abs(ora.prior_kl())
    Xs = X[:100] + 0.05
    mu_o, var_o = ora.predict_f(Xs)
    for fn in ["predict_f"] + (["new_predict_f"] if model == "t_SVGP" else []):
        mu_h, var_h = getattr(hip, fn)(Xs)
        assert relerr(mu_h.cpu().numpy(), mu_o) < 1e-8 and relerr(var_h.cpu().numpy(), var_o) < 1e-8
    if model == "t_SVGP":
        mu_h, var_h = hip.predict_f(Xs, full_output_cov=True)
        assert tuple(var_h.shape) == (100, 1, 1)
        assert relerr(var_h.cpu().numpy()[:, 0], var_o) < 1e-8
    ym_o, yv_o = ora.likelihood.predict_mean_and_var(mu_o, var_o)
    ym_h, yv_h = hip.predict_y(Xs)
    assert relerr(ym_h.cpu().numpy(), ym_o) < 1e-8 and relerr(yv_h.cpu().numpy(), yv_o) < 1e-8
    if model == "t_SVGP":  # (t_SVGP_white has no predict_log_density, as in the reference)
        ld_o = ora.likelihood.predict_log_density(mu_o, var_o, Y[:100])
        ld_h = hip.predict_log_density((Xs, Y[:100]))
        assert relerr(ld_h.cpu().numpy().reshape(-1), np.asarray(ld_o).reshape(-1)) < 1e-8


def test_minibatch_scaling_matches_oracle():
    """num_data = 3 N: the minibatch scale of the step and of the ELBO."""
    X, Y, Z = _problem("gaussian")
    hip, ora = _pair("t_SVGP", "gaussian", Z, num_data=3 * N)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
    _state_close(hip, ora)
    e_o = float(ora.elbo((X, Y)))
    assert abs(float(hip.elbo((X, Y))) - e_o) < 1e-9 * abs(e_o)


@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
@pytest.mark.parametrize("model", ["t_SVGP", "t_SVGP_white"])
def test_fp32_compute_against_fp64_oracle(model, lik):
    X, Y, Z = _problem(lik)
    hip, ora = _pair(model, lik, Z, num_data=N, compute_dtype=torch.float32)
    for _ in range(4):
        hip.natgrad_step((X, Y), lr=0.8)
        ora.natgrad_step((X, Y), lr=0.8)
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    assert abs(e_h - e_o) < 1e-4 * abs(e_o)
    mu_h, var_h = hip.predict_f(X[:100] + 0.05)
    mu_o, var_o = ora.predict_f(X[:100] + 0.05)
    np.testing.assert_allclose(mu_h.cpu().numpy(), mu_o, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(var_h.cpu().numpy(), var_o, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("model,n,m,graph", [("t_SVGP", 1000, 32, True), ("t_SVGP", 300, 24, False), ("t_SVGP_white", 300, 24, False)])
def test_a_component_parameter_assigned_between_steps_reaches_the_next_step(model, n, m, graph):
    """The carried-over K(X, Z), the route gate and the captured graph are keyed on EVERY component's parameters: after two steps
    (the second captured and replayed at N = 1000, M = 32) component 1's lengthscales are assigned, then component 0's variance;
    the same in place on the oracle; the state after each next step agrees at 1e-8."""
    X, Y, _ = synthetic(N=n, M=m, D=D, P=1, lik="gaussian", seed=3)
    Z = np.random.RandomState(5).randn(m, D) * 1.2
    kw = dict(use_graph=graph) if model == "t_SVGP" else {}
    hip, ora = _pair(model, "gaussian", Z, num_data=n, **kw)
    Xd, Yd = torch.as_tensor(X, device=DEV), torch.as_tensor(Y, device=DEV)  # the same buffers every step: what a graph is keyed on
    for _ in range(2):
        hip.natgrad_step((Xd, Yd), lr=0.6)
        ora.natgrad_step((X, Y), lr=0.6)
    _state_close(hip, ora)
    if graph:
        assert any(isinstance(v, dict) for v in hip._graphs.values()), "the second step was meant to be captured"
    hip.kernel.kernels[1].lengthscales.assign([1.7, 1.1])
    ora.kernel.kernels[1].lengthscales = [1.7, 1.1]
    for _ in range(2):
        hip.natgrad_step((Xd, Yd), lr=0.6)
        ora.natgrad_step((X, Y), lr=0.6)
        _state_close(hip, ora)
    hip.kernel.kernels[0].variance.assign(0.6)
    ora.kernel.kernels[0].variance = 0.6
    for _ in range(2):
        hip.natgrad_step((Xd, Yd), lr=0.6)
        ora.natgrad_step((X, Y), lr=0.6)
        _state_close(hip, ora)
    e_o = float(ora.elbo((X, Y)))
    assert abs(float(hip.elbo((Xd, Yd))) - e_o) < 1e-9 * abs(e_o)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("model", ["t_SVGP", "t_SVGP_white"])
def test_full_cov(model, dtype):
    X, Y, Z = _problem("bernoulli")
    hip, ora = _pair(model, "bernoulli", Z, num_data=N, compute_dtype=dtype)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.7)
        ora.natgrad_step((X, Y), lr=0.7)
    Xs = np.random.RandomState(9).randn(70, D)
    mean, cov = hip.predict_f(Xs, full_cov=True)
    mu, var = hip.predict_f(Xs)
    assert tuple(cov.shape) == (1, 70, 70)
    diag = cov[0].diagonal().cpu().numpy()
    mean_r, cov_r = fullcov_ref.predict_f_full_cov(ora, Xs)
    if dtype == torch.float64:
        assert relerr(diag, var.cpu().numpy()[:, 0]) < 1e-10
        assert relerr(cov.cpu().numpy(), cov_r) < 1e-8 and relerr(mean.cpu().numpy(), mean_r) < 1e-8
    else:
        np.testing.assert_allclose(diag, var.cpu().numpy()[:, 0], rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(cov.cpu().numpy(), cov_r, rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(mean.cpu().numpy(), mean_r, rtol=1e-3, atol=1e-4)
    eps = np.random.RandomState(2).randn(3, 70, 1)
    f = hip.predict_f_samples(Xs, 3, epsilon=eps)
    want = fullcov_ref.sample_mvn_full_cov(mean_r, cov_r, eps)
    if dtype == torch.float64:
        assert relerr(f.cpu().numpy(), want) < 1e-6  # (through a Cholesky factor of cov + 1e-6 I)
    else:
        np.testing.assert_allclose(f.cpu().numpy(), want, rtol=1e-2, atol=1e-2)


# ---------------------------------------------------------------------------------------------------------------------
# M-step gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
def test_elbo_gradients_match_oracle_finite_differences(lik):
    """Every entry: both components' variance and lengthscales (an isotropic one on one column, an ARD one on two), Z, and the
    likelihood variance."""
    n = 500
    X, Y, _ = synthetic(N=n, M=M, D=D, P=1, lik=lik, seed=7)
    Z = np.random.RandomState(41).randn(M, D) * 1.2
    noise = 0.2
    hip, ora = _pair("t_SVGP", lik, Z, num_data=n, noise=noise)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.7)
        ora.natgrad_step((X, Y), lr=0.7)
    state = (ora.lambda_1.copy(), ora.lambda_2_sqrt.copy())
    elbo, grads = hip.elbo_and_grads((X, Y))

    def f(spec=SPEC, Zv=Z, nv=noise):
        m = O.t_SVGP(R.build(spec), _lik(O, lik, nv), Zv, num_data=n, lambda_1=state[0], lambda_2_sqrt=state[1])
        return m.elbo((X, Y))

    assert abs(float(elbo) - f()) < 1e-9 * abs(f())
    names = sorted(k for k in grads if k.startswith("components."))
    assert names == sorted(f"components.{c}.{q}" for c in range(2) for q in ("variance", "lengthscales"))
    assert "variance" not in grads and "lengthscales" not in grads

    def with_entry(c, field, idx, value):
        spec = [list(s) for s in SPEC]
        if idx is None:
            spec[c][field] = value
        else:
            arr = np.array(spec[c][field], dtype=np.float64)
            arr[idx] = value
            spec[c][field] = arr
        return [tuple(s) for s in spec]

    def fd_spec(c, field, idx=None, h=1e-5):
        base = float(SPEC[c][field] if idx is None else SPEC[c][field][idx])
        step = h * max(1.0, abs(base))
        return (f(spec=with_entry(c, field, idx, base + step)) - f(spec=with_entry(c, field, idx, base - step))) / (2 * step)

    scale = max(abs(fd_spec(0, 1)), 1.0)
    for c in range(2):
        ref = fd_spec(c, 1)
        got = float(grads[f"components.{c}.variance"])
        print(f"components.{c}.variance: hip {got:.10e} fd {ref:.10e}")
        assert abs(got - ref) < 2e-6 * max(abs(ref), scale)
        g_ls = grads[f"components.{c}.lengthscales"].cpu().numpy()
        assert g_ls.shape == np.shape(SPEC[c][2])
        for idx in ([None] if g_ls.ndim == 0 else range(g_ls.shape[0])):
            ref = fd_spec(c, 2, idx)
            got = float(g_ls if idx is None else g_ls[idx])
            print(f"components.{c}.lengthscales[{idx}]: hip {got:.10e} fd {ref:.10e}")
            assert abs(got - ref) < 2e-6 * max(abs(ref), scale), (c, idx, got, ref)
    g_Z = grads["Z"].cpu().numpy()
    for (m_, d) in [(0, 0), (5, 1), (M - 1, 2), (11, 0)]:
        up, dn = Z.copy(), Z.copy()
        step = 1e-5 * max(1.0, abs(Z[m_, d]))
        up[m_, d] += step
        dn[m_, d] -= step
        ref = (f(Zv=up) - f(Zv=dn)) / (2 * step)
        assert abs(g_Z[m_, d] - ref) < 2e-6 * max(abs(ref), scale), (m_, d, g_Z[m_, d], ref)
    if lik == "gaussian":
        ref = (f(nv=noise + 1e-5) - f(nv=noise - 1e-5)) / 2e-5
        assert abs(float(grads["likelihood_variance"]) - ref) < 2e-6 * max(abs(ref), scale)
    else:
        assert "likelihood_variance" not in grads


def test_em_fit_does_not_lower_the_elbo():
    p = pkg()
    X, Y, Z = _problem("gaussian")
    hip = p.t_SVGP(R.build_pkg(p, SPEC), p.Gaussian(0.5), Z.copy(), num_data=N)
    logf, _ = p.training.em_fit(hip, (X, Y), iterations=3, n_e_steps=4, n_m_steps=5)
    print("ELBO per iteration:", logf)
    assert logf[1] >= logf[0] and logf[2] >= logf[1]
    assert hip.kernel.kernels[1].lengthscales.value[0].item() != 1.2 and hip.kernel.kernels[0].variance.item() != 1.3


def test_product_of_two_squared_exponentials_is_the_ard_squared_exponential():
    """SE(dims [0, 1]) * SE(dims [2]) against the ARD SquaredExponential of the product variance: the state after three steps
    within 1e-8."""
    p = pkg()
    X, Y, Z = _problem("gaussian")
    prod = p.SquaredExponential(1.3, [0.9, 1.2], active_dims=[0, 1]) * p.SquaredExponential(0.7, 1.5, active_dims=[2])
    ard = p.SquaredExponential(1.3 * 0.7, [0.9, 1.2, 1.5])
    a = p.t_SVGP(prod, p.Gaussian(0.2), Z.copy(), num_data=N)
    b = p.t_SVGP(ard, p.Gaussian(0.2), Z.copy(), num_data=N)
    for _ in range(3):
        a.natgrad_step((X, Y), lr=0.8)
        b.natgrad_step((X, Y), lr=0.8)
    assert relerr(a.lambda_1.numpy(), b.lambda_1.numpy()) < 1e-8
    assert relerr(_lambda_2(a), _lambda_2(b)) < 1e-8


def test_refusals_on_the_device():
    """What needs a kernel of its own for a product is refused by name, on a model that has taken steps."""
    p = pkg()
    X, Y, Z = _problem("gaussian")
    hip = p.t_SVGP(R.build_pkg(p, SPEC), p.Gaussian(0.2), Z.copy(), num_data=N)
    hip.natgrad_step((X, Y), lr=0.8)
    with pytest.raises(NotImplementedError, match="predict_f_vjp does not take a Product"):
        hip.predict_f_vjp(X[:5], np.ones((5, 1)))
    with pytest.raises(NotImplementedError, match="requires grad does not take a Product"):
        hip.predict_f(torch.tensor(X[:5], device=DEV, requires_grad=True))
    with pytest.raises(NotImplementedError, match="sample_functions does not take a Product"):
        hip.sample_functions(2)
    with pytest.raises(NotImplementedError, match="select_inducing_points does not take a Product"):
        p.select_inducing_points(X, hip.kernel, 4)
    with pytest.raises(NotImplementedError, match="t_SVGP_sites does not take a Product"):
        p.t_SVGP_sites((X, Y), hip.kernel, p.Gaussian(0.2), Z.copy())
    with pytest.raises(NotImplementedError, match="t_VGP does not take a Product"):
        p.t_VGP((X, Y), hip.kernel, p.Gaussian(0.2))
    with pytest.raises(NotImplementedError, match="SeparateIndependent does not take a Product"):
        p.SeparateIndependent([hip.kernel, p.SquaredExponential()])
    with pytest.raises(NotImplementedError, match="LinearCoregionalization does not take a Product"):
        p.LinearCoregionalization([hip.kernel], np.ones((2, 1)))
    rng = np.random.RandomState(0)
    X33, Z33 = rng.randn(40, 33), rng.randn(6, 33)
    wide = p.t_SVGP(p.SquaredExponential() * p.Matern32(), p.Gaussian(0.2), Z33)
    with pytest.raises(NotImplementedError, match="Product kernel takes at most 32"):
        wide.natgrad_step((X33, rng.randn(40, 1)), lr=0.5)
    X17, Z17 = rng.randn(40, 17), rng.randn(6, 17)
    mid = p.t_SVGP(p.SquaredExponential(lengthscales=4.0) * p.Matern32(lengthscales=4.0), p.Gaussian(0.2), Z17)
    Y17 = rng.randn(40, 1)
    mid.natgrad_step((X17, Y17), lr=0.5)
    with pytest.raises(NotImplementedError, match="Product kernel takes at most 16"):
        mid.elbo_and_grads((X17, Y17))
