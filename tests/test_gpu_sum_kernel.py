"""``Sum`` kernels and ``active_dims`` on the models, on the GPU: t_SVGP and t_SVGP_white with SE + Matern32(active_dims=[2])
against the CPU oracle on the duck-typed NumPy ``Sum`` of tests/sum_kernel_ref.py.  N = 300, M = 24, D = 3 unless said.

Tolerances (tests/test_gpu_model.py): fp64 relerr < 1e-8 on lambda_1, Lambda_2 and the predictions,
|dELBO| < 1e-9 |ELBO|; fp32 compute: mean, var atol 1e-4 + rtol 1e-3, ELBO 1e-4 relative.  Gradients: central differences of the
oracle's ELBO / predict_f at 2e-6 max(|ref|, scale) (tests/test_gpu_mstep.py, tests/test_gpu_predict_grad.py)."""
import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests import fullcov_ref
from tests import sum_kernel_ref as R
from tests.helpers import pkg, relerr, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, M, D = 300, 24, 3
LS = [0.9, 1.2, 1.5]
SPEC = [("SquaredExponential", 1.3, LS, None), ("Matern32", 0.7, 0.8, [2])]


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
    for _ in range(5):
        hip.natgrad_step((X, Y), lr=0.8)
        ora.natgrad_step((X, Y), lr=0.8)
        _state_close(hip, ora)
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    assert abs(e_h - e_o) < 1e-9 * abs(e_o)
    assert abs(float(hip.prior_kl()) - ora.prior_kl()) < 1e-8 * abs(ora.prior_kl())
    m_h, cS_h = hip.get_mean_chol_cov_inducing_posterior()
    m_o, cS_o = ora.get_mean_chol_cov_inducing_posterior()
    assert relerr(m_h.cpu().numpy(), m_o) < 1e-8 and relerr(cS_h.cpu().numpy(), cS_o) < 1e-7  # (1e-7: tests/test_gpu_white.py)
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
    (the second captured and replayed at N = 1000, M = 32) component 1's lengthscale is assigned, then component 0's variance; the
    same in place on the oracle; the state after each next step agrees at 1e-8."""
    p = pkg()
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
    hip.kernel.kernels[1].lengthscales.assign(1.7)
    ora.kernel.kernels[1].lengthscales = 1.7
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


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own pin (tests/models/test_tsvgp.py:91-120): with Z = X the fixed point of the Gaussian model is the exact GP
# ---------------------------------------------------------------------------------------------------------------------
FIX_SPEC = [("SquaredExponential", 2.25, 2.0, None), ("Matern32", 0.5, 0.7, None)]


def _fixed_point_problem():
    rng = np.random.RandomState(123)
    func = lambda x: np.sin(x * 3 * 3.14) + 0.3 * np.cos(x * 9 * 3.14) + 0.5 * np.sin(x * 7 * 3.14)
    X = rng.rand(50, 1) * 2 - 1
    Y = func(X) + 0.2 * rng.randn(50, 1)
    return X, Y


def test_gaussian_fixed_point_is_the_exact_gp_of_the_sum_kernel():
    p = pkg()
    X, Y = _fixed_point_problem()
    hip = p.t_SVGP(R.build_pkg(p, FIX_SPEC), p.Gaussian(0.3), X.copy())
    for _ in range(10):
        hip.natgrad_step((X, Y), lr=0.9)
    kern = R.build(FIX_SPEC)
    lml = O.gpr_log_marginal_likelihood(kern, X, Y, 0.3)
    elbo = float(hip.elbo((X, Y)))
    print(f"ELBO {elbo:.8f}, exact log marginal likelihood {lml:.8f}")
    assert abs(elbo - lml) <= 1.5e-4
    mu, var = hip.predict_f(X + 1.0)
    mu_gpr, var_gpr = O.gpr_predict_f(kern, X, Y, 0.3, X + 1.0)
    np.testing.assert_array_almost_equal(mu.cpu().numpy(), mu_gpr, decimal=4)
    np.testing.assert_array_almost_equal(var.cpu().numpy(), var_gpr, decimal=4)


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
GRAD_SPEC = [("SquaredExponential", 1.3, 1.1, None), ("Matern52", 0.7, [0.8, 1.4], [2, 0]), ("Matern32", 0.4, [1.0, 1.3, 0.9], None)]


@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
def test_elbo_gradients_match_oracle_finite_differences(lik):
    """Every entry: component variances, component lengthscales (isotropic, an ARD component with active_dims in another order
    than the columns', a full ARD one), Z, and the likelihood variance."""
    p = pkg()
    n = 500
    X, Y, _ = synthetic(N=n, M=M, D=D, P=1, lik=lik, seed=7)
    Z = np.random.RandomState(41).randn(M, D) * 1.2
    noise = 0.2
    hip, ora = _pair("t_SVGP", lik, Z, spec=GRAD_SPEC, num_data=n, noise=noise)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.7)
        ora.natgrad_step((X, Y), lr=0.7)
    state = (ora.lambda_1.copy(), ora.lambda_2_sqrt.copy())
    elbo, grads = hip.elbo_and_grads((X, Y))

    def f(spec=GRAD_SPEC, Zv=Z, nv=noise):
        m = O.t_SVGP(R.build(spec), _lik(O, lik, nv), Zv, num_data=n, lambda_1=state[0], lambda_2_sqrt=state[1])
        return m.elbo((X, Y))

    assert abs(float(elbo) - f()) < 1e-9 * abs(f())
    names = sorted(k for k in grads if k.startswith("components."))
    assert names == sorted(f"components.{c}.{q}" for c in range(3) for q in ("variance", "lengthscales"))
    assert "variance" not in grads and "lengthscales" not in grads

    def with_entry(c, field, idx, value):
        spec = [list(s) for s in GRAD_SPEC]
        if idx is None:
            spec[c][field] = value
        else:
            arr = np.array(spec[c][field], dtype=np.float64)
            arr[idx] = value
            spec[c][field] = arr
        return [tuple(s) for s in spec]

    def fd_spec(c, field, idx=None, h=1e-5):
        base = float(GRAD_SPEC[c][field] if idx is None else GRAD_SPEC[c][field][idx])
        step = h * max(1.0, abs(base))
        return (f(spec=with_entry(c, field, idx, base + step)) - f(spec=with_entry(c, field, idx, base - step))) / (2 * step)

    scale = max(abs(fd_spec(0, 1)), 1.0)
    for c in range(3):
        ref = fd_spec(c, 1)
        got = float(grads[f"components.{c}.variance"])
        print(f"components.{c}.variance: hip {got:.10e} fd {ref:.10e}")
        assert abs(got - ref) < 2e-6 * max(abs(ref), scale)
        g_ls = grads[f"components.{c}.lengthscales"].cpu().numpy()
        assert g_ls.shape == np.shape(GRAD_SPEC[c][2])
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


def test_em_fit_raises_the_elbo():
    p = pkg()
    X, Y, Z = _problem("gaussian")
    hip = p.t_SVGP(R.build_pkg(p, SPEC), p.Gaussian(0.5), Z.copy(), num_data=N)
    logf, _ = p.training.em_fit(hip, (X, Y), iterations=2, n_e_steps=4, n_m_steps=5)
    print("ELBO per iteration:", logf)
    assert logf[1] > logf[0]
    assert hip.kernel.kernels[1].lengthscales.item() != 0.8 and hip.kernel.kernels[0].variance.item() != 1.3


# ---------------------------------------------------------------------------------------------------------------------
# input gradients of predict_f
# ---------------------------------------------------------------------------------------------------------------------
def _quotient(predict, Xn, combine):
    out = np.empty_like(Xn)
    for d in range(Xn.shape[1]):
        h = 1e-5 * np.maximum(1.0, np.abs(Xn[:, d]))
        up, dn = Xn.copy(), Xn.copy()
        up[:, d] += h
        dn[:, d] -= h
        out[:, d] = (combine(*predict(up)) - combine(*predict(dn))) / (up[:, d] - dn[:, d])
    return out


@pytest.mark.parametrize("model", ["t_SVGP", "t_SVGP_white"])
def test_predict_f_vjp(model):
    """Bit for bit what autograd through ``predict_f`` returns, and the oracle's difference quotient at the tolerance of
    tests/test_gpu_predict_grad.py (2e-6 max(|ref|, mean |ref|); cond(K_uu + 1e-6 I) <= 1e4 asserted as there)."""
    X, Y, Z = _problem("bernoulli")
    hip, ora = _pair(model, "bernoulli", Z, num_data=N)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.7)
        ora.natgrad_step((X, Y), lr=0.7)
    assert np.linalg.cond(ora.kernel.K(Z) + 1e-6 * np.eye(M)) <= 1e4
    rng = np.random.RandomState(3)
    Xn, cm, cv = rng.randn(40, D) * 1.1, rng.randn(40, 1), rng.randn(40, 1)
    got = hip.predict_f_vjp(Xn, cm, cv)
    leaf = torch.tensor(Xn, dtype=torch.float64, device=DEV, requires_grad=True)
    mean, var = hip.predict_f(leaf)
    (g,) = torch.autograd.grad((torch.as_tensor(cm, device=DEV) * mean + torch.as_tensor(cv, device=DEV) * var).sum(), leaf)
    assert torch.equal(g, got)
    ref = _quotient(ora.predict_f, Xn, lambda mean, var: np.sum(cm * mean + cv * var, axis=1))
    scale = float(np.mean(np.abs(ref)))
    err = np.abs(got.cpu().numpy() - ref)
    print(f"{model} predict_f_vjp: worst |got - ref| / max(|ref|, scale) = {float(np.max(err / np.maximum(np.abs(ref), scale))):.2e}")
    assert np.all(err <= 2e-6 * np.maximum(np.abs(ref), scale))


# ---------------------------------------------------------------------------------------------------------------------
# a base kernel with active_dims alone: the oracle kernel on the sliced columns
# ---------------------------------------------------------------------------------------------------------------------
def test_base_kernel_with_active_dims():
    X, Y, Z = _problem("gaussian")
    spec = [("Matern52", 1.1, [0.9, 1.4], [2, 0])]
    hip, ora = _pair("t_SVGP", "gaussian", Z, spec=spec, num_data=N)
    assert not isinstance(hip.kernel, pkg().Sum)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.8)
        ora.natgrad_step((X, Y), lr=0.8)
        _state_close(hip, ora)
    mu_h, var_h = hip.predict_f(X[:100] + 0.05)
    mu_o, var_o = ora.predict_f(X[:100] + 0.05)
    assert relerr(mu_h.cpu().numpy(), mu_o) < 1e-8 and relerr(var_h.cpu().numpy(), var_o) < 1e-8
