"""Input gradients of the marginal prediction on the models: ``predict_f_vjp`` and ``predict_f`` under torch autograd on t_SVGP,
t_SVGP_white and t_SVGP_sites, against CENTRAL DIFFERENCES OF THE ORACLE'S ``predict_f`` in Xnew (an independent derivation: the
oracle has no gradient code; tests/sites_ref.py for the sites model).

Setup as tests/test_gpu_mstep.py: N = 300 training rows, M = 24, D = 3, three natural-gradient steps on the HIP model and the oracle
side by side, 40 random Xnew rows that are not inducing points.  Step h = 1e-5 max(1, |x|); the quotient is good to ~1e-7
relative, asserted entry by entry at 2e-6 max(|ref|, scale), scale = the mean |ref| of the case.  The quotient is only trustworthy on a well-conditioned
K_uu: every case asserts cond(K_uu + 1e-6 I) <= 1e4 for its lengthscales.  fp32 compute dtype: 1e-4 + 1e-3 max|ref|."""
import functools

import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests import sites_ref
from tests.helpers import pkg, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, M, D, NEW = 300, 24, 3, 40
LS = np.array([0.9, 1.2, 1.5])
CASES = ["tsvgp-gauss-p1", "tsvgp-bern-p2", "tsvgp-separate-p2", "white-direct", "white-whitened", "white-two-product", "sites"]


def _kern(mod, name, var=1.3, ls=LS):
    return getattr(mod, name)(var, ls)


def _lik(mod, lik):
    return mod.Gaussian(0.2) if lik == "gaussian" else mod.Bernoulli()


def _build(case, compute_dtype=torch.float64):
    """(HIP model, oracle model, P, the oracle's kernels) after three natural-gradient steps on both."""
    p = pkg()
    rng = np.random.RandomState(41)
    Z = rng.randn(M, D) * 1.2
    kw = dict(compute_dtype=compute_dtype)
    if case.startswith("tsvgp"):
        P = 1 if case.endswith("p1") else 2
        lik = "bernoulli" if "bern" in case else "gaussian"
        X, Y, _ = synthetic(N=N, M=M, D=D, P=P, lik=lik, seed=7)

        def mk(mod, **k):
            if "separate" in case:
                kern = mod.SeparateIndependent([_kern(mod, "SquaredExponential"), _kern(mod, "Matern32", 0.8, LS + 0.1)])
                return mod.t_SVGP(kern, _lik(mod, lik), mod.SharedIndependentInducingVariables(Z), num_latent_gps=P, num_data=N, **k)
            return mod.t_SVGP(_kern(mod, "Matern52" if "bern" in case else "SquaredExponential"), _lik(mod, lik), Z, num_latent_gps=P,
                              num_data=N, **k)

        hip, ora = mk(p, **kw), mk(O)
        step = lambda m: m.natgrad_step((X, Y), lr=0.7)
    elif case.startswith("white"):
        P = 1
        lik = "bernoulli" if case == "white-direct" else "gaussian"
        X, Y, _ = synthetic(N=N, M=M, D=D, P=1, lik=lik, seed=7)
        mk = lambda mod, **k: mod.t_SVGP_white(_kern(mod, "SquaredExponential"), _lik(mod, lik), Z, num_data=N, **k)
        hip, ora = mk(p, projection="direct" if case == "white-direct" else "whitened", **kw), mk(O)
        step = lambda m: m.natgrad_step((X, Y), lr=0.7)
    else:
        P = 1
        X, Y, _ = synthetic(N=N, M=M, D=D, P=1, lik="bernoulli", seed=7)
        mk = lambda cls, mod, **k: cls((X, Y), _kern(mod, "Matern52"), _lik(mod, "bernoulli"), Z, **k)
        hip, ora = mk(p.t_SVGP_sites, p, **kw), mk(sites_ref.t_SVGP_sites, O)
        step = lambda m: m.natgrad_step(lr=0.7)
    for _ in range(3):
        step(hip)
        step(ora)
    if case == "white-two-product":
        hip._two_product = True  # the reference's own two-product variance: the route an indefinite Lambda_2 sends the model to
    kernels = list(ora.kernel.kernels) if hasattr(ora.kernel, "kernels") else [ora.kernel]
    for k in kernels:  # the condition under which the oracle's difference quotient is trustworthy
        assert np.linalg.cond(k.K(Z) + 1e-6 * np.eye(M)) <= 1e4
    return hip, ora, P


@functools.lru_cache(maxsize=None)
def _fp64(case):
    return _build(case)


def _new_rows(P, seed=3):
    rng = np.random.RandomState(seed)
    return rng.randn(NEW, D) * 1.1, rng.randn(NEW, P), rng.randn(NEW, P)


def _quotient(predict, Xn, combine):
    """Central differences of combine(*predict(X)) [NEW] in every coordinate: a row's prediction depends on that row alone, so one
    pair of evaluations moves dimension d of all rows.  h = 1e-5 max(1, |x|)."""
    out = np.empty_like(Xn)
    for d in range(Xn.shape[1]):
        h = 1e-5 * np.maximum(1.0, np.abs(Xn[:, d]))
        up, dn = Xn.copy(), Xn.copy()
        up[:, d] += h
        dn[:, d] -= h
        out[:, d] = (combine(*predict(up)) - combine(*predict(dn))) / (up[:, d] - dn[:, d])
    return out


def _assert_close(got, ref, what, rel=2e-6):
    """|got - ref| <= rel max(|ref|, scale) entry by entry, scale = the mean |ref| of the case (the typical size of a gradient
    entry, from the reference alone): an entry above it is held relatively, a small one to 2e-6 of the typical entry."""
    scale = float(np.mean(np.abs(ref)))
    assert scale > 0
    tol = rel * np.maximum(np.abs(ref), scale)
    err = np.abs(got - ref)
    print(f"{what}: worst |got - ref| / max(|ref|, scale) = {float(np.max(err / np.maximum(np.abs(ref), scale))):.2e} (scale {scale:.3f})")
    assert np.all(err <= tol), f"{what}: {float(np.max(err / tol)):.2f} of the tolerance at {np.unravel_index(np.argmax(err / tol), err.shape)}"


def _t(a):
    return torch.tensor(a, dtype=torch.float64, device=DEV)


@pytest.mark.parametrize("case", CASES)
def test_predict_f_vjp_against_oracle_difference_quotients(case):
    hip, ora, P = _fp64(case)
    Xn, cm, cv = _new_rows(P)
    ref = _quotient(ora.predict_f, Xn, lambda mean, var: np.sum(cm * mean + cv * var, axis=1))
    got = hip.predict_f_vjp(Xn, cm, cv)
    assert got.dtype == torch.float64 and tuple(got.shape) == (NEW, D) and got.device.type == "cuda"
    _assert_close(got.cpu().numpy(), ref, f"{case} predict_f_vjp")
    # the mean alone (cot_var = None) is the same call with zeros
    ref_m = _quotient(ora.predict_f, Xn, lambda mean, var: np.sum(cm * mean, axis=1))
    _assert_close(hip.predict_f_vjp(Xn, cm).cpu().numpy(), ref_m, f"{case} predict_f_vjp, mean alone")


@pytest.mark.parametrize("case", CASES)
def test_autograd_is_predict_f_vjp_and_the_forward_is_untouched(case):
    hip, _, P = _fp64(case)
    Xn, cm, cv = _new_rows(P, seed=4)
    plain_mean, plain_var = hip.predict_f(_t(Xn))
    assert plain_mean.grad_fn is None and plain_var.grad_fn is None
    X = _t(Xn).requires_grad_(True)
    mean, var = hip.predict_f(X)
    assert mean.grad_fn is not None and var.grad_fn is not None
    assert torch.equal(mean, plain_mean) and torch.equal(var, plain_var)  # bit for bit the values of a call without grad
    (g,) = torch.autograd.grad((mean * _t(cm) + var * _t(cv)).sum(), X)
    assert torch.equal(g, hip.predict_f_vjp(Xn, cm, cv))
    with torch.no_grad():  # grad mode off: no graph, whatever the input says
        m2, v2 = hip.predict_f(X)
    assert m2.grad_fn is None and torch.equal(m2, plain_mean) and torch.equal(v2, plain_var)
    # a CPU fp32 leaf gets its gradient through torch's own conversion
    leaf = torch.tensor(Xn, dtype=torch.float32, requires_grad=True)
    mean32, var32 = hip.predict_f(leaf)
    (mean32 * _t(cm) + var32 * _t(cv)).sum().backward()
    assert leaf.grad.dtype == torch.float32 and leaf.grad.device.type == "cpu"
    want = hip.predict_f_vjp(leaf.detach(), cm, cv).to(torch.float32).cpu()
    assert torch.equal(leaf.grad, want)


@pytest.mark.parametrize("case", ["tsvgp-gauss-p1", "tsvgp-bern-p2", "tsvgp-separate-p2", "white-whitened"])
def test_plain_sums_backpropagate_without_a_dense_cotangent(case):
    """``mean.sum()``, ``var.sum()`` and ``(mean + var).sum()`` backpropagated directly: autograd then hands the backward expanded
    (stride 0) gradients, and a materialised zero for the output that was not used, in layouts that differ between the two.  Each
    equals ``predict_f_vjp`` with ones / zeros bit for bit, and so does a caller's own expanded cotangent."""
    hip, _, P = _fp64(case)
    Xn, _, _ = _new_rows(P, seed=9)
    ones, zeros = np.ones((NEW, P)), np.zeros((NEW, P))
    for name, loss, cm, cv in (("mean", lambda m, v: m.sum(), ones, zeros), ("var", lambda m, v: v.sum(), zeros, ones),
                               ("mean + var", lambda m, v: (m + v).sum(), ones, ones),
                               ("ucb", lambda m, v: (m + 2.0 * v.sqrt()).sum(), None, None)):
        X = _t(Xn).requires_grad_(True)
        mean, var = hip.predict_f(X)
        (g,) = torch.autograd.grad(loss(mean, var), X)
        assert tuple(g.shape) == (NEW, D) and bool(torch.isfinite(g).all()), name
        if cm is None:  # d/d var of 2 sqrt(var), in the operations of torch's own backward of sqrt
            cm, cv = ones, 2.0 / (2.0 * var.detach().sqrt())
        assert torch.equal(g, hip.predict_f_vjp(Xn, cm, cv)), f"{case}: {name}.sum().backward() is not predict_f_vjp"
    X = _t(Xn).requires_grad_(True)
    hip.predict_y(X)[0].sum().backward()
    assert bool(torch.isfinite(X.grad).all())
    expanded = torch.ones((1, 1), dtype=torch.float64, device=DEV).expand(NEW, P)
    assert expanded.stride(0) == 0
    assert torch.equal(hip.predict_f_vjp(Xn, expanded), hip.predict_f_vjp(Xn, ones))
    assert torch.equal(hip.predict_f_vjp(Xn, expanded, expanded.t().contiguous().t()), hip.predict_f_vjp(Xn, ones, ones))


def test_a_parameter_assigned_between_forward_and_backward_does_not_reach_the_gradient():
    hip, _, P = _build("tsvgp-gauss-p1")
    Xn, cm, cv = _new_rows(P, seed=5)
    want = hip.predict_f_vjp(Xn, cm, cv)
    X = _t(Xn).requires_grad_(True)
    mean, var = hip.predict_f(X)
    old = hip.kernel.lengthscales.value.clone()
    hip.kernel.lengthscales.assign(old * 1.7)
    hip.kernel.variance.assign(0.4)
    (g,) = torch.autograd.grad((mean * _t(cm) + var * _t(cv)).sum(), X)
    assert torch.equal(g, want)
    assert not torch.equal(hip.predict_f_vjp(Xn, cm, cv), want)  # (the model itself did change)


def test_flags_and_errors():
    hip, _, P = _fp64("tsvgp-gauss-p1")
    Xn, cm, cv = _new_rows(P, seed=6)
    X = _t(Xn).requires_grad_(True)
    mean, var = hip.predict_f(X)
    w = _t(cm).requires_grad_(True)  # a cotangent that is itself differentiable: the second derivative is then asked for in earnest
    (g,) = torch.autograd.grad((mean * w + var * _t(cv)).sum(), X, create_graph=True, retain_graph=True)
    assert torch.equal(g.detach(), hip.predict_f_vjp(Xn, cm, cv))
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    # full_cov / full_output_cov with an input that requires grad: what they return today, no graph
    m_plain, c_plain = hip.predict_f(_t(Xn), full_cov=True)
    m_cov, c_cov = hip.predict_f(X, full_cov=True)
    assert not m_cov.requires_grad and not c_cov.requires_grad and torch.equal(m_cov, m_plain) and torch.equal(c_cov, c_plain)
    m_out, c_out = hip.predict_f(X, full_output_cov=True)
    assert not m_out.requires_grad and not c_out.requires_grad and tuple(c_out.shape) == (NEW, P, P)
    p = pkg()
    wide = p.t_SVGP(p.SquaredExponential(1.0, 6.0), p.Gaussian(0.1), np.random.RandomState(0).randn(5, 33))
    with pytest.raises(ValueError, match="32"):
        wide.predict_f_vjp(np.zeros((4, 33)), np.ones((4, 1)))
    with pytest.raises(ValueError):
        hip.predict_f_vjp(Xn, cm[:, :0])


def test_fp32_compute_dtype_against_the_fp64_quotient():
    hip, ora, P = _build("tsvgp-gauss-p1", torch.float32)
    Xn, cm, cv = _new_rows(P)
    ref = _quotient(ora.predict_f, Xn, lambda mean, var: np.sum(cm * mean + cv * var, axis=1))
    got = hip.predict_f_vjp(Xn, cm, cv)
    assert got.dtype == torch.float64
    err, bound = float(np.max(np.abs(got.cpu().numpy() - ref))), 1e-4 + 1e-3 * float(np.max(np.abs(ref)))
    print(f"fp32 predict_f_vjp: max abs err {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_gradient_through_predict_y_of_a_bernoulli_model():
    """``predict_y`` inherits differentiability through the likelihood's torch code: against the same quotient of the oracle's
    moments pushed through that code."""
    hip, ora, P = _fp64("tsvgp-bern-p2")
    Xn, c1, c2 = _new_rows(P, seed=8)
    lik = hip.likelihood

    def pushed(mean, var):
        ym, yv = lik.predict_mean_and_var(torch.as_tensor(mean), torch.as_tensor(var))
        return np.sum(c1 * ym.numpy() + c2 * yv.numpy(), axis=1)

    ref = _quotient(ora.predict_f, Xn, pushed)
    X = _t(Xn).requires_grad_(True)
    ym, yv = hip.predict_y(X)
    (g,) = torch.autograd.grad((ym * _t(c1) + yv * _t(c2)).sum(), X)
    _assert_close(g.cpu().numpy(), ref, "predict_y (Bernoulli) under autograd")
    # and predict_log_density
    Y = (np.random.RandomState(2).rand(NEW, P) > 0.5).astype(np.float64)
    dens = lambda mean, var: lik.predict_log_density(torch.as_tensor(mean), torch.as_tensor(var), torch.as_tensor(Y)).numpy()
    ref_d = _quotient(ora.predict_f, Xn, dens)
    X2 = _t(Xn).requires_grad_(True)
    (g2,) = torch.autograd.grad(hip.predict_log_density((X2, _t(Y))).sum(), X2)
    _assert_close(g2.cpu().numpy(), ref_d, "predict_log_density (Bernoulli) under autograd")
