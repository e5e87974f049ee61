"""CPU checks of the MultiClass likelihood with the RobustMax link: the restatement (tests/robustmax_ref.py) -- its closed-form
gradients against difference quotients of its own ``prob_is_largest`` value, the identities of the map, the two-class case against
a scalar quadrature, the clip path; the package's likelihood class against the restatement; constructor and model errors; the
C-ABI's argument validation; the host logic of t_SVGP with MultiClass over a NumPy engine double (tests/robustmax_engine.py)
against the oracle, its fixed point, and two gloo ranks against one.

Every tolerance of the restatement's own checks is computed in the test from the step size and printed (run with -s), as in
tests/test_scalar_lik_cpu.py."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import robustmax_ref as R
from tests.helpers import free_port, pkg, relerr
from tests.robustmax_engine import RobustMaxNumpyEngine
from tests.robustmax_problem import blobs, clip_rows, map_inputs, pair, problem

MultiClass = pkg().MultiClass  # the class under test: without it this file is not collected (nothing here passes on a tree that lacks it)

EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------------- the restatement
def _central(fun, x, h):
    """Central difference quotients of fun at x with steps h and h / 2 and the a-posteriori bound of the finer one: the scheme
    is O(h^2), so its truncation error at h / 2 is |D_h - D_{h/2}| / 3 to leading order (doubled here), and each quotient carries
    2 eps |fun| / step of rounding (tests/test_scalar_lik_cpu.py)."""
    d1 = (fun(x + h) - fun(x - h)) / (2.0 * h)
    d2 = (fun(x + 0.5 * h) - fun(x - 0.5 * h)) / h
    tol = 2.0 * np.abs(d1 - d2) / 3.0 + 8.0 * EPS * np.max(np.abs(fun(x))) / h + 1e-300
    return d2, tol


def _assert_within(name, got, ref, tol):
    err = np.abs(got - ref)
    worst = np.argmax(err / tol)
    print(f"{name}: max |diff| {err.max():.3e}, max tol {tol.max():.3e}, worst ratio {float((err / tol).flat[worst]):.3f}")
    assert np.all(err <= tol)


def _column(a, c, col):
    out = a.copy()
    out[:, c] = col
    return out


@pytest.mark.parametrize("C", [2, 3, 10, 32])
def test_gradients_match_difference_quotients_of_the_value(C):
    mu, var, y = map_inputs(300, C, seed=C)
    assert set(y[:, 0]) == set(range(C))
    lik = R.MultiClass(C)
    g0, g1 = lik.variational_expectations_grads(mu, var, y)
    # the value bends on the scale of the row's smallest standard deviation (0.01 at v = 1e-4): steps relative to it
    h = 1e-3 * np.sqrt(var.min(axis=1))
    for c in range(C):
        d0, t0 = _central(lambda col: lik.variational_expectations(_column(mu, c, col), var, y), mu[:, c], h)
        d1, t1 = _central(lambda col: lik.variational_expectations(mu, _column(var, c, col), y), var[:, c], 1e-4 * var[:, c])
        _assert_within(f"robustmax C={C} g0[:, {c}]", g0[:, c], d0, t0)
        _assert_within(f"robustmax C={C} g1[:, {c}]", g1[:, c], d1, t1)
    # the labelled latent's gain is the others' loss, node by node: 64 roundings of the largest entry bound the row sums
    tol = 64 * EPS * np.abs(g0).max() * C
    print(f"robustmax C={C}: max |sum_c g0| {np.abs(g0.sum(axis=1)).max():.2e}, tol {tol:.2e}")
    assert np.abs(g0.sum(axis=1)).max() <= tol
    # RobustMax is not log-concave: the crop of tsvgp.py:262-263 is active on many entries
    assert (g1 > 0).any() and (g1 > -1e-8).mean() > 0.3


def test_two_classes_match_the_scalar_quadrature():
    """C = 2: p is a one-dimensional quadrature of one jittered normal cdf; here in plain scalars."""
    mu, var, y = map_inputs(40, 2, seed=7)
    eps = 0.01
    lik = R.MultiClass(2, eps)
    x, w = np.polynomial.hermite.hermgauss(20)
    want = np.zeros(40)
    for n in range(40):
        k = int(y[n, 0])
        o = 1 - k
        p = 0.0
        for xi, wi in zip(x, w):
            d = (mu[n, k] + xi * math.sqrt(2.0 * var[n, k]) - mu[n, o]) / math.sqrt(var[n, o])
            p += wi / math.sqrt(math.pi) * (0.5 * (1.0 + math.erf(d / math.sqrt(2.0))) * (1.0 - 2e-4) + 1e-4)
        want[n] = p * math.log(1.0 - eps) + (1.0 - p) * math.log(eps)
    got = lik.variational_expectations(mu, var, y)
    tol = 64 * EPS * np.abs(want).max()
    print(f"robustmax C=2 ve: max |diff| {np.abs(got - want).max():.2e}, tol {tol:.2e}")
    assert np.abs(got - want).max() <= tol


def test_log_prob_at_a_clear_argmax():
    lik = R.MultiClass(4, 0.03)
    F = np.array([[3.0, 0.0, -1.0, 0.5], [0.0, 0.1, 5.0, 0.2], [1.0, 2.0, 0.0, -4.0]])
    y = np.array([[0.0], [1.0], [1.0]])
    want = np.array([math.log(0.97), math.log(0.01), math.log(0.97)])
    np.testing.assert_allclose(lik.log_prob(F, y), want, rtol=1e-15)
    got = MultiClass(4, epsilon=0.03).log_prob(torch.as_tensor(F), torch.as_tensor(y))
    assert got.shape == (3,) and got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-15)


def test_clip_path_has_zero_derivative_and_finite_values():
    mu, var, y = clip_rows()
    lik = R.MultiClass(3)
    g0, g1 = lik.variational_expectations_grads(mu, var, y)
    ve = lik.variational_expectations(mu, var, y)
    assert np.isfinite(g0).all() and np.isfinite(g1).all() and np.isfinite(ve).all()
    assert g1[0, 0] == 0.0 and g1[1, 1] == 0.0 and (g1[0, 1:] != 0.0).all() and g1[1, 0] != 0.0 and g1[1, 2] != 0.0
    # the value does not move with a clipped variance, and moves with the others
    for n, c in ((0, 0), (1, 1)):
        up = var.copy()
        up[n, c] = 3e-12
        assert lik.variational_expectations(mu, up, y)[n] == ve[n]
    h = 1e-4
    for c in range(3):  # the means and the unclipped variances of both rows still differentiate as usual
        d0, t0 = _central(lambda col: lik.variational_expectations(_column(mu, c, col), var, y), mu[:, c], h)
        _assert_within(f"clip rows g0[:, {c}]", g0[:, c], d0, t0)
    d1, t1 = _central(lambda col: lik.variational_expectations(mu, _column(var, 2, col), y), var[:, 2], h * var[:, 2])
    _assert_within("clip rows g1[:, 2]", g1[:, 2], d1, t1)


# ------------------------------------------------------------------------------------------------------- the class
@pytest.mark.parametrize("C", [2, 5, 32])
def test_package_helpers_match_restatement(C):
    p = pkg()
    mu, var, y = map_inputs(60, C, seed=4)
    lik, ref = p.MultiClass(C, epsilon=0.02), R.MultiClass(C, 0.02)
    assert lik.latent_dim == lik.num_classes == C and lik.num_gauss_hermite_points == 20 and lik.epsilon == 0.02
    assert lik.lik_id == p._backend.LIK_MULTICLASS == 7 and lik.lik_id in p._backend.COUPLED_LIKS and lik.lik_id in p._backend.MAPPED_LIKS
    assert lik.lik_param is lik and lik.graph_key() == (C, 0.02)
    assert not hasattr(lik, "draw") and not hasattr(lik, "advance") and not hasattr(lik, "rng_state")
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    ps, pv = lik.predict_mean_and_var(t(mu), t(var))
    ps_r, pv_r = ref.predict_mean_and_var(mu, var)
    assert ps.shape == (60, C) and pv.shape == (60, C)
    np.testing.assert_allclose(ps.numpy(), ps_r, rtol=1e-12)
    np.testing.assert_allclose(pv.numpy(), pv_r, rtol=1e-12)
    lpd = lik.predict_log_density(t(mu), t(var), t(y))
    assert lpd.shape == (60,)
    np.testing.assert_allclose(lpd.numpy(), ref.predict_log_density(mu, var, y), rtol=1e-12)
    F = mu + 0.0
    np.testing.assert_array_equal(lik.log_prob(t(F), t(y)).numpy(), ref.log_prob(F, y))
    # chunked over rows: a tiny chunk gives the same values
    small = p.MultiClass(C, epsilon=0.02)
    small._CHUNK = 7 * 20 * C * C
    np.testing.assert_array_equal(small.predict_mean_and_var(t(mu), t(var))[0].numpy(), ps.numpy())
    with pytest.raises(TypeError):
        lik.predict_mean_and_var(t(mu), t(var), epsilon=None)  # no draws argument


def test_constructor_errors_and_the_link_holder():
    p = pkg()
    for bad in (1, 33, 2.5, 0):
        with pytest.raises(ValueError):
            p.MultiClass(bad)
        with pytest.raises(ValueError):
            p.RobustMax(bad)
    for eps in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            p.MultiClass(3, epsilon=eps)
        with pytest.raises(ValueError):
            p.RobustMax(3, eps)
    for link in (torch.softmax, "robustmax", object()):
        with pytest.raises(NotImplementedError):
            p.MultiClass(3, invlink=link)
    with pytest.raises(ValueError):
        p.MultiClass(3, invlink=p.RobustMax(4))
    link = p.RobustMax(3, 0.05)
    lik = p.MultiClass(3, invlink=link)
    assert lik.invlink is link and lik.epsilon == 0.05 and lik.graph_key() == (3, 0.05)
    assert p.MultiClass(3).epsilon == 1e-3 and p.MultiClass(3).invlink.epsilon == 1e-3
    assert "MultiClass" in p.__all__ and "RobustMax" in p.__all__
    lik = p.MultiClass(3)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    with pytest.raises(ValueError, match="MultiClass"):
        lik.predict_mean_and_var(t(np.zeros((4, 2))), t(np.ones((4, 2))))
    with pytest.raises(ValueError, match="MultiClass"):
        lik.predict_log_density(t(np.zeros((4, 3))), t(np.ones((4, 3))), t(np.zeros(4)))


def test_model_errors_on_every_model_class():
    p = pkg()
    X, Y, Z = problem(N=10, M=6)
    lik = p.MultiClass(3)
    for P in (1, 2, 4):
        with pytest.raises(ValueError, match=r"MultiClass likelihood needs num_latent_gps = 3 \(its latent_dim\)"):
            p.t_SVGP(p.Matern52(), lik, Z, num_latent_gps=P)
    with pytest.raises(ValueError):
        p.t_SVGP(p.SeparateIndependent([p.SquaredExponential(), p.SquaredExponential()]), lik,
                 p.SharedIndependentInducingVariables(Z), num_latent_gps=2)
    m = p.t_SVGP(p.Matern52(), lik, Z, num_latent_gps=3)
    for Yb in (np.zeros((10, 3)), np.zeros(10), np.zeros((9, 1))):
        for call in (m.natgrad_step, m.elbo, m.elbo_and_grads, m.moments_and_gradients, m.predict_log_density):
            with pytest.raises(ValueError, match="MultiClass"):
                call((X, Yb))
    with pytest.raises(NotImplementedError, match="MultiClass"):
        p.t_SVGP_white(p.Matern52(), lik, Z, num_latent_gps=1)
    with pytest.raises(NotImplementedError):
        p.t_SVGP_white(p.Matern52(), lik, Z, num_latent_gps=3)
    with pytest.raises(NotImplementedError, match="MultiClass"):
        p.t_SVGP_sites((X, Y), p.Matern52(), lik, Z, num_latent_gps=1)
    with pytest.raises(NotImplementedError):
        p.t_SVGP_sites((X, Y), p.Matern52(), lik, Z, num_latent_gps=3)
    with pytest.raises(ValueError, match="MultiClass"):
        p.t_VGP((X, Y), p.Matern52(), lik)
    # the engine's own check names the likelihood too
    Yt = torch.zeros(10, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match="the MultiClass likelihood needs 3 latent GPs"):
        p.estep.EStepEngine._check_y(Yt, 10, 2, p._backend.LIK_MULTICLASS, lik)
    with pytest.raises(ValueError, match="the MultiClass likelihood needs 3 latent GPs"):
        p.estep.EStepEngine._check_y(torch.zeros(10, 3, dtype=torch.float64), 10, 3, p._backend.LIK_MULTICLASS | p._backend.LIK_NOCROP, lik)
    p.estep.EStepEngine._check_y(Yt, 10, 3, p._backend.LIK_MULTICLASS, lik)


# ------------------------------------------------------------------------------------------------------- the C-ABI
def test_map_argument_validation_needs_no_gpu():
    B = pkg()._backend
    lib = B.lib()
    f = 4096  # never dereferenced: every call below is rejected before a launch
    for fn in (lib.tsvgp_lik_map_robustmax_f64, lib.tsvgp_lik_map_robustmax_f32):
        call = lambda flags=B.LIK_MULTICLASS, C=3, eps=1e-3, ptrs=(f,) * 3, outs=(f,) * 4, N=10, Np=128: fn(
            *ptrs, flags, C, eps, *outs, N, Np, None)
        for C in (1, 0, -3, 33):
            assert call(C=C) == 1
        for eps in (0.0, 1.0, -1e-3, 2.0, float("nan"), float("inf")):
            assert call(eps=eps) == 1
        for i in range(3):
            assert call(ptrs=tuple(None if j == i else f for j in range(3))) == 1
        for i in range(4):
            assert call(outs=tuple(None if j == i else f for j in range(4))) == 1
        for flags in (B.LIK_NONE, B.LIK_GAUSSIAN, B.LIK_BERNOULLI, B.LIK_HETERO, B.LIK_SOFTMAX, B.LIK_STUDENT_T, B.LIK_POISSON, 8,
                      B.LIK_MULTICLASS | B.LIK_MEANONLY, B.LIK_MULTICLASS | B.LIK_NOCROP | B.LIK_MEANONLY, B.LIK_MULTICLASS | 0x400):
            assert call(flags=flags) == 1
        assert call(Np=100) == 1 and call(N=200) == 1 and call(N=0) == 1 and call(N=-5) == 1 and call(Np=0) == 1
    # the other maps and the moments kernels reject the selector, and the ABI number did not move
    s7 = B.LIK_MULTICLASS
    for sfx in ("f64", "f32"):
        g = lambda name: getattr(lib, f"{name}_{sfx}")
        assert g("tsvgp_lik_map")(f, f, f, s7, 0.0, f, f, f, f, 10, 128, 3, None) == 1
        assert g("tsvgp_lik_map_hetero")(f, f, f, s7, f, f, f, f, 10, 128, None) == 1
        assert g("tsvgp_lik_map_scalar")(f, f, f, 1, s7, 1.0, 3.0, f, f, 1, f, None, f, 10, 128, None) == 1
        assert g("tsvgp_lik_map_softmax")(f, f, f, s7, 3, 10, f, 0, None, f, f, f, f, 10, 128, None) == 1
        assert g("tsvgp_moments")(f, f, f, f, 1.0, s7, 0.0, f, f, f, f, f, f, 10, 128, 128, 3, 1, None) == 1
        assert g("tsvgp_moments_batched")(f, 0, f, f, f, f, s7, 0.0, f, f, f, f, f, f, 10, 128, 128, 3, 1, None) == 1
    assert lib.tsvgp_abi_version() == B.ABI_VERSION == 5


# ------------------------------------------------------------------------------------------------------- host logic
def _cpu_pair(Z, C, kind, **kw):
    hip, ora = pair(Z, C, kind, device="cpu", **kw)
    hip._engine = RobustMaxNumpyEngine()  # test double: the HIP engine cannot exist without a GPU
    return hip, ora


@pytest.mark.parametrize("kind", ["shared", "separate"])
def test_host_logic_matches_oracle(kind):
    X, Y, Z = problem(N=200, M=8)
    hip, ora = _cpu_pair(Z, 3, kind, num_data=len(X))
    for _ in range(5):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < 1e-8 and relerr(hip.lambda_2.numpy(), ora.lambda_2) < 1e-8
    e_h, e_o = float(hip.elbo((X, Y))), ora.elbo((X, Y))
    assert abs(e_h - e_o) < 1e-9 * abs(e_o)
    assert float(hip.elbo((X, Y))) == e_h  # deterministic: nothing is drawn, nothing advances


def test_natgrad_step_at_the_optimum_leaves_the_elbo_unchanged():
    """The reference's own pin (its tests/models/test_tsvgp_sites.py::test_tsvgp_unchanged_at_optimum: one more step at the fixed
    point of the E-step, to ``decimal=4``), which the Monte Carlo likelihood cannot state.  The pin needs an optimum to stand at,
    and the steps at lr = 0.8 have to reach it: RobustMax is not log-concave, most g1 sit on the crop of tsvgp.py:262-263, and on
    data with label noise (tests/softmax_problem.py) the REFERENCE'S iteration -- the oracle alone, driven by the restatement --
    settles into a two-cycle at lr = 0.8 (ELBO -257.96 / -252.18, step after step) instead of a point.  On the three overlapping
    clusters below it contracts (the ELBO's change per step falls below 1e-5 after 128 steps and keeps falling), so 140 steps
    stand within 1e-5 of the fixed point, a tenth of what ``decimal=4`` (1.5e-4) asks for."""
    X, Y, Z = blobs()
    hip, _ = _cpu_pair(Z, 3, "shared", num_data=len(X))
    for _ in range(140):
        hip.natgrad_step((X, Y), lr=0.8)
    before = float(hip.elbo((X, Y)))
    hip.natgrad_step((X, Y), lr=0.8)
    after = float(hip.elbo((X, Y)))
    print(f"robustmax fixed point: elbo {before:.8f} -> {after:.8f}")
    np.testing.assert_almost_equal(after, before, decimal=4)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = pkg()
        X, Y, Z = problem(N=401)  # uneven shards
        hip, _ = _cpu_pair(Z, 3, "shared", num_data=401)
        Xs, Ys = p.distributed.shard_rows(X, Y)
        assert hip._reduce() and len(Xs) in (200, 201)
        for _ in range(3):
            hip.natgrad_step((Xs, Ys), lr=0.5)
        elbo = float(hip.elbo((Xs, Ys)))
        if rank == 0:
            np.savez(out, l1=hip.lambda_1.numpy(), L2=hip.lambda_2.numpy(), elbo=elbo)
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_match_one():
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "r0.npz")
        mp.spawn(_worker, args=(2, free_port(), out), nprocs=2, join=True)
        got = dict(np.load(out))
    X, Y, Z = problem(N=401)
    one, _ = _cpu_pair(Z, 3, "shared", num_data=401)
    for _ in range(3):
        one.natgrad_step((X, Y), lr=0.5)
    assert relerr(got["l1"], one.lambda_1.numpy()) < 1e-10 and relerr(got["L2"], one.lambda_2.numpy()) < 1e-10
    e = float(one.elbo((X, Y)))
    assert abs(float(got["elbo"]) - e) < 1e-10 * abs(e)
