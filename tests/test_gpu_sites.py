"""t_SVGP_sites (reference src/models/tsvgp_sites.py) on the GPU: the fused site-step kernel against NumPy, the model against
the NumPy restatement (tests/sites_ref.py), the reference's relational tests restated on the HIP model, the fixtures, sharding,
and one step at the headline size.  Tolerances as tests/test_gpu_model.py:
  fp64: max rel err <= 1e-8 on the sites and the predictive moments, |dELBO| / |ELBO| <= 1e-9
  fp32 (against the fp64 restatement): mean, var atol 1e-4 + rtol 1e-3, |dELBO| / |ELBO| <= 1e-4"""
import glob
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import tsvgp_oracle as O
from tests import sites_ref as R
from tests.helpers import free_port, pkg, relerr, synthetic

pytestmark = pytest.mark.gpu

SITES_FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sites", "*.npz")))


# ---------------------------------------------------------------------------------------------------------------------
# the map kernel
# ---------------------------------------------------------------------------------------------------------------------
def _np_step(lik, noise, mean, var, Y, l1, l2, lr):
    L = O.Gaussian(variance=noise) if lik == "gaussian" else O.Bernoulli()
    g0, g1 = L.variational_expectations_grads(mean, var, Y)
    ve = L.variational_expectations(mean, var, Y)
    n1, n2 = R.t_SVGP_sites.site_update(l1, l2, mean, g0, g1, lr)
    return n1, n2, ve


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
def test_site_step_kernel_against_numpy(lik, dtype):
    p = pkg()
    B = p._backend
    from importlib import import_module

    eng = import_module("t-svgp_amd.estep").EStepEngine(dtype)
    rng = np.random.RandomState(7)
    N, lr = 300, 0.6  # not a multiple of 128
    Np = B.round_up(N)
    mean = rng.randn(N, 1)
    var = rng.rand(N, 1) + 0.05
    Y = rng.randn(N, 1) if lik == "gaussian" else (rng.rand(N, 1) > 0.5).astype(np.float64)
    noise = 0.3
    l1 = rng.randn(N, 1)
    l2 = rng.rand(N, 1) * 2.0
    if lik == "gaussian":
        # a noise variance of 1e7 makes g1 = -5e-8; on rows 0..39 the value under the crop,
        # (1 - lr)(-lambda_2 / 2) + lr g1 = -0.2 lambda_2 - 3e-8, then lands on either side of -1e-8
        noise = 1e7
        l2[:40, 0] = np.linspace(-1.2e-7, -2e-8, 40)
        var[5, 0], var[17, 0] = 0.0, -0.5  # non-positive variances: counted
    to = lambda a: torch.as_tensor(a, dtype=dtype, device="cuda")
    sentinel = 7.0
    s1 = torch.full((Np, 1), sentinel, dtype=torch.float64, device="cuda")
    s2 = s1.clone()
    s1[:N], s2[:N] = torch.as_tensor(l1), torch.as_tensor(l2)
    c1 = torch.full((Np, 1), sentinel, dtype=torch.float32, device="cuda") if dtype == torch.float32 else None
    c2 = c1.clone() if c1 is not None else None
    m_d, v_d, y_d = to(mean), to(var), to(Y)
    ve_sum, nonpos = eng.diag_site_step(m_d, v_d, y_d, p.Gaussian(noise).lik_id if lik == "gaussian" else B.LIK_BERNOULLI,
                                        noise if lik == "gaussian" else 0.0, lr, s1, s2, c1, c2)
    # the NumPy reference on the moments the kernel saw (fp32 inputs rounded)
    mean_r, var_r, Y_r = (m_d.double().cpu().numpy(), v_d.double().cpu().numpy(), y_d.double().cpu().numpy())
    live = (var_r[:, 0] > 0) if lik == "bernoulli" else np.ones(N, bool)
    n1, n2, ve = _np_step(lik, noise, mean_r, np.where(var_r > 0, var_r, 1.0) if lik == "bernoulli" else var_r, Y_r, l1, l2, lr)
    g1 = s1.cpu().numpy()
    g2 = s2.cpu().numpy()
    tol = 1e-12 if (dtype == torch.float64 or lik == "gaussian") else 2e-5
    assert relerr(g1[:N][live], n1[live]) < tol
    assert relerr(g2[:N][live], n2[live]) < tol
    assert np.all(g1[N:] == sentinel) and np.all(g2[N:] == sentinel)  # padding rows are not touched
    assert np.all(g2[:N][live] >= 2e-8 * (1 - 1e-15))
    if lik == "gaussian":
        cropped = (1 - lr) * (-0.5 * l2[:40, 0]) + lr * (-0.5 / noise) > -1e-8
        assert cropped.any() and (~cropped).any()  # both sides of the crop
        assert np.all(g2[:40, 0][cropped] == 2e-8)
        np.testing.assert_allclose(g2[:40, 0][~cropped], n2[:40, 0][~cropped], rtol=1e-12)
        assert float(nonpos) == 2
        np.testing.assert_allclose(float(ve_sum), np.sum(ve), rtol=1e-12)
    else:
        assert float(nonpos) == 0
        np.testing.assert_allclose(float(ve_sum), np.sum(ve), rtol=1e-12 if dtype == torch.float64 else 1e-5)
    if c1 is not None:  # the fp32 copies of the new sites, padding untouched
        assert np.array_equal(c1[:N].cpu().numpy(), g1[:N].astype(np.float32))
        assert np.array_equal(c2[:N].cpu().numpy(), g2[:N].astype(np.float32))
        assert np.all(c1[N:].cpu().numpy() == sentinel) and np.all(c2[N:].cpu().numpy() == sentinel)


def test_site_step_kernel_without_variance():
    """var = NULL (Gaussian, skip_unused_variance): the same sites, NaN ve partials, non-finite means counted."""
    p = pkg()
    from importlib import import_module

    eng = import_module("t-svgp_amd.estep").EStepEngine(torch.float64)
    rng = np.random.RandomState(8)
    N = 200
    mean, Y, l1, l2 = rng.randn(N, 1), rng.randn(N, 1), rng.randn(N, 1), rng.rand(N, 1)
    mean[3, 0] = np.inf
    Np = 256
    s = [torch.zeros((Np, 1), dtype=torch.float64, device="cuda") for _ in range(4)]
    for t in s[:2]:
        t[:N] = torch.as_tensor(l1)
    for t in s[2:]:
        t[:N] = torch.as_tensor(l2)
    m_d, y_d = torch.as_tensor(mean, device="cuda"), torch.as_tensor(Y, device="cuda")
    v_d = torch.full((N, 1), 0.4, dtype=torch.float64, device="cuda")
    ve_a, np_a = eng.diag_site_step(m_d, v_d, y_d, 1, 0.2, 0.5, s[0], s[2])
    ve_b, np_b = eng.diag_site_step(m_d, None, y_d, 1, 0.2, 0.5, s[1], s[3])
    ok = np.isfinite(mean[:, 0])
    assert np.array_equal(s[0][:N].cpu().numpy()[ok], s[1][:N].cpu().numpy()[ok])
    assert np.array_equal(s[2].cpu().numpy(), s[3].cpu().numpy())
    assert np.isnan(float(ve_b)) and float(np_b) == 1 and float(np_a) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the model against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _pair(lik, N=700, M=24, D=4, seed=5, ls=1.0, **kw):
    p = pkg()
    X, Y, _ = synthetic(N=N, M=M, D=D, P=1, lik=lik, seed=seed)
    Z = np.random.RandomState(seed + 1).randn(M, D) * 1.2
    mk = lambda mod, cls, **k: cls((X, Y), mod.SquaredExponential(1.1, ls), mod.Gaussian(0.2) if lik == "gaussian" else mod.Bernoulli(),
                                   Z, **k)
    return X, Y, Z, mk(p, p.t_SVGP_sites, **kw), mk(O, R.t_SVGP_sites)


def _route(m):
    return "direct" if m._use_direct() and not m._two_product else ("two-product" if m._two_product else "whitened")


@pytest.mark.parametrize("projection,D,ls", [("auto", 4, 1.0), ("direct", 4, 1.0), ("whitened", 4, 1.0), ("auto", 3, 1.6)])
@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
def test_model_steps_match_restatement_fp64(lik, projection, D, ls):
    X, Y, Z, hip, ref = _pair(lik, D=D, ls=ls, projection=projection)
    if projection == "auto":
        assert _route(hip) == ("direct" if D == 4 else "whitened")  # both routes of "auto" are exercised
    e_o = ref.elbo()
    assert abs(float(hip.elbo()) - e_o) < 1e-9 * abs(e_o)
    for _ in range(6):
        hip.natgrad_step(lr=0.7)
        ref.natgrad_step(lr=0.7)
        assert relerr(hip.lambda_1.numpy(), ref.lambda_1) < 1e-8
        assert relerr(hip.lambda_2.numpy(), ref.lambda_2) < 1e-8
    e_o = ref.elbo()
    assert abs(float(hip.elbo()) - e_o) < 1e-9 * abs(e_o)
    assert abs(float(hip.prior_kl()) - ref.prior_kl()) < 1e-8 * abs(ref.prior_kl())
    Xn = X[:150] + 0.05
    mu_h, var_h = hip.predict_f(Xn)
    mu_o, var_o = ref.predict_f(Xn)
    assert relerr(mu_h.cpu().numpy(), mu_o) < 1e-8 and relerr(var_h.cpu().numpy(), var_o) < 1e-8
    m_h, cS_h = hip.get_mean_chol_cov_inducing_posterior()
    m_o, cS_o = ref.get_mean_chol_cov_inducing_posterior()
    assert relerr(m_h.cpu().numpy(), m_o) < 1e-8 and relerr(cS_h.cpu().numpy(), cS_o) < 1e-7
    ym, yv = hip.predict_y(Xn)
    ym_o, yv_o = ref.likelihood.predict_mean_and_var(mu_o, var_o)
    assert relerr(ym.cpu().numpy(), ym_o) < 1e-8 and relerr(yv.cpu().numpy(), yv_o) < 1e-8
    lp = hip.predict_log_density((Xn, Y[:150]))
    assert relerr(lp.cpu().numpy(), ref.likelihood.predict_log_density(mu_o, var_o, Y[:150])) < 1e-8


@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
def test_model_fp32_against_fp64_restatement(lik):
    X, Y, Z, hip, ref = _pair(lik, N=2000, compute_dtype=torch.float32)
    for _ in range(4):
        hip.natgrad_step(lr=0.8)
        ref.natgrad_step(lr=0.8)
    e_h, e_o = float(hip.elbo()), ref.elbo()
    assert abs(e_h - e_o) / abs(e_o) < 1e-4
    mu_h, var_h = hip.predict_f(X[:300])
    mu_o, var_o = ref.predict_f(X[:300])
    np.testing.assert_allclose(mu_h.cpu().numpy(), mu_o, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(var_h.cpu().numpy(), var_o, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("projection", ["auto", "whitened"])
def test_skip_unused_variance_gives_the_same_sites(projection):
    _, _, _, a, _ = _pair("gaussian", projection=projection)
    _, _, _, b, _ = _pair("gaussian", projection=projection, skip_unused_variance=True)
    for _ in range(5):
        a.natgrad_step(lr=0.7)
        b.natgrad_step(lr=0.7)
    assert relerr(b.lambda_1.numpy(), a.lambda_1.numpy()) < 1e-12
    assert relerr(b.lambda_2.numpy(), a.lambda_2.numpy()) < 1e-12
    assert abs(float(a.elbo()) - float(b.elbo())) < 1e-12 * abs(float(a.elbo()))


def test_assigned_sites_are_used():
    """A site assigned through the parameter reaches the projection (fp64 state and the fp32 weights)."""
    for dtype in (torch.float64, torch.float32):
        X, Y, Z, hip, ref = _pair("gaussian", compute_dtype=dtype)
        rng = np.random.RandomState(2)
        l1, l2 = rng.randn(*ref.lambda_1.shape), rng.rand(*ref.lambda_2.shape) + 0.1
        hip.lambda_1.assign(l1)
        hip.lambda_2.assign(l2)
        ref.lambda_1, ref.lambda_2 = l1, l2
        hip.natgrad_step(lr=0.5)
        ref.natgrad_step(lr=0.5)
        assert relerr(hip.lambda_1.numpy(), ref.lambda_1) < (1e-8 if dtype == torch.float64 else 1e-3)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own tests (reference tests/models/test_tsvgp_sites.py), restated on the HIP model
# ---------------------------------------------------------------------------------------------------------------------
def _ref_setup():
    rng = np.random.RandomState(123)
    func = lambda x: np.sin(x * 3 * 3.14) + 0.3 * np.cos(x * 9 * 3.14) + 0.5 * np.sin(x * 7 * 3.14)
    X = rng.rand(8, 1) * 2 - 1
    Y = func(X) + 0.2 * rng.randn(8, 1)
    return X, Y


@pytest.fixture(name="optim_setup")
def _optim_setup():
    p = pkg()
    X, Y = _ref_setup()
    m = p.t_SVGP_sites((X, Y), p.SquaredExponential(variance=2.25, lengthscales=2.0), p.Gaussian(variance=0.3), X.copy())
    for _ in range(10):
        m.natgrad_step(lr=0.9)
    return m, X, Y


def test_elbo_optimal(optim_setup):
    m, X, Y = optim_setup
    np.testing.assert_almost_equal(float(m.elbo()), O.gpr_log_marginal_likelihood(O.SquaredExponential(2.25, 2.0), X, Y, 0.3),
                                   decimal=4)


def test_unchanged_at_optimum(optim_setup):
    m, _, _ = optim_setup
    e0 = float(m.elbo())
    m.natgrad_step(lr=0.5)
    np.testing.assert_almost_equal(e0, float(m.elbo()), decimal=4)


def test_optimal_sites_closed_form(optim_setup):
    m, _, Y = optim_setup
    np.testing.assert_allclose(m.lambda_1.numpy(), Y / 0.3)
    np.testing.assert_allclose(m.lambda_2.numpy(), np.ones_like(Y) / 0.3)


@pytest.mark.parametrize("path", SITES_FIXTURES, ids=[os.path.basename(p)[:-4] for p in SITES_FIXTURES])
def test_golden_fixture(path):
    p = pkg()
    g = np.load(path)
    lik = p.Gaussian(float(g["noise"])) if "gaussian" in os.path.basename(path) else p.Bernoulli()
    m = p.t_SVGP_sites((g["X"], g["Y"]), p.SquaredExponential(float(g["variance"]), float(g["lengthscales"])), lik, g["Z"])
    for s in range(1, int(g["steps"].max()) + 1):
        m.natgrad_step(lr=float(g["lr"]))
        if s in g["steps"]:
            assert relerr(m.lambda_1.numpy(), g[f"lambda_1_{s}"]) < 1e-8
            assert relerr(m.lambda_2.numpy(), g[f"lambda_2_{s}"]) < 1e-8
            assert abs(float(m.elbo()) - float(g[f"elbo_{s}"])) < 1e-9 * abs(float(g[f"elbo_{s}"]))


def test_not_implemented_cases():
    p = pkg()
    X, Y, Z = synthetic(N=50, M=8, D=2, P=2, seed=0)
    with pytest.raises(NotImplementedError):
        p.t_SVGP_sites((X, Y), p.SquaredExponential(), p.Gaussian(0.1), Z, lambda_2=np.ones((50, 2)))
    with pytest.raises(NotImplementedError):
        p.t_SVGP_sites((X, Y[:, :1]), p.SquaredExponential(), p.HeteroskedasticTFPConditional(), Z)
    m = p.t_SVGP_sites((X, Y[:, :1]), p.SquaredExponential(), p.Gaussian(0.1), Z)
    with pytest.raises(NotImplementedError):
        m.elbo_and_grads()


# ---------------------------------------------------------------------------------------------------------------------
# sharding: rank-local sites, one all-reduce of the projection per step
# ---------------------------------------------------------------------------------------------------------------------
N_SHARD, STEPS_SHARD = 1001, 4


def _shard_problem(lik):
    X, Y, _ = synthetic(N=N_SHARD, M=20, D=4, P=1, lik=lik, seed=21)
    Z = np.random.RandomState(4).randn(20, 4)
    return X, Y, Z


def _worker(rank, world, port, out, backend, lik):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = pkg()
        if world == 1:
            p.distributed.FORCE_COLLECTIVES = True
        calls = []
        real = p.distributed.all_reduce_sum
        p.distributed.all_reduce_sum = lambda t: (calls.append(t.numel()), real(t))[1]
        X, Y, Z = _shard_problem(lik)
        Xs, Ys = p.distributed.shard_rows(X, Y)
        m = p.t_SVGP_sites((Xs, Ys), p.SquaredExponential(1.0, 1.0), p.Gaussian(0.2) if lik == "gaussian" else p.Bernoulli(), Z,
                           device="cuda:0")
        for _ in range(STEPS_SHARD):
            m.natgrad_step(lr=0.8)
        steps_calls = len(calls)
        e = float(m.elbo())
        np.savez(out % rank, l1=m.lambda_1.numpy(), l2=m.lambda_2.numpy(), elbo=e, calls=steps_calls)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,backend,lik", [(2, "gloo", "gaussian"), (2, "gloo", "bernoulli"), (1, "nccl", "gaussian")])
def test_sharded_sites_match_one_process(tmp_path, world, backend, lik):
    out = str(tmp_path / "r%d.npz")
    mp.spawn(_worker, args=(world, free_port(), out, backend, lik), nprocs=world, join=True)
    p = pkg()
    X, Y, Z = _shard_problem(lik)
    one = p.t_SVGP_sites((X, Y), p.SquaredExponential(1.0, 1.0), p.Gaussian(0.2) if lik == "gaussian" else p.Bernoulli(), Z)
    for _ in range(STEPS_SHARD):
        one.natgrad_step(lr=0.8)
    e1 = float(one.elbo())
    for r in range(world):
        got = np.load(out % r)
        lo, hi = p.distributed.shard_bounds(N_SHARD, world, r)
        assert got["l1"].shape[0] == hi - lo  # each rank holds its own rows' sites only
        assert relerr(got["l1"], one.lambda_1.numpy()[lo:hi]) < 1e-9
        assert relerr(got["l2"], one.lambda_2.numpy()[lo:hi]) < 1e-9
        assert abs(float(got["elbo"]) - e1) < 1e-10 * abs(e1)
        assert int(got["calls"]) == STEPS_SHARD  # one all-reduce per step


# ---------------------------------------------------------------------------------------------------------------------
# one step at the headline size
# ---------------------------------------------------------------------------------------------------------------------
def test_one_step_at_headline_size():
    """N = 1e6, M = 1024, D = 8, fp64: the projection against a chunked fp64 reference, and the new sites on 4096 sampled rows
    against the restatement's update driven by that projection."""
    p = pkg()
    N, M, D = 1_000_000, 1024, 8
    g = torch.Generator(device="cpu").manual_seed(0)
    X = torch.randn(N, D, generator=g, dtype=torch.float64)
    w = torch.randn(D, 1, generator=g, dtype=torch.float64)
    Y = torch.sin(X @ w) + 0.3 * torch.randn(N, 1, generator=g, dtype=torch.float64)
    Z = X[:M].clone()
    ls = 2.0
    m = p.t_SVGP_sites((X, Y), p.SquaredExponential(1.0, ls), p.Gaussian(0.1), Z.numpy())
    rng = np.random.RandomState(1)
    l1 = torch.as_tensor(rng.randn(N, 1) * 0.1)
    l2 = torch.as_tensor(rng.rand(N, 1) + 0.5)
    m.lambda_1.assign(l1)
    m.lambda_2.assign(l2)
    # the projection, on the GPU, against a chunked fp64 reference computed there with torch (k_n = K(Z, x_n))
    l, L, _ = m._project()
    Xd, Zd, l1d, l2d = X.cuda(), Z.cuda(), l1.cuda(), l2.cuda()
    acc2 = torch.zeros((M, M), dtype=torch.float64, device="cuda")
    acc1 = torch.zeros((M, 1), dtype=torch.float64, device="cuda")
    for s in range(0, N, 125_000):
        Xs, Zs = Xd[s:s + 125_000] / ls, Zd / ls
        d2 = (Xs * Xs).sum(1, keepdim=True) + (Zs * Zs).sum(1)[None] - 2.0 * Xs @ Zs.T
        K = torch.exp(-0.5 * d2.clamp_min(0.0))
        acc2 += K.T @ (l2d[s:s + 125_000] * K)
        acc1 += K.T @ l1d[s:s + 125_000]
    assert relerr(L[0].cpu().numpy(), acc2.cpu().numpy()) < 1e-11
    assert relerr(l.cpu().numpy(), acc1.cpu().numpy()) < 1e-11
    # the step, and the restatement's update on a sample of rows driven by the same projection
    rows = np.sort(rng.choice(N, 4096, replace=False))
    ref = R.t_SVGP_sites((X[rows].numpy(), Y[rows].numpy()), O.SquaredExponential(1.0, ls), O.Gaussian(0.1), Z.numpy(),
                         lambda_1=l1[rows].numpy(), lambda_2=l2[rows].numpy())
    # mean = k^T (K6 + L + 1e-9 I)^-1 l (what conditional() gives on posterior_from_dense_site_white's q(u)); the Gaussian
    # gradients do not read the variance
    Kzz = ref.kernel.K(Z.numpy()) + (1e-6 + 1e-9) * np.eye(M)
    mean = ref.kernel.K(X[rows].numpy(), Z.numpy()) @ np.linalg.solve(Kzz + L[0].cpu().numpy(), l.cpu().numpy())
    g0, g1 = ref.likelihood.variational_expectations_grads(mean, np.ones_like(mean), Y[rows].numpy())
    n1, n2 = R.t_SVGP_sites.site_update(ref.lambda_1, ref.lambda_2, mean, g0, g1, 0.5)
    m.natgrad_step(lr=0.5)
    assert relerr(m.lambda_1.numpy()[rows], n1) < 1e-8
    assert relerr(m.lambda_2.numpy()[rows], n2) < 1e-8
