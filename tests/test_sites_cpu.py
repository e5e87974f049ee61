"""CPU checks of t_SVGP_sites: the NumPy restatement (tests/sites_ref.py) against the reference's own relational tests
(reference tests/models/test_tsvgp_sites.py), the committed fixtures against the restatement, and the product's HOST logic --
projection, all-reduce, M x M operands, route checks, site state -- over a NumPy test double of the engine's new calls, with
gloo world sizes 2 and 3 on uneven shards against one process."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import tsvgp_oracle as O
from tests import sites_ref as R
from tests.cpu_engine import NumpyShardEngine
from tests.helpers import free_port, pkg, relerr, synthetic

LENGTH_SCALE, VARIANCE, NOISE_VARIANCE = 2.0, 2.25, 0.3
FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sites", "*.npz")))


def _ref_setup():
    """reference tests/models/test_tsvgp_sites.py:93-105 (RandomState(123), N = 8)."""
    rng = np.random.RandomState(123)
    func = lambda x: np.sin(x * 3 * 3.14) + 0.3 * np.cos(x * 9 * 3.14) + 0.5 * np.sin(x * 7 * 3.14)
    X = rng.rand(8, 1) * 2 - 1
    Y = func(X) + 0.2 * rng.randn(8, 1)
    return X, Y


@pytest.fixture(name="optim")
def _optim():
    X, Y = _ref_setup()
    kern = O.SquaredExponential(variance=VARIANCE, lengthscales=LENGTH_SCALE)
    m = R.t_SVGP_sites((X, Y), kern, O.Gaussian(variance=NOISE_VARIANCE), X.copy())
    for _ in range(10):
        m.natgrad_step(lr=0.9)
    return m, kern, X, Y


def test_restatement_elbo_optimal(optim):
    m, kern, X, Y = optim
    np.testing.assert_almost_equal(m.elbo(), O.gpr_log_marginal_likelihood(kern, X, Y, NOISE_VARIANCE), decimal=4)


def test_restatement_unchanged_at_optimum(optim):
    m, _, _, _ = optim
    e0 = m.elbo()
    m.natgrad_step(lr=0.5)
    np.testing.assert_almost_equal(e0, m.elbo(), decimal=4)


def test_restatement_optimal_sites_closed_form(optim):
    m, _, _, Y = optim
    np.testing.assert_allclose(m.lambda_1, Y / NOISE_VARIANCE)
    np.testing.assert_allclose(m.lambda_2, np.ones_like(Y) / NOISE_VARIANCE)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_fixtures_match_restatement(path):
    g = np.load(path)
    assert os.path.getsize(path) < 64 * 1024
    lik = O.Gaussian(float(g["noise"])) if "gaussian" in os.path.basename(path) else O.Bernoulli()
    m = R.t_SVGP_sites((g["X"], g["Y"]), O.SquaredExponential(float(g["variance"]), float(g["lengthscales"])), lik, g["Z"])
    for s in range(1, int(g["steps"].max()) + 1):
        m.natgrad_step(lr=float(g["lr"]))
        if s in g["steps"]:
            assert relerr(m.lambda_1, g[f"lambda_1_{s}"]) < 1e-12
            assert relerr(m.lambda_2, g[f"lambda_2_{s}"]) < 1e-12
            assert abs(m.elbo() - float(g[f"elbo_{s}"])) < 1e-12 * abs(float(g[f"elbo_{s}"]))


# ---------------------------------------------------------------------------------------------------------------------
# host logic over a NumPy test double of the new engine calls
# ---------------------------------------------------------------------------------------------------------------------
class SitesShardEngine(NumpyShardEngine):
    """``project_diag`` / ``diag_sites_moments`` / ``diag_site_step`` of EStepEngine in NumPy (fp64)."""

    def _k(self, kernel):
        return getattr(O, type(kernel).__name__)(variance=float(kernel.variance.value), lengthscales=kernel.lengthscales.numpy())

    def project_diag(self, X, Z, kernel, w1, w2):
        N = X.shape[0]
        K = self._k(kernel).K(X.cpu().numpy(), Z.cpu().numpy())
        acc2 = np.einsum("nm,no,n->mo", K, K, w2[:N, 0].cpu().numpy())[None]
        acc1 = (K.T @ w1[:N].cpu().numpy()).T
        return torch.as_tensor(acc2), torch.as_tensor(acc1), {}

    def diag_sites_moments(self, X, Z, kernel, ticket, *, whiten_T, moment_Tm, moment_mode, gamma, mean_only=False):
        st = self.run(X, None, Z, kernel, moment_Tm=moment_Tm, moment_mode=moment_mode, gamma=gamma, whiten_T=whiten_T,
                      want_moments=True, prefill=ticket)
        return st.mean, (None if mean_only else st.var)

    def diag_site_step(self, mean, var, Y, lik_id, lik_param, lr, l1, l2, l1c=None, l2c=None):
        N = mean.shape[0]
        lik = O.Gaussian(variance=lik_param) if lik_id == 1 else O.Bernoulli()
        mn = mean.numpy()
        vn = np.ones_like(mn) if var is None else var.numpy()
        g0, g1 = lik.variational_expectations_grads(mn, vn, Y.numpy())
        n1, n2 = R.t_SVGP_sites.site_update(l1[:N].numpy(), l2[:N].numpy(), mn, g0, g1, lr)
        l1[:N], l2[:N] = torch.as_tensor(n1), torch.as_tensor(n2)
        ve = float(np.sum(lik.variational_expectations(mn, vn, Y.numpy())))
        return torch.tensor(ve, dtype=torch.float64), torch.tensor(float(np.sum(~(vn > 0))), dtype=torch.float64)


N_HOST, STEPS_HOST = 47, 3


def _host_problem(lik):
    X, Y, _ = synthetic(N=N_HOST, M=9, D=3, P=1, lik=lik, seed=11)
    Z = np.random.RandomState(12).randn(9, 3)
    return X, Y, Z


def _host_model(X, Y, Z, lik, projection):
    p = pkg()
    m = p.t_SVGP_sites((X, Y), p.SquaredExponential(1.0, 1.3), p.Gaussian(0.2) if lik == "gaussian" else p.Bernoulli(), Z,
                       device="cpu", projection=projection)
    m._engine = SitesShardEngine()  # test double: the HIP engine cannot exist without a GPU
    return m


def _host_run(lik, projection, rows=None):
    X, Y, Z = _host_problem(lik)
    if rows is not None:
        X, Y = X[rows[0]:rows[1]], Y[rows[0]:rows[1]]
    m = _host_model(X, Y, Z, lik, projection)
    for _ in range(STEPS_HOST):
        m.natgrad_step(lr=0.8)
    return m


@pytest.mark.parametrize("projection", ["direct", "whitened"])
@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
def test_host_logic_matches_restatement(lik, projection):
    m = _host_run(lik, projection)
    X, Y, Z = _host_problem(lik)
    ref = R.t_SVGP_sites((X, Y), O.SquaredExponential(1.0, 1.3), O.Gaussian(0.2) if lik == "gaussian" else O.Bernoulli(), Z)
    for _ in range(STEPS_HOST):
        ref.natgrad_step(lr=0.8)
    assert relerr(m.lambda_1.numpy(), ref.lambda_1) < 1e-9
    assert relerr(m.lambda_2.numpy(), ref.lambda_2) < 1e-9
    assert abs(float(m.elbo()) - ref.elbo()) < 1e-9 * abs(ref.elbo())
    mu, var = m.predict_f(X[:5] + 0.1)
    mu_o, var_o = ref.predict_f(X[:5] + 0.1)
    assert relerr(mu.numpy(), mu_o) < 1e-8 and relerr(var.numpy(), var_o) < 1e-8


def test_state_and_api_on_host():
    p = pkg()
    X, Y, Z = _host_problem("gaussian")
    m = _host_model(X, Y, Z, "gaussian", "auto")
    assert m.num_data == N_HOST and m.whiten is False
    assert np.all(m.lambda_1.numpy() == 0) and np.all(m.lambda_2.numpy() == 1e-6)
    l1, l2 = m.sites.padded()
    assert l1.shape == (128, 1) and np.all(l2[N_HOST:].numpy() == 0)
    m.lambda_2.assign(np.full((N_HOST, 1), 0.5))  # an assigned parameter is re-bound to the padded state
    assert np.all(m.sites.padded()[1][:N_HOST].numpy() == 0.5)
    assert isinstance(m.sites, p.DiagSites)
    with pytest.raises(NotImplementedError):
        m.elbo_and_grads()
    with pytest.raises(NotImplementedError):
        p.t_SVGP_sites((X, Y), p.SquaredExponential(), p.HeteroskedasticTFPConditional(), Z, device="cpu")
    with pytest.raises(NotImplementedError):
        p.t_SVGP_sites((X, np.hstack([Y, Y])), p.SquaredExponential(), p.Gaussian(0.1), Z, device="cpu",
                       lambda_2=np.ones((N_HOST, 2)))
    with pytest.raises(ValueError):
        p.t_SVGP_sites((X, Y), p.SquaredExponential(), p.Gaussian(0.1), Z, device="cpu", projection="nope")


def _worker(rank, world, port, out, lik, projection):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = pkg()
        calls = []
        real = p.distributed.all_reduce_sum
        p.distributed.all_reduce_sum = lambda t: (calls.append(t.numel()), real(t))[1]
        m = _host_run(lik, projection, rows=p.distributed.shard_bounds(N_HOST, world, rank))
        n_calls = len(calls)
        e = float(m.elbo())
        np.savez(out % rank, l1=m.lambda_1.numpy(), l2=m.lambda_2.numpy(), elbo=e, calls=n_calls)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,lik,projection", [(2, "gaussian", "auto"), (3, "bernoulli", "whitened"), (3, "gaussian", "direct")])
def test_sharded_host_logic_gloo(tmp_path, world, lik, projection):
    """Each rank holds its own rows' sites; one all-reduce of the projection per step; the same sites and ELBO as one process."""
    out = str(tmp_path / "r%d.npz")
    mp.spawn(_worker, args=(world, free_port(), out, lik, projection), nprocs=world, join=True)
    one = _host_run(lik, projection)
    e1 = float(one.elbo())
    p = pkg()
    for r in range(world):
        got = np.load(out % r)
        lo, hi = p.distributed.shard_bounds(N_HOST, world, r)
        assert got["l1"].shape == (hi - lo, 1)
        assert relerr(got["l1"], one.lambda_1.numpy()[lo:hi]) < 1e-10
        assert relerr(got["l2"], one.lambda_2.numpy()[lo:hi]) < 1e-10
        assert abs(float(got["elbo"]) - e1) < 1e-10 * abs(e1)
        assert int(got["calls"]) == STEPS_HOST


def test_site_step_argument_validation_needs_no_gpu():
    """tsvgp_diag_site_step_* reject bad arguments before any launch (fake pointers are never dereferenced)."""
    B = pkg()._backend
    lib = B.lib()
    f64, f32 = lib.tsvgp_diag_site_step_f64, lib.tsvgp_diag_site_step_f32
    fake = 4096
    assert f64(None, None, None, B.LIK_GAUSSIAN, 0.1, 0.5, None, None, None, None, 10, 128, 1, None) == 1
    assert f64(fake, fake, fake, B.LIK_GAUSSIAN, 0.1, 0.5, fake, fake, fake, fake, 10, 100, 1, None) == 1  # Np % 128
    assert f64(fake, fake, fake, B.LIK_GAUSSIAN, 0.1, 0.5, fake, fake, fake, fake, 200, 128, 1, None) == 1  # Np < N
    assert f64(fake, fake, fake, B.LIK_GAUSSIAN, 0.0, 0.5, fake, fake, fake, fake, 10, 128, 1, None) == 1  # noise variance
    assert f64(fake, fake, fake, B.LIK_GAUSSIAN, 0.1, 1.5, fake, fake, fake, fake, 10, 128, 1, None) == 1  # lr
    for lik in (B.LIK_NONE, B.LIK_HETERO, B.LIK_GAUSSIAN | B.LIK_MEANONLY):
        assert f64(fake, fake, fake, lik, 0.1, 0.5, fake, fake, fake, fake, 10, 128, 1, None) == 1
    assert f64(fake, None, fake, B.LIK_BERNOULLI, 0.0, 0.5, fake, fake, fake, fake, 10, 128, 1, None) == 1  # var needed
    assert f32(fake, fake, fake, B.LIK_GAUSSIAN, 0.1, 0.5, fake, fake, None, None, fake, fake, 10, 128, 1, None) == 1  # fp32 copies
