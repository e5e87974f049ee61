"""CPU checks of the Softmax likelihood: the generator's restatement (tests/softmax_ref.py) against the Philox4x32-10 known-answer
vectors and its own row splits; the restated estimator against finite differences at a fixed epsilon and, at C = 2, against an
independent Gauss-Hermite value; the package's likelihood class against the restatement; the host logic of t_SVGP with Softmax
over a NumPy engine double (tests/softmax_engine.py) against the oracle, over two gloo ranks, and its errors; one golden fixture."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import tsvgp_oracle as O
from tests import softmax_ref as R
from tests.helpers import free_port, pkg, relerr
from tests.softmax_engine import CoupledNumpyEngine
from tests.softmax_problem import pair, problem

Softmax = pkg().Softmax  # the class under test: without it this file is not collected (nothing here passes on a tree that lacks it)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "softmax", "c3_steps.npz")


# ------------------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, out):
    assert " ".join("%08x" % int(x) for x in R.philox4x32_10(ctr, key)) == out


def test_normals_are_a_function_of_the_global_row():
    full = R.normals(11, 4, np.arange(200), 7, 10)
    assert full.shape == (7, 200, 10)
    for lo, hi in ((0, 1), (0, 77), (77, 200), (128, 129), (199, 200)):
        np.testing.assert_array_equal(R.normals(11, 4, lo + np.arange(hi - lo), 7, 10), full[:, lo:hi])
    # fewer samples / classes are prefixes (the counter holds s and c >> 2, not S or C); another draw or seed is another stream
    np.testing.assert_array_equal(R.normals(11, 4, np.arange(200), 3, 6), full[:3, :, :6])
    assert not np.array_equal(R.normals(11, 5, np.arange(200), 7, 10), full)
    assert not np.array_equal(R.normals(12, 4, np.arange(200), 7, 10), full)
    big = R.normals(-1, 2 ** 32 + 4, [2 ** 33 + 5], 2, 3)  # 64-bit rows and seeds; draw modulo 2^32
    np.testing.assert_array_equal(big, R.normals(-1, 4, [2 ** 33 + 5], 2, 3))
    assert np.isfinite(big).all()


def _moments(n, C, seed=0):
    rng = np.random.RandomState(seed)
    return rng.randn(n, C), rng.uniform(0.05, 2.0, (n, C)), rng.randint(0, C, (n, 1)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ the estimator
@pytest.mark.parametrize("C", [2, 3, 10])
def test_gradients_are_the_derivative_of_the_estimator_at_fixed_epsilon(C):
    """Step sizes and bounds of the matching check in tests/test_hetero_cpu.py."""
    mu, var, y = _moments(12, C, seed=1)
    lik = R.Softmax(C)
    eps = np.random.RandomState(2).randn(30, 12, C)
    g0, g1 = lik.variational_expectations_grads(mu, var, y, epsilon=eps)
    ve = lambda m, v: lik.variational_expectations(m, v, y, epsilon=eps)
    for p in range(C):
        h = 1e-6
        up, dn = mu.copy(), mu.copy()
        up[:, p] += h
        dn[:, p] -= h
        np.testing.assert_allclose(g0[:, p], (ve(up, var) - ve(dn, var)) / (2 * h), rtol=1e-6, atol=1e-8)
        hv = 1e-7
        up, dn = var.copy(), var.copy()
        up[:, p] += hv
        dn[:, p] -= hv
        np.testing.assert_allclose(g1[:, p], (ve(mu, up) - ve(mu, dn)) / (2 * hv), rtol=1e-5, atol=1e-7)
    assert lik.draw == 0  # an explicit epsilon consumes no draw


def test_g0_sums_to_zero_and_predicted_means_to_one():
    mu, var, y = _moments(50, 10, seed=3)
    lik = R.Softmax(10, seed=5)
    g0, _ = lik.variational_expectations_grads(mu, var, y)
    assert np.abs(g0.sum(axis=1)).max() < 1e-14
    ey, vy = lik.predict_mean_and_var(mu, var)
    np.testing.assert_allclose(ey.sum(axis=1), 1.0, rtol=1e-14)
    assert (vy > 0).all() and lik.draw == 2


def test_two_class_value_matches_gauss_hermite_within_five_standard_errors():
    """C = 2: log softmax(f)_y = log sigmoid(+-(f1 - f0)), and f1 - f0 ~ N(m1 - m0, v0 + v1): a one-dimensional integral, here by
    100-point Gauss-Hermite, against the restated estimator fed by the restated generator at S = 2e5.  The standard error comes
    from the per-sample values of the same run; 5 sigma over these 6 cases is a false-alarm rate below 1e-5 (fixed seeds).  This
    pins the generator's normality (mean, variance and tails as log sigmoid weighs them) too."""
    mu = np.array([[0.3, -0.2], [-1.0, 0.4], [0.0, 0.0], [2.0, -1.5], [0.5, 0.5], [-0.3, 1.1]])
    var = np.array([[0.4, 0.05], [0.2, 1.0], [1.0, 2.0], [0.5, 0.5], [3.0, 0.1], [0.01, 0.02]])
    y = np.array([[0.0], [1.0], [1.0], [1.0], [0.0], [0.0]])
    z, w = O.gh_points_and_weights(100)
    lik = R.Softmax(2, seed=17)
    lik.num_monte_carlo_points = 200000
    lp = lik.log_prob_samples(mu, var, y)  # [S, 6]
    est, se = lp.mean(axis=0), lp.std(axis=0, ddof=1) / np.sqrt(lp.shape[0])
    for n in range(6):
        d = (mu[n, 1] - mu[n, 0]) + np.sqrt(var[n, 0] + var[n, 1]) * z
        d = d if y[n, 0] == 1.0 else -d
        gh = np.sum(w * -np.logaddexp(0.0, -d))
        assert abs(est[n] - gh) < 5 * se[n], (n, est[n], gh, se[n])


# ------------------------------------------------------------------------------------------------------------ the class
def test_likelihood_class_matches_the_restatement_with_a_shared_epsilon():
    p = pkg()
    mu, var, y = _moments(40, 5, seed=4)
    lik = p.Softmax(5, seed=9)
    assert lik.latent_dim == lik.num_classes == 5 and lik.num_monte_carlo_points == 100 and lik.lik_id == p._backend.LIK_SOFTMAX == 4
    assert lik.seed == 9 and lik.draw == 0 and lik.row_offset == 0
    eps = np.random.RandomState(5).randn(100, 40, 5)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    ref = R.Softmax(5)
    ey, vy = lik.predict_mean_and_var(t(mu), t(var), epsilon=t(eps))
    ey_r, vy_r = ref.predict_mean_and_var(mu, var, epsilon=eps)
    np.testing.assert_allclose(ey.numpy(), ey_r, rtol=1e-13)
    np.testing.assert_allclose(vy.numpy(), vy_r, rtol=1e-12, atol=1e-15)
    lpd = lik.predict_log_density(t(mu), t(var), t(y), epsilon=t(eps))
    assert lpd.shape == (40,)
    np.testing.assert_allclose(lpd.numpy(), ref.predict_log_density(mu, var, y, epsilon=eps), rtol=1e-13)
    assert lik.draw == 0
    lik.draw = 12
    assert lik.draw == 12
    lik.seed = 4
    assert lik.seed == 4 and lik.draw == 12
    with pytest.raises(p.HipExtensionError):  # the default draws are made by a HIP kernel: no CPU generator behind the class
        lik.predict_mean_and_var(t(mu), t(var))
    for bad in (1, 33, 2.5):
        with pytest.raises(ValueError):
            p.Softmax(bad)


def test_map_argument_validation_needs_no_gpu():
    B = pkg()._backend
    lib = B.lib()
    f = 4096  # never dereferenced: every call below is rejected before a launch
    for fn in (lib.tsvgp_lik_map_softmax_f64, lib.tsvgp_lik_map_softmax_f32):
        call = lambda flags=B.LIK_SOFTMAX, C=3, S=10, rng=f, off=0, eps=None, ptrs=(f,) * 3, outs=(f,) * 4, N=10, Np=128: fn(
            *ptrs, flags, C, S, rng, off, eps, *outs, N, Np, None)
        assert call(C=1) == 1 and call(C=33) == 1 and call(S=0) == 1 and call(off=-1) == 1
        assert call(rng=None) == 1  # no generator state and no epsilon
        for i in range(3):
            assert call(ptrs=tuple(None if j == i else f for j in range(3))) == 1
        for i in range(4):
            assert call(outs=tuple(None if j == i else f for j in range(4))) == 1
        for flags in (B.LIK_HETERO, B.LIK_GAUSSIAN, B.LIK_NONE, B.LIK_SOFTMAX | B.LIK_MEANONLY):
            assert call(flags=flags) == 1
        assert call(Np=100) == 1 and call(N=200) == 1 and call(N=0) == 1
    for fn in (lib.tsvgp_mc_normals_f64, lib.tsvgp_mc_normals_f32):
        assert fn(None, 0, 0, 0, 10, 10, 3, None) == 1
        assert fn(f, 0, 0, 0, 0, 10, 3, None) == 1 and fn(f, 0, 0, 0, 10, 0, 3, None) == 1
        assert fn(f, 0, 0, 0, 10, 10, 0, None) == 1 and fn(f, 0, 0, 0, 10, 10, 33, None) == 1 and fn(f, 0, 0, -1, 10, 10, 3, None) == 1
        # S * N * ceil(C / 4) beyond the grid (and, further out, beyond int64) is refused, not wrapped
        assert fn(f, 0, 0, 0, 2 ** 28, 2 ** 40, 32, None) == 1 and fn(f, 0, 0, 0, 2 ** 28, 2 ** 33, 32, None) == 1
        assert fn(f, 0, 0, 0, 100, 2 ** 62, 10, None) == 1
    # the other maps reject the selector, and the ABI number did not move
    assert lib.tsvgp_lik_map_f64(f, f, f, B.LIK_SOFTMAX, 0.0, f, f, f, f, 10, 128, 2, None) == 1
    assert lib.tsvgp_lik_map_hetero_f64(f, f, f, B.LIK_SOFTMAX, f, f, f, f, 10, 128, None) == 1
    assert lib.tsvgp_moments_f64(f, f, f, f, 1.0, B.LIK_SOFTMAX, 0.0, f, f, f, f, f, f, 10, 128, 128, 2, 1, None) == 1
    assert lib.tsvgp_abi_version() == B.ABI_VERSION == 5


# ------------------------------------------------------------------------------------------------------------ host logic
def _cpu_pair(Z, C, kind, **kw):
    hip, ora = pair(Z, C, kind, device="cpu", **kw)
    hip._engine = CoupledNumpyEngine()  # test double: the HIP engine cannot exist without a GPU
    return hip, ora


@pytest.mark.parametrize("kind", ["shared", "separate"])
def test_host_logic_matches_oracle(kind):
    X, Y, Z = problem()
    hip, ora = _cpu_pair(Z, 3, kind, num_data=len(X))
    for step in range(5):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < 1e-8 and relerr(hip.lambda_2.numpy(), ora.lambda_2) < 1e-8
        assert hip.likelihood.draw == ora.likelihood.draw == step + 1  # one draw per evaluation
    e_h, e_o = float(hip.elbo((X, Y))), ora.elbo((X, Y))
    assert abs(e_h - e_o) < 1e-9 * abs(e_o) and hip.likelihood.draw == ora.likelihood.draw == 6
    hip.likelihood.draw = ora.likelihood.draw = 2  # a set draw is the one the next evaluation takes
    assert abs(float(hip.elbo((X, Y))) - ora.elbo((X, Y))) < 1e-9 * abs(e_o)
    assert abs(float(hip.elbo((X, Y))) - e_o) > 1e-6 * abs(e_o)  # (another draw is another estimate)


def test_golden_steps():
    g = np.load(GOLDEN)
    np.testing.assert_array_equal(R.normals(3, 2, np.arange(5, 9), 4, 3), g["normals"])
    hip, _ = _cpu_pair(g["Z"], 3, "shared", num_data=len(g["X"]))
    for step in range(4):
        hip.natgrad_step((g["X"], g["Y"]), lr=0.5)
        assert relerr(hip.lambda_1.numpy(), g["lambda_1"][step]) < 1e-8
        assert relerr(hip.lambda_2.numpy(), g["lambda_2"][step]) < 1e-8
    assert abs(float(hip.elbo((g["X"], g["Y"]))) - float(g["elbo"])) < 1e-9 * abs(float(g["elbo"]))


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = pkg()
        X, Y, Z = problem(N=401)  # uneven shards
        hip, _ = _cpu_pair(Z, 3, "shared", num_data=401)
        lo, _hi = p.distributed.shard_bounds(401)
        hip.likelihood.row_offset = lo  # the shard's first global row: its draws are those of the one-rank run
        Xs, Ys = p.distributed.shard_rows(X, Y)
        assert hip._reduce() and (rank == 0) == (lo == 0)
        for _ in range(3):
            hip.natgrad_step((Xs, Ys), lr=0.5)
        elbo = float(hip.elbo((Xs, Ys)))
        if rank == 0:
            np.savez(out, l1=hip.lambda_1.numpy(), L2=hip.lambda_2.numpy(), elbo=elbo)
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_with_row_offsets_match_one():
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
    assert abs(float(got["elbo"]) - e) < 1e-11 * abs(e)


def test_model_errors():
    p = pkg()
    X, Y, Z = problem(N=10, M=6)
    lik = p.Softmax(3)
    for P in (1, 2, 4):
        with pytest.raises(ValueError, match="latent_dim"):
            p.t_SVGP(p.Matern52(), lik, Z, num_latent_gps=P)
    with pytest.raises(ValueError):
        p.t_SVGP(p.SeparateIndependent([p.SquaredExponential(), p.SquaredExponential()]), lik,
                 p.SharedIndependentInducingVariables(Z), num_latent_gps=2)
    m = p.t_SVGP(p.Matern52(), lik, Z, num_latent_gps=3)
    for Yb in (np.zeros((10, 3)), np.zeros(10), np.zeros((9, 1))):
        for call in (m.natgrad_step, m.elbo, m.elbo_and_grads, m.moments_and_gradients, m.predict_log_density):
            with pytest.raises(ValueError, match="Softmax"):
                call((X, Yb))
    for P in (1, 3):
        with pytest.raises(NotImplementedError):
            p.t_SVGP_white(p.Matern52(), lik, Z, num_latent_gps=P)
        with pytest.raises(NotImplementedError):
            p.t_SVGP_sites((X, Y), p.Matern52(), lik, Z, num_latent_gps=P)
    # the heteroskedastic messages are what they were
    with pytest.raises(ValueError, match=r"the heteroskedastic likelihood needs num_latent_gps = 2 \(its latent_dim\), got 3"):
        p.t_SVGP(p.SquaredExponential(), p.HeteroskedasticTFPConditional(), Z, num_latent_gps=3)
