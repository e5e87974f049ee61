"""LinearCoregionalization on the GPU: the two row-parallel kernels ``tsvgp_lmc_mix_*`` / ``tsvgp_lmc_unmix_*`` against the NumPy
restatement (tests/lmc_ref.py), and t_SVGP with P outputs mixed from L latents against the oracle driven by ``lmc_ref.Mixed``.

Kernel tolerances: a sum of K terms accumulated in fp64 in index order (fused multiply-adds) is within K 2^-53 sum |terms| of the
exact value and so is NumPy's; the bound used is 4 K 2^-53 sum |terms|, plus one rounding of the output, 2^-24 |ref|, for fp32
arrays (their inputs are fp32 values to begin with).  Model tolerances are SURVEY 8(d)'s: fp64 1e-8 on lambda_1, Lambda_2, mean,
var and 1e-9 on the ELBO; fp32 against the fp64 reference atol 1e-4 + rtol 1e-3 and 1e-4 on the ELBO.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import tsvgp_oracle as O
from tests import lmc_ref
from tests.helpers import free_port, pkg, relerr
from tests.scalar_lik_ref import Poisson as RefPoisson

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U53, U24 = 2.0 ** -53, 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- the kernels
def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _mix(mean_g, var_g, W, dtype, count=True):
    B = pkg()._backend
    lib = B.lib()
    N, L = mean_g.shape
    P = W.shape[0]
    Np = B.round_up(N)
    m, v, Wd = _t(mean_g, dtype), _t(var_g, dtype), _t(W, torch.float64)
    Fmu = torch.full((N, P), 7.0, dtype=dtype, device=DEV)
    Fvar = torch.full((N, P), 7.0, dtype=dtype, device=DEV)
    bad = torch.full((Np // 128,), 7, dtype=torch.int32, device=DEV)
    fn = lib.tsvgp_lmc_mix_f64 if dtype == torch.float64 else lib.tsvgp_lmc_mix_f32
    st = fn(m.data_ptr(), v.data_ptr(), Wd.data_ptr(), Fmu.data_ptr(), Fvar.data_ptr(), bad.data_ptr() if count else None, N, Np, L, P,
            torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    return Fmu.cpu().numpy().astype(np.float64), Fvar.cpu().numpy().astype(np.float64), bad.cpu().numpy()


def _unmix(g0_f, g1_f, W, dtype, N, nocrop, mean_g=None, var_g=None):
    """g0_f, g1_f [Np, P] -> (g0_g, g1_g [Np, L], dW partials [Np / 128, P, L] or None)."""
    B = pkg()._backend
    lib = B.lib()
    Np, P = g0_f.shape
    L = W.shape[1]
    a, b, Wd = _t(g0_f, dtype), _t(g1_f, dtype), _t(W, torch.float64)
    g0 = torch.full((Np, L), 7.0, dtype=dtype, device=DEV)  # the padding rows must come back zero
    g1 = torch.full((Np, L), 7.0, dtype=dtype, device=DEV)
    want_dW = mean_g is not None
    m = _t(mean_g, dtype) if want_dW else None
    v = _t(var_g, dtype) if want_dW else None
    part = torch.full((Np // 128, P, L), 7.0, dtype=torch.float64, device=DEV) if want_dW else None
    fn = lib.tsvgp_lmc_unmix_f64 if dtype == torch.float64 else lib.tsvgp_lmc_unmix_f32
    st = fn(a.data_ptr(), b.data_ptr(), Wd.data_ptr(), B.LIK_NOCROP if nocrop else 0, g0.data_ptr(), g1.data_ptr(),
            m.data_ptr() if want_dW else None, v.data_ptr() if want_dW else None, part.data_ptr() if want_dW else None, N, Np, L, P,
            torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    return (g0.cpu().numpy().astype(np.float64), g1.cpu().numpy().astype(np.float64),
            part.cpu().numpy() if want_dW else None)


def _weights(L, P, seed=0):
    """W [P, L] with mixed signs and one zero column (the last); L = 1 leaves only zeros there, so that shape also gets the full W."""
    W = np.random.RandomState(100 + seed).uniform(0.3, 1.5, (P, L)) * np.where(np.arange(P * L).reshape(P, L) % 3 == 1, -1.0, 1.0)
    Wz = W.copy()
    Wz[:, L - 1] = 0.0
    return [Wz] + ([W] if L == 1 else [])


def _kernel_inputs(N, L, P, dtype, seed=0):
    B = pkg()._backend
    rng = np.random.RandomState(seed)
    rd = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == torch.float32 else (lambda a: a)  # what the kernel reads
    Np = B.round_up(N)
    mean_g, var_g = rd(rng.randn(N, L)), rd(rng.uniform(0.05, 2.0, (N, L)))
    g0_f, g1_f = np.zeros((Np, P)), np.zeros((Np, P))
    g0_f[:N], g1_f[:N] = rd(rng.randn(N, P)), rd(rng.randn(N, P) * 0.5)  # both signs: the crop has something to move
    g0_f[N:], g1_f[N:] = 3.0, 3.0  # the kernel must not read the padding rows of its inputs into anything
    return mean_g, var_g, g0_f, g1_f


def _within(name, got, ref, tol):
    err = np.abs(got - ref)
    print(f"{name}: max |diff| {err.max():.3e}, largest bound {tol.max():.3e}, worst ratio {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert np.all(err <= tol), name


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("L,P", [(1, 1), (1, 2), (2, 3), (3, 2), (32, 32)])
@pytest.mark.parametrize("N", [1, 127, 128, 129, 300])
def test_kernels_match_restatement(N, L, P, dtype):
    out32 = dtype == torch.float32
    mean_g, var_g, g0_f, g1_f = _kernel_inputs(N, L, P, dtype, seed=N + L)
    Np = g0_f.shape[0]
    for wi, W in enumerate(_weights(L, P)):
        W2 = W * W
        # mix
        Fmu, Fvar, bad = _mix(mean_g, var_g, W, dtype)
        rmu, rvar = lmc_ref.mix(W, mean_g, var_g)
        _within(f"Fmu W{wi}", Fmu, rmu, 4 * L * U53 * (np.abs(mean_g) @ np.abs(W).T) + (U24 * np.abs(rmu) if out32 else 0.0))
        _within(f"Fvar W{wi}", Fvar, rvar, 4 * L * U53 * (np.abs(var_g) @ W2.T) + (U24 * np.abs(rvar) if out32 else 0.0))
        assert not bad.any()
        again = _mix(mean_g, var_g, W, dtype)
        assert np.array_equal(again[0], Fmu) and np.array_equal(again[1], Fvar)  # bit for bit
        # un-mix, cropped and not, with the block sums of dW
        r0, r1 = lmc_ref.unmix(W, g0_f[:N], g1_f[:N], crop=False)
        t0 = 4 * P * U53 * (np.abs(g0_f[:N]) @ np.abs(W)) + (U24 * np.abs(r0) if out32 else 0.0)
        t1 = 4 * P * U53 * (np.abs(g1_f[:N]) @ W2) + (U24 * np.abs(r1) if out32 else 0.0)
        g0n, g1n, part = _unmix(g0_f, g1_f, W, dtype, N, True, mean_g, var_g)
        g0c, g1c, none = _unmix(g0_f, g1_f, W, dtype, N, False)
        assert none is None
        _within(f"g0_g W{wi}", g0n[:N], r0, t0)
        _within(f"g1_g nocrop W{wi}", g1n[:N], r1, t1)
        _within(f"g1_g crop W{wi}", g1c[:N], np.minimum(r1, -1e-8), t1 + (U24 * 1e-8 if out32 else 0.0))
        assert np.array_equal(g0c, g0n)
        for g in (g0n, g1n, g0c, g1c):  # rows >= N are zeros
            assert not g[N:Np].any()
        # crop and NOCROP differ only where g1_g > -1e-8
        moved = g1c[:N] != g1n[:N]
        assert np.array_equal(moved, g1n[:N] > np.float64(np.float32(-1e-8) if out32 else -1e-8))
        assert np.all(g1c[:N][moved] == (np.float64(np.float32(-1e-8)) if out32 else -1e-8))
        # dW: the blocks added in order, K = 2 N terms
        got = np.zeros((P, L))
        for blk in part:
            got += blk
        terms = np.abs(g0_f[:N]).T @ np.abs(mean_g) + 2.0 * np.abs(W) * (np.abs(g1_f[:N]).T @ np.abs(var_g))
        _within(f"dW W{wi}", got, lmc_ref.dW(W, g0_f[:N], g1_f[:N], mean_g, var_g), 4 * 2 * N * U53 * terms)
        g0a, g1a, parta = _unmix(g0_f, g1_f, W, dtype, N, True, mean_g, var_g)
        assert np.array_equal(g0a, g0n) and np.array_equal(g1a, g1n) and np.array_equal(parta, part)  # bit for bit


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_identity_W_reproduces_its_inputs_bit_for_bit(dtype):
    N, L = 300, 3
    mean_g, var_g, g0_f, g1_f = _kernel_inputs(N, L, L, dtype, seed=11)
    Fmu, Fvar, _ = _mix(mean_g, var_g, np.eye(L), dtype)
    assert np.array_equal(Fmu, mean_g) and np.array_equal(Fvar, var_g)
    g0, g1, _ = _unmix(g0_f, g1_f, np.eye(L), dtype, N, True)
    assert np.array_equal(g0[:N], g0_f[:N]) and np.array_equal(g1[:N], g1_f[:N])


def test_mix_counts_rows_with_a_bad_latent_moment_per_block():
    N, L = 400, 2
    mean_g, var_g, _, _ = _kernel_inputs(N, L, 3, torch.float64, seed=12)
    var_g[5, 0] = 0.0
    var_g[200, 1] = -1.0
    var_g[399, 0] = -2.0  # two bad entries in one row: the row counts once
    var_g[399, 1] = 0.0
    mean_g[130, 0] = np.inf
    var_g[131, 1] = np.nan
    W = _weights(L, 3)[0]  # (the zero column hides latent 1 from the outputs: the count sees it all the same)
    _, _, bad = _mix(mean_g, var_g, W, torch.float64)
    np.testing.assert_array_equal(bad, [1, 3, 0, 1])
    Fmu, Fvar, untouched = _mix(mean_g, var_g, W, torch.float64, count=False)
    assert np.all(untouched == 7)


def test_entries_reject_bad_arguments_on_device():
    B = pkg()._backend
    lib = B.lib()
    t = torch.zeros(256 * 4, dtype=torch.float64, device=DEV)
    ib = torch.zeros(2, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    a = t.data_ptr()
    assert lib.tsvgp_lmc_mix_f64(a, a, None, a, a, ib.data_ptr(), 200, 256, 2, 3, s) == 1
    assert lib.tsvgp_lmc_mix_f64(a, a, a, a, a, ib.data_ptr(), 200, 384, 2, 3, s) == 1
    assert lib.tsvgp_lmc_mix_f64(a, a, a, a, a, ib.data_ptr(), 200, 256, 33, 3, s) == 1
    assert lib.tsvgp_lmc_unmix_f64(a, a, a, 0, a, a, None, None, a, 200, 256, 2, 3, s) == 1
    assert lib.tsvgp_lmc_unmix_f64(a, a, a, B.LIK_GAUSSIAN, a, a, None, None, None, 200, 256, 2, 3, s) == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the model
N_, M_, D_ = 300, 16, 2
W32 = np.array([[0.9, -0.4], [0.0, 1.3], [-0.7, 0.5]])  # P = 3, L = 2
KPAR = ((1.0, 0.6), (0.7, 0.8))  # (variance, lengthscale) per latent: cond(K_uu + 1e-9 I) <= 40 on the grid below


def _problem(lik="gaussian", W=W32, seed=0, N=N_):
    """X [N, 2], Y [N, P] from L smooth latents mixed by W, Z on a 4 x 4 grid."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(-2.0, 2.0, (N, D_))
    G = np.sin(X @ rng.randn(D_, W.shape[1]) * 1.5)
    F = G @ W.T
    if lik == "gaussian":
        Y = F + np.sqrt(0.1) * rng.randn(*F.shape)
    elif lik == "bernoulli":
        Y = (F + 0.3 * rng.randn(*F.shape) > 0).astype(np.float64)
    else:
        Y = rng.poisson(np.exp(0.7 * F)).astype(np.float64)
    g = np.linspace(-1.5, 1.5, 4)
    Z = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, D_)
    assert Z.shape == (M_, D_)
    return X, Y, Z


def _liks(lik, noise=0.1):
    p = pkg()
    if lik == "gaussian":
        return p.Gaussian(noise), O.Gaussian(noise)
    if lik == "bernoulli":
        return p.Bernoulli(), O.Bernoulli()
    return p.Poisson(), RefPoisson()


def _pair(Z, lik="gaussian", W=W32, kpar=KPAR, noise=0.1, state=None, **kw):
    """(HIP model with LinearCoregionalization, oracle with SeparateIndependent kernels and the ``Mixed`` likelihood)."""
    p = pkg()
    lh, lo = _liks(lik, noise)
    kh = p.LinearCoregionalization([p.SquaredExponential(v, l) for v, l in kpar], W)
    ko = O.SeparateIndependent([O.SquaredExponential(v, l) for v, l in kpar])
    L = len(kpar)
    hip = p.t_SVGP(kh, lh, p.SharedIndependentInducingVariables(Z), num_latent_gps=L, device=DEV, **kw)
    ora = O.t_SVGP(ko, lmc_ref.Mixed(W, lo), O.SharedIndependentInducingVariables(Z), num_latent_gps=L,
                   num_data=kw.get("num_data"), **(state or {}))
    return hip, ora


def test_identity_W_equals_separate_independent():
    """(a) L = P = 2, W = I, Gaussian: the mixed-output model IS the SeparateIndependent model (whose Gaussian runs in the moments
    kernel's epilogue, not behind it): 1e-10 relative on the sites, the ELBO and predict_f."""
    p = pkg()
    X, Y, Z = _problem(W=np.eye(2))
    mk = lambda kern: p.t_SVGP(kern, p.Gaussian(0.1), p.SharedIndependentInducingVariables(Z), num_latent_gps=2, device=DEV)
    ks = lambda: [p.SquaredExponential(v, l) for v, l in KPAR]
    lmc, sep = mk(p.LinearCoregionalization(ks(), np.eye(2))), mk(p.SeparateIndependent(ks()))
    for _ in range(3):
        lmc.natgrad_step((X, Y), lr=0.8)
        sep.natgrad_step((X, Y), lr=0.8)
    assert relerr(lmc.lambda_1.numpy(), sep.lambda_1.numpy()) < 1e-10
    assert relerr(lmc.lambda_2.cpu().numpy(), sep.lambda_2.cpu().numpy()) < 1e-10
    e1, e2 = float(lmc.elbo((X, Y))), float(sep.elbo((X, Y)))
    assert abs(e1 - e2) < 1e-10 * abs(e2)
    (m1, v1), (m2, v2) = lmc.predict_f(X[:50]), sep.predict_f(X[:50])
    assert relerr(m1.cpu().numpy(), m2.cpu().numpy()) < 1e-10 and relerr(v1.cpu().numpy(), v2.cpu().numpy()) < 1e-10


def test_one_latent_two_outputs_equals_the_pooled_one_output_model():
    """(b) L = 1, P = 2, Gaussian, W = (w1, w2)^T: the two outputs are two noisy views of one latent, i.e. ONE observation
    y' = sum_p w_p y_p / sum_p w_p^2 with noise s2 / sum_p w_p^2 (complete the square in g): the same sites, and predict_f[:, p] =
    (w_p mean', w_p^2 var')."""
    p = pkg()
    w = np.array([[0.8], [-1.4]])
    s2, ss = 0.1, float(np.sum(w * w))
    X, Y, Z = _problem(W=w, seed=1)
    lmc = p.t_SVGP(p.LinearCoregionalization([p.SquaredExponential(*KPAR[0])], w), p.Gaussian(s2),
                   p.SharedIndependentInducingVariables(Z), num_latent_gps=1, device=DEV)
    one = p.t_SVGP(p.SquaredExponential(*KPAR[0]), p.Gaussian(s2 / ss), Z, device=DEV)
    Y1 = (Y @ w) / ss
    for _ in range(3):
        lmc.natgrad_step((X, Y), lr=0.8)
        one.natgrad_step((X, Y1), lr=0.8)
    assert relerr(lmc.lambda_1.numpy(), one.lambda_1.numpy()) < 1e-10
    assert relerr(lmc.lambda_2.cpu().numpy(), one.lambda_2.cpu().numpy()) < 1e-10
    (Fmu, Fvar), (m1, v1) = lmc.predict_f(X[:40]), one.predict_f(X[:40])
    assert Fmu.shape == (40, 2) and Fvar.shape == (40, 2)
    for q in range(2):
        assert relerr(Fmu[:, q].cpu().numpy(), w[q, 0] * m1[:, 0].cpu().numpy()) < 1e-10
        assert relerr(Fvar[:, q].cpu().numpy(), w[q, 0] ** 2 * v1[:, 0].cpu().numpy()) < 1e-10


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("projection", ["direct", "whitened", "projected"])
@pytest.mark.parametrize("lik", ["gaussian", "bernoulli", "poisson"])
def test_natgrad_steps_match_oracle_with_mixed_likelihood(lik, projection, dtype):
    """(c) L = 2, P = 3 on every route (direct and whitened run the batched launches, projected one pass per latent)."""
    X, Y, Z = _problem(lik)
    hip, ora = _pair(Z, lik, projection=projection, compute_dtype=dtype)
    assert hip._routes(1e-9) == [projection] * 2
    f64 = dtype == torch.float64
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.8)
        ora.natgrad_step((X, Y), lr=0.8)
        if f64:
            assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < 1e-8
            assert relerr(hip.lambda_2.cpu().numpy(), ora.lambda_2) < 1e-8
    assert hip._get_engine().last_batched == (projection != "projected")
    Fmu, Fvar = hip.predict_f(X)
    rmu, rvar = lmc_ref.mix(W32, *ora.predict_f(X))
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    print(f"{lik} {projection} {dtype}: mean {relerr(Fmu.cpu().numpy(), rmu):.2e} var {relerr(Fvar.cpu().numpy(), rvar):.2e} "
          f"elbo {abs(e_h - e_o) / abs(e_o):.2e}")
    if f64:
        assert relerr(Fmu.cpu().numpy(), rmu) < 1e-8 and relerr(Fvar.cpu().numpy(), rvar) < 1e-8
        assert abs(e_h - e_o) < 1e-9 * abs(e_o)
    else:
        np.testing.assert_allclose(Fmu.cpu().numpy(), rmu, rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(Fvar.cpu().numpy(), rvar, rtol=1e-3, atol=1e-4)
        assert abs(e_h - e_o) < 1e-4 * abs(e_o)


@pytest.mark.parametrize("projection", ["direct", "projected"])
def test_graph_replay_matches_eager_bit_for_bit_and_follows_W(projection):
    """(d) the step replayed from a captured graph (direct: the batched launches, projected: one pass per latent) equals the eager
    step bit for bit; W is read through a device pointer whose stamp is part of the graph's key, so after ``W.assign`` the next
    steps -- eager, captured anew, replayed -- use the new W."""
    X, Y, Z = _problem("bernoulli", seed=8)
    Xd, Yd = torch.as_tensor(X, device=DEV), torch.as_tensor(Y, device=DEV)
    eager, _ = _pair(Z, "bernoulli", projection=projection, use_graph=False)
    graph, _ = _pair(Z, "bernoulli", projection=projection, use_graph=True)

    def steps(n):
        for step in range(n):
            eager.natgrad_step((Xd, Yd), lr=0.8)
            graph.natgrad_step((Xd, Yd), lr=0.8)
            assert np.array_equal(graph.lambda_1.numpy(), eager.lambda_1.numpy()), step
            assert np.array_equal(graph.lambda_2_sqrt.value.cpu().numpy(), eager.lambda_2_sqrt.value.cpu().numpy()), step

    steps(4)  # eager, capture + replay, two more replays
    captured = lambda: len([e for e in graph._graphs.values() if isinstance(e, dict)])
    assert captured() == 1 and not eager._graphs
    before = graph.lambda_1.numpy().copy()
    W2 = W32 * np.array([[1.0, -1.0]]) + 0.2
    eager.kernel.W.assign(W2)
    graph.kernel.W.assign(W2)
    steps(4)
    assert captured() == 2  # a key of its own for the new W
    # ... and the new W is what the replayed steps used: the same four steps under the old W end elsewhere
    stale, _ = _pair(Z, "bernoulli", projection=projection, use_graph=False)
    for _ in range(8):
        stale.natgrad_step((Xd, Yd), lr=0.8)
    assert relerr(graph.lambda_1.numpy(), stale.lambda_1.numpy()) > 1e-3 and not np.array_equal(graph.lambda_1.numpy(), before)


def test_targets_must_have_one_column_per_row_of_W():
    X, Y, Z = _problem()
    hip, _ = _pair(Z)
    with pytest.raises(ValueError, match=r"\[300, 3\]"):
        hip.natgrad_step((X, Y[:, :2]), lr=0.8)
    with pytest.raises(ValueError, match=r"\[300, 3\]"):
        hip.elbo((X, Y[:, :2]))


@pytest.mark.parametrize("lik", ["gaussian", "poisson"])
def test_elbo_and_grads_match_central_differences(lik):
    """(e) every entry of the gradient against central differences of the reference ELBO (step 1e-6, 1e-5 relative to
    max(1, |value|), as tests/test_gpu_hetero.py), and "W" against ``lmc_ref.dW`` on the reference's own moments to 1e-9."""
    nd = 400
    X, Y, Z = _problem(lik, seed=4)
    hip, ora = _pair(Z, lik, num_data=nd)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.8)
        ora.natgrad_step((X, Y), lr=0.8)
    elbo, grads = hip.elbo_and_grads((X, Y))
    assert abs(float(elbo) - ora.elbo((X, Y))) < 1e-9 * abs(ora.elbo((X, Y)))
    assert set(grads) == ({"Z", "W"} | {f"kernels.{k}.{n}" for k in range(2) for n in ("variance", "lengthscales")}
                          | ({"likelihood_variance"} if lik == "gaussian" else set()))
    mean_g, var_g = ora.predict_f(X)
    g0_f, g1_f = ora.likelihood.output_grads(mean_g, var_g, Y)
    want_W = (nd / len(X)) * lmc_ref.dW(W32, g0_f, g1_f, mean_g, var_g)
    gW = grads["W"].cpu().numpy()
    assert gW.shape == (3, 2) and relerr(gW, want_W) < 1e-9
    state = dict(lambda_1=ora.lambda_1.copy(), lambda_2_sqrt=ora.lambda_2_sqrt.copy())

    def elbo_at(kpar=KPAR, W=W32, Zc=Z, noise=0.1):
        return _pair(Zc, lik, W=W, kpar=kpar, noise=noise, num_data=nd, state=state)[1].elbo((X, Y))

    h = 1e-6

    def check(name, got, up, dn):
        want = (elbo_at(**up) - elbo_at(**dn)) / (2 * h)
        assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (name, got, want)

    for k in range(2):
        for j, name in enumerate(("variance", "lengthscales")):
            def moved(s):
                kp = [list(q) for q in KPAR]
                kp[k][j] += s
                return dict(kpar=tuple(tuple(q) for q in kp))
            check(f"kernels.{k}.{name}", float(grads[f"kernels.{k}.{name}"].sum()), moved(h), moved(-h))
    gZ = grads["Z"].cpu().numpy()
    for m, d in ((0, 0), (5, 1), (15, 0)):
        def zmoved(s):
            Zc = Z.copy()
            Zc[m, d] += s
            return dict(Zc=Zc)
        check(f"Z[{m},{d}]", gZ[m, d], zmoved(h), zmoved(-h))
    for q in range(3):
        for l in range(2):
            def wmoved(s):
                Wc = W32.copy()
                Wc[q, l] += s
                return dict(W=Wc)
            check(f"W[{q},{l}]", gW[q, l], wmoved(h), wmoved(-h))
    if lik == "gaussian":
        check("likelihood_variance", float(grads["likelihood_variance"]), dict(noise=0.1 + h), dict(noise=0.1 - h))


def test_em_fit_raises_the_elbo_and_moves_W():
    p = pkg()
    X, Y, Z = _problem(seed=5)
    W0 = W32 + 0.3 * np.random.RandomState(0).randn(3, 2)  # start off the generating W
    hip, _ = _pair(Z, W=W0)
    logf, _ = p.training.em_fit(hip, (X, Y), iterations=2, n_e_steps=2, n_m_steps=3, nat_lr=0.8, adam_lr=0.05)
    assert logf[1] > logf[0]
    assert np.max(np.abs(hip.kernel.W.numpy() - W0)) > 1e-3
    assert np.isfinite(float(hip.elbo((X, Y))))


@pytest.mark.parametrize("lik", ["gaussian", "bernoulli", "poisson"])
def test_predictions_match_reference_likelihood_on_mixed_moments(lik):
    """(g) predict_y / predict_log_density are the likelihood's own on (Fmu, Fvar); full_output_cov is W diag(v) W^T."""
    X, Y, Z = _problem(lik, seed=6)
    hip, ora = _pair(Z, lik)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.8)
        ora.natgrad_step((X, Y), lr=0.8)
    Xt, Yt = X[::5] + 0.01, Y[::5]
    ey, vy = hip.predict_y(Xt)
    ey_o, vy_o = ora.predict_y(Xt)
    assert ey.shape == (len(Xt), 3) and vy.shape == (len(Xt), 3)
    assert relerr(ey.cpu().numpy(), ey_o) < 1e-8 and relerr(vy.cpu().numpy(), vy_o) < 1e-8
    lpd = hip.predict_log_density((Xt, Yt)).cpu().numpy()
    np.testing.assert_allclose(lpd.reshape(-1), np.asarray(ora.predict_log_density((Xt, Yt))).reshape(-1), rtol=1e-8, atol=1e-9)
    Fmu, Fcov = hip.predict_f(Xt, full_output_cov=True)
    mean_g, var_g = ora.predict_f(Xt)
    assert Fcov.shape == (len(Xt), 3, 3)
    assert relerr(Fcov.cpu().numpy(), lmc_ref.full_output_cov(W32, var_g)) < 1e-8
    assert relerr(Fmu.cpu().numpy(), lmc_ref.mix(W32, mean_g, var_g)[0]) < 1e-8


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = pkg()
        X, Y, Z = _problem("bernoulli", seed=7, N=301)
        hip, _ = _pair(Z, "bernoulli", num_data=301)
        Xs, Ys = p.distributed.shard_rows(X, Y)
        Xd, Yd = torch.as_tensor(Xs, device=DEV), torch.as_tensor(Ys, device=DEV)
        assert not hip._latent_split(hip._routes(1e-9))
        for _ in range(3):
            hip.natgrad_step((Xd, Yd), lr=0.8)
        e = float(hip.elbo((Xd, Yd)))
        e2, grads = hip.elbo_and_grads((Xd, Yd))
        if rank == 0:
            np.savez(out, l1=hip.lambda_1.numpy(), L2=hip.lambda_2.cpu().numpy(), elbo=e, elbo2=float(e2), gW=grads["W"].cpu().numpy())
    finally:
        dist.destroy_process_group()


def test_two_ranks_match_one(tmp_path):
    """(f) two gloo ranks on the one GPU, each with its own rows: the sites, the ELBO and dW (which rides in the all-reduced tail)
    equal the single-process reference."""
    out = str(tmp_path / "r0.npz")
    mp.spawn(_worker, args=(2, free_port(), out), nprocs=2, join=True)
    got = np.load(out)
    X, Y, Z = _problem("bernoulli", seed=7, N=301)
    _, ora = _pair(Z, "bernoulli", num_data=301)
    for _ in range(3):
        ora.natgrad_step((X, Y), lr=0.8)
    assert relerr(got["l1"], ora.lambda_1) < 1e-8 and relerr(got["L2"], ora.lambda_2) < 1e-8
    e_o = ora.elbo((X, Y))
    assert abs(float(got["elbo"]) - e_o) < 1e-9 * abs(e_o) and abs(float(got["elbo2"]) - e_o) < 1e-9 * abs(e_o)
    mean_g, var_g = ora.predict_f(X)
    g0_f, g1_f = ora.likelihood.output_grads(mean_g, var_g, Y)
    assert relerr(got["gW"], lmc_ref.dW(W32, g0_f, g1_f, mean_g, var_g)) < 1e-8
