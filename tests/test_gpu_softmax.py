"""The Softmax likelihood on the GPU (reference docs/notebooks/mnist.py): the in-kernel generator ``tsvgp_mc_normals_*`` and the
coupled map ``tsvgp_lik_map_softmax_*`` against the NumPy restatement (tests/softmax_ref.py), and t_SVGP with C latents against
the oracle driven by the restated likelihood at the same (seed, draw) -- every engine path (one shared kernel, separate kernels
batched and one pass per latent), every projection route, hipGraph replay, fp32, minibatches, the M-step gradient, the
predictive helpers, two ranks, the example's loop and one full-size step.

Tolerances as tests/test_gpu_hetero.py: the map 1e-13 per column on g0 / g1 and 1e-12 on the block sums of ve; the model fp64
lambda_1 / Lambda_2 <= 1e-8 per step, ELBO <= 1e-9; fp32 against the fp64 oracle atol 1e-4 + rtol 1e-3 on the moments, 1e-4 on the
ELBO.  The generator: bit-identical to the restatement wherever the device's log / sqrt / sin / cos round as NumPy's do; each of
those is specified to a few ulp at most on either side, the draw is a product of two such values of magnitude <= 6.7 and 1, so
8 ulp of the largest draw (6.7: 2^3 * 2^-52 * 8 = 1.4e-14) bounds an honest difference; the observed one goes to
profiles/softmax_parity.txt.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import tsvgp_oracle as O
from tests import softmax_ref as R
from tests.helpers import free_port, pkg, relerr
from tests.softmax_problem import pair, problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _note(line):
    """Observed figures, printed and (where the tree is writable) appended to profiles/softmax_parity.txt by the measuring run."""
    print("softmax_parity:", line)
    path = os.environ.get("TSVGP_SOFTMAX_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _normals(seed, draw, row_offset, S, N, C, dtype=torch.float64):
    lib = pkg()._backend.lib()
    out = torch.full((S, N, C), 7.0, dtype=dtype, device=DEV)
    fn = lib.tsvgp_mc_normals_f64 if dtype == torch.float64 else lib.tsvgp_mc_normals_f32
    assert fn(out.data_ptr(), seed, draw, row_offset, S, N, C, _stream()) == 0
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------- generator
@pytest.mark.parametrize("S,N,C,seed,draw,off", [(100, 300, 10, 0, 0, 0), (3, 1, 2, -5, 7, 2 ** 33 + 1), (7, 129, 32, 2 ** 40 + 3, 2, 500),
                                                 (5, 64, 5, 1, 2 ** 32 + 9, 0)])
def test_generator_matches_restatement(S, N, C, seed, draw, off):
    got = _normals(seed, draw, off, S, N, C).cpu().numpy()
    ref = R.normals(seed, draw, off + np.arange(N), S, C)
    diff = np.abs(got - ref)
    _note(f"mc_normals_f64 S={S} N={N} C={C}: {np.mean(got == ref):.6f} of the draws bit-identical, max |diff| = {diff.max():.3e}")
    assert diff.max() <= 1.4e-14
    got32 = _normals(seed, draw, off, S, N, C, torch.float32).cpu().numpy()
    np.testing.assert_array_equal(got32, got.astype(np.float32))  # the same fp64 draw, rounded once


# ---------------------------------------------------------------------------------------------------------------- the map
def _map(mean, var, y, flags, dtype, N, C, S, eps=None, seed=0, draw=0, off=0):
    B = pkg()._backend
    lib = B.lib()
    Np = B.round_up(N)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)
    m, v, yy = t(mean), t(var), t(y)
    e = None if eps is None else t(eps)
    state = torch.tensor([seed, draw], dtype=torch.int64, device=DEV)
    g0 = torch.full((Np, C), 7.0, dtype=dtype, device=DEV)  # the padding rows must come back zero
    g1 = torch.full((Np, C), 7.0, dtype=dtype, device=DEV)
    ve = torch.full((Np // 128,), 7.0, dtype=torch.float64, device=DEV)
    nonpos = torch.full((Np // 128,), 7, dtype=torch.int32, device=DEV)
    fn = lib.tsvgp_lik_map_softmax_f64 if dtype == torch.float64 else lib.tsvgp_lik_map_softmax_f32
    st = fn(m.data_ptr(), v.data_ptr(), yy.data_ptr(), flags, C, S, state.data_ptr(), off, None if e is None else e.data_ptr(),
            g0.data_ptr(), g1.data_ptr(), ve.data_ptr(), nonpos.data_ptr(), N, Np, _stream())
    assert st == 0
    torch.cuda.synchronize()
    return g0.cpu().numpy(), g1.cpu().numpy(), ve.cpu().numpy(), nonpos.cpu().numpy()


def _inputs(N, C, S, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.randn(N, C), rng.uniform(0.01, 3.0, (N, C)), rng.randint(0, C, (N, 1)).astype(np.float64), rng.randn(S, N, C))


def _colerr(a, b):
    return max(relerr(a[:, p], b[:, p]) for p in range(a.shape[1]))


def _blocks(ve, Np):
    return np.array([ve[b * 128:(b + 1) * 128].sum() for b in range(Np // 128)])


@pytest.mark.parametrize("S", [1, 100])
@pytest.mark.parametrize("C", [2, 3, 10, 32])
@pytest.mark.parametrize("N", [300, 128, 1])
def test_map_f64_matches_restatement(N, C, S):
    B = pkg()._backend
    mean, var, y, eps = _inputs(N, C, S, seed=N + C + S)
    ref = R.Softmax(C)
    r0, r1 = ref.variational_expectations_grads(mean, var, y, epsilon=eps)
    rve = ref.variational_expectations(mean, var, y, epsilon=eps)
    Np = B.round_up(N)
    for flags in (B.LIK_SOFTMAX, B.LIK_SOFTMAX | B.LIK_NOCROP):
        g0, g1, ve, nonpos = _map(mean, var, y, flags, torch.float64, N, C, S, eps=eps)
        e1 = r1 if flags & B.LIK_NOCROP else np.minimum(r1, -1e-8)
        errs = (_colerr(g0[:N], r0), _colerr(g1[:N], e1), float(np.max(np.abs(ve - _blocks(rve, Np)) / (1e-12 + 1e-12 * np.abs(_blocks(rve, Np))))))
        _note(f"map_f64 N={N} C={C} S={S} flags={flags:#x}: g0 {errs[0]:.2e} g1 {errs[1]:.2e} (bound 1e-13), ve / (atol + rtol) {errs[2]:.2e} (bound 1)")
        assert errs[0] < 1e-13 and errs[1] < 1e-13
        assert not g0[N:Np].any() and not g1[N:Np].any()
        np.testing.assert_allclose(ve, _blocks(rve, Np), rtol=1e-12, atol=1e-12)
        assert not nonpos.any()
    assert np.abs(g0[:N].sum(axis=1)).max() < 1e-14


def test_map_counts_non_positive_variances_per_block():
    B = pkg()._backend
    N, C, S = 400, 5, 10
    mean, var, y, eps = _inputs(N, C, S, seed=3)
    var[5, 0] = 0.0
    var[200, 4] = -1.0
    var[399, 0] = -2.0
    var[399, 3] = 0.0
    _, _, _, nonpos = _map(mean, var, y, B.LIK_SOFTMAX, torch.float64, N, C, S, eps=eps)
    np.testing.assert_array_equal(nonpos, [1, 1, 0, 2])


def test_crop_keeps_the_nan_of_a_negative_variance():
    """sqrt of a negative variance is NaN: that row's g0 and g1 are NaN with the crop too, as np.minimum leaves them (fmin alone
    would hand back a plausible -1e-8); the other rows are untouched and the row is counted."""
    B = pkg()._backend
    N, C, S = 130, 3, 10
    mean, var, y, eps = _inputs(N, C, S, seed=9)
    var[7, 1] = -0.5
    ref = R.Softmax(C)
    with np.errstate(invalid="ignore"):
        r0, r1 = ref.variational_expectations_grads(mean, var, y, epsilon=eps)
        e1 = np.minimum(r1, -1e-8)
    assert np.isnan(e1[7, 1]) and np.isnan(r0[7]).all()
    g0, g1, _, nonpos = _map(mean, var, y, B.LIK_SOFTMAX, torch.float64, N, C, S, eps=eps)
    np.testing.assert_array_equal(np.isnan(g0[:N]), np.isnan(r0))
    np.testing.assert_array_equal(np.isnan(g1[:N]), np.isnan(e1))
    ok = np.arange(N) != 7
    assert _colerr(g0[:N][ok], r0[ok]) < 1e-13 and _colerr(g1[:N][ok], e1[ok]) < 1e-13
    np.testing.assert_array_equal(nonpos, [1, 0])


def test_map_rejects_bad_arguments_on_device():
    B = pkg()._backend
    lib = B.lib()
    t = torch.zeros(256, 3, dtype=torch.float64, device=DEV)
    t[:, :] = 1.0
    yl = torch.zeros(256, 1, dtype=torch.float64, device=DEV)
    ve = torch.zeros(2, dtype=torch.float64, device=DEV)
    npos = torch.zeros(2, dtype=torch.int32, device=DEV)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    s = _stream()
    ins = (t.data_ptr(), t.data_ptr(), yl.data_ptr())
    g = torch.zeros(256, 3, dtype=torch.float64, device=DEV)
    outs = (g.data_ptr(), g.data_ptr(), ve.data_ptr(), npos.data_ptr())
    fn = lib.tsvgp_lik_map_softmax_f64
    call = lambda ins=ins, flags=B.LIK_SOFTMAX, C=3, S=4, rng=state.data_ptr(), outs=outs: fn(*ins, flags, C, S, rng, 0, None, *outs,
                                                                                             200, 256, s)
    assert call(C=1) == 1 and call(C=33) == 1 and call(S=0) == 1 and call(rng=None) == 1
    assert call(ins=(None,) + ins[1:]) == 1 and call(ins=ins[:2] + (None,)) == 1
    assert call(outs=(None,) + outs[1:]) == 1 and call(outs=outs[:3] + (None,)) == 1
    for flags in (B.LIK_HETERO, B.LIK_GAUSSIAN, B.LIK_SOFTMAX | B.LIK_MEANONLY):
        assert call(flags=flags) == 1
    assert call() == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [2, 10, 13, 32])
def test_in_kernel_generator_equals_the_map_fed_mc_normals(C):
    B = pkg()._backend
    N, S, seed, draw, off = 300, 100, 11, 5, 1000
    mean, var, y, _ = _inputs(N, C, 1, seed=C)
    eps = _normals(seed, draw, off, S, N, C).cpu().numpy()
    a = _map(mean, var, y, B.LIK_SOFTMAX, torch.float64, N, C, S, eps=eps)
    b = _map(mean, var, y, B.LIK_SOFTMAX, torch.float64, N, C, S, seed=seed, draw=draw, off=off)
    for x, z in zip(a, b):
        np.testing.assert_array_equal(x, z)
    c = _map(mean, var, y, B.LIK_SOFTMAX, torch.float64, N, C, S, seed=seed, draw=draw + 1, off=off)
    assert not np.array_equal(a[0], c[0])


def test_row_range_with_offset_equals_rows_of_the_full_launch():
    B = pkg()._backend
    N, C, S = 500, 10, 100
    mean, var, y, _ = _inputs(N, C, 1, seed=8)
    g0, g1, _, _ = _map(mean, var, y, B.LIK_SOFTMAX, torch.float64, N, C, S, seed=4, draw=2)
    for a, b in ((0, 130), (130, 500), (257, 258)):
        p0, p1, _, _ = _map(mean[a:b], var[a:b], y[a:b], B.LIK_SOFTMAX, torch.float64, b - a, C, S, seed=4, draw=2, off=a)
        np.testing.assert_array_equal(p0[:b - a], g0[a:b])
        np.testing.assert_array_equal(p1[:b - a], g1[a:b])


def test_map_f32_against_fp64_restatement():
    B = pkg()._backend
    N, C, S = 1000, 10, 100
    mean, var, y, eps = _inputs(N, C, S, seed=1)
    mean, var, eps = (a.astype(np.float32).astype(np.float64) for a in (mean, var, eps))  # what the kernel reads
    ref = R.Softmax(C)
    r0, r1 = ref.variational_expectations_grads(mean, var, y, epsilon=eps)
    g0, g1, ve, _ = _map(mean, var, y, B.LIK_SOFTMAX | B.LIK_NOCROP, torch.float32, N, C, S, eps=eps)
    np.testing.assert_allclose(g0[:N], r0, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(g1[:N], r1, rtol=1e-3, atol=1e-4)
    rve = ref.variational_expectations(mean, var, y, epsilon=eps).sum()
    assert abs(ve.sum() - rve) < 1e-4 * abs(rve)
    # the in-kernel draws of the fp32 entry are the fp64 draws: against the restated generator
    h0, h1, hve, _ = _map(mean, var, y, B.LIK_SOFTMAX | B.LIK_NOCROP, torch.float32, N, C, S, seed=3, draw=1)
    epsg = R.normals(3, 1, np.arange(N), S, C)
    q0, q1 = ref.variational_expectations_grads(mean, var, y, epsilon=epsg)
    np.testing.assert_allclose(h0[:N], q0, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(h1[:N], q1, rtol=1e-3, atol=1e-4)


def test_bad_labels_give_nan_rows_only():
    B = pkg()._backend
    N, C, S = 200, 3, 10
    mean, var, y, eps = _inputs(N, C, S, seed=6)
    bad = {3: 3.0, 77: -1.0, 130: 1.5, 199: np.nan}
    for n, v in bad.items():
        y[n, 0] = v
    g0, g1, ve, _ = _map(mean, var, y, B.LIK_SOFTMAX, torch.float64, N, C, S, eps=eps)
    rows = np.zeros(N, bool)
    rows[list(bad)] = True
    assert np.isnan(g0[:N][rows]).all() and np.isnan(g1[:N][rows]).all() and np.isnan(ve).all()
    assert np.isfinite(g0[:N][~rows]).all() and np.isfinite(g1[:N][~rows]).all()
    assert not g0[N:].any() and not g1[N:].any()


# ---------------------------------------------------------------------------------------------------------------- the model
def _gpu_pair(Z, C, kind, projection="auto", **kw):
    hip, ora = pair(Z, C, kind, projection=projection, **kw)
    if kind == "perlatent":
        hip._get_engine().batch_separate = False
    return hip, ora


def _compare_state(hip, ora, tol):
    assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < tol
    assert relerr(hip.lambda_2.cpu().numpy(), ora.lambda_2) < tol


@pytest.mark.parametrize("projection", ["direct", "whitened", "projected"])
@pytest.mark.parametrize("kind", ["shared", "separate", "perlatent"])
def test_natgrad_steps_match_oracle(kind, projection):
    X, Y, Z = problem()
    hip, ora = _gpu_pair(Z, 3, kind, projection, num_data=len(X))
    assert hip._routes(1e-9) == [projection] * 3
    for step in range(6):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        _compare_state(hip, ora, 1e-8)
        assert hip.likelihood.draw == ora.likelihood.draw == step + 1
    if kind != "shared":
        assert hip._get_engine().last_batched == (kind == "separate" and projection != "projected")
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    assert abs(e_h - e_o) < 1e-9 * abs(e_o)
    assert int(hip.likelihood.rng_state(DEV)[1]) == hip.likelihood.draw == 7  # the device count keeps level
    mu, var, g0, g1 = hip.moments_and_gradients((X, Y))
    mu_o, var_o = ora.predict_f(X)
    r0, r1 = ora.likelihood.variational_expectations_grads(mu_o, var_o, Y)
    assert relerr(mu.cpu().numpy(), mu_o) < 1e-8 and relerr(var.cpu().numpy(), var_o) < 1e-8
    assert _colerr(g0.cpu().numpy(), r0) < 1e-7 and _colerr(g1.cpu().numpy(), np.minimum(r1, -1e-8)) < 1e-7


def test_ten_classes_shared_kernel_match_oracle():
    X, Y, Z = problem(N=400, M=16, D=3, C=10, seed=2)
    hip, ora = _gpu_pair(Z, 10, "shared", num_data=len(X))
    for _ in range(4):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        _compare_state(hip, ora, 1e-8)


@pytest.mark.parametrize("projection", ["direct", "whitened", "projected"])
def test_graph_replay_matches_eager(projection):
    """The draw advances INSIDE the graph (the map reads (seed, draw) from device memory, the add is a captured node): replays
    equal eager steps, which equal the oracle's."""
    X, Y, Z = problem(seed=1)
    Xd, Yd = torch.as_tensor(X, device=DEV), torch.as_tensor(Y, device=DEV)
    eager, ora = _gpu_pair(Z, 3, "shared", projection)
    graph, _ = _gpu_pair(Z, 3, "shared", projection, use_graph=True)
    for step in range(6):
        eager.natgrad_step((Xd, Yd), lr=0.5)
        graph.natgrad_step((Xd, Yd), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        assert relerr(graph.lambda_1.numpy(), eager.lambda_1.numpy()) < 1e-13, step
        assert relerr(graph.lambda_2.cpu().numpy(), eager.lambda_2.cpu().numpy()) < 1e-13, step
        assert graph.likelihood.draw == step + 1 == int(graph.likelihood.rng_state(DEV)[1])
        _compare_state(graph, ora, 1e-8)
    assert len([e for e in graph._graphs.values() if isinstance(e, dict)]) == 1


def test_seed_change_between_replays_matches_eager():
    """The captured map and the captured draw + 1 hold the address of the likelihood's device words: a new seed is written into
    those words in place (never into a new tensor), with or without an eager evaluation in between, and the replays that follow
    draw from the new seed exactly as eager steps and the oracle do."""
    X, Y, Z = problem(seed=5)
    Xd, Yd = torch.as_tensor(X, device=DEV), torch.as_tensor(Y, device=DEV)
    eager, ora = _gpu_pair(Z, 3, "shared")
    graph, _ = _gpu_pair(Z, 3, "shared", use_graph=True)

    def steps(n):
        for _ in range(n):
            eager.natgrad_step((Xd, Yd), lr=0.5)
            graph.natgrad_step((Xd, Yd), lr=0.5)
            ora.natgrad_step((X, Y), lr=0.5)
            assert relerr(graph.lambda_1.numpy(), eager.lambda_1.numpy()) < 1e-13
            assert relerr(graph.lambda_2.cpu().numpy(), eager.lambda_2.cpu().numpy()) < 1e-13
            _compare_state(graph, ora, 1e-8)

    steps(3)  # eager, capture + replay, replay
    entries = [e for e in graph._graphs.values() if isinstance(e, dict)]
    assert len(entries) == 1
    state = graph.likelihood.rng_state(DEV)
    assert entries[0]["lik_state"] is state
    ptr = state.data_ptr()
    for seed, with_eager_call in ((41, False), (42, True)):
        for m in (eager, graph, ora):
            m.likelihood.seed = seed
        if with_eager_call:  # an eager evaluation between the seed change and the next replay
            e_o = ora.elbo((X, Y))
            assert abs(float(graph.elbo((Xd, Yd))) - e_o) < 1e-9 * abs(e_o)
            assert abs(float(eager.elbo((Xd, Yd))) - e_o) < 1e-9 * abs(e_o)
        assert graph.likelihood.rng_state(DEV) is state and state.data_ptr() == ptr
        assert state.tolist() == [seed, graph.likelihood.draw]
        steps(2)
    assert len([e for e in graph._graphs.values() if isinstance(e, dict)]) == 1  # all of them replays of the one capture
    assert state.tolist() == [42, graph.likelihood.draw] and graph.likelihood.draw == ora.likelihood.draw == 8


@pytest.mark.parametrize("kind", ["shared", "separate", "perlatent"])
def test_fp32_against_fp64_oracle(kind):
    X, Y, Z = problem(seed=2)
    hip, ora = _gpu_pair(Z, 3, kind, "whitened", compute_dtype=torch.float32)
    for _ in range(4):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
    mu_h, var_h = hip.predict_f(X)
    mu_o, var_o = ora.predict_f(X)
    np.testing.assert_allclose(mu_h.cpu().numpy(), mu_o, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(var_h.cpu().numpy(), var_o, rtol=1e-3, atol=1e-4)
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    assert abs(e_h - e_o) < 1e-4 * abs(e_o)


def test_minibatch_sequence_with_num_data_rescaling():
    X, Y, Z = problem(N=600, seed=3)
    hip, ora = _gpu_pair(Z, 3, "shared", num_data=600)
    rng = np.random.RandomState(0)
    for _ in range(6):
        idx = rng.choice(600, 100, replace=False)
        hip.natgrad_step((X[idx], Y[idx]), lr=0.3)
        ora.natgrad_step((X[idx], Y[idx]), lr=0.3)
        _compare_state(hip, ora, 1e-8)


@pytest.mark.parametrize("kind", ["shared", "separate"])
def test_predict_y_and_log_density_match_restatement(kind):
    X, Y, Z = problem(seed=3)
    hip, ora = _gpu_pair(Z, 3, kind)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
    Xt, Yt = X[::7] + 0.01, Y[::7]
    # the default draws: (seed, draw) of both sides agree, and each call consumes one
    ey, vy = hip.predict_y(Xt)
    ey_o, vy_o = ora.predict_y(Xt)
    assert ey.shape == (len(Xt), 3) and vy.shape == (len(Xt), 3)
    assert relerr(ey.cpu().numpy(), ey_o) < 1e-8 and relerr(vy.cpu().numpy(), vy_o) < 1e-8
    lpd = hip.predict_log_density((Xt, Yt)).cpu().numpy()
    np.testing.assert_allclose(lpd, ora.predict_log_density((Xt, Yt)), rtol=1e-8, atol=1e-9)
    assert hip.likelihood.draw == ora.likelihood.draw == 5
    # test points are numbered from 0 whatever the training shard's row offset is
    hip.likelihood.row_offset = ora.likelihood.row_offset = 1234
    ey2, _ = hip.predict_y(Xt)
    assert relerr(ey2.cpu().numpy(), ora.predict_y(Xt)[0]) < 1e-8
    hip.likelihood.row_offset = ora.likelihood.row_offset = 0
    hip.likelihood.draw = ora.likelihood.draw = 5
    # a shared epsilon
    eps = np.random.RandomState(1).randn(100, len(Xt), 3)
    Fmu, Fvar = hip.predict_f(Xt)
    mu_o, var_o = ora.predict_f(Xt)
    ey, vy = hip.likelihood.predict_mean_and_var(Fmu, Fvar, epsilon=torch.as_tensor(eps, device=DEV))
    ey_o, vy_o = ora.likelihood.predict_mean_and_var(mu_o, var_o, epsilon=eps)
    assert relerr(ey.cpu().numpy(), ey_o) < 1e-8 and relerr(vy.cpu().numpy(), vy_o) < 1e-8
    lpd = hip.likelihood.predict_log_density(Fmu, Fvar, torch.as_tensor(Yt, device=DEV), epsilon=torch.as_tensor(eps, device=DEV))
    np.testing.assert_allclose(lpd.cpu().numpy(), ora.likelihood.predict_log_density(mu_o, var_o, Yt, epsilon=eps), rtol=1e-8, atol=1e-9)
    assert hip.likelihood.draw == 5


@pytest.mark.parametrize("kind", ["shared", "separate", "perlatent"])
def test_elbo_and_grads_match_central_differences_at_a_frozen_draw(kind):
    X, Y, Z = problem(N=200, M=8, seed=4)
    C = 3
    hip, ora = _gpu_pair(Z, C, kind, num_data=300)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
    d = hip.likelihood.draw
    elbo, grads = hip.elbo_and_grads((X, Y))
    assert hip.likelihood.draw == d + 1  # one coupled pass, one draw
    kernels = ora.kernel.kernels if kind != "shared" else [ora.kernel]
    state = dict(lambda_1=ora.lambda_1.copy(), lambda_2_sqrt=ora.lambda_2_sqrt.copy())

    def elbo_at(edit):
        cls = type(kernels[0])
        ks = [cls(float(k.variance), float(k.lengthscales)) for k in kernels]
        ko = O.SeparateIndependent(ks) if kind != "shared" else ks[0]
        Zc = Z.copy()
        edit(ko, Zc)
        iv = O.SharedIndependentInducingVariables(Zc) if kind != "shared" else Zc
        lik = R.Softmax(C, seed=ora.likelihood.seed)
        lik.draw = d  # the draw elbo_and_grads took
        return O.t_SVGP(ko, lik, iv, num_latent_gps=C, num_data=300, **state).elbo((X, Y))

    base = elbo_at(lambda ko, Zc: None)
    assert abs(float(elbo) - base) < 1e-9 * abs(base)
    fd = lambda up, dn, h: (elbo_at(up) - elbo_at(dn)) / (2 * h)
    for ki in range(len(kernels)):
        pre = f"kernels.{ki}." if kind != "shared" else ""
        kk = (lambda ko, ki=ki: ko.kernels[ki]) if kind != "shared" else (lambda ko: ko)
        for name in ("variance", "lengthscales"):
            h = 1e-6
            up = lambda ko, Zc, n=name: setattr(kk(ko), n, np.asarray(float(getattr(kk(ko), n)) + h))
            dn = lambda ko, Zc, n=name: setattr(kk(ko), n, np.asarray(float(getattr(kk(ko), n)) - h))
            want = fd(up, dn, h)
            got = float(grads[pre + name].sum())
            assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (pre + name, got, want)
    gZ = grads["Z"].cpu().numpy()
    for m in (0, 4, 7):
        h = 1e-6
        want = fd(lambda ko, Zc: Zc.__setitem__((m, 0), Zc[m, 0] + h), lambda ko, Zc: Zc.__setitem__((m, 0), Zc[m, 0] - h), h)
        assert abs(gZ[m, 0] - want) < 1e-5 * max(1.0, abs(want)), (m, gZ[m, 0], want)


def _worker(rank, world, port, out, backend):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        p = pkg()
        X, Y, Z = problem(N=1001, seed=6)
        m, _ = pair(Z, 3, "shared", num_data=len(X), device=DEV, projection="whitened")
        lo, _hi = p.distributed.shard_bounds(len(X))
        m.likelihood.row_offset = lo
        Xs, Ys = p.distributed.shard_rows(X, Y)
        Xd, Yd = torch.as_tensor(Xs, device=DEV), torch.as_tensor(Ys, device=DEV)
        for _ in range(3):
            m.natgrad_step((Xd, Yd), lr=0.5)
        e = float(m.elbo((Xd, Yd)))
        if rank == 0:
            np.savez(out, l1=m.lambda_1.numpy(), L2=m.lambda_2.cpu().numpy(), elbo=e)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_ranks_match_one(tmp_path, backend, world):
    out = str(tmp_path / "r0.npz")
    mp.spawn(_worker, args=(world, free_port(), out, backend), nprocs=world, join=True)
    got = np.load(out)
    X, Y, Z = problem(N=1001, seed=6)
    _, ora = pair(Z, 3, "shared", num_data=len(X))
    for _ in range(3):
        ora.natgrad_step((X, Y), lr=0.5)
    assert relerr(got["l1"], ora.lambda_1) < 1e-8 and relerr(got["L2"], ora.lambda_2) < 1e-8
    assert abs(float(got["elbo"]) - ora.elbo((X, Y))) < 1e-9 * abs(ora.elbo((X, Y)))


# ---------------------------------------------------------------------------------------------------------------- example
def test_example_loop_matches_oracle_driven_loop():
    """Two iterations of examples/multiclass.py at a small size (its own functions).  In each, the minibatch E-steps agree with the
    oracle running the same minibatches from the same state -- in the second iteration at the kernel parameters and inducing inputs
    the HIP M-steps of the first left -- and the reported figures are finite."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("multiclass", os.path.join(ROOT, "examples", "multiclass.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    p = pkg()
    C, D, M, N = 4, 5, 20, 600
    X, Y, Xt, Yt = ex.make_data(N, 200, D, C, seed=0)
    model, Z0 = ex.make_model(X, C, M, N, seed=0)
    opt = p.training.Adam(0.01)
    rng_e, rng_m = np.random.RandomState(1), np.random.RandomState(2)
    for it in range(2):
        kern = O.Matern52(float(model.kernel.variance.item()), model.kernel.lengthscales.numpy().astype(np.float64).reshape(-1))
        Zc = model.inducing_variable.Z.numpy().astype(np.float64)
        if it == 0:
            np.testing.assert_array_equal(Zc, Z0)
        lik = R.Softmax(C, seed=model.likelihood.seed)
        lik.draw = model.likelihood.draw
        ora = O.t_SVGP(kern, lik, Zc, num_latent_gps=C, num_data=N, lambda_1=model.lambda_1.numpy().copy(),
                       lambda_2_sqrt=model.lambda_2_sqrt.value.cpu().numpy().copy())
        seen = []
        ex.e_steps(model, X, Y, batch=100, steps=3, lr=0.5, rng=rng_e, on_batch=lambda idx: seen.append(idx))
        for idx in seen:
            ora.natgrad_step((X[idx], Y[idx]), lr=0.5)
        _compare_state(model, ora, 1e-8)
        assert model.likelihood.draw == ora.likelihood.draw
        before = (float(model.kernel.variance.item()), model.inducing_variable.Z.numpy().copy())
        ex.m_steps(model, X, Y, batch=100, steps=2, opt=opt, rng=rng_m)
        assert float(model.kernel.variance.item()) != before[0] and not np.array_equal(model.inducing_variable.Z.numpy(), before[1])
    nlpd, acc = ex.evaluate(model, Xt, Yt)
    assert np.isfinite(nlpd) and 0.0 <= acc <= 1.0 and np.isfinite(float(model.elbo((X, Y))))


# ---------------------------------------------------------------------------------------------------------------- full size
def test_full_size_step_completes_and_matches_on_a_row_sample():
    """N = 1e6, C = 10, M = 1024, shared Matern-5/2: one natural-gradient step completes with a finite state; the moments of a row
    sample agree with the oracle's conditional at that state, and g0 / g1 of those rows with the restatement at their GLOBAL
    row numbers (the in-kernel generator over the whole row range)."""
    p = pkg()
    N, M, D, C = 1_000_000, 1024, 8, 10
    rng = np.random.RandomState(0)
    X = rng.randn(N, D)
    Y = np.argmax(X @ rng.randn(D, C) + 0.5 * rng.randn(N, C), axis=1)[:, None].astype(np.float64)
    Z = X[:M].copy()
    model = p.t_SVGP(p.Matern52(1.0, 3.0), p.Softmax(C, seed=5), Z, num_latent_gps=C, num_data=N)
    Xd, Yd = torch.as_tensor(X, device=DEV), torch.as_tensor(Y, device=DEV)
    model.natgrad_step((Xd, Yd), lr=0.5)
    assert np.isfinite(model.lambda_1.numpy()).all() and torch.isfinite(model.lambda_2).all() and model.likelihood.draw == 1
    mu, var, g0, g1 = model.moments_and_gradients((Xd, Yd))  # draw 1
    idx = np.arange(N)[::1999][:400]
    ora = O.t_SVGP(O.Matern52(1.0, 3.0), R.Softmax(C, seed=5), Z, num_latent_gps=C, num_data=N)
    ora.sites.lambda_1 = model.lambda_1.numpy()
    ora.sites._lambda_2_sqrt = np.tril(model.lambda_2_sqrt.numpy())
    mu_o, var_o = ora.predict_f(X[idx])
    mu_s, var_s = mu.cpu().numpy()[idx], var.cpu().numpy()[idx]
    assert relerr(mu_s, mu_o) < 1e-8 and relerr(var_s, var_o) < 1e-8
    eps = R.normals(5, 1, idx, 100, C)
    r0, r1 = ora.likelihood.variational_expectations_grads(mu_s, var_s, Y[idx], epsilon=eps)
    assert _colerr(g0.cpu().numpy()[idx], r0) < 1e-12 and _colerr(g1.cpu().numpy()[idx], np.minimum(r1, -1e-8)) < 1e-12
