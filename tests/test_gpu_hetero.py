"""The heteroskedastic Gaussian likelihood on the GPU (reference docs/notebooks/heteroskedastic.py:58-150): the coupled map
``tsvgp_lik_map_hetero_*`` against the NumPy restatement (tests/hetero_ref.py), and t_SVGP with two latents against the oracle
driven by the restated likelihood -- every engine path (one shared kernel, separate kernels batched and one pass per latent),
every projection route, hipGraph replay, fp32, the M-step gradient, two ranks, and the notebook's E/M loop on its data.

Tolerances as tests/test_gpu_model.py: fp64 lambda_1 / Lambda_2 <= 1e-8 per step, ELBO <= 1e-9; fp32 against the fp64 oracle
atol 1e-4 + rtol 1e-3 on the moments, 1e-4 on the ELBO.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import tsvgp_oracle as O
from tests.hetero_ref import HeteroskedasticTFPConditional as RefHetero
from tests.helpers import free_port, pkg, relerr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mcycle.csv")


# ---------------------------------------------------------------------------------------------------------------- the map
def _map(mean, var, y, flags, dtype, N):
    B = pkg()._backend
    lib = B.lib()
    Np = B.round_up(N)
    dev = "cuda:0"
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)
    m, v, yy = t(mean), t(var), t(y)
    g0 = torch.full((Np, 2), 7.0, dtype=dtype, device=dev)  # the padding rows must come back zero
    g1 = torch.full((Np, 2), 7.0, dtype=dtype, device=dev)
    ve = torch.full((Np // 128,), 7.0, dtype=torch.float64, device=dev)
    nonpos = torch.full((Np // 128,), 7, dtype=torch.int32, device=dev)
    fn = lib.tsvgp_lik_map_hetero_f64 if dtype == torch.float64 else lib.tsvgp_lik_map_hetero_f32
    st = fn(m.data_ptr(), v.data_ptr(), yy.data_ptr(), flags, g0.data_ptr(), g1.data_ptr(), ve.data_ptr(), nonpos.data_ptr(),
            N, Np, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    return g0.cpu().numpy(), g1.cpu().numpy(), ve.cpu().numpy(), nonpos.cpu().numpy()


def _inputs(N, seed=0, m1=(-1.0, 1.0), v1=(0.01, 2.0)):
    rng = np.random.RandomState(seed)
    mean = np.stack([rng.randn(N), rng.uniform(*m1, N)], axis=1)
    var = np.stack([rng.uniform(0.01, 3.0, N), rng.uniform(*v1, N)], axis=1)
    y = mean[:, :1] + rng.randn(N, 1) * np.exp(mean[:, 1:])
    return mean, var, y


def _colerr(a, b):
    return max(relerr(a[:, p], b[:, p]) for p in range(a.shape[1]))


@pytest.mark.parametrize("N", [300, 128, 1])
def test_map_f64_matches_restatement(N):
    B = pkg()._backend
    mean, var, y = _inputs(N)
    ref = RefHetero()
    r0, r1 = ref.variational_expectations_grads(mean, var, y)
    rve = ref.variational_expectations(mean, var, y)
    Np = B.round_up(N)
    for flags in (B.LIK_HETERO, B.LIK_HETERO | B.LIK_NOCROP):
        g0, g1, ve, nonpos = _map(mean, var, y, flags, torch.float64, N)
        e1 = r1 if flags & B.LIK_NOCROP else np.minimum(r1, -1e-8)
        assert _colerr(g0[:N], r0) < 1e-13 and _colerr(g1[:N], e1) < 1e-13
        assert not g0[N:Np].any() and not g1[N:Np].any()
        blk = np.array([rve[b * 128:(b + 1) * 128].sum() for b in range(Np // 128)])
        np.testing.assert_allclose(ve, blk, rtol=1e-12, atol=1e-12)
        assert not nonpos.any()


def test_map_crop_moves_only_g1_above_the_bound():
    """Both g1 of this likelihood are negative (log p is concave in f0 and in f1), but the location latent's
    g1 = -1/2 E[exp(-2 f1)] is tiny where the log scale is large: the crop (reference tsvgp.py:262-263) moves exactly the values
    above -1e-8 there, NOCROP keeps them."""
    B = pkg()._backend
    mean, var, y = _inputs(256, seed=5)
    mean[::3, 1] = 12.0  # exp(-2 f1) ~ 1e-11
    g0c, g1c, _, _ = _map(mean, var, y, B.LIK_HETERO, torch.float64, 256)
    g0n, g1n, _, _ = _map(mean, var, y, B.LIK_HETERO | B.LIK_NOCROP, torch.float64, 256)
    assert (g1n[:, 0] > -1e-8).sum() > 20 and (g1n < 0).all()
    np.testing.assert_array_equal(g0c, g0n)
    np.testing.assert_array_equal(g1c, np.minimum(g1n, -1e-8))


def test_map_f32_within_input_rounding():
    B = pkg()._backend
    N = 1000
    mean, var, y = _inputs(N, seed=1)
    mean, var, y = (a.astype(np.float32).astype(np.float64) for a in (mean, var, y))  # what the kernel reads
    r0, r1 = RefHetero().variational_expectations_grads(mean, var, y)
    g0, g1, ve, _ = _map(mean, var, y, B.LIK_HETERO | B.LIK_NOCROP, torch.float32, N)
    assert _colerr(g0[:N], r0) < 1e-6 and _colerr(g1[:N], r1) < 1e-6  # only the fp32 rounding of the outputs
    np.testing.assert_allclose(ve.sum(), RefHetero().variational_expectations(mean, var, y).sum(), rtol=1e-12)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_map_finite_over_wide_log_scale_range(dtype):
    B = pkg()._backend
    N = 2000
    mean, var, y = _inputs(N, seed=2, m1=(-5.0, 5.0), v1=(0.0001, 25.0))
    g0, g1, ve, nonpos = _map(mean, var, y, B.LIK_HETERO, dtype, N)
    assert np.isfinite(g0).all() and np.isfinite(g1).all() and np.isfinite(ve).all() and not nonpos.any()
    if dtype == torch.float64:
        r0, r1 = RefHetero().variational_expectations_grads(mean, var, y)
        for p in range(2):
            np.testing.assert_allclose(g0[:N, p], r0[:, p], rtol=1e-11, atol=1e-11 * np.abs(r0[:, p]).max())


def test_map_counts_non_positive_variances_per_block():
    B = pkg()._backend
    N = 400
    mean, var, y = _inputs(N, seed=3)
    var[5, 0] = 0.0
    var[200, 1] = -1.0
    var[399, 0] = -2.0
    var[399, 1] = 0.0
    with np.errstate(invalid="ignore"):
        _, _, _, nonpos = _map(mean, var, y, B.LIK_HETERO, torch.float64, N)
    np.testing.assert_array_equal(nonpos, [1, 1, 0, 2])


def test_map_rejects_bad_arguments_on_device():
    B = pkg()._backend
    lib = B.lib()
    t = torch.zeros(256, 2, dtype=torch.float64, device="cuda:0")
    ve = torch.zeros(2, dtype=torch.float64, device="cuda:0")
    npos = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    ok = (t.data_ptr(), t.data_ptr(), t.data_ptr())
    outs = (t.data_ptr(), t.data_ptr(), ve.data_ptr(), npos.data_ptr())
    assert lib.tsvgp_lik_map_hetero_f64(None, *ok[1:], B.LIK_HETERO, *outs, 200, 256, s) == 1
    assert lib.tsvgp_lik_map_hetero_f64(*ok, B.LIK_HETERO, None, *outs[1:], 200, 256, s) == 1
    assert lib.tsvgp_lik_map_hetero_f64(*ok, B.LIK_HETERO, *outs[:3], None, 200, 256, s) == 1
    for flags in (B.LIK_GAUSSIAN, B.LIK_BERNOULLI, B.LIK_HETERO | B.LIK_MEANONLY):
        assert lib.tsvgp_lik_map_hetero_f64(*ok, flags, *outs, 200, 256, s) == 1
    assert lib.tsvgp_lik_map_hetero_f64(*ok, B.LIK_HETERO, *outs, 200, 256, s) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the model
def _problem(N=500, M=12, seed=0):
    rng = np.random.RandomState(seed)
    X = np.sort(rng.rand(N, 1) * 6 - 3, axis=0)
    f0 = np.sin(2 * X)
    f1 = 0.5 * np.cos(X) - 0.7
    Y = f0 + np.exp(f1) * rng.randn(N, 1)
    Z = np.linspace(-3.5, 3.5, M)[:, None]  # cond(K_uu + 1e-9 I) <= 6e2 at M = 12 for the lengthscales below
    return X, Y, Z


def _pair(Z, kind, projection="auto", compute_dtype=torch.float64, use_graph=False, num_data=None, **kw):
    """(HIP model, oracle with the restated likelihood): one shared SE kernel, or one per latent ("separate" / "perlatent")."""
    p = pkg()
    ls, var = (0.7, 0.8), (1.0, 0.5)
    if kind == "shared":
        kh, ko, ivh, ivo = p.SquaredExponential(1.0, 0.8), O.SquaredExponential(1.0, 0.8), Z, Z
    else:
        kh = p.SeparateIndependent([p.SquaredExponential(v, l) for v, l in zip(var, ls)])
        ko = O.SeparateIndependent([O.SquaredExponential(v, l) for v, l in zip(var, ls)])
        ivh, ivo = p.SharedIndependentInducingVariables(Z), O.SharedIndependentInducingVariables(Z)
    hip = p.t_SVGP(kh, p.HeteroskedasticTFPConditional(), ivh, num_latent_gps=2, projection=projection,
                   compute_dtype=compute_dtype, use_graph=use_graph, num_data=num_data, **kw)
    if kind == "perlatent":
        hip._get_engine().batch_separate = False
    ora = O.t_SVGP(ko, RefHetero(), ivo, num_latent_gps=2, num_data=num_data)
    return hip, ora


def _compare_state(hip, ora, tol):
    assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < tol
    assert relerr(hip.lambda_2.cpu().numpy(), ora.lambda_2) < tol


@pytest.mark.parametrize("projection", ["direct", "whitened", "projected"])
@pytest.mark.parametrize("kind", ["shared", "separate", "perlatent"])
def test_natgrad_steps_match_oracle(kind, projection):
    X, Y, Z = _problem()
    hip, ora = _pair(Z, kind, projection, num_data=len(X))
    assert hip._routes(1e-9) == [projection, projection]
    for step in range(8):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        _compare_state(hip, ora, 1e-8)
    if kind != "shared":
        assert hip._get_engine().last_batched == (kind == "separate" and projection != "projected")
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    assert abs(e_h - e_o) < 1e-9 * abs(e_o)
    mu, var, g0, g1 = hip.moments_and_gradients((X, Y))
    mu_o, var_o = ora.predict_f(X)
    r0, r1 = RefHetero().variational_expectations_grads(mu_o, var_o, Y)
    assert relerr(mu.cpu().numpy(), mu_o) < 1e-8 and relerr(var.cpu().numpy(), var_o) < 1e-8
    assert _colerr(g0.cpu().numpy(), r0) < 1e-7 and _colerr(g1.cpu().numpy(), np.minimum(r1, -1e-8)) < 1e-7


@pytest.mark.parametrize("projection", ["direct", "whitened", "projected"])
def test_graph_replay_matches_eager(projection):
    """One shared kernel is the configuration the step captures (separate kernels decline capture, as for every likelihood);
    the coupled map is an ordinary launch on the capturing stream."""
    X, Y, Z = _problem(seed=1)
    Xd, Yd = torch.as_tensor(X, device="cuda:0"), torch.as_tensor(Y, device="cuda:0")
    eager, _ = _pair(Z, "shared", projection)
    graph, _ = _pair(Z, "shared", projection, use_graph=True)
    for step in range(6):
        eager.natgrad_step((Xd, Yd), lr=0.5)
        graph.natgrad_step((Xd, Yd), lr=0.5)
        assert relerr(graph.lambda_1.numpy(), eager.lambda_1.numpy()) < 1e-13, step
        assert relerr(graph.lambda_2.cpu().numpy(), eager.lambda_2.cpu().numpy()) < 1e-13, step
    assert len([e for e in graph._graphs.values() if isinstance(e, dict)]) == 1
    sep_auto, _ = _pair(Z, "separate", use_graph=True)
    for _ in range(3):
        sep_auto.natgrad_step((Xd, Yd), lr=0.5)
    assert not any(isinstance(e, dict) for e in sep_auto._graphs.values())


@pytest.mark.parametrize("kind", ["shared", "separate", "perlatent"])
def test_fp32_against_fp64_oracle(kind):
    X, Y, Z = _problem(seed=2)
    hip, ora = _pair(Z, kind, "whitened", compute_dtype=torch.float32)
    for _ in range(4):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
    mu_h, var_h = hip.predict_f(X)
    mu_o, var_o = ora.predict_f(X)
    np.testing.assert_allclose(mu_h.cpu().numpy(), mu_o, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(var_h.cpu().numpy(), var_o, rtol=1e-3, atol=1e-4)
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    assert abs(e_h - e_o) < 1e-4 * abs(e_o)


@pytest.mark.parametrize("kind", ["shared", "separate"])
def test_predict_y_and_log_density_match_restatement(kind):
    X, Y, Z = _problem(seed=3)
    hip, ora = _pair(Z, kind)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
    Xt = X[::7] + 0.01
    Yt = Y[::7]
    ey, vy = hip.predict_y(Xt)
    ey_o, vy_o = ora.predict_y(Xt)
    assert ey.shape == (len(Xt), 1) and vy.shape == (len(Xt), 1)
    assert relerr(ey.cpu().numpy(), ey_o) < 1e-8 and relerr(vy.cpu().numpy(), vy_o) < 1e-8
    lpd = hip.predict_log_density((Xt, Yt)).cpu().numpy()
    np.testing.assert_allclose(lpd, ora.predict_log_density((Xt, Yt)), rtol=1e-8, atol=1e-9)


@pytest.mark.parametrize("kind", ["shared", "separate", "perlatent"])
def test_elbo_and_grads_match_central_differences(kind):
    X, Y, Z = _problem(N=300, M=10, seed=4)
    hip, ora = _pair(Z, kind, num_data=400)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
    elbo, grads = hip.elbo_and_grads((X, Y))
    assert abs(float(elbo) - ora.elbo((X, Y))) < 1e-9 * abs(ora.elbo((X, Y)))
    kernels = ora.kernel.kernels if kind != "shared" else [ora.kernel]
    state = dict(lambda_1=ora.lambda_1.copy(), lambda_2_sqrt=ora.lambda_2_sqrt.copy())

    def elbo_at(edit):
        ko = O.SeparateIndependent([O.SquaredExponential(float(k.variance), float(k.lengthscales)) for k in kernels]) \
            if kind != "shared" else O.SquaredExponential(float(kernels[0].variance), float(kernels[0].lengthscales))
        Zc = Z.copy()
        edit(ko, Zc)
        iv = O.SharedIndependentInducingVariables(Zc) if kind != "shared" else Zc
        return O.t_SVGP(ko, RefHetero(), iv, num_latent_gps=2, num_data=400, **state).elbo((X, Y))

    def fd(edit_up, edit_dn, h):
        return (elbo_at(edit_up) - elbo_at(edit_dn)) / (2 * h)

    for ki in range(len(kernels)):
        pre = f"kernels.{ki}." if kind != "shared" else ""
        kk = (lambda ko: ko.kernels[ki]) if kind != "shared" else (lambda ko: ko)
        for name in ("variance", "lengthscales"):
            h = 1e-6
            up = lambda ko, Zc, n=name: setattr(kk(ko), n, np.asarray(float(getattr(kk(ko), n)) + h))
            dn = lambda ko, Zc, n=name: setattr(kk(ko), n, np.asarray(float(getattr(kk(ko), n)) - h))
            want = fd(up, dn, h)
            got = float(grads[pre + name].sum())
            assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (pre + name, got, want)
    gZ = grads["Z"].cpu().numpy()
    for m in (0, 4, 9):
        h = 1e-6
        want = fd(lambda ko, Zc: Zc.__setitem__((m, 0), Zc[m, 0] + h), lambda ko, Zc: Zc.__setitem__((m, 0), Zc[m, 0] - h), h)
        assert abs(gZ[m, 0] - want) < 1e-5 * max(1.0, abs(want)), (m, gZ[m, 0], want)


def _worker_split(rank, world, port, out, split):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = pkg()
        X, Y, Z = _problem(N=1001, seed=6)
        m = p.t_SVGP(p.SeparateIndependent([p.SquaredExponential(1.0, 0.7), p.SquaredExponential(0.5, 0.8)]),
                     p.HeteroskedasticTFPConditional(), p.SharedIndependentInducingVariables(Z), num_latent_gps=2,
                     num_data=len(X), device="cuda:0", latent_split=split, projection="whitened")
        Xs, Ys = p.distributed.shard_rows(X, Y)
        Xd, Yd = torch.as_tensor(Xs, device="cuda:0"), torch.as_tensor(Ys, device="cuda:0")
        assert m._latent_split(m._routes(1e-9)) == (split is None)
        for _ in range(3):
            m.natgrad_step((Xd, Yd), lr=0.5)
        e = float(m.elbo((Xd, Yd)))
        if rank == 0:
            np.savez(out, l1=m.lambda_1.numpy(), L2=m.lambda_2.cpu().numpy(), elbo=e)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("split", [None, False])
def test_two_ranks_match_one(tmp_path, split):
    """Two ranks over gloo on the one GPU, each mapping its own rows, with and without the latents' M x M work split over the
    ranks: equal to the single-process step of the restated reference."""
    out = str(tmp_path / "r0.npz")
    mp.spawn(_worker_split, args=(2, free_port(), out, split), nprocs=2, join=True)
    got = np.load(out)
    X, Y, Z = _problem(N=1001, seed=6)
    ora = O.t_SVGP(O.SeparateIndependent([O.SquaredExponential(1.0, 0.7), O.SquaredExponential(0.5, 0.8)]), RefHetero(),
                   O.SharedIndependentInducingVariables(Z), num_latent_gps=2, num_data=len(X))
    for _ in range(3):
        ora.natgrad_step((X, Y), lr=0.5)
    assert relerr(got["l1"], ora.lambda_1) < 1e-8
    assert relerr(got["L2"], ora.lambda_2) < 1e-8
    assert abs(float(got["elbo"]) - ora.elbo((X, Y))) < 1e-9 * abs(ora.elbo((X, Y)))


# ---------------------------------------------------------------------------------------------------------------- notebook
def test_notebook_em_loop_matches_oracle_driven_loop():
    """docs/notebooks/heteroskedastic.py:40-150 on its own data (mcycle, 133 rows, Y scaled to unit deviation): M = 50
    inducing points on a linspace, per iteration 2 E-steps at lr 0.5 and one Adam step (lr 0.1) on the kernels' parameters,
    10 iterations.  The oracle runs the same E-steps with the hyperparameters the HIP M-step produced; every E-step state
    agrees and the ELBO rises."""
    p = pkg()
    T = p.training
    data = np.loadtxt(GOLDEN, delimiter=",", skiprows=1)
    X, Y = data[:, :1], data[:, 1:2]
    Y = Y / Y.std()
    N, M = len(X), 50
    Z = np.linspace(X.min(), X.max(), M)[:, None]
    hip = p.t_SVGP(p.SeparateIndependent([p.SquaredExponential(), p.SquaredExponential()]), p.HeteroskedasticTFPConditional(),
                   p.SharedIndependentInducingVariables(p.InducingPoints(Z)), num_data=N, num_latent_gps=2)
    assert hip._wants_graph(torch.as_tensor(X, device="cuda:0"))  # launch-bound: "auto" would replay (separate kernels decline)
    opt = T.Adam(0.1)
    names = [f"kernels.{k}.{n}" for k in range(2) for n in ("variance", "lengthscales")]
    elbos = []
    for it in range(10):
        ko = O.SeparateIndependent([O.SquaredExponential(float(k.variance.item()), float(k.lengthscales.item()))
                                    for k in hip.kernel.kernels])
        ora = O.t_SVGP(ko, RefHetero(), O.SharedIndependentInducingVariables(Z), num_data=N, num_latent_gps=2,
                       lambda_1=hip.lambda_1.numpy().copy(), lambda_2_sqrt=hip.lambda_2_sqrt.value.cpu().numpy().copy())
        for _ in range(2):
            hip.natgrad_step((X, Y), lr=0.5)
            ora.natgrad_step((X, Y), lr=0.5)
            _compare_state(hip, ora, 1e-8)
        elbos.append(float(hip.elbo((X, Y))))
        assert abs(elbos[-1] - ora.elbo((X, Y))) < 1e-9 * abs(elbos[-1])
        _, grads = hip.elbo_and_grads((X, Y))
        params = {n: par for n, (par, _) in T.trainable_parameters(hip).items() if n in names}
        u = {n: T._softplus_inv(params[n].value.detach().to(torch.float64)) for n in names}
        gu = {n: -grads[n].reshape(u[n].shape) * torch.sigmoid(u[n]) for n in names}
        opt.step(u, gu)
        for n in names:
            params[n].assign(torch.nn.functional.softplus(u[n]))
    assert elbos[-1] > elbos[0]
    ey, vy = hip.predict_y(X)
    assert torch.isfinite(ey).all() and (vy > 0).all()
