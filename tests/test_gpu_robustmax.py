"""The MultiClass likelihood with the RobustMax link on the GPU: the coupled map ``tsvgp_lik_map_robustmax_*`` entry by entry
against the NumPy restatement (tests/robustmax_ref.py), and t_SVGP with C latents against the oracle driven by the restated
likelihood -- every engine path (one shared kernel, separate kernels batched and one pass per latent), every projection route,
hipGraph replay, fp32, minibatches, the predictive helpers, two ranks, the M-step gradient and a short E/M fit.

Bounds (tests/test_gpu_scalar_lik.py): fp64 max relative error <= 1e-8 on g0, g1, lambda_1, Lambda_2 and <= 1e-9 on
the sums of ve and the ELBO; fp32 arrays against the fp64 restatement atol 1e-4 + rtol 1e-3; ``elbo_and_grads`` against central
difference quotients at h = 1e-5 relative to 2e-6 relative (tests/test_gpu_mstep.py).  Everything here is deterministic: no draw,
no frozen generator state.
"""
import functools
import importlib
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import robustmax_ref as R
from tests.helpers import free_port, pkg, relerr
from tests.robustmax_problem import blobs, clip_rows, map_inputs, pair, problem

pytestmark = pytest.mark.gpu

MultiClass = pkg().MultiClass  # without the feature nothing here is collected
DEV = "cuda:0"
DTYPES = {"f64": torch.float64, "f32": torch.float32}


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------- the map
def _map(mean, var, y, flags, dtype, C, epsilon=1e-3):
    """One call of the C-ABI on sentinel-filled outputs: (g0, g1 [Np, C], ve_partial, nonpos_partial [Np / 128]) as NumPy."""
    B = pkg()._backend
    lib = B.lib()
    N = mean.shape[0]
    Np = B.round_up(N)
    t = lambda a: torch.as_tensor(np.array(a, order="C"), dtype=dtype, device=DEV)  # a copy: the shared references are read-only
    m, v, yy = t(mean), t(var), t(y)
    g0 = torch.full((Np, C), 7.0, dtype=dtype, device=DEV)  # the padding rows must come back zero
    g1 = torch.full((Np, C), 7.0, dtype=dtype, device=DEV)
    ve = torch.full((Np // 128,), 7.0, dtype=torch.float64, device=DEV)
    nonpos = torch.full((Np // 128,), 7, dtype=torch.int32, device=DEV)
    fn = lib.tsvgp_lik_map_robustmax_f64 if dtype == torch.float64 else lib.tsvgp_lik_map_robustmax_f32
    st = fn(m.data_ptr(), v.data_ptr(), yy.data_ptr(), flags, C, epsilon, g0.data_ptr(), g1.data_ptr(), ve.data_ptr(),
            nonpos.data_ptr(), N, Np, _stream())
    assert st == 0
    torch.cuda.synchronize()
    return g0.cpu().numpy().astype(np.float64), g1.cpu().numpy().astype(np.float64), ve.cpu().numpy(), nonpos.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(N, C, dt):
    """(inputs as the kernel reads them, the restatement's g0, g1 uncropped and ve per row): computed once per shape and type."""
    mean, var, y = map_inputs(N, C, seed=100 * C + N)
    if dt == "f32":  # fp32 inputs are rounded before the restatement sees them
        mean, var = (a.astype(np.float32).astype(np.float64) for a in (mean, var))
    ref = R.MultiClass(C)
    r0, r1 = ref.variational_expectations_grads(mean, var, y)
    out = (mean, var, y, r0, r1, ref.variational_expectations(mean, var, y))
    for a in out:
        a.setflags(write=False)
    return out


def _colerr(a, b):
    return max(relerr(a[:, p], b[:, p]) for p in range(a.shape[1]))


def _blocks(ve, Np):
    padded = np.zeros(Np)
    padded[:len(ve)] = ve
    return padded.reshape(-1, 128).sum(axis=1)


@pytest.mark.parametrize("C", [2, 3, 10, 32])
@pytest.mark.parametrize("N", [1, 127, 128, 129, 300])
def test_map_matches_restatement_entry_by_entry(N, C):
    B = pkg()._backend
    Np = B.round_up(N)
    for dt, dtype in DTYPES.items():
        mean, var, y, r0, r1, rve = _reference(N, C, dt)
        if N >= C:
            assert set(y[:, 0]) == set(range(C))
        for flags in (B.LIK_MULTICLASS, B.LIK_MULTICLASS | B.LIK_NOCROP):
            e1 = r1 if flags & B.LIK_NOCROP else np.minimum(r1, -1e-8)
            g0, g1, ve, nonpos = _map(mean, var, y, flags, dtype, C)
            again = _map(mean, var, y, flags, dtype, C)
            for a, b in zip((g0, g1, ve, nonpos), again):
                np.testing.assert_array_equal(a, b)  # no atomics, one summation order
            assert not g0[N:].any() and not g1[N:].any() and g0.shape == (Np, C)
            assert not nonpos.any()
            want_ve = _blocks(rve, Np)
            err_ve = float(np.max(np.abs(ve - want_ve) / np.abs(want_ve)))
            if dt == "f64":
                errs = (_colerr(g0[:N], r0), _colerr(g1[:N], e1))
                print(f"robustmax map f64 N={N} C={C} flags={flags:#x}: g0 {errs[0]:.2e} g1 {errs[1]:.2e} (bound 1e-8), ve {err_ve:.2e} (bound 1e-9)")
                assert errs[0] <= 1e-8 and errs[1] <= 1e-8
            else:
                print(f"robustmax map f32 N={N} C={C} flags={flags:#x}: g0 {np.abs(g0[:N] - r0).max():.2e} g1 {np.abs(g1[:N] - e1).max():.2e} "
                      f"absolute, ve {err_ve:.2e} (bound 1e-9: the sums are fp64 for either array type)")
                np.testing.assert_allclose(g0[:N], r0, rtol=1e-3, atol=1e-4)
                np.testing.assert_allclose(g1[:N], e1, rtol=1e-3, atol=1e-4)
            assert err_ve <= 1e-9


def test_bad_rows_are_nan_or_counted_and_leave_the_others_alone():
    B = pkg()._backend
    N, C = 130, 3
    mean, var, y = (a.copy() for a in map_inputs(N, C, seed=5))
    cm, cv, cy = clip_rows()
    mean[20:22], var[20:22], y[20:22] = cm, cv, cy  # the two clip rows of the CPU test
    var[10, 1] = 0.0  # counted in block 0; the clip keeps the row finite
    mean[129, 2] = np.nan  # counted in block 1; the row is NaN
    labels = {3: 1.5, 40: -1.0, 77: float(C)}  # NaN rows, not counted
    y_ref = y.copy()
    for n, v in labels.items():
        y[n, 0] = v
    ref = R.MultiClass(C)
    with np.errstate(invalid="ignore"):
        r0, r1 = ref.variational_expectations_grads(mean, var, y_ref)
    assert np.isnan(r0[129]).all() and np.isnan(r1[129]).all() and np.isfinite(r0[:129]).all() and np.isfinite(r1[:129]).all()
    assert r1[10, 1] == 0.0 and r1[20, 0] == 0.0 and r1[21, 1] == 0.0
    nan_rows = np.zeros(N, bool)
    nan_rows[list(labels) + [129]] = True
    for flags in (B.LIK_MULTICLASS, B.LIK_MULTICLASS | B.LIK_NOCROP):
        e1 = r1 if flags & B.LIK_NOCROP else np.minimum(r1, -1e-8)
        g0, g1, ve, nonpos = _map(mean, var, y, flags, torch.float64, C)
        np.testing.assert_array_equal(nonpos, [1, 1])
        assert np.isnan(g0[:N][nan_rows]).all() and np.isnan(g1[:N][nan_rows]).all() and np.isnan(ve).all()
        ok = ~nan_rows
        assert np.isfinite(g0[:N][ok]).all() and np.isfinite(g1[:N][ok]).all()
        assert _colerr(g0[:N][ok], r0[ok]) <= 1e-8 and _colerr(g1[:N][ok], e1[ok]) <= 1e-8
        # the clipped variances: derivative zero, -1e-8 under the crop
        clipped = 0.0 if flags & B.LIK_NOCROP else -1e-8
        assert g1[10, 1] == clipped and g1[20, 0] == clipped and g1[21, 1] == clipped
        assert not g0[N:].any() and not g1[N:].any()


def test_map_rejects_bad_arguments_on_device():
    B = pkg()._backend
    lib = B.lib()
    t = torch.ones(256, 3, dtype=torch.float64, device=DEV)
    yl = torch.zeros(256, 1, dtype=torch.float64, device=DEV)
    ve = torch.zeros(2, dtype=torch.float64, device=DEV)
    npos = torch.zeros(2, dtype=torch.int32, device=DEV)
    g = torch.zeros(256, 3, dtype=torch.float64, device=DEV)
    ins = (t.data_ptr(), t.data_ptr(), yl.data_ptr())
    outs = (g.data_ptr(), g.data_ptr(), ve.data_ptr(), npos.data_ptr())
    call = lambda ins=ins, flags=B.LIK_MULTICLASS, C=3, eps=1e-3, outs=outs: lib.tsvgp_lik_map_robustmax_f64(
        *ins, flags, C, eps, *outs, 200, 256, _stream())
    assert call(C=1) == 1 and call(C=33) == 1 and call(eps=0.0) == 1 and call(eps=1.0) == 1
    assert call(ins=(None,) + ins[1:]) == 1 and call(outs=outs[:3] + (None,)) == 1
    for flags in (B.LIK_SOFTMAX, B.LIK_HETERO, B.LIK_MULTICLASS | B.LIK_MEANONLY):
        assert call(flags=flags) == 1
    assert call() == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the model
N_, M_, C_ = 300, 16, 3


def _gpu_pair(Z, kind, projection="auto", **kw):
    hip, ora = pair(Z, C_, kind, projection=projection, **kw)
    if kind == "perlatent":
        hip._get_engine().batch_separate = False
    return hip, ora


def _compare_state(hip, ora, tol):
    assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < tol
    assert relerr(hip.lambda_2.cpu().numpy(), ora.lambda_2) < tol


@pytest.mark.parametrize("projection", ["direct", "whitened", "projected"])
@pytest.mark.parametrize("kind", ["shared", "separate", "perlatent"])
def test_natgrad_steps_match_oracle(kind, projection):
    X, Y, Z = problem(N=N_, M=M_)
    hip, ora = _gpu_pair(Z, kind, projection, num_data=N_)
    assert hip._routes(1e-9) == [projection] * C_
    for _ in range(5):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        _compare_state(hip, ora, 1e-8)
    if kind != "shared":
        assert hip._get_engine().last_batched == (kind == "separate" and projection != "projected")
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    assert abs(e_h - e_o) < 1e-9 * abs(e_o)
    assert float(hip.elbo((X, Y))) == e_h  # nothing is drawn: the same number again
    mu, var, g0, g1 = hip.moments_and_gradients((X, Y))
    mu_o, var_o = ora.predict_f(X)
    mu, var = mu.cpu().numpy(), var.cpu().numpy()
    assert relerr(mu, mu_o) < 1e-8 and relerr(var, var_o) < 1e-8
    r0, r1 = ora.likelihood.variational_expectations_grads(mu, var, Y)  # the map at the moments it was given
    assert _colerr(g0.cpu().numpy(), r0) <= 1e-8 and _colerr(g1.cpu().numpy(), np.minimum(r1, -1e-8)) <= 1e-8


@pytest.mark.parametrize("projection", ["direct", "whitened", "projected"])
def test_graph_replay_equals_eager_bit_for_bit(projection):
    X, Y, Z = problem(N=N_, M=M_, seed=1)
    Xd, Yd = torch.as_tensor(X, device=DEV), torch.as_tensor(Y, device=DEV)
    eager, ora = _gpu_pair(Z, "shared", projection)
    graph, _ = _gpu_pair(Z, "shared", projection, use_graph=True)
    for step in range(5):
        eager.natgrad_step((Xd, Yd), lr=0.5)
        graph.natgrad_step((Xd, Yd), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        print(f"robustmax graph vs eager step {step}: lambda_1 {relerr(graph.lambda_1.numpy(), eager.lambda_1.numpy()):.1e} "
              f"Lambda_2 {relerr(graph.lambda_2.cpu().numpy(), eager.lambda_2.cpu().numpy()):.1e}")
        np.testing.assert_array_equal(graph.lambda_1.numpy(), eager.lambda_1.numpy())
        np.testing.assert_array_equal(graph.lambda_2.cpu().numpy(), eager.lambda_2.cpu().numpy())
        _compare_state(graph, ora, 1e-8)
    assert len([e for e in graph._graphs.values() if isinstance(e, dict)]) == 1  # steps 3.. were replays of one capture
    assert float(graph.elbo((Xd, Yd))) == float(eager.elbo((Xd, Yd)))


@pytest.mark.parametrize("kind", ["shared", "separate", "perlatent"])
def test_fp32_against_fp64_oracle(kind):
    X, Y, Z = problem(N=N_, M=M_, seed=2)
    hip, ora = _gpu_pair(Z, kind, "whitened", compute_dtype=torch.float32)
    for _ in range(5):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
    mu_h, var_h = hip.predict_f(X)
    mu_o, var_o = ora.predict_f(X)
    np.testing.assert_allclose(mu_h.cpu().numpy(), mu_o, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(var_h.cpu().numpy(), var_o, rtol=1e-3, atol=1e-4)
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    print(f"robustmax fp32 {kind}: elbo {e_h:.6f} oracle {e_o:.6f}")
    assert abs(e_h - e_o) <= 1e-4 + 1e-3 * abs(e_o)


# Ten classes and more than one tile: M = 150 pads to Mp = 256 -- two diagonal tiles and an off-diagonal one in the site sums, which
# above eight latents run in syrk_kernel<T>; with separate kernels the latent-batched entries carry P = 10.
N10_, M10_, C10_, D10_ = 300, 150, 10, 7


def _ten_class_problem(kind, projection, **kw):
    """``problem`` at D = 7 and the pair of ``pair``: 150 inducing points spread over [-2, 2]^7 keep cond(K_uu + jitter I) <= 1e4 for
    every latent's kernel (NumPy on the CPU: 81 for the shared Matern-5/2, 35 .. 2.9e3 for the ten SE kernels of lengthscale
    1.2 .. 2.1; at D = 6 the last of them is at 1.5e4), which the 1e-8 bound of ``_compare_state`` assumes.  All ten classes occur."""
    from oracle import tsvgp_oracle as O

    X, Y, Z = problem(N=N10_, M=M10_, D=D10_, C=C10_, seed=0)
    assert set(Y[:, 0]) == set(range(C10_))
    hip, ora = pair(Z, C10_, kind, projection=projection, **kw)
    if kind == "perlatent":
        hip._get_engine().batch_separate = False
    kernels = [ora.kernel] if kind == "shared" else ora.kernel.kernels
    conds = [float(np.linalg.cond(k.K(Z, Z) + O.DEFAULT_JITTER * np.eye(M10_))) for k in kernels]
    print(f"robustmax C=10 {kind}: cond(K_uu + jitter I) per kernel " + " ".join(f"{c:.2e}" for c in conds))
    assert max(conds) <= 1e4
    return X, Y, hip, ora


@pytest.mark.parametrize("projection", ["direct", "whitened"])
@pytest.mark.parametrize("kind", ["shared", "separate", "perlatent"])
def test_ten_classes_on_two_tiles_match_oracle(kind, projection):
    X, Y, hip, ora = _ten_class_problem(kind, projection, num_data=N10_)
    assert hip._routes(1e-9) == [projection] * C10_
    assert pkg()._backend.round_up(M10_) == 256 and C10_ > 8
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        _compare_state(hip, ora, 1e-8)
    if kind != "shared":
        assert hip._get_engine().last_batched == (kind == "separate")
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    print(f"robustmax C=10 {kind} {projection}: elbo {e_h:.10f} oracle {e_o:.10f}")
    assert abs(e_h - e_o) < 1e-9 * abs(e_o)
    assert float(hip.elbo((X, Y))) == e_h  # nothing is drawn: the same number again


def test_ten_classes_on_two_tiles_fp32_against_fp64_oracle():
    X, Y, hip, ora = _ten_class_problem("separate", "whitened", compute_dtype=torch.float32)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
    mu_h, var_h = hip.predict_f(X)
    mu_o, var_o = ora.predict_f(X)
    np.testing.assert_allclose(mu_h.cpu().numpy(), mu_o, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(var_h.cpu().numpy(), var_o, rtol=1e-3, atol=1e-4)
    e_h, e_o = float(hip.elbo((X, Y))), float(ora.elbo((X, Y)))
    print(f"robustmax C=10 fp32 separate: elbo {e_h:.6f} oracle {e_o:.6f}")
    assert abs(e_h - e_o) <= 1e-4 + 1e-3 * abs(e_o)


def test_minibatch_step_with_num_data_rescaling():
    X, Y, Z = problem(N=N_, M=M_, seed=3)
    hip, ora = _gpu_pair(Z, "shared", num_data=N_)
    rng = np.random.RandomState(0)
    for _ in range(3):
        idx = rng.choice(N_, 100, replace=False)
        hip.natgrad_step((X[idx], Y[idx]), lr=0.3)
        ora.natgrad_step((X[idx], Y[idx]), lr=0.3)
        _compare_state(hip, ora, 1e-8)


@pytest.mark.parametrize("kind", ["shared", "separate"])
def test_predict_y_and_log_density_match_restatement(kind):
    X, Y, Z = problem(N=N_, M=M_, seed=3)
    hip, ora = _gpu_pair(Z, kind)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
    Xt, Yt = X[::6] + 0.01, Y[::6]
    assert len(Xt) == 50
    ps, pv = hip.predict_y(Xt)
    ps_o, pv_o = ora.predict_y(Xt)
    assert ps.shape == (50, C_) and pv.shape == (50, C_)
    assert relerr(ps.cpu().numpy(), ps_o) < 1e-8 and relerr(pv.cpu().numpy(), pv_o) < 1e-8
    lpd = hip.predict_log_density((Xt, Yt))
    assert lpd.shape == (50,)
    np.testing.assert_allclose(lpd.cpu().numpy(), ora.predict_log_density((Xt, Yt)), rtol=1e-8, atol=1e-9)


def _worker(rank, world, port, out, backend):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        p = pkg()
        X, Y, Z = problem(N=301, M=M_, seed=6)  # uneven shards
        m, _ = pair(Z, C_, "shared", num_data=len(X), device=DEV, projection="whitened")
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
    X, Y, Z = problem(N=301, M=M_, seed=6)
    _, ora = pair(Z, C_, "shared", num_data=len(X))
    for _ in range(3):
        ora.natgrad_step((X, Y), lr=0.5)
    assert relerr(got["l1"], ora.lambda_1) < 1e-8 and relerr(got["L2"], ora.lambda_2) < 1e-8
    assert abs(float(got["elbo"]) - ora.elbo((X, Y))) < 1e-9 * abs(ora.elbo((X, Y)))


# ---------------------------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("kind", ["shared", "separate"])
def test_elbo_and_grads_match_central_differences_of_the_models_own_elbo(kind):
    """The bound is deterministic, so the difference quotients are those of the model's own ``elbo`` at perturbed parameters --
    no frozen draw, no second implementation.  h = 1e-5 relative, agreement to 2e-6 relative (tests/test_gpu_mstep.py)."""
    X, Y, Z = problem(N=N_, M=M_, seed=4)
    hip, _ = _gpu_pair(Z, kind, num_data=N_)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.5)
    elbo, grads = hip.elbo_and_grads((X, Y))
    base = float(hip.elbo((X, Y)))
    assert abs(float(elbo) - base) <= 1e-9 * abs(base)

    def fd(par, idx=None, h=1e-5):
        """Central difference quotient of the ELBO in entry ``idx`` of a Parameter (all entries of a scalar one)."""
        theta = par.value.detach().clone()
        step = h * max(1.0, abs(float(theta.reshape(-1)[0] if idx is None else theta[idx])))
        vals = []
        for sign in (1.0, -1.0):
            moved = theta.clone()
            if idx is None:
                moved += sign * step
            else:
                moved[idx] += sign * step
            par.assign(moved)
            vals.append(float(hip.elbo((X, Y))))
        par.assign(theta)
        return (vals[0] - vals[1]) / (2 * step)

    kernels = list(hip.kernel.kernels) if kind != "shared" else [hip.kernel]
    scale = None
    for ki, kern in enumerate(kernels):
        pre = f"kernels.{ki}." if kind != "shared" else ""
        for name in ("variance", "lengthscales"):
            want = fd(getattr(kern, name))
            scale = max(abs(want), 1.0) if scale is None else scale
            got = float(grads[pre + name].sum())
            print(f"robustmax grads {kind} {pre + name}: hip {got:.10e} fd {want:.10e}")
            assert abs(got - want) < 2e-6 * max(abs(want), scale), (pre + name, got, want)
    gZ = grads["Z"].cpu().numpy()
    for idx in ((0, 0), (5, 1), (M_ - 1, 0)):
        want = fd(hip.inducing_variable.Z, idx)
        print(f"robustmax grads {kind} Z{idx}: hip {gZ[idx]:.10e} fd {want:.10e}")
        assert abs(gZ[idx] - want) < 2e-6 * max(abs(want), scale), (idx, gZ[idx], want)
    assert abs(float(hip.elbo((X, Y))) - base) <= 1e-12 * abs(base)  # every parameter is back where it was


def test_short_em_fit_does_not_lower_the_bound_and_classifies():
    """Two iterations of ``training.em_fit`` (one optimizer carried through, as one call with ``iterations=2`` does; split in two so
    that the bound behind each M-block can be printed).  What is asserted is what ``em_fit`` logs, as tests/test_gpu_tvgp_grad.py
    and tests/test_gpu_scalar_lik.py assert it: the bound after the E-steps of the second iteration is not below that of the first,
    the M-steps in between included, and the fit does not end below where it began.  A single M-block is NOT asserted to raise the
    bound: Adam moves every coordinate by about its learning rate whatever the size of the gradient, and its moments come from
    the previous block, whose sites were others -- near the optimum, where the gradient is small, a block may give a little back
    (seen on an MI355X: -222.146 -> -211.440 behind the first block, -25.721 -> -25.976 behind the second).  The direction of
    the M-step is pinned by the gradient test above, to 2e-6."""
    p = pkg()
    training = importlib.import_module("t-svgp_amd.training")
    X, Y, Z = blobs(N=450, seed=3, sep=2.0, sd=0.4)  # well separated: the class of a point is its cluster
    (X, Y), (Xt, Yt) = (X[:300], Y[:300]), (X[300:], Y[300:])
    model = p.t_SVGP(p.Matern52(1.0, 1.5), p.MultiClass(3), Z, num_latent_gps=3, num_data=len(X))
    opt = training.Adam(0.01)
    logged, after = [], None
    for it in range(2):
        logf, nlpd = training.em_fit(model, (X, Y), iterations=1, n_e_steps=4, n_m_steps=5, nat_lr=0.5, test_data=(Xt, Yt), optimizer=opt)
        after = float(model.elbo((X, Y)))
        print(f"robustmax em_fit {it}: elbo after the E-steps {logf[0]:.6f}, after the M-steps {after:.6f}, test NLPD {nlpd[0]:.4f}")
        assert len(logf) == 1 and np.isfinite(logf[0]) and np.isfinite(nlpd[0]) and np.isfinite(after)
        logged.append(logf[0])
    assert logged[1] >= logged[0] and after >= logged[0], (logged, after)
    pred = model.predict_y(Xt)[0].argmax(dim=1).cpu().numpy()
    majority = max(np.mean(Yt[:, 0] == c) for c in range(3))
    acc = float(np.mean(pred == Yt[:, 0]))
    print(f"robustmax em_fit: held-out accuracy {acc:.3f}, majority-class rate {majority:.3f}")
    assert acc > majority
