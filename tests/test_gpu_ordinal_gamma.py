"""The Ordinal, Gamma and Exponential likelihoods on the GPU: ``tsvgp_lik_map_ordinal_*`` and the Gamma arm of
``tsvgp_lik_map_scalar_*`` entry by entry through the C-ABI against the NumPy restatement (tests/ordinal_gamma_ref.py), then t_SVGP
and t_SVGP_white against the host-side step (the oracle driven by the restated likelihood): every projection route, the two-product
form, hipGraph replay, the M-step gradient with the likelihood's own parameter and a short E/M fit.

Bounds (the project's stated ones, tests/test_gpu_scalar_lik.py): fp64 max relative error <= 1e-8 on g0, g1, lambda_1, Lambda_2 and
the predictions; |d sum ve| / |sum ve| and the ELBO <= 1e-9; fp32 against the fp64 restatement atol 1e-4 + rtol 1e-3;
``elbo_and_grads`` against difference quotients at h = 1e-5, 2e-6 relative (tests/test_gpu_mstep.py).  The parameter sums
(d ve / d sigma, d ve / d shape) have terms of both signs, so their bound is 1e-9 of the sum of their magnitudes.
"""
import importlib

import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests.helpers import pkg, relerr
from tests.ordinal_gamma_ref import Exponential as RefExponential
from tests.ordinal_gamma_ref import Gamma as RefGamma
from tests.ordinal_gamma_ref import Ordinal as RefOrdinal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EDGES = {2: np.array([0.0]), 5: np.array([-1.5, -0.4, 0.3, 1.7]), 256: np.linspace(-6.0, 6.0, 255)}
# (kind, K or shape, sigma): Ordinal at K in {2, 5, 256} and sigma in {0.7, 3}; Gamma at three shapes, 1 being Exponential's arm
MAP_CASES = [("ordinal", K, s) for K in (2, 5, 256) for s in (0.7, 3.0)] + [("gamma", a, None) for a in (0.5, 1.0, 2.5)]


def _ref(kind, par, sigma):
    return RefOrdinal(EDGES[par], sigma) if kind == "ordinal" else RefGamma(par)


def _map_inputs(kind, par, N, seed):
    """mean in [-6, 6], var log-uniform in [1e-6, 4]; Ordinal: labels over all K bins with 0 and K - 1 there; Gamma: y log-uniform
    over 1e-3 .. 1e3 with both ends there."""
    rng = np.random.RandomState(seed)
    m = rng.uniform(-6.0, 6.0, N)
    v = np.exp(rng.uniform(np.log(1e-6), np.log(4.0), N))
    if kind == "ordinal":
        y = rng.randint(0, par, N).astype(np.float64)
        y[0] = par - 1.0
        if N > 2:
            y[N // 2] = 0.0
    else:
        y = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), N))
        y[0] = 1e3
        if N > 2:
            y[N // 2] = 1e-3
    return m, v, y


def _call(kind, par, sigma, m, v, y, N, P, col, dtype, nocrop, want_dparam=True, offset=0, rows=None):
    """One call on column ``col`` of [N, P] buffers whose other columns hold NaN (inputs) / a sentinel (outputs); ``offset`` and
    ``rows``: the call starts at that row of the buffers and passes that many."""
    B = pkg()._backend
    lib = B.lib()
    n = N - offset if rows is None else rows
    Np = B.round_up(n)
    t = lambda a: torch.as_tensor(a, dtype=dtype, device=DEV)

    def column(a):
        buf = torch.full((N, P), float("nan"), dtype=dtype, device=DEV)
        buf[:, col] = t(a)
        return buf

    mb, vb, yb = column(m), column(v), column(y)
    g0 = torch.full((Np, P), 7.0, dtype=dtype, device=DEV)
    g1 = torch.full((Np, P), 7.0, dtype=dtype, device=DEV)
    ve = torch.full((Np // 128,), 7.0, dtype=torch.float64, device=DEV)
    dpar = torch.full((Np // 128,), 7.0, dtype=torch.float64, device=DEV)
    bad = torch.full((Np // 128,), 7, dtype=torch.int32, device=DEV)
    sfx = "f64" if dtype == torch.float64 else "f32"
    off = col * mb.element_size()
    ioff = off + offset * P * mb.element_size()
    flag = B.LIK_NOCROP if nocrop else 0
    stream = torch.cuda.current_stream().cuda_stream
    dp = dpar.data_ptr() if want_dparam else None
    if kind == "ordinal":
        edges = torch.as_tensor(EDGES[par], dtype=torch.float64, device=DEV)
        st = getattr(lib, f"tsvgp_lik_map_ordinal_{sfx}")(
            mb.data_ptr() + ioff, vb.data_ptr() + ioff, yb.data_ptr() + ioff, P, B.LIK_ORDINAL | flag, edges.data_ptr(), len(EDGES[par]),
            sigma, g0.data_ptr() + off, g1.data_ptr() + off, P, ve.data_ptr(), dp, bad.data_ptr(), n, Np, stream)
    else:
        st = getattr(lib, f"tsvgp_lik_map_scalar_{sfx}")(
            mb.data_ptr() + ioff, vb.data_ptr() + ioff, yb.data_ptr() + ioff, P, B.LIK_GAMMA | flag, par, 0.0, g0.data_ptr() + off,
            g1.data_ptr() + off, P, ve.data_ptr(), dp, bad.data_ptr(), n, Np, stream)
    assert st == 0
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (g0, g1, ve, dpar, bad))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("N", [1, 127, 128, 129, 300])
def test_map_entry_by_entry(N, P, dtype):
    B = pkg()._backend
    Np = B.round_up(N)
    col = P - 1
    f64 = dtype == torch.float64
    cropped = 0
    for li, (kind, par, sigma) in enumerate(MAP_CASES):
        m, v, y = _map_inputs(kind, par, N, seed=10 * N + li)
        if not f64:
            m, v, y = (a.astype(np.float32).astype(np.float64) for a in (m, v, y))  # what the kernel reads
        ref = _ref(kind, par, sigma)
        r0, r1 = ref.variational_expectations_grads(m, v, y)
        rve = ref.variational_expectations(m, v, y)
        rdp = ref.variational_expectations_dsigma(m, v, y) if kind == "ordinal" else ref.variational_expectations_dshape(m, v, y)
        cropped += int((r1 > -1e-8).sum()) if kind == "ordinal" else 0
        for nocrop in (False, True):
            out = _call(kind, par, sigma, m, v, y, N, P, col, dtype, nocrop)
            again = _call(kind, par, sigma, m, v, y, N, P, col, dtype, nocrop)
            for a, b in zip(out, again):  # two calls: bit for bit (NaN-free, sentinels included)
                np.testing.assert_array_equal(a, b)
            g0, g1, ve, dpar, bad = out
            e1 = r1 if nocrop else np.minimum(r1, -1e-8)
            err0, err1 = relerr(g0[:N, col], r0), relerr(g1[:N, col], e1)
            errv = abs(ve.sum() - rve.sum()) / abs(rve.sum())
            errp = abs(dpar.sum() - rdp.sum()) / np.abs(rdp).sum()
            print(f"{kind} {par} sigma={sigma} N={N} P={P} {'f64' if f64 else 'f32'} nocrop={nocrop}: g0 {err0:.2e} g1 {err1:.2e} "
                  f"ve {errv:.2e} dparam {errp:.2e}")
            if f64:
                assert err0 <= 1e-8 and err1 <= 1e-8
                assert errv <= 1e-9
                blk = np.array([rve[b * 128:(b + 1) * 128].sum() for b in range(Np // 128)])
                np.testing.assert_allclose(ve, blk, rtol=1e-9, atol=1e-9 * np.abs(blk).max())
            else:
                np.testing.assert_allclose(g0[:N, col], r0, rtol=1e-3, atol=1e-4)
                np.testing.assert_allclose(g1[:N, col], e1, rtol=1e-3, atol=1e-4)
                np.testing.assert_allclose(ve.sum(), rve.sum(), rtol=1e-3, atol=1e-4)
            assert errp <= 1e-9
            if kind == "gamma":
                assert (g1[:N, col] < 0).all()  # -e / 2: log-concave, the crop never lifts a value
            assert not g0[N:Np, col].any() and not g1[N:Np, col].any()  # the padding rows come back zero
            if P == 2:  # the other column was neither read (NaN inputs) nor written (sentinel)
                assert (g0[:, 0] == 7.0).all() and (g1[:, 0] == 7.0).all()
            assert np.isfinite(g0[:, col]).all() and np.isfinite(g1[:, col]).all() and not bad.any()
    print(f"N={N}: {cropped} of {6 * N} ordinal rows have g1 > -1e-8")
    assert cropped > 0 or N == 1  # the crop has something to do


def test_map_without_the_optional_output():
    for kind, par, sigma in (("ordinal", 5, 0.7), ("gamma", 2.5, None)):
        m, v, y = _map_inputs(kind, par, 129, seed=3)
        full = _call(kind, par, sigma, m, v, y, 129, 1, 0, torch.float64, True)
        bare = _call(kind, par, sigma, m, v, y, 129, 1, 0, torch.float64, True, want_dparam=False)
        for i in (0, 1, 2, 4):
            np.testing.assert_array_equal(full[i], bare[i])
        assert (bare[3] == 7.0).all() and not (full[3] == 7.0).any()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind,par,sigma", [("ordinal", 256, 0.7), ("gamma", 2.5, None)])
def test_slice_call_reproduces_the_rows_bit_for_bit(kind, par, sigma, dtype):
    N, a, b = 300, 37, 210
    m, v, y = _map_inputs(kind, par, N, seed=8)
    full = _call(kind, par, sigma, m, v, y, N, 2, 1, dtype, False)
    part = _call(kind, par, sigma, m, v, y, N, 2, 1, dtype, False, offset=a, rows=b - a)
    for i in (0, 1):
        np.testing.assert_array_equal(part[i][:b - a, 1], full[i][a:b, 1])
        assert not part[i][b - a:, 1].any()


def test_map_counts_bad_rows_per_block():
    N = 400
    with np.errstate(invalid="ignore", divide="ignore"):
        m, v, y = _map_inputs("ordinal", 5, N, seed=5)
        v[5] = 0.0
        v[200] = -1.0
        m[201] = float("nan")
        m[399] = float("inf")
        y[130] = 1.5  # not an integer
        y[131] = 5.0  # == K
        y[300] = -1.0
        g0, g1, ve, _, bad = _call("ordinal", 5, 0.7, m, v, y, N, 1, 0, torch.float64, False)
        np.testing.assert_array_equal(bad, [1, 4, 1, 1])
        for r in (130, 131, 300):
            assert np.isnan(g0[r, 0]) and np.isnan(g1[r, 0])
        assert np.isnan(ve[1]) and np.isnan(ve[2]) and np.isfinite(ve[0])
        ok = np.ones(N, bool)
        ok[[5, 200, 201, 399, 130, 131, 300]] = False
        r0, _ = RefOrdinal(EDGES[5], 0.7).variational_expectations_grads(m[ok], v[ok], y[ok])
        assert relerr(g0[:N, 0][ok], r0) <= 1e-8  # a bad label's row does not disturb its neighbours

        m, v, y = _map_inputs("gamma", 2.5, N, seed=6)
        v[5] = 0.0
        m[201] = float("nan")
        y[130] = 0.0  # outside the support at shape != 1
        y[131] = -2.0
        y[399] = float("nan")
        _, _, ve, _, bad = _call("gamma", 2.5, None, m, v, y, N, 1, 0, torch.float64, False)
        np.testing.assert_array_equal(bad, [1, 3, 0, 1])
        assert np.isfinite(ve[2]) and np.isnan(ve[1]) and np.isnan(ve[3])

        m, v, y = _map_inputs("gamma", 1.0, N, seed=7)
        y[::9] = 0.0  # Exponential's arm: a waiting time of zero is a target
        y[131] = -2.0
        g0, g1, ve, _, bad = _call("gamma", 1.0, None, m, v, y, N, 1, 0, torch.float64, False, want_dparam=False)
        np.testing.assert_array_equal(bad, [0, 1, 0, 0])
        assert np.isfinite(ve[[0, 2, 3]]).all() and np.isnan(ve[1])
        ok = np.ones(N, bool)
        ok[131] = False
        ref = RefExponential()
        r0, r1 = ref.variational_expectations_grads(m, v, y)
        assert relerr(g0[:N, 0][ok], r0[ok]) <= 1e-8 and relerr(g1[:N, 0][ok], np.minimum(r1, -1e-8)[ok]) <= 1e-8
        blk0 = ref.variational_expectations(m, v, y)[:128].sum()
        assert abs(ve[0] - blk0) <= 1e-9 * abs(blk0)


def test_map_rejects_bad_arguments_on_device():
    B = pkg()._backend
    lib = B.lib()
    t = torch.ones(256, dtype=torch.float64, device=DEV)
    edges = torch.as_tensor(EDGES[5], device=DEV)
    ve = torch.zeros(2, dtype=torch.float64, device=DEV)
    npos = torch.zeros(2, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    a = t.data_ptr()
    call = lambda flags=B.LIK_ORDINAL, e=edges.data_ptr(), ne=4, sigma=1.0, N=200, Np=256: lib.tsvgp_lik_map_ordinal_f64(
        a, a, a, 1, flags, e, ne, sigma, a, a, 1, ve.data_ptr(), None, npos.data_ptr(), N, Np, s)
    assert call(flags=B.LIK_GAMMA) == 1 and call(flags=B.LIK_MULTICLASS) == 1 and call(e=None) == 1
    assert call(ne=0) == 1 and call(ne=256) == 1 and call(sigma=0.0) == 1 and call(N=300) == 1 and call(Np=200) == 1
    g0 = torch.empty(256, dtype=torch.float64, device=DEV)
    assert lib.tsvgp_lik_map_ordinal_f64(a, a, a, 1, B.LIK_ORDINAL, edges.data_ptr(), 4, 1.0, g0.data_ptr(), g0.data_ptr(), 1,
                                         ve.data_ptr(), None, npos.data_ptr(), 200, 256, s) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the models
N_, M_, D_ = 300, 16, 2
KINDS = ["ordinal", "gamma", "exponential"]
SIGMA, SHAPE = 0.7, 2.5
MODEL_EDGES = EDGES[5]


def problem(kind, P=1, seed=0):
    """N = 300, M = 16, D = 2: a smooth latent; ratings in 5 bins, Gamma(2.5) amounts or exponential waiting times (a few of
    them zero); Z spread over the inputs (cond(K_uu + 1e-9 I) ~ 1e3 for the kernel below)."""
    rng = np.random.RandomState(seed)
    X = rng.randn(N_, D_)
    F = np.sin(X @ rng.randn(D_, P)) + 0.3 * np.cos(2.0 * X[:, :1])
    if kind == "ordinal":
        Y = np.sum((2.0 * F + SIGMA * rng.randn(N_, P))[..., None] > MODEL_EDGES, axis=-1).astype(np.float64)
    elif kind == "gamma":
        Y = rng.gamma(SHAPE, np.exp(F))
    else:
        Y = rng.exponential(np.exp(F))
        Y[::29] = 0.0
    Z = rng.randn(M_, D_) * 1.3
    return X, Y, Z


def liks(kind, par=None):
    p = pkg()
    if kind == "ordinal":
        lh = p.Ordinal(MODEL_EDGES)
        lh.sigma.assign(SIGMA if par is None else par)
        return lh, RefOrdinal(MODEL_EDGES, SIGMA if par is None else par)
    if kind == "gamma":
        return p.Gamma(shape=SHAPE if par is None else par), RefGamma(SHAPE if par is None else par)
    return p.Exponential(), RefExponential()


def _state_close(hip, ora, tol=1e-8):
    assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < tol
    l2 = hip.lambda_2  # a tensor (t_SVGP) or the Parameter itself (t_SVGP_white)
    assert relerr(l2.cpu().numpy() if torch.is_tensor(l2) else l2.numpy(), ora.lambda_2) < tol


def _elbo_close(hip, ora, data):
    e_o = float(ora.elbo(data))
    assert abs(float(hip.elbo(data)) - e_o) < 1e-9 * abs(e_o)


@pytest.mark.parametrize("projection", ["direct", "whitened", "projected"])
@pytest.mark.parametrize("kind", KINDS)
def test_tsvgp_steps_match_host_side_step(kind, projection):
    p = pkg()
    X, Y, Z = problem(kind)
    lh, lo = liks(kind)
    hip = p.t_SVGP(p.SquaredExponential(1.1, 1.0), lh, Z, num_data=N_, projection=projection, use_graph=False)
    ora = O.t_SVGP(O.SquaredExponential(1.1, 1.0), lo, Z, num_data=N_)
    assert hip._routes(1e-9) == [projection]
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        _state_close(hip, ora)
    _elbo_close(hip, ora, (X, Y))
    mu, var, g0, g1 = hip.moments_and_gradients((X, Y))
    mu_o, var_o = ora.predict_f(X)
    r0, r1 = lo.variational_expectations_grads(mu_o, var_o, Y)
    assert relerr(g0.cpu().numpy(), r0) < 1e-8 and relerr(g1.cpu().numpy(), np.minimum(r1, -1e-8)) < 1e-8
    Xs = X[:50] + 0.05
    for a, b in zip(hip.predict_y(Xs), ora.predict_y(Xs)):
        assert relerr(a.cpu().numpy(), b) < 1e-8
    assert relerr(hip.predict_log_density((Xs, Y[:50])).cpu().numpy(), ora.predict_log_density((Xs, Y[:50]))) < 1e-8


@pytest.mark.parametrize("kind", KINDS)
def test_tsvgp_graph_replay_matches_host_side_step(kind):
    p = pkg()
    X, Y, Z = problem(kind, seed=1)
    lh, lo = liks(kind)
    hip = p.t_SVGP(p.SquaredExponential(1.1, 1.0), lh, Z, use_graph=True)
    eager = p.t_SVGP(p.SquaredExponential(1.1, 1.0), liks(kind)[0], Z, use_graph=False)
    ora = O.t_SVGP(O.SquaredExponential(1.1, 1.0), lo, Z)
    Xd, Yd = torch.as_tensor(X, device=DEV), torch.as_tensor(Y, device=DEV)
    for _ in range(4):  # eager, capture, replay, replay
        hip.natgrad_step((Xd, Yd), lr=0.5)
        eager.natgrad_step((Xd, Yd), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        _state_close(hip, ora)
        np.testing.assert_array_equal(hip.lambda_1.numpy(), eager.lambda_1.numpy())  # the replayed step IS the eager one
    assert any(isinstance(v, dict) for v in hip._graphs.values()), "the step was not captured"


@pytest.mark.parametrize("batched", [True, False])
def test_tsvgp_separate_kernels_two_ordinal_columns(batched):
    p = pkg()
    X, Y, Z = problem("ordinal", P=2, seed=2)
    lh, lo = liks("ordinal")
    ks = [(1.0, 0.8), (0.6, 1.2)]
    hip = p.t_SVGP(p.SeparateIndependent([p.SquaredExponential(v, l) for v, l in ks]), lh, p.SharedIndependentInducingVariables(Z),
                   num_latent_gps=2, use_graph=False)
    ora = O.t_SVGP(O.SeparateIndependent([O.SquaredExponential(v, l) for v, l in ks]), lo, O.SharedIndependentInducingVariables(Z),
                   num_latent_gps=2)
    hip._get_engine().batch_separate = batched
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        _state_close(hip, ora)
    _elbo_close(hip, ora, (X, Y))
    assert hip._get_engine().last_batched == batched


def test_tsvgp_fp32_compute_dtype():
    """The fp32 entries behind the model: one step of an fp32 model lands on the fp64 host-side step to fp32's stated bound."""
    p = pkg()
    for kind in KINDS:
        X, Y, Z = problem(kind, seed=7)
        lh, lo = liks(kind)
        hip = p.t_SVGP(p.SquaredExponential(1.1, 1.0), lh, Z, num_data=N_, compute_dtype=torch.float32, use_graph=False)
        ora = O.t_SVGP(O.SquaredExponential(1.1, 1.0), lo, Z, num_data=N_)
        hip.natgrad_step((X, Y), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        scale = np.abs(ora.lambda_1).max()
        np.testing.assert_allclose(hip.lambda_1.numpy(), ora.lambda_1, rtol=1e-3, atol=1e-4 * scale)
        e_o = float(ora.elbo((X, Y)))
        np.testing.assert_allclose(float(hip.elbo((X, Y))), e_o, rtol=1e-3)


@pytest.mark.parametrize("projection", ["direct", "whitened"])
@pytest.mark.parametrize("kind", KINDS)
def test_white_steps_match_host_side_step(kind, projection):
    p = pkg()
    X, Y, Z = problem(kind, seed=3)
    lh, lo = liks(kind)
    hip = p.t_SVGP_white(p.SquaredExponential(1.1, 1.0), lh, Z, num_data=N_, projection=projection)
    ora = O.t_SVGP_white(O.SquaredExponential(1.1, 1.0), lo, Z, num_data=N_)
    assert hip._use_direct() == (projection == "direct")
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.3)
        ora.natgrad_step((X, Y), lr=0.3)
        _state_close(hip, ora)
    _elbo_close(hip, ora, (X, Y))
    # (the host-side t_SVGP_white has no predict_y: the restated likelihood on its predict_f)
    for a, b in zip(hip.predict_y(X[:40]), lo.predict_mean_and_var(*ora.predict_f(X[:40]))):
        assert relerr(a.cpu().numpy(), b) < 1e-8


@pytest.mark.parametrize("kind", KINDS)
def test_white_two_product_form(kind):
    """Lambda_2 + 1e-9 I without a Cholesky factor: the model moves to the reference's two-product variance, whose likelihood map
    is the stand-alone call behind the assembled moments (``EStepEngine.run_two_product``)."""
    p = pkg()
    rng = np.random.RandomState(32)
    # (Ordinal: a mean far from the ratings puts rows where log p is not concave, t_SVGP_white does not crop g1, and the
    # host-side step itself then loses K + Lambda_2 > 0 in its first step from 0.3 randn; from 0.05 randn it keeps it and stays in
    # the two-product form -- Lambda_2 indefinite -- for all three steps.  The ratings move Lambda_2 less than the amounts do, so
    # K + Lambda_2 keeps about 40 times the condition number of K_uu: the Z of seed 20, cond(K_uu) = 5e2, leaves it at 2e4, where
    # 1000 cond eps is under the 1e-8 asked of the state; seed 4's Z, cond(K_uu) = 5e4, does not)
    X, Y, Z = problem(kind, seed=20 if kind == "ordinal" else 4)
    Kuu = O.SquaredExponential(1.1, 1.0).K(Z)
    lam2, lam1 = (-0.45 * Kuu)[None], (0.05 if kind == "ordinal" else 0.3) * rng.randn(M_, 1)
    lh, lo = liks(kind)
    mk = lambda mod, lik: mod.t_SVGP_white(mod.SquaredExponential(1.1, 1.0), lik, Z, num_data=N_, lambda_1=lam1.copy(),
                                           lambda_2=lam2.copy())
    hip, ora = mk(p, lh), mk(O, lo)
    _elbo_close(hip, ora, (X, Y))
    assert hip._two_product
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.3)
        ora.natgrad_step((X, Y), lr=0.3)
        _state_close(hip, ora)
    _elbo_close(hip, ora, (X, Y))


@pytest.mark.parametrize("kind", KINDS)
def test_elbo_and_grads_match_difference_quotients(kind):
    p = pkg()
    X, Y, Z = problem(kind, seed=5)
    k0 = (1.3, np.array([0.9, 1.2]))
    par0 = {"ordinal": 0.9, "gamma": 1.8, "exponential": None}[kind]
    name = {"ordinal": "likelihood_sigma", "gamma": "likelihood_shape", "exponential": None}[kind]

    def models(par=par0, k=k0, Z=Z, state=None):
        kw = {} if state is None else dict(lambda_1=state[0], lambda_2_sqrt=state[1])
        lh, lo = liks(kind, par)
        return (lambda: p.t_SVGP(p.SquaredExponential(*k), lh, Z, num_data=N_, use_graph=False)), \
            O.t_SVGP(O.SquaredExponential(*k), lo, Z, num_data=N_, **kw)

    mk_hip, ora = models()
    hip = mk_hip()
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.7)
        ora.natgrad_step((X, Y), lr=0.7)
    state = (ora.lambda_1.copy(), ora.lambda_2_sqrt.copy())
    elbo, grads = hip.elbo_and_grads((X, Y))
    f = lambda **kw: float(models(state=state, **kw)[1].elbo((X, Y)))
    assert abs(float(elbo) - f()) < 1e-9 * abs(f())
    h = 1e-5

    def fd(make, base):
        step = h * max(1.0, abs(base))
        return (f(**make(base + step)) - f(**make(base - step))) / (2 * step)

    scale = max(abs(fd(lambda x: dict(k=(x, k0[1])), k0[0])), 1.0)
    ref = fd(lambda x: dict(k=(x, k0[1])), k0[0])
    assert abs(float(grads["variance"]) - ref) < 2e-6 * max(abs(ref), scale), ref
    g_ls = grads["lengthscales"].cpu().numpy()
    for d in range(D_):
        def bump(x, d=d):
            ls = k0[1].copy()
            ls[d] = x
            return dict(k=(k0[0], ls))
        ref = fd(bump, float(k0[1][d]))
        assert abs(g_ls[d] - ref) < 2e-6 * max(abs(ref), scale), (d, g_ls[d], ref)
    g_Z = grads["Z"].cpu().numpy()
    for (m_, d) in [(0, 0), (5, 1), (M_ - 1, 0)]:
        def bump(x, m_=m_, d=d):
            Zn = Z.copy()
            Zn[m_, d] = x
            return dict(Z=Zn)
        ref = fd(bump, float(Z[m_, d]))
        assert abs(g_Z[m_, d] - ref) < 2e-6 * max(abs(ref), scale), (m_, d, g_Z[m_, d], ref)
    if name is not None:
        ref = fd(lambda x: dict(par=x), par0)
        print(f"{name}: {float(grads[name]):.10e} against {ref:.10e}")
        assert abs(float(grads[name]) - ref) < 2e-6 * max(abs(ref), scale), ref
    assert {"likelihood_sigma", "likelihood_shape", "likelihood_scale", "likelihood_variance"} & set(grads) == ({name} if name else set())


@pytest.mark.parametrize("kind,start", [("ordinal", 2.0), ("gamma", 1.0)])
def test_em_fit_trains_the_parameter(kind, start):
    p = pkg()
    training = importlib.import_module("t-svgp_amd.training")
    X, Y, Z = problem(kind, seed=6)
    lik = liks(kind, start)[0]
    par = lik.sigma if kind == "ordinal" else lik.shape
    model = p.t_SVGP(p.SquaredExponential(1.0, 1.0), lik, Z, num_data=N_, use_graph=False)
    logf, _ = training.em_fit(model, (X, Y), iterations=2, n_e_steps=4, n_m_steps=5, nat_lr=0.5, adam_lr=0.05)
    assert len(logf) == 2 and logf[0] < logf[1], logf
    assert abs(par.item() - start) > 0.05 and par.item() > 0.0
