"""The StudentT and Poisson likelihoods on the GPU: ``tsvgp_lik_map_scalar_*`` entry by entry through the C-ABI against the NumPy
restatement (tests/scalar_lik_ref.py), then t_SVGP and t_SVGP_white against the host-side step (the oracle driven by the restated
likelihood): every projection route, the two-product form, hipGraph replay, separate kernels, the M-step gradient and a short
E/M fit.

Bounds (the project's stated ones): fp64 max relative error <= 1e-8 on g0, g1, lambda_1, Lambda_2; |d sum ve| / |sum ve| and the
ELBO <= 1e-9; fp32 against the fp64 restatement atol 1e-4 + rtol 1e-3; ``elbo_and_grads`` against difference quotients at
h = 1e-5, 2e-6 relative (tests/test_gpu_mstep.py).  sum d ve / d scale has terms of both signs, so its bound is 1e-9 of the sum of
their magnitudes.
"""
import importlib

import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests.helpers import pkg, relerr
from tests.scalar_lik_ref import Poisson as RefPoisson
from tests.scalar_lik_ref import StudentT as RefStudentT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LIKS = [("student", 2.5), ("student", 3.0), ("student", 30.0), ("poisson", None)]
SCALE, BINSIZE = 0.7, 0.5


def _ref(kind, df):
    return RefStudentT(SCALE, df) if kind == "student" else RefPoisson(BINSIZE)


def _map_inputs(kind, N, seed):
    """mean, var, y [N]: StudentT residuals up to 1e3 scale; Poisson counts in {0, 1, 7, 1000}, m in [-5, 5], v in [1e-6, 4]."""
    rng = np.random.RandomState(seed)
    if kind == "student":
        m = rng.randn(N)
        v = rng.uniform(0.01, 3.0, N)
        r = rng.standard_t(3.0, N)
        r[rng.rand(N) < 0.3] *= 100.0
        r = np.clip(r, -1e3, 1e3)
        r[0] = 1e3  # the largest residual is always there, N = 1 included
        if N > 2:
            r[N // 2] = -1e3
        return m, v, m + SCALE * r
    m = rng.uniform(-5.0, 5.0, N)
    v = np.exp(rng.uniform(np.log(1e-6), np.log(4.0), N))
    y = rng.choice([0.0, 1.0, 7.0, 1000.0], N)
    m[0], v[0], y[0] = 5.0, 4.0, 1000.0
    return m, v, y


def _call(kind, df, m, v, y, N, P, col, dtype, nocrop, want_dparam=True):
    """One call on column ``col`` of [N, P] buffers whose other columns hold NaN (inputs) / a sentinel (outputs)."""
    B = pkg()._backend
    lib = B.lib()
    Np = B.round_up(N)
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
    student = kind == "student"
    lik = (B.LIK_STUDENT_T if student else B.LIK_POISSON) | (B.LIK_NOCROP if nocrop else 0)
    p0, p1 = (SCALE, df) if student else (BINSIZE, 0.0)
    fn = lib.tsvgp_lik_map_scalar_f64 if dtype == torch.float64 else lib.tsvgp_lik_map_scalar_f32
    off = col * mb.element_size()
    st = fn(mb.data_ptr() + off, vb.data_ptr() + off, yb.data_ptr() + off, P, lik, p0, p1, g0.data_ptr() + off, g1.data_ptr() + off,
            P, ve.data_ptr(), dpar.data_ptr() if (student and want_dparam) else None, bad.data_ptr(), N, Np,
            torch.cuda.current_stream().cuda_stream)
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
    for li, (kind, df) in enumerate(LIKS):
        m, v, y = _map_inputs(kind, N, seed=10 * N + li)
        if not f64:
            m, v, y = (a.astype(np.float32).astype(np.float64) for a in (m, v, y))  # what the kernel reads
        ref = _ref(kind, df)
        r0, r1 = ref.variational_expectations_grads(m, v, y)
        rve = ref.variational_expectations(m, v, y)
        rds = ref.variational_expectations_dscale(m, v, y) if kind == "student" else None
        for nocrop in (False, True):
            out = _call(kind, df, m, v, y, N, P, col, dtype, nocrop)
            again = _call(kind, df, m, v, y, N, P, col, dtype, nocrop)
            for a, b in zip(out, again):  # two calls: bit for bit (NaN-free, sentinels included)
                np.testing.assert_array_equal(a, b)
            g0, g1, ve, dpar, bad = out
            e1 = r1 if nocrop else np.minimum(r1, -1e-8)
            err0, err1 = relerr(g0[:N, col], r0), relerr(g1[:N, col], e1)
            errv = abs(ve.sum() - rve.sum()) / abs(rve.sum())
            print(f"{kind} df={df} N={N} P={P} {'f64' if f64 else 'f32'} nocrop={nocrop}: g0 {err0:.2e} g1 {err1:.2e} ve {errv:.2e}")
            if f64:
                assert err0 <= 1e-8 and err1 <= 1e-8
                assert errv <= 1e-9
                blk = np.array([rve[b * 128:(b + 1) * 128].sum() for b in range(Np // 128)])
                np.testing.assert_allclose(ve, blk, rtol=1e-9, atol=1e-9 * np.abs(blk).max())
            else:
                np.testing.assert_allclose(g0[:N, col], r0, rtol=1e-3, atol=1e-4)
                np.testing.assert_allclose(g1[:N, col], e1, rtol=1e-3, atol=1e-4)
                np.testing.assert_allclose(ve.sum(), rve.sum(), rtol=1e-3, atol=1e-4)
            if kind == "student":
                assert abs(dpar.sum() - rds.sum()) <= 1e-9 * np.abs(rds).sum()
                if nocrop:
                    assert (g1[:N, col] > 0).any() or N == 1  # not log-concave: the crop has something to do
            else:
                assert (dpar == 7.0).all()  # no parameter gradient for Poisson: never written
            assert not g0[N:Np, col].any() and not g1[N:Np, col].any()  # the padding rows come back zero
            if P == 2:  # the other column was neither read (NaN inputs) nor written (sentinel)
                assert (g0[:, 0] == 7.0).all() and (g1[:, 0] == 7.0).all()
            assert np.isfinite(g0[:, col]).all() and np.isfinite(g1[:, col]).all() and not bad.any()


def test_map_without_the_optional_output():
    m, v, y = _map_inputs("student", 129, seed=3)
    full = _call("student", 3.0, m, v, y, 129, 1, 0, torch.float64, True)
    bare = _call("student", 3.0, m, v, y, 129, 1, 0, torch.float64, True, want_dparam=False)
    for i in (0, 1, 2, 4):
        np.testing.assert_array_equal(full[i], bare[i])
    assert (bare[3] == 7.0).all()


@pytest.mark.parametrize("kind,df", [("student", 3.0), ("poisson", None)])
def test_map_counts_bad_rows_per_block(kind, df):
    N = 400
    m, v, y = _map_inputs(kind, N, seed=5)
    v[5] = 0.0
    v[200] = -1.0
    m[201] = float("nan")
    m[399] = float("inf")
    v[398] = -2.0
    with np.errstate(invalid="ignore"):
        _, _, _, _, bad = _call(kind, df, m, v, y, N, 1, 0, torch.float64, False)
    np.testing.assert_array_equal(bad, [1, 2, 0, 2])


def test_map_rejects_bad_arguments_on_device():
    B = pkg()._backend
    lib = B.lib()
    t = torch.ones(256, dtype=torch.float64, device=DEV)
    ve = torch.zeros(2, dtype=torch.float64, device=DEV)
    npos = torch.zeros(2, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    a = t.data_ptr()
    call = lambda lik, p0, p1, dp=None, N=200, Np=256: lib.tsvgp_lik_map_scalar_f64(a, a, a, 1, lik, p0, p1, a, a, 1, ve.data_ptr(), dp,
                                                                                    npos.data_ptr(), N, Np, s)
    assert call(B.LIK_GAUSSIAN, 1.0, 3.0) == 1 and call(B.LIK_HETERO, 1.0, 3.0) == 1
    assert call(B.LIK_STUDENT_T, 0.0, 3.0) == 1 and call(B.LIK_STUDENT_T, 1.0, 0.0) == 1
    assert call(B.LIK_POISSON, 1.0, 0.0, dp=ve.data_ptr()) == 1
    assert call(B.LIK_STUDENT_T, 1.0, 3.0, N=300) == 1 and call(B.LIK_STUDENT_T, 1.0, 3.0, Np=200) == 1
    g0 = torch.empty(256, dtype=torch.float64, device=DEV)
    assert lib.tsvgp_lik_map_scalar_f64(a, a, a, 1, B.LIK_POISSON, 1.0, 0.0, g0.data_ptr(), g0.data_ptr(), 1, ve.data_ptr(), None,
                                        npos.data_ptr(), 200, 256, s) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the models
N_, M_, D_ = 300, 16, 2


def problem(kind, P=1, seed=0):
    """N = 300, M = 16, D = 2: a smooth latent, Student-t noise with gross outliers or Poisson counts; Z spread over the inputs
    (cond(K_uu + 1e-9 I) ~ 1e3 for the kernel below: the oracle's own rounding stays well under the 1e-8 bound)."""
    rng = np.random.RandomState(seed)
    X = rng.randn(N_, D_)
    F = np.sin(X @ rng.randn(D_, P)) + 0.3 * np.cos(2.0 * X[:, :1])
    if kind == "student":
        Y = F + 0.3 * rng.standard_t(3.0, (N_, P))
        Y[::23] += 25.0  # gross outliers
    else:
        Y = rng.poisson(np.exp(1.0 + F) * BINSIZE).astype(np.float64)
    Z = rng.randn(M_, D_) * 1.3
    return X, Y, Z


def liks(kind, df=3.0):
    p = pkg()
    return (p.StudentT(SCALE, df), RefStudentT(SCALE, df)) if kind == "student" else (p.Poisson(BINSIZE), RefPoisson(BINSIZE))


def _state_close(hip, ora, tol=1e-8):
    assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < tol
    l2 = hip.lambda_2  # a tensor (t_SVGP) or the Parameter itself (t_SVGP_white)
    assert relerr(l2.cpu().numpy() if torch.is_tensor(l2) else l2.numpy(), ora.lambda_2) < tol


def _elbo_close(hip, ora, data):
    e_o = float(ora.elbo(data))
    assert abs(float(hip.elbo(data)) - e_o) < 1e-9 * abs(e_o)


@pytest.mark.parametrize("projection", ["direct", "whitened", "projected"])
@pytest.mark.parametrize("kind", ["student", "poisson"])
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
    if kind == "student":
        assert (r1 > -1e-8).any()  # the crop of the site update is exercised
    Xs = X[:50] + 0.05
    for a, b in zip(hip.predict_y(Xs), ora.predict_y(Xs)):
        assert relerr(a.cpu().numpy(), b) < 1e-8
    assert relerr(hip.predict_log_density((Xs, Y[:50])).cpu().numpy(), ora.predict_log_density((Xs, Y[:50]))) < 1e-8


@pytest.mark.parametrize("kind", ["student", "poisson"])
def test_tsvgp_graph_replay_matches_host_side_step(kind):
    p = pkg()
    X, Y, Z = problem(kind, seed=1)
    lh, lo = liks(kind)
    hip = p.t_SVGP(p.SquaredExponential(1.1, 1.0), lh, Z, use_graph=True)
    ora = O.t_SVGP(O.SquaredExponential(1.1, 1.0), lo, Z)
    Xd, Yd = torch.as_tensor(X, device=DEV), torch.as_tensor(Y, device=DEV)
    for _ in range(4):  # eager, capture, replay, replay
        hip.natgrad_step((Xd, Yd), lr=0.5)
        ora.natgrad_step((X, Y), lr=0.5)
        _state_close(hip, ora)
    assert any(isinstance(v, dict) for v in hip._graphs.values()), "the step was not captured"


@pytest.mark.parametrize("batched", [True, False])
def test_tsvgp_separate_kernels_two_columns(batched):
    p = pkg()
    X, Y, Z = problem("student", P=2, seed=2)
    lh, lo = liks("student")
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


@pytest.mark.parametrize("projection", ["direct", "whitened"])
@pytest.mark.parametrize("kind", ["student", "poisson"])
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
    want = ora.compute_data_natural_params((X, Y))
    got = hip.compute_data_natural_params((X, Y))
    K = O.Kuu(ora.inducing_variable, ora.kernel)
    tol = max(1e-8, 1000 * np.linalg.cond(K + 1e-9 * np.eye(M_)) * 2.2e-16)  # explicit K9^-1 products on both sides (tests/test_gpu_white.py)
    assert relerr(got[0].cpu().numpy(), want[0]) < tol and relerr(got[1].cpu().numpy(), want[1]) < tol
    # (the host-side t_SVGP_white has no predict_y: the restated likelihood on its predict_f)
    for a, b in zip(hip.predict_y(X[:40]), lo.predict_mean_and_var(*ora.predict_f(X[:40]))):
        assert relerr(a.cpu().numpy(), b) < 1e-8


@pytest.mark.parametrize("kind", ["student", "poisson"])
def test_white_two_product_form(kind):
    """Lambda_2 + 1e-9 I without a Cholesky factor: the model moves to the reference's two-product variance, whose likelihood map
    is the stand-alone call behind the assembled moments (``EStepEngine.run_two_product``)."""
    p = pkg()
    rng = np.random.RandomState(32)
    X, Y, Z = problem(kind, seed=4)
    Kuu = O.SquaredExponential(1.1, 1.0).K(Z)
    lam2, lam1 = (-0.45 * Kuu)[None], 0.3 * rng.randn(M_, 1)
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


@pytest.mark.parametrize("kind,sep", [("student", False), ("poisson", False), ("student", True)])
def test_elbo_and_grads_match_difference_quotients(kind, sep):
    p = pkg()
    P = 2 if sep else 1
    X, Y, Z = problem(kind, P=P, seed=5)
    ls0, var0 = np.array([0.9, 1.2]), 1.3
    ks = [(var0, ls0), (0.8, np.array([1.1, 0.7]))][:P]
    df = 4.0

    def models(scale=SCALE, ks=ks, Z=Z, state=None):
        kw = {} if state is None else dict(lambda_1=state[0], lambda_2_sqrt=state[1])
        if kind == "student":
            lh, lo = p.StudentT(scale, df), RefStudentT(scale, df)
        else:
            lh, lo = liks(kind)
        if sep:
            kh = p.SeparateIndependent([p.SquaredExponential(v, l) for v, l in ks])
            ko = O.SeparateIndependent([O.SquaredExponential(v, l) for v, l in ks])
            ih, io = p.SharedIndependentInducingVariables(Z), O.SharedIndependentInducingVariables(Z)
        else:
            kh, ko, ih, io = p.SquaredExponential(*ks[0]), O.SquaredExponential(*ks[0]), Z, Z
        return (lambda: p.t_SVGP(kh, lh, ih, num_latent_gps=P, num_data=N_, use_graph=False)), \
            O.t_SVGP(ko, lo, io, num_latent_gps=P, num_data=N_, **kw)

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

    def with_k(k, var=None, ls=None):
        new = list(ks)
        new[k] = (new[k][0] if var is None else var, new[k][1] if ls is None else ls)
        return dict(ks=new)

    scale = max(abs(fd(lambda x: with_k(0, var=x), ks[0][0])), 1.0)
    for k in range(P):
        pre = f"kernels.{k}." if sep else ""
        ref = fd(lambda x: with_k(k, var=x), ks[k][0])
        assert abs(float(grads[pre + "variance"]) - ref) < 2e-6 * max(abs(ref), scale), (k, ref)
        g_ls = grads[pre + "lengthscales"].cpu().numpy()
        for d in range(D_):
            def bump(x, d=d, k=k):
                ls = ks[k][1].copy()
                ls[d] = x
                return with_k(k, ls=ls)
            ref = fd(bump, float(ks[k][1][d]))
            assert abs(g_ls[d] - ref) < 2e-6 * max(abs(ref), scale), (k, d, g_ls[d], ref)
    g_Z = grads["Z"].cpu().numpy()
    for (m_, d) in [(0, 0), (5, 1), (M_ - 1, 0)]:
        def bump(x, m_=m_, d=d):
            Zn = Z.copy()
            Zn[m_, d] = x
            return dict(Z=Zn)
        ref = fd(bump, float(Z[m_, d]))
        assert abs(g_Z[m_, d] - ref) < 2e-6 * max(abs(ref), scale), (m_, d, g_Z[m_, d], ref)
    if kind == "student":
        ref = fd(lambda x: dict(scale=x), SCALE)
        assert abs(float(grads["likelihood_scale"]) - ref) < 2e-6 * max(abs(ref), scale), ref
    else:
        assert "likelihood_scale" not in grads
    assert "likelihood_variance" not in grads


def test_em_fit_trains_the_scale():
    p = pkg()
    training = importlib.import_module("t-svgp_amd.training")
    X, Y, Z = problem("student", seed=6)
    lik = p.StudentT(scale=1.5, df=4.0)
    model = p.t_SVGP(p.SquaredExponential(1.0, 1.0), lik, Z, num_data=N_, use_graph=False)
    logf, _ = training.em_fit(model, (X, Y), iterations=3, n_e_steps=4, n_m_steps=5, nat_lr=0.5, adam_lr=0.05)
    assert len(logf) == 3 and logf[0] < logf[1] < logf[2], logf
    assert abs(lik.scale.item() - 1.5) > 0.05 and lik.scale.item() > 0.0
