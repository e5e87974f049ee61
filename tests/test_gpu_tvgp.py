"""t_VGP on the GPU: the two entry points entry by entry against NumPy, the model against the restatement of the reference
(tests/tvgp_ref.py), and the reference's own pins (reference tests/models/test_tvgp.py) through the HIP path.

Shapes: N = 8 (a lone partial tile), 128 (an exact tile), 129 (a second tile with one live row), 300 (three block steps: the
right-hand sides ride two trailing updates); D = 1, 3, 8; SE and Matern52; once with lds > Np.

Bounds.  Kernel values: relative 1e-10 of the largest entry, what test_gpu_kernels.py holds tsvgp_kernel_fill_f64 to.  Row sums
and the likelihood map: test_gpu_kernels.py::test_moments_and_likelihood_map's (2e-10 on the moments, 1e-10 rtol + atol on g0,
g1 and what is linear in them; a partial sum of n such terms n times that).  The solved rows: fp64 rounding times cond(B) times
the row length, B = I + s s^T * K~ with eigenvalues in [1, 1 + N max(s^2) variance] -- below 1e3 here -- so 1e-16 * 1e3 * 300 =
3e-11, held to 1e-10.  Model: the fp64 tolerances of SURVEY.md section 8(d), 1e-8 on sites and predictions, 1e-9 on the ELBO;
tests/test_tvgp_cpu.py shows the problems are conditioned an order of magnitude inside them.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests import tvgp_ref as R
from tests.helpers import pkg, relerr
from tests.test_tvgp_cpu import MODEL_CASES, reference_setup

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = {"SquaredExponential": 0, "Matern52": 3}


@pytest.fixture(scope="module")
def eng():
    from importlib import import_module

    return import_module("t-svgp_amd.estep").EStepEngine(torch.float64, DEV)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def _system_inputs(N, D, kernel):
    rng = np.random.RandomState(11 * N + D)
    X = rng.randn(N, D)
    ls = 0.7 + rng.rand(D)
    l1 = rng.randn(N)
    l2 = 0.1 + rng.rand(N)
    l2[N // 2] *= -1.0  # s = sqrt|lambda_2|, y~ keeps the sign
    Np = pkg()._backend.round_up(N)
    pad = lambda v: np.concatenate([v, np.full(Np - N, np.nan)])  # the padding of the sites is not read
    K = getattr(O, kernel)(variance=1.3, lengthscales=ls).K(X) + 1e-6 * np.eye(N)
    s = np.sqrt(np.abs(l2))
    return X, ls, pad(l1), pad(l2), K, s, Np


@pytest.mark.parametrize("N,D,kernel,extra", [(8, 1, "SquaredExponential", 0), (128, 3, "Matern52", 0), (129, 8, "SquaredExponential", 0),
                                              (300, 1, "Matern52", 0), (300, 3, "SquaredExponential", 64), (129, 3, "Matern52", 2)])
def test_system_kernel_and_the_factorisation_behind_it(eng, N, D, kernel, extra):
    B = pkg()._backend
    X, ls, l1, l2, K, s, Np = _system_inputs(N, D, kernel)
    lds = Np + extra
    Xt, ilt, l1t, l2t = _t(X), _t(1.0 / ls), _t(l1), _t(l2)
    fn = eng.lib.tsvgp_vgp_system_f64

    def build(flags):
        S = torch.full((2 * Np + 128, lds), float("nan"), dtype=torch.float64, device=DEV)
        B.check(fn(KINDS[kernel], Xt.data_ptr(), ilt.data_ptr(), 1.3, 1e-6, l1t.data_ptr(), l2t.data_ptr(), S.data_ptr(), N, Np, D,
                   lds, flags, eng._stream()), "vgp_system")
        torch.cuda.synchronize()
        return S

    S = build(0)
    Sn = S.cpu().numpy()
    Bref = np.eye(Np)
    Bref[:N, :N] += np.outer(s, s) * K
    Rref = np.zeros((Np, Np))
    Rref[:N, :N] = K * s[None, :]
    rref = np.zeros((128, Np))
    rref[0, :N] = s * (l1[:N] / l2[:N])
    # B: the lower block triangle, diagonal tiles in full; nothing above it
    written = np.kron(np.tril(np.ones((Np // 128, Np // 128))), np.ones((128, 128))).astype(bool)
    Bk = Sn[:Np, :Np]
    assert not np.isnan(Bk[written]).any() and np.isnan(Bk[~written]).all()
    assert np.max(np.abs(Bk[written] - Bref[written])) < 1e-10 * np.max(np.abs(Bref))
    assert np.array_equal(Bk[N:][written[N:]], Bref[N:][written[N:]])  # the identity block, exactly
    Rk, rk = Sn[Np:2 * Np, :Np], Sn[2 * Np:, :Np]
    assert relerr(Rk, Rref) < 1e-10 and relerr(rk, rref) < 1e-10
    assert np.all(Rk[N:] == 0) and np.all(Rk[:, N:] == 0) and np.all(rk[1:] == 0) and np.all(rk[0, N:] == 0)
    assert np.isnan(Sn[:, Np:]).all()  # columns beyond Np of a wider buffer are left alone
    # TSVGP_VGP_NO_ROWS: the same B, bit for bit, and nothing below it
    Sb = build(B.VGP_NO_ROWS).cpu().numpy()
    assert np.array_equal(Sb[:Np, :Np][written], Bk[written]) and np.isnan(Sb[Np:]).all()

    # the factorisation reads no more of B than was written (the rest is still NaN) and solves the rows that ride along
    info = torch.ones(1, dtype=torch.int32, device=DEV)
    work = torch.empty(128 * 128, dtype=torch.float64, device=DEV)
    B.check(eng.lib.tsvgp_potrf_solve_f64(S.data_ptr(), Np, lds, 1, (2 * Np + 128) * lds, info.data_ptr(), work.data_ptr(), Np + 128,
                                          0, eng._stream()), "potrf_solve")
    torch.cuda.synchronize()
    assert int(info[0]) == 0
    Sn = S.cpu().numpy()
    L = np.linalg.cholesky(Bref)
    assert relerr(np.tril(Sn[:Np, :Np]), L) < 1e-10
    Cref = np.linalg.solve(L, Rref.T).T
    assert relerr(Sn[Np:2 * Np, :Np], Cref) < 1e-10
    assert relerr(Sn[2 * Np, :Np], np.linalg.solve(L, rref[0])) < 1e-10
    assert np.linalg.cond(Bref) < 1e3  # what the 1e-10 above rests on (module docstring)


@pytest.mark.parametrize("lik", ["none", "gaussian", "bernoulli"])
@pytest.mark.parametrize("N,K,extra", [(8, 128, 0), (128, 128, 0), (129, 256, 0), (300, 384, 64), (300, 130, 2)])
def test_rows_kernel(eng, lik, N, K, extra):
    B = pkg()._backend
    rng = np.random.RandomState(5 * N + K)
    Np, ldc = B.round_up(N), K + extra
    C = np.full((Np, ldc), np.nan)
    C[:, :K] = 0.5 * rng.randn(Np, K) / np.sqrt(K)
    z = rng.randn(K)
    l1, l2 = rng.randn(Np), 0.1 + rng.rand(Np)
    Y = (rng.rand(N) > 0.5).astype(float) if lik == "bernoulli" else rng.randn(N)
    kdiag, s2, beta = 1.3, 0.3, 0.5
    lik_id = {"none": 0, "gaussian": 1, "bernoulli": 2}[lik]
    Ct, zt, Yt = _t(C), _t(z), _t(Y)
    nb = Np // 128

    def run(b, with_z=True):
        l1t, l2t = _t(l1), _t(l2)
        mean = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
        var = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
        vep = torch.full((nb,), float("nan"), dtype=torch.float64, device=DEV)
        eqp = torch.full((nb,), float("nan"), dtype=torch.float64, device=DEV)
        npp = torch.full((nb,), -1, dtype=torch.int32, device=DEV)
        B.check(eng.lib.tsvgp_vgp_rows_f64(Ct.data_ptr(), ldc, zt.data_ptr() if with_z else None, Yt.data_ptr() if lik_id else None,
                                           l1t.data_ptr() if lik_id else None, l2t.data_ptr() if lik_id else None, kdiag, lik_id, s2, b,
                                           mean.data_ptr(), var.data_ptr(), vep.data_ptr() if lik_id else None,
                                           eqp.data_ptr() if lik_id else None, npp.data_ptr(), N, Np, K, eng._stream()), "vgp_rows")
        torch.cuda.synchronize()
        return [a.cpu().numpy() for a in (mean, var, vep, eqp, npp, l1t, l2t)]

    mean, var, vep, eqp, npp, n1, n2 = run(beta)
    mref, vref = C[:N, :K] @ z, kdiag - np.sum(C[:N, :K] ** 2, axis=1)
    assert relerr(mean, mref) < 2e-10
    assert np.max(np.abs(var - vref)) < 2e-10 * kdiag
    assert np.all(vref > 0) and int(npp.sum()) == 0 and np.all(npp >= 0)
    again = run(beta)
    for a, b in zip((mean, var, vep, eqp, npp, n1, n2), again):
        assert np.array_equal(a, b, equal_nan=True)  # run to run, bit for bit
    if lik == "none":
        assert np.array_equal(n1, l1) and np.array_equal(n2, l2)
        m0, v0 = run(0.0, with_z=False)[:2]  # z == NULL skips the mean
        assert np.all(m0 == 0) and np.array_equal(v0, var)
        return
    olik = O.Gaussian(variance=s2) if lik == "gaussian" else O.Bernoulli()
    g0, g1 = olik.variational_expectations_grads(mean[:, None], var[:, None], Y[:, None])
    g0, g1 = g0[:, 0], g1[:, 0]
    ve = np.array([olik.variational_expectations(mean[i:i + 1, None], var[i:i + 1, None], Y[i:i + 1, None])[0] for i in range(N)])
    eqt = -0.5 * l2[:N] * ((l1[:N] / l2[:N] - mean) ** 2 + var)
    np.testing.assert_allclose(n1[:N], (1 - beta) * l1[:N] + beta * (g0 - 2 * g1 * mean), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(n2[:N], (1 - beta) * l2[:N] + beta * (-2 * g1), rtol=1e-10, atol=1e-10)
    assert np.array_equal(n1[N:], l1[N:]) and np.array_equal(n2[N:], l2[N:])  # rows >= N are not touched
    for k in range(nb):
        sl = slice(128 * k, min(128 * k + 128, N))
        assert abs(vep[k] - ve[sl].sum()) <= 1e-10 * np.sum(1 + np.abs(ve[sl]))
        assert abs(eqp[k] - eqt[sl].sum()) <= 1e-10 * np.sum(1 + np.abs(eqt[sl]))
    # beta = 0: the same sums, the sites bit for bit
    out0 = run(0.0)
    assert np.array_equal(out0[5], l1) and np.array_equal(out0[6], l2)
    assert np.array_equal(out0[2], vep) and np.array_equal(out0[3], eqp)


def test_rows_kernel_counts_bad_rows(eng):
    B = pkg()._backend
    N, K = 130, 128
    Np = B.round_up(N)
    C = np.zeros((Np, K))
    C[3, 0] = 2.0  # q = 4 > kdiag
    C[129, 5] = np.inf
    Ct = _t(C)
    var = torch.empty(N, dtype=torch.float64, device=DEV)
    npp = torch.zeros(Np // 128, dtype=torch.int32, device=DEV)
    B.check(eng.lib.tsvgp_vgp_rows_f64(Ct.data_ptr(), K, None, None, None, None, 1.0, 0, 0.0, 0.0, None, var.data_ptr(), None, None,
                                       npp.data_ptr(), N, Np, K, eng._stream()), "vgp_rows")
    torch.cuda.synchronize()
    assert npp.cpu().tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(N, D, kernel, lik):
    """Five beta = 0.5 updates of the restatement, computed once per case: (problem, sites, elbo, predictions)."""
    X, Y, k, l, Xnew = R.problem(N, D, lik, kernel)
    ref = R.TVGPRef(X, Y, k, l)
    for _ in range(5):
        ref.update(0.5)
    out = dict(X=X, Y=Y, Xnew=Xnew, k=k, l=l, l1=ref.lambda_1.copy(), l2=ref.lambda_2.copy(), elbo=ref.elbo(),
               alpha=ref.current_alpha())
    out["mean"], out["var"] = ref.predict_f(Xnew)
    out["cov"] = ref.predict_f(Xnew, full_cov=True)[1]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _hip_model(ref, kernel, lik):
    p = pkg()
    k = getattr(p, kernel)(variance=ref["k"].variance, lengthscales=ref["k"].lengthscales)
    l = p.Gaussian(variance=ref["l"].variance) if lik == "gaussian" else p.Bernoulli()
    return p.t_VGP((ref["X"].copy(), ref["Y"].copy()), k, l, device=DEV)


@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
@pytest.mark.parametrize("N,D,kernel", MODEL_CASES)
def test_model_against_the_restatement(N, D, kernel, lik):
    ref = _reference(N, D, kernel, lik)
    m = _hip_model(ref, kernel, lik)
    for _ in range(5):
        assert m.update_variational_parameters(beta=0.5) is None
    e1, e2 = relerr(m.lambda_1.numpy(), ref["l1"]), relerr(m.lambda_2.numpy(), ref["l2"])
    elbo = float(m.elbo())
    ee = abs(elbo - ref["elbo"]) / abs(ref["elbo"])
    mean, var = m.predict_f(ref["Xnew"])
    mean2, cov = m.predict_f(ref["Xnew"], full_cov=True)
    mean, var, cov = mean.cpu().numpy(), var.cpu().numpy(), cov.cpu().numpy()
    em, ev, ec = relerr(mean, ref["mean"]), relerr(var, ref["var"]), relerr(cov, ref["cov"])
    ea = relerr(m.q_alpha.cpu().numpy(), ref["alpha"])
    print(f"t_VGP N={N} D={D} {kernel} {lik}: lambda_1 {e1:.2e} lambda_2 {e2:.2e} elbo {ee:.2e} mean {em:.2e} var {ev:.2e} "
          f"cov {ec:.2e} alpha {ea:.2e}")
    assert e1 < 1e-8 and e2 < 1e-8
    assert ee < 1e-9
    assert mean.shape == (37, 1) and var.shape == (37, 1) and cov.shape == (1, 37, 37)
    assert em < 1e-8 and ev < 1e-8 and ec < 1e-8 and ea < 1e-8
    assert np.array_equal(mean2.cpu().numpy(), mean)
    assert np.array_equal(cov[0], cov[0].T)  # symmetric bit for bit
    assert relerr(np.diagonal(cov[0])[:, None], var) < 1e-8  # the joint form against the diagonal form
    # elbo() leaves the sites alone, bit for bit; maximum_log_likelihood_objective is elbo
    l1, l2 = m.lambda_1.numpy().copy(), m.lambda_2.numpy().copy()
    assert float(m.maximum_log_likelihood_objective()) == elbo
    assert np.array_equal(m.lambda_1.numpy(), l1) and np.array_equal(m.lambda_2.numpy(), l2)
    Fy, Vy = m.predict_y(ref["Xnew"])
    ry, rv = ref["l"].predict_mean_and_var(ref["mean"], ref["var"])
    assert relerr(Fy.cpu().numpy(), ry) < 1e-8 and relerr(Vy.cpu().numpy(), rv) < 1e-8


def test_kernel_parameters_are_read_fresh_and_alpha_follows_them():
    N, D, kernel, lik = MODEL_CASES[1][0], MODEL_CASES[1][1], MODEL_CASES[1][2], "gaussian"
    ref = _reference(N, D, kernel, lik)
    m = _hip_model(ref, kernel, lik)
    m.update_variational_parameters(beta=1.0)
    a0 = m.q_alpha
    assert m.q_alpha is a0  # cached on the stamps
    m.kernel.variance.assign(2.0)
    k2 = getattr(O, kernel)(variance=2.0, lengthscales=ref["k"].lengthscales)
    r = R.TVGPRef(ref["X"], ref["Y"], ref["k"], ref["l"])
    r.update(1.0)
    r.kernel = k2
    assert relerr(m.q_alpha.cpu().numpy(), r.current_alpha()) < 1e-8
    assert abs(float(m.elbo()) - r.elbo()) < 1e-9 * abs(r.elbo())


def test_reference_pins_through_the_hip_path():
    """reference tests/models/test_tvgp.py:96-129 on its own setup."""
    p = pkg()
    X, Y, kern, s2 = reference_setup()
    m = p.t_VGP((X, Y), p.SquaredExponential(**kern), p.Gaussian(variance=s2), device=DEV)
    m.update_variational_parameters(beta=1.0)
    np.testing.assert_allclose(m.lambda_1.numpy(), Y / s2)
    np.testing.assert_allclose(m.lambda_2.numpy(), np.ones((8, 1)) / s2)
    lml = O.gpr_log_marginal_likelihood(O.SquaredExponential(**kern), X, Y, s2)
    optim = float(m.elbo())
    np.testing.assert_almost_equal(optim, lml, decimal=4)
    m.update_variational_parameters(beta=1.0)
    np.testing.assert_almost_equal(optim, float(m.elbo()), decimal=4)


def test_failures_raise_and_leave_the_sites():
    p = pkg()
    X, Y, kern, s2 = reference_setup()
    m = p.t_VGP((X, Y), p.SquaredExponential(**kern), p.Gaussian(variance=s2), device=DEV)
    m.update_variational_parameters(beta=1.0)
    l1, l2 = m.lambda_1.numpy().copy(), m.lambda_2.numpy().copy()
    m.kernel.variance.assign(float("nan"))  # every pivot is NaN: info != 0
    with pytest.raises(FloatingPointError):
        m.update_variational_parameters(beta=0.5)
    with pytest.raises(FloatingPointError):
        m.elbo()
    assert np.array_equal(m.lambda_1.numpy(), l1) and np.array_equal(m.lambda_2.numpy(), l2)
