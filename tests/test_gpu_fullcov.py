"""GPU tests of the joint predictions: the ``tsvgp_cov_*`` kernel against NumPy, ``predict_f(full_cov=True)`` of the three models
against tests/fullcov_ref.py (GPflow's base_conditional(full_cov=True) restated on the oracle's q(u)), and ``predict_f_samples``.

Tolerances: fp64 ``relerr`` (max-abs over max-abs) <= 1e-8; fp32 compute dtype against the fp64 restatement
atol 1e-4 + rtol 1e-3 * max|reference|.  The models take the ORACLE's state after its E-steps (through their constructors), so
what is compared is the prediction path alone."""
import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests import fullcov_ref as R
from tests import sites_ref, softmax_ref
from tests.helpers import pkg, relerr, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = {"se": 0, "matern32": 2, "matern52": 3}


def _close(got, ref, dtype, what=""):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if dtype == torch.float64:
        e = relerr(got, ref)
        print(f"{what} fp64 relerr {e:.3e}")
        assert e <= 1e-8, f"{what}: relerr {e:.3e}"
    else:
        e, bound = float(np.max(np.abs(got - ref))), 1e-4 + 1e-3 * float(np.max(np.abs(ref)))
        print(f"{what} fp32 max abs err {e:.3e} (bound {bound:.3e})")
        assert e <= bound, f"{what}: max abs err {e:.3e} > {bound:.3e}"


# ------------------------------------------------------------------------------------------------ the kernel alone
def _profile(kind, s):
    if kind == "se":
        return np.exp(-0.5 * s)
    r = np.sqrt(np.maximum(s, 1e-36))
    if kind == "matern32":
        return (1.0 + np.sqrt(3.0) * r) * np.exp(-np.sqrt(3.0) * r)
    return (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * np.exp(-np.sqrt(5.0) * r)


def _launch_cov(dtype, kind, T, X, inv_ls, variance, sign, C, N, flags):
    B = pkg()._backend
    fn = getattr(B.lib(), "tsvgp_cov_f64" if dtype == torch.float64 else "tsvgp_cov_f32")
    Np, Mp = T.shape
    with torch.cuda.device(C.device):
        st = fn(KINDS[kind], T.data_ptr(), None if X is None else X.data_ptr(), None if inv_ls is None else inv_ls.data_ptr(),
                float(variance), float(sign), C.data_ptr(), N, Np, Mp, 0 if X is None else X.shape[1], C.stride(0), flags,
                torch.cuda.current_stream(C.device).cuda_stream)
    assert st == 0, f"tsvgp_cov returned {st}"
    torch.cuda.synchronize(C.device)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("N", [1, 127, 128, 300, 1000])
def test_cov_kernel_against_numpy(dtype, N):
    """Every shape x kind x sign x base mode: the valid block against NumPy, the padding (0 off, 1 on the diagonal) and the
    columns beyond Np against a buffer pre-filled with 7, bitwise symmetry, and a second run bit for bit."""
    Np = (N + 127) // 128 * 128
    vw = 2 if dtype == torch.float64 else 4
    for Mp in (128, 384):
        for D in (1, 3, 32):
            rng = np.random.RandomState(1000 * D + Mp + N)
            Th = np.zeros((Np, Mp))
            Th[:N] = 0.1 * rng.randn(N, Mp)  # the tile tsvgp_trmm_* writes: padding rows zero
            Xh, ils, variance = rng.randn(N, D), 0.5 + rng.rand(D), 1.3
            Xs = Xh * ils
            s = np.sum((Xs[:, None, :] - Xs[None, :, :]) ** 2, axis=-1)
            T = torch.as_tensor(Th, dtype=dtype, device=DEV)
            X, inv_ls = torch.as_tensor(Xh, dtype=dtype, device=DEV), torch.as_tensor(ils, dtype=dtype, device=DEV)
            # the references see the operands as the kernel does (rounded to the array type)
            T64, gram = T.double().cpu().numpy(), None
            gram = T64[:N] @ T64[:N].T
            B0 = rng.randn(N, N)
            B0 = 0.5 * (B0 + B0.T)
            for ci, (kind, sign, accumulate) in enumerate([(k, sg, False) for k in KINDS for sg in (-1.0, 1.0)]
                                                          + [("se", -1.0, True), ("se", 1.0, True)]):
                ldc = Np + (2 * vw if ci % 3 == 0 else 0)
                C = torch.full((Np, ldc), 7.0, dtype=dtype, device=DEV)
                if accumulate:  # the base sits in the LOWER triangle; the 7s above it must not be read
                    base = torch.as_tensor(B0, dtype=dtype, device=DEV)
                    C[:N, :N] = torch.where(torch.ones(N, N, device=DEV).tril().bool(), base, C[:N, :N])
                    ref = base.double().cpu().numpy() + sign * gram
                    _launch_cov(dtype, kind, T, None, None, 0.0, sign, C, N, 1)
                else:
                    ref = variance * _profile(kind, s) + sign * gram
                    _launch_cov(dtype, kind, T, X, inv_ls, variance, sign, C, N, 0)
                what = f"N={N} Mp={Mp} D={D} {kind} sign={sign:+.0f} acc={accumulate}"
                _close(C[:N, :N].cpu().numpy(), ref, dtype, what)
                sq = C[:, :Np]
                assert torch.equal(sq, sq.t()), f"{what}: not bitwise symmetric"
                pad = torch.zeros((Np, Np), dtype=dtype, device=DEV)
                pad.diagonal()[N:] = 1.0
                assert torch.equal(sq[N:], pad[N:]) and torch.equal(sq[:, N:], pad[:, N:]), f"{what}: padding is not the identity block"
                assert bool((C[:, Np:] == 7.0).all()), f"{what}: wrote beyond column Np"
                C2 = torch.full((Np, ldc), 7.0, dtype=dtype, device=DEV)
                if accumulate:
                    C2[:N, :N] = torch.where(torch.ones(N, N, device=DEV).tril().bool(), base, C2[:N, :N])
                    _launch_cov(dtype, kind, T, None, None, 0.0, sign, C2, N, 1)
                else:
                    _launch_cov(dtype, kind, T, X, inv_ls, variance, sign, C2, N, 0)
                assert torch.equal(C, C2), f"{what}: two runs differ"


# ------------------------------------------------------------------------------------------------ models
def _xnew(D, n=300, seed=77):
    return np.random.RandomState(seed).randn(n, D) * 0.9


def _kern(mod, name, variance=1.0, ls=1.0):
    return {"se": mod.SquaredExponential, "matern32": mod.Matern32, "matern52": mod.Matern52}[name](variance, ls)


def _tsvgp_pair(case, compute_dtype):
    """(HIP model, oracle) with the oracle's state after 3 E-steps at lr 0.8 on helpers.synthetic(500, 40, D)."""
    p = pkg()
    D = 40 if case == "d40" else 3
    P = 2 if case in ("bernoulli2", "separate") else 1
    lik = "bernoulli" if case == "bernoulli2" else "gaussian"
    X, Y, Z = synthetic(500, 40, D, P=P, lik=lik, seed=11)
    ls = 6.0 if case == "d40" else 1.0  # 40 dimensions: distances ~ sqrt(80)
    if case == "separate":
        kern = lambda mod: mod.SeparateIndependent([_kern(mod, "se", 1.0, 0.9), _kern(mod, "matern32", 0.7, 1.4)])
        iv = lambda mod: mod.SharedIndependentInducingVariables(Z)
    else:
        kern = lambda mod: _kern(mod, "matern52" if case == "matern52" else "se", 1.1, ls)
        iv = lambda mod: Z
    mk_lik = lambda mod: mod.Bernoulli() if lik == "bernoulli" else mod.Gaussian(0.1)
    ora = O.t_SVGP(kern(O), mk_lik(O), iv(O), num_latent_gps=P)
    for _ in range(3):
        ora.natgrad_step((X, Y), lr=0.8)
    hip = p.t_SVGP(kern(p), mk_lik(p), iv(p), num_latent_gps=P, lambda_1=np.array(ora.lambda_1),
                   lambda_2_sqrt=np.array(ora.lambda_2_sqrt), compute_dtype=compute_dtype)
    return hip, ora, _xnew(D)


def _check_joint(hip, ref_model, Xs, dtype, what, mean_slack=0.0):
    mean_r, cov_r = R.predict_f_full_cov(ref_model, Xs)
    mean, cov = hip.predict_f(Xs, full_cov=True)
    N, P = mean_r.shape
    assert tuple(mean.shape) == (N, P) and tuple(cov.shape) == (P, N, N) and cov.dtype == torch.float64 and mean.dtype == torch.float64
    mu, var = hip.predict_f(Xs)
    _close(cov.cpu().numpy(), cov_r, dtype, what + " cov")
    if mean_slack:  # one case only, see SITES_FP32_MEAN_SLACK
        e = float(np.max(np.abs(mean.cpu().numpy() - mean_r)))
        bound = 1e-4 + 1e-3 * float(np.max(np.abs(mean_r))) + mean_slack
        print(f"{what} mean fp32 max abs err {e:.3e}; predict_f's {float(np.max(np.abs(mu.cpu().numpy() - mean_r))):.3e}; "
              f"bound {bound:.3e} of which slack {mean_slack:.1e}")
        assert e <= bound, f"{what} mean: max abs err {e:.3e} > {bound:.3e}"
    else:
        _close(mean.cpu().numpy(), mean_r, dtype, what + " mean")
    assert torch.equal(cov, cov.transpose(-1, -2))
    diag = cov.diagonal(dim1=-2, dim2=-1).t()
    if dtype == torch.float64:  # a different summation order of the same product, nothing else
        e_d, e_m = relerr(diag.cpu().numpy(), var.cpu().numpy()), relerr(mean.cpu().numpy(), mu.cpu().numpy())
        print(f"{what} diag vs predict_f {e_d:.3e}, mean vs predict_f {e_m:.3e}")
        assert e_d <= 1e-12 and (torch.equal(mean, mu) or e_m <= 1e-13)
    else:
        _close(diag.cpu().numpy(), var.cpu().numpy(), dtype, what + " diag vs predict_f")
        _close(mean.cpu().numpy(), mu.cpu().numpy(), dtype, what + " mean vs predict_f")
    m2, full_out = hip.predict_f(Xs, full_output_cov=True)
    assert tuple(full_out.shape) == (N, P, P) and torch.equal(full_out, torch.diag_embed(var)) and torch.equal(m2, mu)
    with pytest.raises(NotImplementedError, match="full_cov and full_output_cov"):
        hip.predict_f(Xs, full_cov=True, full_output_cov=True)
    return mean, cov


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", ["gaussian1", "bernoulli2", "separate", "matern52", "d40"])
def test_tsvgp_full_cov(case, dtype):
    hip, ora, Xs = _tsvgp_pair(case, dtype)
    mean, cov = _check_joint(hip, ora, Xs, dtype, f"t_SVGP {case}")
    if case in ("gaussian1", "bernoulli2"):  # one shared kernel: the site form of the reference (tsvgp.py:215-232)
        m2, c2 = hip.new_predict_f(Xs, full_cov=True)
        assert torch.equal(m2, mean) and torch.equal(c2, cov)
        with pytest.raises(NotImplementedError):
            hip.new_predict_f(Xs, full_cov=True, full_output_cov=True)


def _white_pair(route, dtype):
    p = pkg()
    X, Y, Z = synthetic(500, 40, 3, P=1, lik="gaussian", seed=12)
    mk = lambda mod, **kw: mod.t_SVGP_white(mod.SquaredExponential(1.1, 1.0), mod.Gaussian(0.2), Z, num_data=500, **kw)
    ora = mk(O)
    for _ in range(3):
        ora.natgrad_step((X, Y), lr=0.8)
    hip = mk(p, lambda_1=np.array(ora.lambda_1), lambda_2=np.array(ora.lambda_2), compute_dtype=dtype,
             projection="direct" if route == "direct" else "whitened")
    if route == "two_product":
        hip._two_product = True  # the form the model moves to when Lambda_2 + 1e-9 I has no factor (tests/test_gpu_white.py)
    return hip, ora, _xnew(3)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("route", ["direct", "whitened", "two_product"])
def test_white_full_cov_every_route(route, dtype):
    hip, ora, Xs = _white_pair(route, dtype)
    _check_joint(hip, ora, Xs, dtype, f"t_SVGP_white {route}")
    assert hip._two_product == (route == "two_product") and hip._use_direct() == (route == "direct")


def test_white_full_cov_indefinite_lambda_2():
    """Lambda_2 = -0.45 K_uu (tests/test_gpu_white.py): the single-product factor does not exist, the joint covariance moves to
    the two-product form on its own, as predict_f does."""
    p = pkg()
    rng = np.random.RandomState(32)
    Z = rng.randn(40, 4) * 1.3
    lam2, lam1 = (-0.45 * O.SquaredExponential(1.2, 0.9).K(Z))[None], 0.3 * rng.randn(40, 1)
    mk = lambda mod: mod.t_SVGP_white(mod.SquaredExponential(1.2, 0.9), mod.Gaussian(0.2), Z, lambda_1=lam1.copy(), lambda_2=lam2.copy())
    hip, ora = mk(p), mk(O)
    _check_joint(hip, ora, _xnew(4, 200), torch.float64, "t_SVGP_white indefinite")
    assert hip._two_product


# The ONE case whose fp32 mean does not meet atol 1e-4 + rtol 1e-3 * max|mean| (= 1.405e-3 here) against the fp64 restatement:
# t_SVGP_sites with fp32 arrays on the issue's problem (synthetic(500, 40, 3), Z = X[:40]).  Measured on an MI355X: max abs error
# 2.240e-3 -- and predict_f(Xnew), the parent's path, has the same 2.240e-3 on the same points; the two means differ from each
# other by 2.4e-7.  The error is made before the prediction: this model alone forms q(u) from an fp32 projection
# l = sum_n lambda_1n k_n (unit roundoff 6e-8 on l), and m = K6 R^-1 l amplifies it by cond(K_uu + L + 1e-9 I), ~1e4-1e5 with
# inducing points drawn from the data.  The joint prediction is held to predict_f's mean at the plain fp32 bound (below, every
# case) and to the restatement with this absolute slack on top of the bound.
SITES_FP32_MEAN_SLACK = 2e-3


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_sites_full_cov(dtype):
    p = pkg()
    X, Y, Z = synthetic(500, 40, 3, P=1, lik="gaussian", seed=13)
    ref = sites_ref.t_SVGP_sites((X, Y), O.SquaredExponential(1.0, 1.0), O.Gaussian(0.2), Z)
    for _ in range(3):
        ref.natgrad_step(lr=0.8)
    hip = p.t_SVGP_sites((X, Y), p.SquaredExponential(1.0, 1.0), p.Gaussian(0.2), Z, lambda_1=ref.lambda_1.copy(),
                         lambda_2=ref.lambda_2.copy(), compute_dtype=dtype)
    _check_joint(hip, ref, _xnew(3), dtype, "t_SVGP_sites", mean_slack=SITES_FP32_MEAN_SLACK if dtype == torch.float32 else 0.0)


def test_full_cov_raises_on_non_positive_variance_as_predict_f():
    """No existing test builds a state with a non-positive predictive variance (q(u) bounds it below by the Nystrom residual), so
    the moments operand itself is inflated: with D -> 3 D, var = knn - 9 |D k|^2 < 0 near the data.  predict_f and
    predict_f(full_cov=True) raise the same FloatingPointError through the same status check."""
    hip, _, Xs = _tsvgp_pair("gaussian1", torch.float64)
    hip.predict_f(Xs, full_cov=True)  # the honest state passes
    plain = hip._site_operands

    def inflated(*a, **kw):
        ops = plain(*a, **kw)
        ops["D"] = 3.0 * ops["D"]
        return ops

    hip._site_operands = inflated
    with pytest.raises(FloatingPointError, match="non-positive predictive variance") as e1:
        hip.predict_f(Xs)
    with pytest.raises(FloatingPointError, match="non-positive predictive variance") as e2:
        hip.predict_f(Xs, full_cov=True)
    assert str(e1.value) == str(e2.value)  # the same rows: the diagonal of the joint covariance is the marginal variance
    with pytest.raises(FloatingPointError, match="non-positive predictive variance"):
        hip.predict_f_samples(Xs, 3)


# ------------------------------------------------------------------------------------------------ predict_f_samples
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", ["gaussian1", "separate", "matern52"])
def test_predict_f_samples_formula(case, dtype):
    hip, ora, Xs = _tsvgp_pair(case, dtype)
    N = Xs.shape[0]
    mean_r, cov_r = R.predict_f_full_cov(ora, Xs)
    P = mean_r.shape[1]
    S = 7
    eps = np.random.RandomState(5).randn(S, N, P)
    f = hip.predict_f_samples(Xs, S, epsilon=eps)
    assert tuple(f.shape) == (S, N, P) and f.dtype == torch.float64
    _close(f.cpu().numpy(), R.sample_mvn_full_cov(mean_r, cov_r, eps), dtype, f"samples {case} epsilon")
    assert hip._sample_draw == 0  # epsilon= leaves the counter alone
    # the generator: the Philox restatement for (seed, draw)
    f = hip.predict_f_samples(Xs, S, seed=1234, draw=3)
    eps_g = softmax_ref.normals(1234, 3, np.arange(N), S, P)
    _close(f.cpu().numpy(), R.sample_mvn_full_cov(mean_r, cov_r, eps_g), dtype, f"samples {case} generator")
    assert torch.equal(f, hip.predict_f_samples(Xs, S, seed=1234, draw=3))  # the same (seed, draw): bit for bit
    # draw=None: the model's counter, 0 then 1
    a, b = hip.predict_f_samples(Xs, S, seed=9), hip.predict_f_samples(Xs, S, seed=9)
    assert not torch.equal(a, b)
    assert torch.equal(a, hip.predict_f_samples(Xs, S, seed=9, draw=0)) and torch.equal(b, hip.predict_f_samples(Xs, S, seed=9, draw=1))
    assert hip._sample_draw == 2
    # shapes, the marginal form
    one = hip.predict_f_samples(Xs, seed=9, draw=0)
    assert tuple(one.shape) == (N, P) and torch.equal(one, hip.predict_f_samples(Xs, 1, seed=9, draw=0)[0])
    mu, var = hip.predict_f(Xs)
    fd = hip.predict_f_samples(Xs, S, full_cov=False, epsilon=eps)
    assert tuple(fd.shape) == (S, N, P)
    np.testing.assert_allclose(fd.cpu().numpy(), R.sample_mvn_diag(mu.cpu().numpy(), var.cpu().numpy(), eps), rtol=1e-14, atol=1e-14)
    assert tuple(hip.predict_f_samples(Xs, full_cov=False, seed=2, draw=0).shape) == (N, P)
    with pytest.raises(NotImplementedError, match="full_cov and full_output_cov"):
        hip.predict_f_samples(Xs, S, full_cov=True, full_output_cov=True)
    with pytest.raises(ValueError):
        hip.predict_f_samples(Xs, S, epsilon=eps[:, :-1])
    with pytest.raises(ValueError):
        hip.predict_f_samples(Xs, 0)


@pytest.mark.parametrize("which", ["white", "sites"])
def test_predict_f_samples_other_models(which):
    if which == "white":
        hip, ref, Xs = _white_pair("whitened", torch.float64)
    else:
        p = pkg()
        X, Y, Z = synthetic(500, 40, 3, P=1, lik="gaussian", seed=13)
        ref = sites_ref.t_SVGP_sites((X, Y), O.SquaredExponential(1.0, 1.0), O.Gaussian(0.2), Z)
        ref.natgrad_step(lr=0.8)
        hip = p.t_SVGP_sites((X, Y), p.SquaredExponential(1.0, 1.0), p.Gaussian(0.2), Z, lambda_1=ref.lambda_1.copy(),
                             lambda_2=ref.lambda_2.copy())
        Xs = _xnew(3)
    mean_r, cov_r = R.predict_f_full_cov(ref, Xs)
    f = hip.predict_f_samples(Xs, 4, seed=5, draw=2)
    eps = softmax_ref.normals(5, 2, np.arange(Xs.shape[0]), 4, 1)
    _close(f.cpu().numpy(), R.sample_mvn_full_cov(mean_r, cov_r, eps), torch.float64, f"samples {which}")


def test_predict_f_samples_too_many_latents():
    p = pkg()
    Z = np.random.RandomState(0).randn(8, 2)
    m = p.t_SVGP(p.SquaredExponential(), p.Gaussian(0.1), Z, num_latent_gps=33)
    with pytest.raises(ValueError, match="TSVGP_MAX_BATCH"):
        m.predict_f_samples(Z)


def test_predict_f_samples_statistics():
    """A sanity line, not a tolerance pin: 4096 joint draws at 64 points; the sample covariance lies within 6 standard errors of
    cov + 1e-6 I entrywise, the standard error of entry (i, j) being sqrt((c_ii c_jj + c_ij^2) / S)."""
    hip, ora, _ = _tsvgp_pair("gaussian1", torch.float64)
    Xs = _xnew(3, 64, seed=3)
    S = 4096
    mean_r, cov_r = R.predict_f_full_cov(ora, Xs)
    c = cov_r[0] + 1e-6 * np.eye(64)
    f = hip.predict_f_samples(Xs, S, seed=42, draw=0).cpu().numpy()[:, :, 0]
    dev = f - mean_r[None, :, 0]
    emp = dev.T @ dev / S
    se = np.sqrt((np.outer(np.diag(c), np.diag(c)) + c * c) / S)
    z = np.abs(emp - c) / se
    print("largest deviation in standard errors", z.max())
    assert z.max() <= 6.0
    assert np.max(np.abs(dev.mean(axis=0)) / np.sqrt(np.diag(c) / S)) <= 6.0
