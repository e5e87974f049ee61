"""GPU checks of the pathwise function draws: ``tsvgp_pathwise_f64`` against the NumPy restatement at the shapes where it can go
wrong, ``sample_functions`` of every sparse model against the restated sampler, and the properties that make a draw a function.

Kernel bound, per entry: 1e-11 * A[s, n] with (tests/pathwise_ref.py::magnitude)

    A = sum_l (|W[s, l]| + |W[s, L + l]|)(1 + sum_d |Omega_ld x~_nd|) + sum_m |V[s, m]| k(x_n, z_m).

Each summand carries a few units of 1.1e-16 of its own size, plus the rounding of the argument of the sine and cosine, which is
that of sum_d |Omega_ld x~_nd|; summing <= 1e4 terms adds <= 1e-12 A.  1e-11 is the project's fp64 kernel-level constant
(SURVEY.md section 8(d)).
"""
import numpy as np
import pytest
import torch

from tests import pathwise_ref as R
from tests.helpers import pkg, synthetic

pytestmark = pytest.mark.gpu

KINDS = [R.SE, R.MATERN32, R.MATERN52]
NS, LS, MS = [1, 127, 129, 257], [1, 63, 65, 257], [0, 1, 127, 130]
KERNEL_TOL = 1e-11
MODEL_TOL = 1e-8  # the project's fp64 model tolerance, relative to 1 + max |reference|


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def _kernel_problem(kind, N, L, M, D, S, seed):
    """ARD lengthscales; half of the rows near an inducing point (kernel values of order one), the others with |x~| up to 20."""
    rng = np.random.RandomState(seed)
    ls = rng.uniform(0.5, 2.0, D)
    inv_ls, variance = 1.0 / ls, 1.7
    Zt = rng.uniform(-3.0, 3.0, (max(M, 1), D))
    Xt = rng.uniform(-20.0, 20.0, (N, D))
    if M > 0:
        near = np.arange(N) % 2 == 0
        Xt[near] = Zt[rng.randint(0, M, near.sum())] + 0.4 * rng.randn(near.sum(), D)
    X, Z = Xt * ls, Zt[:M] * ls
    Omega = R.spectral(kind, seed, 1, L, D)
    W = rng.randn(S, 2 * L) * np.sqrt(variance / L)
    V = 3.0 * rng.randn(S, M)
    return X, Z, inv_ls, variance, Omega, W, V


def _call(kind, X, Z, inv_ls, variance, Omega, W, V, ldo):
    """One raw call of the entry point; the output buffer carries a sentinel everywhere, which must survive beyond column N."""
    B = pkg()._backend
    N, D = X.shape
    L, S, M = Omega.shape[0], W.shape[0], Z.shape[0]
    sentinel = -777.25
    out = torch.full((S, ldo), sentinel, dtype=torch.float64, device="cuda")
    t = [_dev(a) for a in (X, inv_ls, Omega, W)]
    Zd, Vd = (_dev(Z), _dev(V)) if M > 0 else (None, None)
    status = B.lib().tsvgp_pathwise_f64(kind, t[0].data_ptr(), Zd.data_ptr() if M else None, t[1].data_ptr(), variance, t[2].data_ptr(),
                                       t[3].data_ptr(), Vd.data_ptr() if M else None, out.data_ptr(), N, M, L, D, S, ldo,
                                       torch.cuda.current_stream().cuda_stream)
    assert status == 0
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.all(out[:, N:] == sentinel), "columns >= N were written"
    return out[:, :N]


@pytest.mark.parametrize("D", [1, 3, 32])
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_matches_the_restatement_at_the_edge_shapes(kind, D):
    """Every N, L, M and S of the lists with every (kind, D): four calls per case, the lists rotated against each other by the
    case's number so that the 36 calls pair the values differently; ldo = N and N + 5 alternate."""
    cap = pkg()._backend.PATHWISE_MAX_S
    SS = [1, 3, cap]
    c = KINDS.index(kind) * 3 + [1, 3, 32].index(D)
    for j in range(4):
        N, L, M, S = NS[j], LS[(j + c) % 4], MS[(j + c // 2) % 4], SS[(j + c) % 3]
        ldo = N + 5 * ((j + c) % 2)
        args = _kernel_problem(kind, N, L, M, D, S, seed=100 + 10 * c + j)
        out = _call(kind, *args, ldo)
        ref = R.evaluate(kind, *args)
        A = R.magnitude(kind, *args)
        ratio = np.max(np.abs(out - ref) / A)
        print(f"kind {kind} D {D} N {N} L {L} M {M} S {S} ldo {ldo}: max err / A = {ratio:.2e}")
        assert ratio <= KERNEL_TOL, (N, L, M, S, ldo)


def test_engine_chunks_the_samples():
    """cap + 1 samples through ``EStepEngine.pathwise``: two launches, the second with one sample; with and without the update."""
    p = pkg()
    cap = p._backend.PATHWISE_MAX_S
    kind, N, L, M, D, S = R.MATERN52, 129, 65, 130, 3, cap + 1
    X, Z, inv_ls, variance, Omega, W, V = _kernel_problem(kind, N, L, M, D, S, seed=77)
    eng = p.estep.EStepEngine(torch.float32)  # (the path is fp64 whatever the engine's compute dtype)
    kern = p.Matern52(variance=variance, lengthscales=1.0 / inv_ls)
    for Vc in (V, None):
        out = eng.pathwise(_dev(X), _dev(Z), kern, _dev(Omega), _dev(W), None if Vc is None else _dev(Vc))
        assert out.dtype == torch.float64 and tuple(out.shape) == (S, N)
        ref, A = R.evaluate(kind, X, Z, inv_ls, variance, Omega, W, Vc), R.magnitude(kind, X, Z, inv_ls, variance, Omega, W, Vc)
        assert np.max(np.abs(out.cpu().numpy() - ref) / A) <= KERNEL_TOL
    with pytest.raises(ValueError, match="32"):
        eng.pathwise(torch.zeros(4, 33), None, kern, torch.zeros(2, 33), torch.zeros(1, 4))


# ---------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------
def _grid_problem(P=1, seed=3):
    """N = 300 rows in two dimensions, M = 16 inducing points on a 4 x 4 grid a lengthscale apart (cond(K6) of a few hundred)."""
    X, Y, _ = synthetic(300, 16, 2, P=P, seed=seed)
    g = np.linspace(-1.5, 1.5, 4)
    Z = np.stack(np.meshgrid(g, g), axis=-1).reshape(16, 2)
    return X, Y, Z


def _build(which, dtype=torch.float64):
    p = pkg()
    ard = lambda cls, v, a, b: cls(variance=v, lengthscales=np.array([a, b]))
    if which == "shared":
        X, Y, Z = _grid_problem(P=2)
        m = p.t_SVGP(ard(p.SquaredExponential, 1.2, 0.7, 0.9), p.Gaussian(0.1), Z, num_latent_gps=2, compute_dtype=dtype)
    elif which == "separate":
        X, Y, Z = _grid_problem(P=2)
        kern = p.SeparateIndependent([ard(p.SquaredExponential, 1.2, 0.7, 0.9), ard(p.Matern32, 0.8, 1.1, 0.8)])
        m = p.t_SVGP(kern, p.Gaussian(0.1), p.SharedIndependentInducingVariables(Z), num_latent_gps=2, compute_dtype=dtype)
    elif which == "white":
        X, Y, Z = _grid_problem()
        m = p.t_SVGP_white(ard(p.Matern52, 1.1, 0.8, 1.0), p.Gaussian(0.2), Z, num_data=300, compute_dtype=dtype)
    else:
        X, Y, Z = _grid_problem()
        m = p.t_SVGP_sites((X, Y), ard(p.SquaredExponential, 1.0, 0.8, 0.7), p.Gaussian(0.2), Z, compute_dtype=dtype)
    for _ in range(3):
        m.natgrad_step(lr=0.8) if which == "sites" else m.natgrad_step((X, Y), lr=0.8)
    return m, Z


def _restated(m, Z, seed, draw, L, S):
    """The restated sampler on the HIP model's own q(u) and kernel parameters: (ops, kinds, inv_ls, variances, K6s)."""
    p = pkg()
    P = int(m.num_latent_gps)
    kernels = p.kernels.latent_kernels(m.kernel, P)
    shared = not isinstance(m.kernel, p.SeparateIndependent)
    kinds = [k.kind for k in kernels]
    inv_ls = [1.0 / np.broadcast_to(k.lengthscales.numpy(), (Z.shape[1],)) for k in kernels]
    variances = [k.variance.item() for k in kernels]
    mq, cholS = m.get_mean_chol_cov_inducing_posterior()
    K6 = np.stack([R.kernel_matrix(kinds[q], Z, Z, inv_ls[q], variances[q]) + p.default_jitter() * np.eye(Z.shape[0]) for q in range(P)])
    for q in range(P):
        assert np.linalg.cond(K6[q]) <= 1e4  # so that the solve for V cannot eat the tolerance
    ops = R.sampler(mq.cpu().numpy(), cholS.cpu().numpy(), K6[0] if shared else K6, kinds, Z, inv_ls, variances, seed, draw, L, S,
                    shared=shared)
    return ops, kinds, inv_ls, variances


def _xnew(N=257, seed=5):
    return np.random.RandomState(seed).uniform(-2.5, 2.5, (N, 2))


@pytest.mark.parametrize("which,dtype", [("shared", torch.float64), ("separate", torch.float64), ("white", torch.float64),
                                         ("sites", torch.float64), ("shared", torch.float32)])
def test_model_draws_match_the_restated_sampler(which, dtype):
    m, Z = _build(which, dtype)
    seed, draw, L, S = 9, 4, 65, 3
    fs = m.sample_functions(S, L, seed=seed, draw=draw)
    assert (fs.num_samples, fs.num_features, fs.seed, fs.draw) == (S, L, seed, draw)
    Xs = _xnew()
    f = fs(Xs)
    P = int(m.num_latent_gps)
    assert f.dtype == torch.float64 and tuple(f.shape) == (S, 257, P) and f.device == m.device
    assert tuple(fs.u.shape) == (S, 16, P)
    ops, kinds, inv_ls, variances = _restated(m, Z, seed, draw, L, S)
    ref = R.sample(ops, kinds, Xs, Z, inv_ls, variances)
    err, scale = np.max(np.abs(f.cpu().numpy() - ref)), 1.0 + np.max(np.abs(ref))
    print(f"{which} {dtype}: max err {err:.2e} (max |ref| {scale - 1:.2f}), u err {np.max(np.abs(fs.u.cpu().numpy() - ops['u'])):.2e}")
    assert err <= MODEL_TOL * scale
    assert np.max(np.abs(fs.u.cpu().numpy() - ops["u"])) <= MODEL_TOL * (1.0 + np.max(np.abs(ops["u"])))


def test_a_draw_is_a_function():
    m, Z = _build("separate")
    fs = m.sample_functions(3, 65, seed=1, draw=2)
    X1, X2 = torch.as_tensor(_xnew(130, 1)).cuda(), torch.as_tensor(_xnew(257, 2)).cuda()
    f1, f2, f12 = fs(X1), fs(X2), fs(torch.cat([X1, X2]))
    assert torch.equal(f12[:, :130], f1) and torch.equal(f12[:, 130:], f2)  # bit for bit on the shared rows
    assert torch.equal(fs(X1), f1)
    again = m.sample_functions(3, 65, seed=1, draw=2)
    assert torch.equal(again(X2), f2) and torch.equal(again.u, fs.u)
    assert not torch.equal(m.sample_functions(3, 65, seed=1, draw=3)(X2), f2)
    # a later change of the model does not reach the object
    m.kernel.kernels[0].lengthscales.assign(np.array([2.0, 3.0]))
    m.kernel.kernels[1].variance.assign(5.0)
    assert torch.equal(fs(X1), f1)
    assert not torch.equal(m.sample_functions(3, 65, seed=1, draw=2)(X1), f1)


def test_draw_counters_are_separate():
    """``sample_functions(draw=None)`` advances a counter of its own: ``predict_f_samples(draw=None)`` before and after gives the
    sequence draw = 0, 1 it gives without it."""
    m, _ = _build("white")
    Xs = _xnew(40)
    a = m.predict_f_samples(Xs, 2, seed=3)
    fs0 = m.sample_functions(2, 8, seed=3)
    fs1 = m.sample_functions(2, 8, seed=3)
    b = m.predict_f_samples(Xs, 2, seed=3)
    assert (fs0.draw, fs1.draw) == (0, 1) and m._sample_draw == 2 and m._function_draw == 2
    assert torch.equal(a, m.predict_f_samples(Xs, 2, seed=3, draw=0)) and torch.equal(b, m.predict_f_samples(Xs, 2, seed=3, draw=1))
    assert m._sample_draw == 2
    assert torch.equal(fs1(Xs), m.sample_functions(2, 8, seed=3, draw=1)(Xs)) and m._function_draw == 2  # an explicit draw leaves it
    assert not torch.equal(fs0(Xs), fs1(Xs))


@pytest.mark.parametrize("which", ["shared", "separate", "white", "sites"])
def test_draws_interpolate_the_inducing_values(which):
    """f_s(Z) = g_s(Z) + (K6 - jitter I) V_s = u_s - jitter V_s: exact algebra whatever L is, so the gap is the rounding of the
    evaluation at Z (the kernel bound above) -- the solve's own residual, M eps |K6| |V|, is far inside it."""
    p = pkg()
    m, Z = _build(which)
    fs = m.sample_functions(3, 33, seed=2, draw=0)
    gap = (fs(Z) - fs.u + p.default_jitter() * fs.V).cpu().numpy()  # [S, M, P]
    P = int(m.num_latent_gps)
    kernels = p.kernels.latent_kernels(m.kernel, P)
    for q, k in enumerate(kernels):
        inv_ls = 1.0 / np.broadcast_to(k.lengthscales.numpy(), (2,))
        A = R.magnitude(k.kind, Z, Z, inv_ls, k.variance.item(), fs.Omega[q].cpu().numpy(), fs.W[q].cpu().numpy(),
                        fs.V[:, :, q].cpu().numpy())
        ratio = np.max(np.abs(gap[:, :, q]) / A)
        print(f"{which} latent {q}: max |f(Z) - u + jitter V| / A = {ratio:.2e}, max |V| {float(fs.V[:, :, q].abs().max()):.1f}")
        assert ratio <= KERNEL_TOL


def test_errors():
    p = pkg()
    m, Z = _build("white")
    with pytest.raises(ValueError, match="num_samples"):
        m.sample_functions(0)
    wide = p.t_SVGP(p.SquaredExponential(1.0, 3.0), p.Gaussian(0.1), np.random.RandomState(0).randn(8, 33))
    with pytest.raises(ValueError, match="32"):
        wide.sample_functions(2, 16)
    assert wide._function_draw == 0  # a call that raised leaves the counter alone
    X, Y, _ = _grid_problem()
    exact = p.t_VGP((X[:50], Y[:50]), p.SquaredExponential(1.0, 1.0), p.Gaussian(0.1))
    with pytest.raises(AttributeError):
        exact.sample_functions(2)
    with pytest.raises(ValueError, match="Xnew"):
        m.sample_functions(2, 16)(np.zeros((5, 3)))
