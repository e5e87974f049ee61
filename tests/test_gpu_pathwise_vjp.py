"""GPU checks of the input gradient of the pathwise function draws: ``tsvgp_pathwise_vjp_f64`` against the NumPy restatement
(tests/pathwise_vjp_ref.py) at the shapes where it can go wrong, ``EStepEngine.pathwise_vjp``, and ``fs(Xnew)`` under torch
autograd for every sparse model.

Kernel bound, per entry: 1e-11 * A[n, d] with ``pathwise_vjp_ref.magnitude_vjp``, the size of the summands (|x~| + |z~| in place of
the cancelling difference).  Each summand carries a few units of 1.1e-16 of its own size plus the rounding of the sine's argument;
tests/test_pathwise_vjp_cpu.py holds the fp64 restatement itself to 1e-12 A against extended precision.  1e-11 is the project's
fp64 kernel-level constant.
"""
import functools

import numpy as np
import pytest
import torch

from tests import pathwise_ref as R
from tests import pathwise_vjp_ref as G
from tests.helpers import pkg
from tests.test_gpu_pathwise import _build, _restated, _xnew

pytestmark = pytest.mark.gpu

KINDS = [R.SE, R.MATERN32, R.MATERN52]
NS, LS, MS = [1, 127, 129, 257], [1, 63, 65, 257], [0, 1, 127, 130]
KERNEL_TOL = 1e-11
MODEL_TOL = 1e-8  # the project's fp64 model tolerance, relative to 1 + max |reference|
FD_TOL = 1e-7  # central differences with h = 1e-5 (tests/test_pathwise_vjp_cpu.py has the reasoning)


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), dtype=torch.float64).cuda()  # (a copy: the shared problems are read-only)


def _call(kind, X, Z, inv_ls, variance, Omega, W, V, C, ldc):
    """One raw call of the entry point.  C sits in a [S, ldc] buffer whose columns >= N are NaN (they must not be read); dX has 3
    rows more than N, filled with a sentinel that must survive."""
    B = pkg()._backend
    N, D = X.shape
    L, S, M = Omega.shape[0], W.shape[0], Z.shape[0]
    sentinel = -777.25
    dX = torch.full((N + 3, D), sentinel, dtype=torch.float64, device="cuda")
    Cd = torch.full((S, ldc), float("nan"), dtype=torch.float64, device="cuda")
    Cd[:, :N] = _dev(C)
    t = [_dev(a) for a in (X, inv_ls, Omega, W)]
    Zd, Vd = (_dev(Z), _dev(V)) if M > 0 else (None, None)
    status = B.lib().tsvgp_pathwise_vjp_f64(kind, t[0].data_ptr(), Zd.data_ptr() if M else None, t[1].data_ptr(), variance,
                                           t[2].data_ptr(), t[3].data_ptr(), Vd.data_ptr() if M else None, Cd.data_ptr(), ldc,
                                           dX.data_ptr(), N, M, L, D, S, torch.cuda.current_stream().cuda_stream)
    assert status == 0
    torch.cuda.synchronize()
    dX = dX.cpu().numpy()
    assert np.all(dX[N:] == sentinel), "rows >= N were written"
    return dX[:N]


@pytest.mark.parametrize("D", [1, 3, 32])
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_matches_the_restatement_at_the_edge_shapes(kind, D):
    """Every N, L, M and S of the lists with every (kind, D): four calls per case, the lists rotated against each other by the
    case's number as tests/test_gpu_pathwise.py rotates them; ldc = N and N + 5 alternate.  With M > 0 every eighth row sits
    exactly on an inducing point."""
    cap = pkg()._backend.PATHWISE_MAX_S
    SS = [1, 3, cap]
    c = KINDS.index(kind) * 3 + [1, 3, 32].index(D)
    for j in range(4):
        N, L, M, S = NS[j], LS[(j + c) % 4], MS[(j + c // 2) % 4], SS[(j + c) % 3]
        ldc = N + 5 * ((j + c) % 2)
        key = (kind, N, L, M, D, S, 100 + 10 * c + j)
        args = G.problem(*key)
        ref, A = G.problem_vjp(*key)
        dX = _call(kind, *args, ldc)
        assert np.all(np.isfinite(dX))
        ratio = np.max(np.abs(dX - ref) / A)
        print(f"kind {kind} D {D} N {N} L {L} M {M} S {S} ldc {ldc}: max err / A = {ratio:.2e}")
        assert ratio <= KERNEL_TOL, (N, L, M, S, ldc)


def test_engine_chunks_the_samples():
    """cap + 1 samples through ``EStepEngine.pathwise_vjp``: two launches, the second with one sample, added on the device; with
    and without the update."""
    p = pkg()
    cap = p._backend.PATHWISE_MAX_S
    kind, N, L, M, D, S = R.MATERN52, 129, 65, 130, 3, cap + 1
    X, Z, inv_ls, variance, Omega, W, V, C = G.problem(kind, N, L, M, D, S, 77)
    eng = p.estep.EStepEngine(torch.float32)  # (the path is fp64 whatever the engine's compute dtype)
    kern = p.Matern52(variance=variance, lengthscales=1.0 / inv_ls)
    for Vc in (V, None):
        dX = eng.pathwise_vjp(_dev(X), _dev(Z), kern, _dev(Omega), _dev(W), None if Vc is None else _dev(Vc), _dev(C))
        assert dX.dtype == torch.float64 and tuple(dX.shape) == (N, D)
        ref = G.vjp(kind, X, Z, inv_ls, variance, Omega, W, Vc, C)
        A = G.magnitude_vjp(kind, X, Z, inv_ls, variance, Omega, W, Vc, C)
        ratio = np.max(np.abs(dX.cpu().numpy() - ref) / A)
        print(f"S {S} update {Vc is not None}: max err / A = {ratio:.2e}")
        assert ratio <= KERNEL_TOL
    with pytest.raises(ValueError, match="32"):
        eng.pathwise_vjp(torch.zeros(4, 33), None, kern, torch.zeros(2, 33), torch.zeros(1, 4), None, torch.zeros(1, 4))
    for bad in (torch.zeros(S, N + 1), torch.zeros(S - 1, N), torch.zeros(N, S), torch.zeros(S, N, 1)):
        with pytest.raises(ValueError, match="C must be"):
            eng.pathwise_vjp(_dev(X), _dev(Z), kern, _dev(Omega), _dev(W), _dev(V), bad)


# ---------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(which, dtype=torch.float64):
    """(model, Z) of ``tests/test_gpu_pathwise.py::_build``, fitted once for the tests here (none of them changes it)."""
    return _build(which, dtype)


def _cotangent(S, N, P, seed=11):
    return np.random.RandomState(seed).randn(S, N, P)


@pytest.mark.parametrize("which,dtype", [("shared", torch.float64), ("separate", torch.float64), ("white", torch.float64),
                                         ("sites", torch.float64), ("shared", torch.float32)])
def test_autograd_matches_the_restated_sampler(which, dtype):
    m, Z = _model(which, dtype)
    seed, draw, L, S = 9, 4, 65, 3
    fs = m.sample_functions(S, L, seed=seed, draw=draw)
    P = int(m.num_latent_gps)
    Xs = _xnew()
    Cw = _cotangent(S, Xs.shape[0], P)
    X = _dev(Xs).requires_grad_()
    f = fs(X)
    assert f.grad_fn is not None and f.requires_grad and tuple(f.shape) == (S, Xs.shape[0], P)
    (f * _dev(Cw)).sum().backward()
    assert X.grad is not None and X.grad.dtype == torch.float64 and tuple(X.grad.shape) == tuple(X.shape)
    ops, kinds, inv_ls, variances = _restated(m, Z, seed, draw, L, S)
    ref = sum(G.vjp(kinds[q], Xs, Z, inv_ls[q], variances[q], ops["Omega"][q], ops["W"][q], ops["V"][q], Cw[:, :, q]) for q in range(P))
    err, scale = np.max(np.abs(X.grad.cpu().numpy() - ref)), 1.0 + np.max(np.abs(ref))
    print(f"{which} {dtype}: max grad err {err:.2e} (max |ref| {scale - 1:.2f})")
    assert err <= MODEL_TOL * scale
    plain = fs(X.detach())
    assert plain.grad_fn is None and not plain.requires_grad
    assert torch.equal(f.detach(), plain)  # the values do not depend on whether a gradient was asked for
    assert torch.equal(fs.vjp(X, _dev(Cw)), X.grad)
    assert torch.equal(fs.vjp(Xs, Cw), X.grad)  # NumPy operands


def test_gradient_is_the_gradient_of_the_draw():
    """No restatement involved: ``X.grad`` against central differences of ``fs`` itself (h = 1e-5) on 16 rows, within 1e-7 A
    with A the size of the gradient's summands on ``fs``'s own operands (summed over the latents)."""
    m, Z = _model("separate")
    S, L, h = 3, 65, 1e-5
    fs = m.sample_functions(S, L, seed=4, draw=1)
    P = int(m.num_latent_gps)
    Xs = _xnew(16, seed=8)
    Xs[3] = Z[5]  # one row on an inducing point
    Cw = _cotangent(S, 16, P, seed=12)
    Cd = _dev(Cw)
    X = _dev(Xs).requires_grad_()
    (fs(X) * Cd).sum().backward()
    fd = np.empty_like(Xs)
    for d in range(Xs.shape[1]):
        e = np.zeros(Xs.shape[1])
        e[d] = h
        fd[:, d] = ((fs(Xs + e) - fs(Xs - e)) * Cd).sum(dim=(0, 2)).cpu().numpy() / (2.0 * h)
    kernels = pkg().kernels.latent_kernels(m.kernel, P)  # (the model was not changed since the draw copied them)
    A = 0.0
    for q, k in enumerate(kernels):
        inv_ls = 1.0 / np.broadcast_to(k.lengthscales.numpy(), (2,))
        A = A + G.magnitude_vjp(k.kind, Xs, Z, inv_ls, k.variance.item(), fs.Omega[q].cpu().numpy(), fs.W[q].cpu().numpy(),
                                fs.V[:, :, q].cpu().numpy(), Cw[:, :, q])
    ratio = np.max(np.abs(X.grad.cpu().numpy() - fd) / A)
    print(f"max |grad - fd| / A = {ratio:.2e}")
    assert ratio <= FD_TOL


def test_gradient_rows_are_independent_and_repeat():
    m, _ = _model("separate")
    S = 3
    fs = m.sample_functions(S, 65, seed=1, draw=2)
    P = int(m.num_latent_gps)
    x1, x2 = _dev(_xnew(130, 1)), _dev(_xnew(257, 2))
    c1, c2 = _dev(_cotangent(S, 130, P, 1)), _dev(_cotangent(S, 257, P, 2))

    def grad(x, c):
        x = x.clone().requires_grad_()
        (fs(x) * c).sum().backward()
        return x.grad

    g1, g2, g12 = grad(x1, c1), grad(x2, c2), grad(torch.cat([x1, x2]), torch.cat([c1, c2], dim=1))
    assert torch.equal(g12[:130], g1) and torch.equal(g12[130:], g2)  # bit for bit on the shared rows
    assert torch.equal(grad(x1, c1), g1)  # a second backward from a fresh forward
    x = x1.clone().requires_grad_()
    with torch.no_grad():
        f = fs(x)
    assert f.grad_fn is None and not f.requires_grad and torch.equal(f, fs(x1))
    fn = fs(x1.cpu().numpy())  # NumPy input: as before
    assert fn.grad_fn is None and torch.equal(fn, fs(x1))
    (g,) = torch.autograd.grad((fs(x) * c1).sum(), x, create_graph=True)
    assert torch.equal(g.detach(), g1)
    with pytest.raises(RuntimeError):
        g.sum().backward()  # once differentiable
    with pytest.raises(ValueError, match="cotangent"):
        fs.vjp(x1, c1[:, :-1])


def test_gradient_reaches_a_cpu_fp32_leaf():
    m, _ = _model("white")
    S = 2
    fs = m.sample_functions(S, 33, seed=6, draw=0)
    leaf = torch.tensor(_xnew(40, 3), dtype=torch.float32, requires_grad=True)  # on the CPU
    c = _dev(_cotangent(S, 40, 1, 5))
    f = fs(leaf)
    assert f.device == m.device and f.dtype == torch.float64 and f.grad_fn is not None
    (f * c).sum().backward()
    assert leaf.grad is not None and leaf.grad.device.type == "cpu" and leaf.grad.dtype == torch.float32
    want = fs.vjp(leaf.detach(), c)  # fp64, at the fp32 rows converted as the call converts them
    assert torch.equal(leaf.grad, want.to(torch.float32).cpu())
    assert float(leaf.grad.abs().max()) > 0.0
