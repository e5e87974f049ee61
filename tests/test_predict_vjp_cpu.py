"""CPU checks of the input gradient of the marginal moments (no GPU): ``tsvgp_moments_vjp_f64/_f32`` are in the built library,
declared, bound and validating; the NumPy restatement tests/predict_vjp_ref.py -- what the GPU tests hold the kernel to -- is the
gradient torch autograd finds through the dense formulas; and the (beta, Q) each model hands to the kernel reproduce the oracle's
``predict_f`` when put through those formulas."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests import predict_vjp_ref as G
from tests.cpu_engine import NumpyShardEngine
from tests.helpers import pkg, relerr, synthetic

NAMES = {"f64": "tsvgp_moments_vjp_f64", "f32": "tsvgp_moments_vjp_f32"}
ARGS = ["kind", "X", "Z", "inv_ls", "variance", "U", "ldu", "cm", "cv", "cstride", "beta", "bstride", "N", "M", "D", "dX", "accumulate",
        "stream"]


def _declared(header, name):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in {header}"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_vjp_symbols_built_declared_and_bound(repo_root, sfx):
    p = pkg()
    B = p._backend
    p.build_library()
    lib = B.lib()
    name = NAMES[sfx]
    assert lib.tsvgp_abi_version() == 5 and B.ABI_VERSION == 5  # new symbols only: the calling conventions did not move
    assert hasattr(lib, name) and name in B.exported_symbols()
    args = _declared(os.path.join(repo_root, "include", "tsvgp_hip.h"), name)
    restype, argtypes = B._PROTOTYPES[name]
    assert restype is ctypes.c_int and len(args) == len(argtypes) == len(ARGS)
    scalar = ctypes.c_double if sfx == "f64" else ctypes.c_float
    for decl, ct in zip(args, argtypes):  # pointers, 64-bit sizes, ints and scalars line up with the header
        want = (ctypes.c_void_p if "*" in decl else ctypes.c_int64 if decl.startswith("int64_t") else
                ctypes.c_int if decl.startswith("int ") else scalar)
        assert ct is want, f"{name}: `{decl}` is bound as {ct.__name__}"
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    assert "double *dX" in args[ARGS.index("dX")]  # fp64 output for both types
    assert [lib.tsvgp_moments_vjp_rows(d) for d in (0, 1, 8, 9, 16, 17, 32, 33)] == [-1, 256, 256, 128, 128, 32, 32, -1]
    assert [lib.tsvgp_moments_vjp_stage_f64(d) for d in (1, 3, 8, 13, 32)] == [1024, 1024, 512, 256, 128]
    assert [lib.tsvgp_moments_vjp_stage_f32(d) for d in (1, 8, 16, 17)] == [1024, 1024, 512, 256]
    assert lib.tsvgp_moments_vjp_stage_f64(0) == -1 and lib.tsvgp_moments_vjp_stage_f32(33) == -1
    for cls in (p.t_SVGP, p.t_SVGP_white, p.t_SVGP_sites):
        assert callable(getattr(cls, "predict_f_vjp", None))
    assert not hasattr(p.t_VGP, "predict_f_vjp")
    assert callable(getattr(p.estep.EStepEngine, "moments_vjp", None)) and callable(getattr(p.estep.EStepEngine, "predict_vjp", None))


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_vjp_argument_validation_needs_no_gpu(sfx):
    """Every refusal of the header, from a call that differs from an accepted one in that single argument.  Fake, aligned, non-null
    pointers that are never dereferenced: none of these calls gets as far as a launch."""
    B = pkg()._backend
    fn = getattr(B.lib(), NAMES[sfx])
    fake, cpl = 4096, (2 if sfx == "f64" else 4)
    good = dict(kind=B.KERNEL_SE, X=fake, Z=fake, inv_ls=fake, variance=1.0, U=fake, ldu=128, cm=fake, cv=fake, cstride=1, beta=fake,
                bstride=1, N=100, M=24, D=3, dX=fake, accumulate=0)

    def call(**kw):
        a = dict(good, **kw)
        return fn(*[a[k] for k in ARGS[:-1]], None)

    bad_cases = [dict(X=None), dict(Z=None), dict(inv_ls=None), dict(U=None), dict(cm=None), dict(cv=None), dict(beta=None),
                 dict(dX=None),  # each pointer
                 dict(N=0), dict(N=-1), dict(M=0), dict(M=-1),
                 dict(D=0), dict(D=33), dict(D=-1),
                 dict(kind=1), dict(kind=4), dict(kind=7), dict(kind=-1),  # 1 is the reserved Matern-1/2
                 dict(ldu=23), dict(ldu=0), dict(M=130),  # ldu < M
                 dict(ldu=128 + cpl // 2), dict(ldu=129),  # a row of U off the 16-byte boundary
                 dict(U=fake + 8), dict(U=fake + 4),  # U itself off it
                 dict(cstride=0), dict(bstride=0), dict(cstride=-1)]
    for bad in bad_cases:
        assert call(**bad) == 1, bad
    # the smallest legal leading dimension is M rounded up to the vector, not the 128 of the engine's buffers
    assert call(ldu=23) == 1 and call(M=24, ldu=24, N=0) == 1


def _torch_profile(kind, s):
    if kind == "se":
        return torch.exp(-0.5 * s)
    r = torch.sqrt(torch.clamp(s, min=1e-36))
    if kind == "matern32":
        a = np.sqrt(3.0) * r
        return (1.0 + a) * torch.exp(-a)
    a = np.sqrt(5.0) * r
    return (1.0 + a + 5.0 / 3.0 * r * r) * torch.exp(-a)


def _problem(N, M, D, P, seed):
    rng = np.random.RandomState(seed)
    X, Z = rng.randn(N, D), rng.randn(M, D)
    ls = (0.7 + rng.rand(D)) * np.sqrt(D)
    beta = rng.randn(M, P)
    R = rng.randn(P, M, M) / np.sqrt(M)
    Q = R @ R.transpose(0, 2, 1)
    cm, cv = rng.randn(N, P), rng.randn(N, P)
    return X, Z, 1.0 / ls, 1.3, beta, Q, cm, cv


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("N,M,D,P", [(37, 11, 1, 1), (50, 24, 3, 2), (9, 40, 8, 1)])
def test_restatement_is_what_autograd_finds_through_the_dense_formulas(kind, N, M, D, P):
    """mean = K beta, var = variance - rowsum((K Q) * K) in torch fp64 on the CPU, differentiated with respect to X by autograd,
    against the restatement: <= 1e-12 relative."""
    X, Z, il, variance, beta, Q, cm, cv = _problem(N, M, D, P, 70 + N + D)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    Xt = t(X).requires_grad_(True)
    sd = (Xt * t(il))[:, None, :] - (t(Z) * t(il))[None, :, :]
    K = variance * _torch_profile(kind, (sd * sd).sum(dim=-1))
    mean = K @ t(beta)
    var = variance - torch.stack([((K @ t(Q[p])) * K).sum(dim=1) for p in range(P)], dim=1)
    (want,) = torch.autograd.grad((mean * t(cm) + var * t(cv)).sum(), Xt)
    got, A = G.predict_vjp(kind, X, Z, il, variance, beta, Q, cm, cv)
    assert got.shape == A.shape == (N, D) and np.all(A > 0)
    e = relerr(got, want.numpy())
    print(f"{kind} N {N} M {M} D {D} P {P}: restatement against autograd, relative {e:.2e}")
    assert e <= 1e-12


@pytest.mark.parametrize("kind", G.KINDS)
def test_restatement_is_an_exact_zero_on_an_inducing_point(kind):
    """A row of X that is a row of Z: that pair's term is 0.0 exactly (s_d = 0 times a finite f', also under the Matern clamp),
    so with that inducing point alone the whole gradient is, and with others present it is theirs."""
    X, Z, il, variance, beta, Q, cm, cv = _problem(6, 5, 3, 1, 11)
    Z[0], Z[3] = X[2], X[4]
    K1 = np.full((6, 1), variance)
    for j, n in ((0, 2), (3, 4)):
        g, A = G.vjp(kind, X[n:n + 1], Z[j:j + 1], il, variance, K1[:1] * 0.7, cm[n:n + 1, 0], cv[n:n + 1, 0], beta[j:j + 1, 0])
        assert np.all(g == 0.0) and np.all(A > 0)
    U = np.random.RandomState(3).randn(6, 5)
    full, _ = G.vjp(kind, X, Z, il, variance, U, cm[:, 0], cv[:, 0], beta[:, 0])
    keep = [1, 2, 3, 4]
    rest, A = G.vjp(kind, X[2:3], Z[keep], il, variance, U[2:3, keep], cm[2:3, 0], cv[2:3, 0], beta[keep, 0])
    assert np.all(np.abs(full[2:3] - rest) <= 8 * 2.0 ** -53 * A)  # (the order of five fp64 additions is all that can differ)


def _dense_moments(kernel, X, Z, beta, Q):
    K = kernel.K(X, Z)
    mean = K @ beta
    var = kernel.variance - np.stack([np.sum((K @ Q[p]) * K, axis=1) for p in range(Q.shape[0])], axis=1)
    return mean, var


def _white_pair(Z, projection):
    p = pkg()
    mk = lambda mod, **kw: mod.t_SVGP_white(mod.SquaredExponential(1.2, 1.5), mod.Bernoulli(), Z, num_data=400, **kw)
    hip = mk(p, device="cpu", projection=projection)
    hip._engine = NumpyShardEngine()  # test double: the HIP engine cannot exist without a GPU
    return hip, mk(O)


@pytest.mark.parametrize("route", ["direct", "whitened", "two_product"])
def test_white_operands_of_every_route_reproduce_the_oracle(route):
    """(beta, Q) as ``t_SVGP_white._predict_operands`` hands them to the kernel, put through mean = K beta and
    var = variance - rowsum((K Q) * K): the oracle's ``predict_f`` to 1e-9.  Host algebra only."""
    rng = np.random.RandomState(5)
    X, Y, _ = synthetic(N=250, M=20, D=3, P=1, lik="bernoulli", seed=8)
    Z = rng.randn(20, 3) * 1.6
    hip, ora = _white_pair(Z, "whitened" if route == "two_product" else route)
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.7)
        ora.natgrad_step((X, Y), lr=0.7)
    if route == "two_product":
        hip._two_product = True
    seen = []
    inner = hip._operands
    hip._operands = lambda *a, **k: (seen.append((k.get("direct"), k.get("two_product"))), inner(*a, **k))[1]
    beta, Q = hip._predict_operands()
    assert seen[-1] == {"direct": (True, False), "whitened": (False, False), "two_product": (False, True)}[route]
    assert tuple(beta.shape) == (20, 1) and tuple(Q.shape) == (1, 20, 20)
    assert relerr(Q[0].numpy(), Q[0].numpy().T) <= 1e-9
    Xn = X[:40] + 0.1
    mean, var = _dense_moments(ora.kernel, Xn, Z, beta.numpy(), Q.numpy())
    mo, vo = ora.predict_f(Xn)
    em, ev = relerr(mean, mo), relerr(var, vo)
    print(f"t_SVGP_white {route}: mean {em:.2e} var {ev:.2e}")
    assert em <= 1e-9 and ev <= 1e-9
    if route != "two_product":  # (the NumPy engine has no two-product pass: tests/test_gpu_predict_grad.py runs that forward)
        mh, vh = hip.predict_f(Xn)  # the forward the operands belong to takes the same route
        assert seen[-1] == seen[0] and relerr(mh.numpy(), mo) <= 1e-9 and relerr(vh.numpy(), vo) <= 1e-9


@pytest.mark.parametrize("P,separate", [(1, False), (2, False), (2, True)])
def test_tsvgp_operands_reproduce_the_oracle(P, separate):
    p = pkg()
    X, Y, Z = synthetic(N=300, M=24, D=3, P=P, lik="bernoulli", seed=2)

    def mk(mod, **kw):
        if separate:
            kern = mod.SeparateIndependent([mod.SquaredExponential(1.0, 1.2), mod.SquaredExponential(0.8, 1.7)])
            return mod.t_SVGP(kern, mod.Bernoulli(), mod.SharedIndependentInducingVariables(Z), num_latent_gps=P, **kw)
        return mod.t_SVGP(mod.SquaredExponential(1.1, 1.4), mod.Bernoulli(), Z, num_latent_gps=P, **kw)

    hip, ora = mk(p, device="cpu"), mk(O)
    hip._engine = NumpyShardEngine()
    for _ in range(3):
        hip.natgrad_step((X, Y), lr=0.7)
        ora.natgrad_step((X, Y), lr=0.7)
    beta, Q = hip._predict_operands()
    assert tuple(beta.shape) == (24, P) and tuple(Q.shape) == (P, 24, 24)
    Xn = X[:40] + 0.1
    mo, vo = ora.predict_f(Xn)
    kernels = ora.kernel.kernels if separate else [ora.kernel] * P
    for q in range(P):
        mean, var = _dense_moments(kernels[q], Xn, Z, beta.numpy()[:, q:q + 1], Q.numpy()[q:q + 1])
        assert relerr(mean, mo[:, q:q + 1]) <= 1e-9 and relerr(var, vo[:, q:q + 1]) <= 1e-9


def test_predict_f_vjp_is_unreachable_without_gpu():
    """No CPU fallback: without a ROCm device the engine cannot be made, so neither the vjp nor a differentiable forward runs."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = pkg()
    m = p.t_SVGP(p.SquaredExponential(), p.Gaussian(0.1), np.zeros((4, 2)) + np.arange(4)[:, None])
    X = torch.zeros((5, 2), dtype=torch.float64, requires_grad=True)
    with pytest.raises(p.HipExtensionError):
        m.predict_f_vjp(X, torch.ones(5, 1))
    with pytest.raises(p.HipExtensionError):
        m.predict_f(X)
    with pytest.raises(ValueError):
        p.t_SVGP(p.SquaredExponential(), p.Gaussian(0.1), np.zeros((4, 33)) + np.arange(4)[:, None]).predict_f_vjp(
            np.zeros((5, 33)), np.ones((5, 1)))
