"""CPU checks of the input gradient of the pathwise function draws (no GPU): ``tsvgp_pathwise_vjp_f64`` is in the built library,
declared, bound and validating; the NumPy restatement tests/pathwise_vjp_ref.py -- what the GPU tests hold the kernel and the
models to -- is the gradient of ``pathwise_ref.evaluate`` (central differences) and is accurate to fp64 rounding of its summands
(the same arithmetic in extended precision)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import pathwise_ref as R
from tests import pathwise_vjp_ref as G
from tests.helpers import pkg

KINDS = [R.SE, R.MATERN32, R.MATERN52]
DS = [1, 3, 32]
SHAPES = [(1, 257, 130, 16), (127, 63, 0, 1), (129, 65, 1, 3), (257, 1, 127, 16)]  # (N, L, M, S)
NAME = "tsvgp_pathwise_vjp_f64"


def _declared(header, name):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in {header}"
    return [a.strip() for a in m.group(1).split(",")]


def test_vjp_symbol_built_declared_and_bound(repo_root):
    p = pkg()
    B = p._backend
    p.build_library()
    lib = B.lib()
    assert lib.tsvgp_abi_version() == 5 and B.ABI_VERSION == 5  # a new symbol only: the calling conventions did not move
    header = os.path.join(repo_root, "include", "tsvgp_hip.h")
    assert hasattr(lib, NAME), f"{NAME} is not exported by the built library"
    assert NAME in B.exported_symbols()
    args = _declared(header, NAME)
    restype, argtypes = B._PROTOTYPES[NAME]
    assert restype is ctypes.c_int and len(args) == len(argtypes) == 17
    for decl, ct in zip(args, argtypes):  # pointers, 64-bit sizes, ints and scalars line up with the header
        want = (ctypes.c_void_p if "*" in decl else ctypes.c_int64 if decl.startswith("int64_t") else
                ctypes.c_int if decl.startswith("int ") else ctypes.c_double)
        assert ct is want, f"{NAME}: `{decl}` is bound as {ct.__name__}"
    assert [a.split()[-1].lstrip("*") for a in args] == ["kind", "X", "Z", "inv_ls", "variance", "Omega", "W", "V", "C", "ldc", "dX", "N",
                                                         "M", "L", "D", "S", "stream"]
    assert callable(getattr(p.FunctionSamples, "vjp", None))
    assert callable(getattr(p.estep.EStepEngine, "pathwise_vjp", None))


def test_vjp_argument_validation_needs_no_gpu():
    """Every refusal of the header, from a call that differs from an accepted one in that single argument.  Fake, aligned, non-null
    pointers that are never dereferenced: none of these calls gets as far as a launch."""
    B = pkg()._backend
    fn = getattr(B.lib(), NAME)
    fake = 4096
    good = dict(kind=B.KERNEL_SE, X=fake, Z=fake, inv_ls=fake, variance=1.0, Omega=fake, W=fake, V=fake, C=fake, ldc=100, dX=fake, N=100,
                M=8, L=16, D=2, S=3)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["kind"], a["X"], a["Z"], a["inv_ls"], a["variance"], a["Omega"], a["W"], a["V"], a["C"], a["ldc"], a["dX"], a["N"],
                  a["M"], a["L"], a["D"], a["S"], None)

    for bad in (dict(X=None), dict(inv_ls=None), dict(Omega=None), dict(W=None), dict(C=None), dict(dX=None),  # each required pointer
                dict(V=None), dict(Z=None),  # required with M > 0
                dict(N=0), dict(N=-1), dict(L=0), dict(L=-1), dict(M=-1),
                dict(D=0), dict(D=33), dict(D=-1),
                dict(S=0), dict(S=-1), dict(S=B.PATHWISE_MAX_S + 1),
                dict(ldc=99), dict(ldc=0),
                dict(variance=0.0), dict(variance=-1.0), dict(variance=float("nan")), dict(variance=float("inf")),
                dict(kind=1), dict(kind=4), dict(kind=-1), dict(kind=7)):  # 1 is the reserved Matern-1/2
        assert call(**bad) == 1, bad
    # M = 0 makes V and Z optional, and nothing else: the call with them absent gets as far as the other checks
    free = dict(M=0, V=None, Z=None)
    for bad in (dict(C=None), dict(dX=None), dict(X=None), dict(S=0), dict(D=33), dict(L=0), dict(ldc=99), dict(kind=1)):
        assert call(**free, **bad) == 1, bad


def _seed(kind, D, j):
    return 500 + 10 * (KINDS.index(kind) * 3 + DS.index(D)) + j


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_is_the_gradient_of_the_restated_evaluation(kind, D):
    """Central differences of ``pathwise_ref.evaluate`` with h = 1e-5 in every row and dimension (a row's values depend on that
    row alone, so one pair of evaluations moves dimension d of all rows), contracted with C.  Bound 1e-7 A: the truncation is
    h^2 / 6 times third derivatives (1e-11 times |Omega|^3-weighted summands) and the rounding eps / h = 1e-11 times the
    evaluation's own summands; both are a few 1e-10 A at the worst of these inputs."""
    h = 1e-5
    for j, (N, L, M, S) in enumerate(SHAPES):
        X, Z, inv_ls, variance, Omega, W, V, C = G.problem(kind, N, L, M, D, S, _seed(kind, D, j))
        ref, A = G.problem_vjp(kind, N, L, M, D, S, _seed(kind, D, j))
        assert ref.shape == A.shape == (N, D) and np.all(A > 0)
        fd = np.empty((N, D))
        for d in range(D):
            e = np.zeros(D)
            e[d] = h
            up, dn = (R.evaluate(kind, X + sgn * e, Z, inv_ls, variance, Omega, W, V) for sgn in (1.0, -1.0))
            fd[:, d] = np.sum(C * (up - dn), axis=0) / (2.0 * h)
        ratio = np.max(np.abs(fd - ref) / A)
        print(f"kind {kind} D {D} N {N} L {L} M {M} S {S}: max |fd - vjp| / A = {ratio:.2e}")
        assert ratio <= 1e-7, (N, L, M, S)
        if M > 0:  # the rows on an inducing point are there, and their own term is an exact zero
            on = np.flatnonzero(np.all((X * inv_ls)[:, None, :] == (Z * inv_ls)[None, :, :], axis=2).any(axis=1))
            assert on.size >= 1


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_is_accurate_to_the_rounding_of_its_summands(kind, D):
    """The fp64 restatement against the same arithmetic in np.longdouble: <= 1e-12 A.  This is what makes 1e-11 A a fair bound
    for the kernel against the fp64 restatement; if it fails, ``magnitude_vjp`` is missing a term."""
    for j, (N, L, M, S) in enumerate(SHAPES):
        args = G.problem(kind, N, L, M, D, S, _seed(kind, D, j))
        ref, A = G.problem_vjp(kind, N, L, M, D, S, _seed(kind, D, j))
        wide = G.vjp(kind, *args, dtype=np.longdouble)
        assert wide.dtype == np.longdouble
        ratio = float(np.max(np.abs(wide - ref) / A))
        print(f"kind {kind} D {D} N {N} L {L} M {M} S {S}: max |fp64 - longdouble| / A = {ratio:.2e}")
        assert ratio <= 1e-12, (N, L, M, S)


def test_vjp_is_unreachable_without_gpu():
    """No CPU fallback: without a ROCm device ``sample_functions`` already raises, so there is no object to differentiate."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = pkg()
    Z = np.zeros((4, 2)) + np.arange(4)[:, None]
    m = p.t_SVGP(p.SquaredExponential(), p.Gaussian(0.1), Z)
    with pytest.raises(p.HipExtensionError):
        m.sample_functions(2, 16)
    assert m._function_draw == 0
