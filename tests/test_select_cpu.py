"""CPU checks around the greedy conditional-variance selection of inducing points: the NumPy restatement (tests/select_ref.py)
against the dense Nystrom residual, the argument errors of ``select_inducing_points`` (raised before any engine exists), the
export, and the C-ABI seam (symbols, ABI number, parameter checks in front of any launch)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import select_ref as R
from tests.helpers import pkg


@pytest.mark.parametrize("case", R.PROBLEMS, ids=lambda c: "N{}_D{}_M{}_k{}".format(*c[:4]))
def test_restatement_meets_the_nystrom_identity(case):
    """On the GPU test's six problems the restatement's residual is the Nystrom residual of its own picks, its pivots are the
    residuals at the moment of the pick and the squared diagonal of chol K(Z, Z), and its smallest pivot stays far from the
    floor -- what the GPU test's tolerance 1e-11 * variance is derived from (count * eps * variance / min pivot <= 4e-14)."""
    N, D, M, kind, ls, seed = case
    X, inv_ls = R.problem(*case)
    v = R.VARIANCE
    idx, piv, d, count = R.greedy_select(X, inv_ls, v, kind, M)
    assert count == min(M, N) and len(set(idx.tolist())) == count and idx[0] == 0
    tol = 1e-11 * v
    assert np.max(np.abs(d - np.maximum(R.nystrom_residual(X, idx, inv_ls, v, kind), 0.0))) <= tol
    assert np.all(d[idx] == 0.0)
    assert piv.min() >= 0.3 * v
    assert count * np.finfo(np.float64).eps * v / piv.min() <= 1e-13
    L = np.linalg.cholesky(R.kmat(kind, X[idx], X[idx], inv_ls, v))
    assert np.max(np.abs(np.diag(L) ** 2 - piv)) <= tol
    assert np.all(np.diff(piv) <= tol)
    for j in sorted(set(np.linspace(0, count - 1, 8).astype(int).tolist())):
        t = R.nystrom_residual(X, idx[:j], inv_ls, v, kind)
        assert t[idx[j]] >= t.max() - tol and abs(piv[j] - t[idx[j]]) <= tol


def test_restatement_skips_duplicates_and_honours_the_threshold():
    case = R.PROBLEMS[4]
    X, inv_ls = R.problem(*case)
    X2 = np.concatenate([X[:64], X[:64]])
    idx, piv, d, count = R.greedy_select(X2, inv_ls, R.VARIANCE, case[3], 128)
    assert count == 64 and len(set((idx % 64).tolist())) == 64
    X1 = np.random.RandomState(3).randn(1000, 1)
    thr = 1e-6 * R.VARIANCE
    idx, piv, d, count = R.greedy_select(X1, np.array([1.0 / 0.3]), R.VARIANCE, R.SE, 64, threshold=thr)
    assert count < 64 and np.all(piv > thr) and d.max() <= thr


def test_argument_errors_need_no_gpu():
    p = pkg()
    k = p.SquaredExponential(variance=1.0, lengthscales=1.0)
    X = np.random.RandomState(0).randn(10, 2)
    with pytest.raises(ValueError, match="SeparateIndependent"):
        p.select_inducing_points(X, p.SeparateIndependent([k, k]), 4)
    with pytest.raises(ValueError, match="32"):
        p.select_inducing_points(np.zeros((10, 33)), k, 4)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="num_inducing"):
            p.select_inducing_points(X, k, bad)
    for empty in (np.zeros((0, 2)), np.zeros((5, 0)), np.zeros(5)):
        with pytest.raises(ValueError, match="non-empty"):
            p.select_inducing_points(empty, k, 4)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="threshold"):
            p.select_inducing_points(X, k, 4, threshold=bad)


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = pkg()
    with pytest.raises(p.HipExtensionError):
        p.select_inducing_points(np.zeros((10, 2)) + np.arange(10)[:, None], p.SquaredExponential(), 4)


def test_name_is_exported():
    p = pkg()
    assert "select_inducing_points" in p.__all__ and callable(p.select_inducing_points)
    assert "InducingSelection" in p.__all__
    assert hasattr(p.estep.EStepEngine, "greedy_select")


def test_header_and_bindings_carry_the_symbols_with_abi_5(repo_root):
    B = pkg()._backend
    header = open(os.path.join(repo_root, "include", "tsvgp_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("tsvgp_greedy_select_f64", "tsvgp_greedy_select_work_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/tsvgp_hip.h"
        assert name in B.exported_symbols()
    assert re.search(r"#define\s+TSVGP_ABI_VERSION\s+5\b", header) and B.ABI_VERSION == 5
    # the prototype has one ctypes entry per declared parameter
    decl = re.search(r"int\s+tsvgp_greedy_select_f64\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(decl.split(",")) == len(B._PROTOTYPES["tsvgp_greedy_select_f64"][1]) == 16
    lib = B.lib()
    assert lib.tsvgp_abi_version() == 5 and hasattr(lib, "tsvgp_greedy_select_f64")


def test_entry_rejects_bad_parameters_before_any_launch():
    """Every call below fails a parameter check, so nothing is launched and the host buffers are never read."""
    lib = pkg()._backend.lib()
    assert lib.tsvgp_greedy_select_work_bytes(1, 1) == 32 + 8 * (1 + 2)
    assert lib.tsvgp_greedy_select_work_bytes(1000000, 1024) == 32 + 8 * (1024 + 2 * 7813)
    assert lib.tsvgp_greedy_select_work_bytes(0, 4) == -1 and lib.tsvgp_greedy_select_work_bytes(4, 0) == -1
    buf = (ctypes.c_double * 1024)()  # 16-byte aligned by the allocator; stands in for every pointer
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert ctypes.addressof(buf) % 16 == 0

    def call(kind=0, variance=1.0, floor=0.0, ldc=128, N=100, M=4, D=2, X=ptr, C=ptr):
        return lib.tsvgp_greedy_select_f64(kind, X, ptr, variance, floor, C, ldc, ptr, ptr, ptr, ptr, ptr, N, M, D, None)

    assert call(X=None) == 1 and call(C=None) == 1
    assert call(N=0) == 1 and call(M=0) == 1 and call(D=0) == 1 and call(D=33) == 1
    assert call(variance=0.0) == 1 and call(variance=-1.0) == 1 and call(variance=math.nan) == 1 and call(variance=math.inf) == 1
    assert call(floor=-1e-300) == 1 and call(floor=math.nan) == 1 and call(floor=math.inf) == 1
    assert call(kind=1) == 1 and call(kind=7) == 1
    assert call(ldc=100) == 1 and call(N=129, ldc=128) == 1 and call(N=129, ldc=257) == 1  # ldc >= Np and even
    assert call(C=ctypes.c_void_p(ptr.value + 8)) == 1  # 16-byte boundary
