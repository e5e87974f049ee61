"""GPU checks of ``select_inducing_points`` / ``tsvgp_greedy_select_f64`` against the dense Nystrom residual (tests/select_ref.py).

Index parity with the NumPy restatement is NOT asserted: far-apart points keep d within an ulp of ``variance``, and an fp64 and a
long-double run of the same NumPy code already pick different points on (1000, 3, 64, SE).  The assertions define correctness
without depending on which of two rounding-level ties wins.

Tolerance: 1e-11 * variance throughout.  On these problems the restatement's smallest pivot is >= 0.37 * variance and it meets
the Nystrom identity to <= 1.3e-15 * variance (tests/test_select_cpu.py); the a-priori bound count * eps * variance / min pivot is
4e-14, so 1e-11 leaves over two orders above it for a different summation order and a 1-ulp exp.
"""
import numpy as np
import pytest

from tests import select_ref as R
from tests.helpers import pkg

pytestmark = pytest.mark.gpu

KERNEL_NAMES = {R.SE: "SquaredExponential", R.MATERN32: "Matern32", R.MATERN52: "Matern52"}
IDS = ["N{}_D{}_M{}_k{}".format(*c[:4]) for c in R.PROBLEMS]


def make_kernel(kind, inv_ls0, variance):
    """(package kernel, the inv_ls it will hand the HIP entry): lengthscales = 1 / inv_ls0, inverted again as the package does."""
    ls = 1.0 / np.asarray(inv_ls0, dtype=np.float64)
    return getattr(pkg(), KERNEL_NAMES[kind])(variance=variance, lengthscales=ls), 1.0 / ls


def to_np(sel):
    return (sel.indices.cpu().numpy(), sel.pivots.cpu().numpy(), sel.residual.cpu().numpy())


@pytest.fixture(scope="module")
def runs():
    """One selection per problem, shared (read-only) by the tests below: (X, inv_ls, kernel, sel, indices, pivots, residual)."""
    out = []
    for case in R.PROBLEMS:
        N, D, M, kind, ls, seed = case
        X, inv_ls0 = R.problem(*case)
        kernel, inv_ls = make_kernel(kind, inv_ls0, R.VARIANCE)
        sel = pkg().select_inducing_points(X, kernel, M)
        out.append((X, inv_ls, kernel, sel) + to_np(sel))
    return out


@pytest.mark.parametrize("k", range(len(R.PROBLEMS)), ids=IDS)
def test_nystrom_identity(runs, k):
    N, D, M, kind, ls, seed = R.PROBLEMS[k]
    X, inv_ls, kernel, sel, idx, piv, res = runs[k]
    tol = 1e-11 * R.VARIANCE
    assert sel.count == min(M, N) == len(idx) == len(piv) and res.shape == (N,)
    assert tuple(sel.Z.shape) == (sel.count, D) and np.array_equal(sel.Z.cpu().numpy(), X[idx])
    assert idx.dtype == np.int64 and len(set(idx.tolist())) == sel.count and idx.min() >= 0 and idx.max() < N
    ref = np.maximum(R.nystrom_residual(X, idx, inv_ls, R.VARIANCE, kind), 0.0)
    err = float(np.max(np.abs(res - ref)))
    print(f"{IDS[k]}: |residual - nystrom| = {err:.3e} (tol {tol:.3e}), min pivot {piv.min():.4f}")
    assert err <= tol
    assert sel.trace.dim() == 0 and float(sel.trace) == float(sel.residual.sum())
    assert np.all(res[idx] == 0.0)


@pytest.mark.parametrize("k", range(len(R.PROBLEMS)), ids=IDS)
def test_greedy_within_rounding(runs, k):
    N, D, M, kind, ls, seed = R.PROBLEMS[k]
    X, inv_ls, kernel, sel, idx, piv, res = runs[k]
    tol = 1e-11 * R.VARIANCE
    for j in sorted(set(np.linspace(0, sel.count - 1, 8).astype(int).tolist())):
        t = R.nystrom_residual(X, idx[:j], inv_ls, R.VARIANCE, kind)
        print(f"{IDS[k]} step {j}: max - picked = {t.max() - t[idx[j]]:.3e}, |pivot - picked| = {abs(piv[j] - t[idx[j]]):.3e}")
        assert t[idx[j]] >= t.max() - tol
        assert abs(piv[j] - t[idx[j]]) <= tol


@pytest.mark.parametrize("k", range(len(R.PROBLEMS)), ids=IDS)
def test_pivots_are_the_squared_cholesky_diagonal_of_kuu(runs, k):
    import torch

    X, inv_ls, kernel, sel, idx, piv, res = runs[k]
    tol = 1e-11 * R.VARIANCE
    engine = pkg().estep.EStepEngine(torch.float64)
    L = torch.linalg.cholesky(engine.kuu(sel.Z, kernel))
    diag2 = (torch.diagonal(L) ** 2).cpu().numpy()
    print(f"{IDS[k]}: |diag(chol Kuu)^2 - pivots| = {np.max(np.abs(diag2 - piv)):.3e}")
    assert np.max(np.abs(diag2 - piv)) <= tol
    assert np.all(np.diff(piv) <= tol)


@pytest.mark.parametrize("k", range(len(R.PROBLEMS)), ids=IDS)
def test_first_pick_is_row_zero(runs, k):
    """All d start exactly equal and the lowest index wins; the first pivot is the prior variance itself."""
    X, inv_ls, kernel, sel, idx, piv, res = runs[k]
    assert idx[0] == 0 and piv[0] == R.VARIANCE
    if X.shape[0] == 1:
        assert sel.count == 1


@pytest.mark.parametrize("k", [3, 4], ids=[IDS[3], IDS[4]])
def test_exhaustion(k):
    N, D, M, kind, ls, seed = R.PROBLEMS[k]
    X, inv_ls0 = R.problem(*R.PROBLEMS[k])
    kernel, _ = make_kernel(kind, inv_ls0, R.VARIANCE)
    sel = pkg().select_inducing_points(X, kernel, 500)
    idx = sel.indices.cpu().numpy()
    assert sel.count <= N and len(idx) == sel.count and len(set(idx.tolist())) == sel.count
    assert tuple(sel.residual.shape) == (N,)


def test_duplicates_are_never_taken_twice():
    N, D, M, kind, ls, seed = R.PROBLEMS[4]
    X, inv_ls0 = R.problem(*R.PROBLEMS[4])
    X2 = np.concatenate([X[:64], X[:64]])
    kernel, _ = make_kernel(kind, inv_ls0, R.VARIANCE)
    sel = pkg().select_inducing_points(X2, kernel, 128)
    idx = sel.indices.cpu().numpy()
    assert sel.count == 64
    assert len(set((idx % 64).tolist())) == 64  # no row together with its copy


def test_threshold():
    X = np.random.RandomState(3).randn(1000, 1)
    thr = 1e-6 * R.VARIANCE
    kernel, _ = make_kernel(R.SE, np.array([1.0 / 0.3]), R.VARIANCE)
    sel = pkg().select_inducing_points(X, kernel, 64, threshold=thr)
    piv = sel.pivots.cpu().numpy()
    print(f"threshold: count = {sel.count}, last pivot {piv[-1]:.3e}, residual max {float(sel.residual.max()):.3e}")
    assert 1 <= sel.count <= 64 and np.all(piv > thr)
    if sel.count < 64:
        assert float(sel.residual.max()) <= thr


@pytest.mark.parametrize("k", [2, 4, 5], ids=[IDS[2], IDS[4], IDS[5]])
def test_two_calls_agree_bit_for_bit(runs, k):
    N, D, M, kind, ls, seed = R.PROBLEMS[k]
    X, inv_ls, kernel, sel, idx, piv, res = runs[k]
    idx2, piv2, res2 = to_np(pkg().select_inducing_points(X, kernel, M))
    assert np.array_equal(idx, idx2) and np.array_equal(piv, piv2) and np.array_equal(res, res2)


def test_better_than_the_first_rows_on_clustered_data():
    """1000 points of which the first 200 sit in a cluster of width 0.05: Z = X[:64] leaves tr(K_ff - Q_ff) = 68.4, the
    restatement's selection 0.141."""
    rng = np.random.RandomState(7)
    X = rng.randn(1000, 2)
    X[:200] = 0.05 * rng.randn(200, 2)
    kernel, inv_ls = make_kernel(R.SE, np.ones(2), 1.0)
    sel = pkg().select_inducing_points(X, kernel, 64)
    first = float(R.nystrom_residual(X, range(64), inv_ls, 1.0, R.SE).sum())
    print(f"trace: selected {float(sel.trace):.4f}, first 64 rows {first:.4f}")
    assert sel.count == 64 and float(sel.trace) < 0.1 * first


def test_selection_feeds_a_model():
    p = pkg()
    rng = np.random.RandomState(0)
    X = rng.randn(500, 2)
    Y = np.sin(X @ rng.randn(2, 1)) + np.sqrt(0.1) * rng.randn(500, 1)
    kernel = p.SquaredExponential(variance=1.0, lengthscales=1.0)
    sel = p.select_inducing_points(X, kernel, 32)
    model = p.t_SVGP(kernel, p.Gaussian(0.1), sel.Z)
    model.natgrad_step((X, Y), lr=0.8)
    assert np.isfinite(float(model.elbo((X, Y))))
    assert p.InducingPoints(sel.Z).num_inducing == sel.count
