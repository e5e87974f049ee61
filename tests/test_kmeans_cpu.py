"""CPU checks around ``kmeans_inducing_points``: the NumPy restatement (tests/kmeans_ref.py) itself, the export, the C-ABI seam
(symbols, one ctypes entry per parameter, ABI number, parameter checks in front of any launch) and every ``ValueError`` of the
public function (raised before any engine exists)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import kmeans_ref as R
from tests.helpers import pkg

LS = np.array([1.0, 0.7, 1.6])
ENTRIES = ("tsvgp_kmeans_assign_f64", "tsvgp_kmeans_update_f64")
HELPERS = ("tsvgp_kmeans_assign_parts", "tsvgp_kmeans_assign_rows", "tsvgp_kmeans_assign_chunk")


@pytest.mark.parametrize("seed,n_iter", [(0, 15), (1, 21), (2, 11)])
def test_restatement_descends_and_stops_on_unchanged_labels(seed, n_iter):
    """The figures the GPU test's exact label comparison stands on: iterations, the smallest relative gap, the smallest count."""
    X, _, _ = R.blobs(seed)
    r = R.lloyd(X, 12, lengthscales=LS)
    assert r.converged and r.n_iter == n_iter and r.inertia_history.shape == (n_iter,)
    assert np.all(np.diff(r.inertia_history) <= 0.0)
    assert r.inertia == r.inertia_history[-1]  # it ended on unchanged labels: no extra pass
    assert r.min_gap >= 1.4e-5 and r.counts.min() >= 102 and r.counts.sum() == 3000
    assert np.array_equal(r.counts, np.bincount(r.labels, minlength=12))
    # the returned Z is the mean of the returned labels
    for m in range(12):
        assert np.allclose(r.Z[m], X[r.labels == m].mean(axis=0), rtol=1e-13, atol=0)


def test_restatement_recovers_well_separated_blobs():
    X, centres, which = R.blobs(5, N=1200, sigma=0.05, spread=6.0)
    first = np.array([int(np.nonzero(which == k)[0][0]) for k in range(6)])  # one row of every blob as the start
    r = R.lloyd(X, 6, init=X[first])
    assert r.converged and np.array_equal(r.labels, which)
    assert np.max(np.abs(r.Z - centres)) <= 5 * 0.05 / np.sqrt(r.counts.min())
    assert r.n_iter == 2  # one update, then the labels repeat


def test_restatement_tie_goes_to_the_lowest_index():
    C = np.array([[0.0, 0.0], [1.0, 1.0], [5.0, 5.0], [1.0, 1.0]])
    X = np.array([[1.0, 1.0], [0.5, 0.5], [3.0, 3.0], [0.9, 1.2]])  # on centres 1 = 3; midway 0 / 1; midway 1 / 2; nearest 1 = 3
    labels, best, second, E = R.assign(X, C, np.ones(2))
    assert labels.tolist() == [1, 0, 1, 1] and best[0] == 0.0 and second[0] == 0.0 and second[1] == best[1]
    assert E.shape == (4, 4) and np.all(E >= 0) and E[0, 1] == 0.0


def test_restatement_empty_cluster_keeps_its_centre():
    X, _, _ = R.blobs(3, N=600)
    init = X[:8].copy()
    init[5] = [1e3, -1e3, 1e3]
    r = R.lloyd(X, 8, init=init, lengthscales=LS)
    assert r.counts[5] == 0 and np.array_equal(r.Z[5], init[5]) and r.counts.sum() == 600
    r1 = R.lloyd(X, 8, init=init, lengthscales=LS, max_iter=1)
    assert r1.n_iter == 1 and not r1.converged and np.array_equal(r1.labels, R.assign(X, r1.Z, 1.0 / LS)[0])
    # the tolerance stop: centres that move by less than tol count as converged, with labels that belong to the returned Z
    rt = R.lloyd(X, 8, init=init, lengthscales=LS, tol=0.05)
    assert rt.converged and rt.n_iter <= r.n_iter and np.array_equal(rt.labels, R.assign(X, rt.Z, 1.0 / LS)[0])


def test_names_are_exported():
    p = pkg()
    assert "kmeans_inducing_points" in p.__all__ and callable(p.kmeans_inducing_points)
    assert "KMeansInducing" in p.__all__ and isinstance(p.KMeansInducing, type)
    assert hasattr(p.estep.EStepEngine, "kmeans_assign") and hasattr(p.estep.EStepEngine, "kmeans_update")
    fields = list(p.KMeansInducing.__dataclass_fields__)
    assert fields == ["Z", "labels", "counts", "inertia", "inertia_history", "n_iter", "converged"]


def test_header_and_bindings_carry_the_symbols_with_abi_5(repo_root):
    B = pkg()._backend
    header = open(os.path.join(repo_root, "include", "tsvgp_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = B.lib()
    for name in ENTRIES + HELPERS:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/tsvgp_hip.h"
        assert name in B.exported_symbols() and hasattr(lib, name)
    assert re.search(r"#define\s+TSVGP_ABI_VERSION\s+5\b", header) and B.ABI_VERSION == 5 and lib.tsvgp_abi_version() == 5
    for name, nargs in zip(ENTRIES, (10, 9)):  # the prototype has one ctypes entry per declared parameter
        decl = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(B._PROTOTYPES[name][1]) == nargs
    assert "(12) Lloyd's k-means" in header


def test_sizing_helpers():
    lib = pkg()._backend.lib()
    chunk = lib.tsvgp_kmeans_assign_chunk()
    assert chunk >= 1
    for D in range(1, 33):
        rows = lib.tsvgp_kmeans_assign_rows(D)
        assert rows >= 64 and rows % 64 == 0
        assert lib.tsvgp_kmeans_assign_parts(1, D) == 1 and lib.tsvgp_kmeans_assign_parts(rows, D) == 1
        assert lib.tsvgp_kmeans_assign_parts(rows + 1, D) == 2
        assert lib.tsvgp_kmeans_assign_parts(1000000, D) == -(-1000000 // rows)
    assert lib.tsvgp_kmeans_assign_rows(0) == -1 and lib.tsvgp_kmeans_assign_rows(33) == -1
    assert lib.tsvgp_kmeans_assign_parts(0, 4) == -1 and lib.tsvgp_kmeans_assign_parts(10, 0) == -1
    assert lib.tsvgp_kmeans_assign_parts(10, 33) == -1
    assert lib.tsvgp_kmeans_assign_parts(lib.tsvgp_kmeans_assign_rows(8) * (2 ** 31 - 1) + 1, 8) == -1


def test_entries_reject_bad_parameters_before_any_launch():
    """Every call below fails a parameter check, so nothing is launched and the host buffers are never read."""
    lib = pkg()._backend.lib()
    buf = (ctypes.c_double * 1024)()  # 16-byte aligned by the allocator; stands in for every pointer
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert ctypes.addressof(buf) % 16 == 0
    off = lambda k: ctypes.c_void_p(ptr.value + k)

    def assign(X=ptr, C=ptr, il=ptr, labels=ptr, dist=ptr, part=ptr, N=100, M=4, D=2):
        return lib.tsvgp_kmeans_assign_f64(X, C, il, labels, dist, part, N, M, D, None)

    def update(X=ptr, order=ptr, offsets=ptr, C_old=ptr, C_new=ptr, N=100, M=4, D=2):
        return lib.tsvgp_kmeans_update_f64(X, order, offsets, C_old, C_new, N, M, D, None)

    for name in ("X", "C", "il", "labels", "dist", "part"):
        assert assign(**{name: None}) == 1, name
    for name in ("X", "order", "offsets", "C_old", "C_new"):
        assert update(**{name: None}) == 1, name
    for call in (assign, update):
        assert call(N=0) == 1 and call(N=-5) == 1 and call(M=0) == 1 and call(M=-1) == 1
        assert call(D=0) == 1 and call(D=33) == 1 and call(D=-2) == 1
    # every buffer on the boundary of its element type: doubles and int64 on 8 bytes, the int32 labels on 4
    for name in ("X", "C", "il", "dist", "part"):
        assert assign(**{name: off(4)}) == 1, name
    assert assign(labels=off(2)) == 1
    for name in ("X", "order", "offsets", "C_old", "C_new"):
        assert update(**{name: off(4)}) == 1, name


def test_argument_errors_need_no_gpu():
    p = pkg()
    km = p.kmeans_inducing_points
    X = np.random.RandomState(0).randn(10, 2)
    for empty in (np.zeros((0, 2)), np.zeros((5, 0)), np.zeros(5), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match="non-empty"):
            km(empty, 4)
    with pytest.raises(ValueError, match="32"):
        km(np.zeros((40, 33)), 4)
    for bad in (0, -3, 2.5, 11):
        with pytest.raises(ValueError, match="num_inducing"):
            km(X, bad)
    for bad in (np.zeros((4, 3)), np.zeros((5, 2)), np.zeros(4), np.zeros((4, 2, 1))):
        with pytest.raises(ValueError, match="init"):
            km(X, 4, init=bad)
    with pytest.raises(ValueError, match="init"):
        km(X, 4, init="random")
    for bad in (0.0, -1.0, float("nan"), float("inf"), [1.0, 0.0], [1.0, float("nan")], [1.0, -2.0]):
        with pytest.raises(ValueError, match="lengthscales"):
            km(X, 4, lengthscales=bad)
    for bad in ([1.0, 1.0, 1.0], np.ones((2, 1))):
        with pytest.raises(ValueError, match="lengthscales"):
            km(X, 4, lengthscales=bad)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="max_iter"):
            km(X, 4, max_iter=bad)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol"):
            km(X, 4, tol=bad)
    k = p.SquaredExponential(variance=1.0, lengthscales=1.0)
    with pytest.raises(ValueError, match="SeparateIndependent"):
        km(X, 4, lengthscales=p.SeparateIndependent([k, k]))


def test_an_inducing_selection_of_another_size_is_refused():
    import torch

    p = pkg()
    X = np.random.RandomState(0).randn(10, 2)
    z = torch.zeros((3, 2), dtype=torch.float64)
    sel = p.InducingSelection(Z=z, indices=torch.arange(3), pivots=torch.ones(3), residual=torch.zeros(10), trace=torch.zeros(()), count=3)
    with pytest.raises(ValueError, match="init holds 3 rows"):
        p.kmeans_inducing_points(X, 4, init=sel)


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = pkg()
    with pytest.raises(p.HipExtensionError):
        p.kmeans_inducing_points(np.zeros((10, 2)) + np.arange(10)[:, None], 4)
