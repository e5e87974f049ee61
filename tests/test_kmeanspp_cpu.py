"""CPU checks around ``kmeanspp_seeds``: the NumPy restatement (tests/kmeanspp_ref.py) itself -- its uniforms, the law of its
draws, what it buys Lloyd's iterations --, the exports, the C-ABI seam (symbols, one ctypes entry per parameter, ABI number,
parameter checks in front of any launch) and every ``ValueError`` of the two public functions (raised before any engine exists)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import kmeans_ref as R
from tests import kmeanspp_ref as P
from tests import softmax_ref as S
from tests.helpers import pkg

LS = np.array([1.0, 0.7, 1.6])
SYMBOLS = ("tsvgp_kmeanspp_f64", "tsvgp_kmeanspp_work", "tsvgp_kmeanspp_rows")


def test_uniform_is_the_stated_function_of_the_generator():
    seed, r, j = 0x123456789ABCDEF, 7, 3
    x = S.philox4x32_10((r, j, 0x6B2B2B, 0), (seed & 0xFFFFFFFF, seed >> 32))
    x0, x1 = int(x[0]), int(x[1])
    num = (x0 >> 5) * 2 ** 26 + (x1 >> 6)  # an integer below 2^53: the quotient is exact in fp64
    u = P.uniforms(seed, 8, 4)
    assert 0 <= num < 2 ** 53 and u[r, j] == num / 2.0 ** 53 and float(u[r, j]) * 2.0 ** 53 == num
    big = P.uniforms(5, 2000, 16)
    assert big.dtype == np.float64 and np.all(big >= 0.0) and np.all(big < 1.0)
    assert np.all(big * 2.0 ** 53 == np.floor(big * 2.0 ** 53))  # 53-bit fractions
    assert abs(big.mean() - 0.5) < 4.0 / math.sqrt(12 * big.size)
    assert not np.array_equal(P.uniforms(6, 4, 4), P.uniforms(5, 4, 4))
    assert np.array_equal(P.uniforms(5, 4, 4), big[:4, :4])  # a function of (seed, r, j) alone


def test_default_trials_is_scikit_learns():
    assert [P.default_trials(M) for M in (1, 2, 3, 8, 12, 16, 256, 1024)] == [2, 2, 3, 4, 4, 4, 7, 8]


def test_pick_never_returns_zero_mass_and_clips_at_the_top():
    mind = np.array([0.0, 2.0, 0.0, 1.0, 0.0])
    assert [P.pick(mind, t) for t in (0.0, 1.9, 2.0, 2.5, 3.0, 4.0)] == [1, 1, 3, 3, 3, 3]
    assert P.pick(np.zeros(5), 0.0) == 4


def test_seeding_frequencies_follow_d2_sampling():
    """L = 1 on the 1-D points {0, 1, 3, 7}, M = 2, seeds 0 .. 3999: the first centre uniform, the second given the first
    proportional to d^2, each count within 4 binomial standard deviations."""
    X = np.array([[0.0], [1.0], [3.0], [7.0]])
    first, second = np.zeros(4, int), np.zeros((4, 4), int)
    for s in range(4000):
        idx = P.seed(X, 2, seed=s, n_local_trials=1).indices
        first[idx[0]] += 1
        second[idx[0], idx[1]] += 1
    assert first.sum() == 4000
    worst = np.max(np.abs(first - 1000.0) / math.sqrt(4000 * 0.25 * 0.75))
    for i in range(4):
        d2 = (X[:, 0] - X[i, 0]) ** 2
        p = d2 / d2.sum()
        assert second[i, i] == 0  # zero mass is never drawn
        for k in range(4):
            if k != i:
                sd = math.sqrt(first[i] * p[k] * (1.0 - p[k]))
                worst = max(worst, abs(second[i, k] - first[i] * p[k]) / sd)
    print(f"largest deviation: {worst:.2f} binomial standard deviations")
    assert worst <= 4.0


def test_restatement_bookkeeping():
    X, _, _ = R.blobs(0, N=400)
    s = P.seed(X, 9, lengthscales=LS, seed=3)
    L = P.default_trials(9)
    assert s.candidates.shape == (9, L) and len(set(s.indices.tolist())) == 9
    assert np.all(np.diff(s.potential_history) <= 0) and s.potential_history[-1] == math.fsum(s.dist)
    assert np.all(s.candidates[0, 1:] == -1) and np.all(np.isinf(s.trial_potentials[0, 1:])) and np.all(s.uniforms[0, 1:] == 0)
    assert np.array_equal(s.dist, R.dist2(X, X[s.indices], 1.0 / LS)[0].min(axis=1))
    for r in range(1, 9):
        js = int(np.argmin(s.trial_potentials[r]))
        assert s.indices[r] == s.candidates[r, js] and s.potential_history[r] == s.trial_potentials[r, js]
    # teacher-forced on its own choices it reproduces itself, and its bounds are rounding-sized
    f = P.forced(X, LS, s.indices[:4], s.candidates[4])
    assert np.array_equal(f.trial, s.trial_potentials[4]) and f.pot == s.potential_history[3]
    assert 0 < f.delta <= 1e-10 * f.pot and np.all(f.trial_bound <= 1e-10 * f.trial)
    for j in range(L):
        n, t = s.candidates[4, j], s.uniforms[4, j] * s.potential_history[3]
        assert f.mind[n] > 0 and (f.cum[n - 1] if n else 0.0) - f.delta <= t <= f.cum[n] + f.delta
    # fewer distinct rows than M: zeros, no NaN, nothing raised
    dup = np.repeat(X[:3], 4, axis=0)
    d = P.seed(dup, 6, seed=1)
    assert np.all(d.potential_history[2:] == 0.0) and np.all(np.isfinite(d.potential_history)) and np.all(d.dist == 0.0)
    assert len({tuple(r) for r in dup[d.indices[:3]]}) == 3


@pytest.mark.parametrize("data", [1, 2])
def test_seeding_rescues_lloyd_on_sorted_blobs(data):
    """X[:12] in one cluster: Lloyd's iterations from "first" stay far from the optimum, from the seeding they end below half
    of that inertia for every seed 0 .. 19."""
    X = P.sorted_blobs(data)
    base = R.lloyd(X, 12, lengthscales=LS).inertia
    worst = max(R.lloyd(X, 12, init=X[P.seed(X, 12, lengthscales=LS, seed=s).indices], lengthscales=LS).inertia for s in range(20))
    print(f"blobs({data}): 'first' ends at {base:.0f}, the worst seeded run at {worst:.0f}")
    assert worst < 0.5 * base


def test_names_are_exported():
    p = pkg()
    for name in ("kmeanspp_seeds", "KMeansSeeding"):
        assert name in p.__all__ and hasattr(p, name)
    assert hasattr(p.estep.EStepEngine, "kmeanspp")
    assert list(p.KMeansSeeding.__dataclass_fields__) == ["Z", "indices", "dist", "potential", "potential_history", "candidates",
                                                          "trial_potentials", "uniforms", "seed", "n_local_trials"]
    assert p.KMeansInducing.seeding is None


def test_header_and_bindings_carry_the_symbols_with_abi_5(repo_root):
    B = pkg()._backend
    header = open(os.path.join(repo_root, "include", "tsvgp_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = B.lib()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/tsvgp_hip.h"
        assert name in B.exported_symbols() and hasattr(lib, name)
    assert re.search(r"#define\s+TSVGP_ABI_VERSION\s+5\b", header) and B.ABI_VERSION == 5 and lib.tsvgp_abi_version() == 5
    assert re.search(r"#define\s+TSVGP_KMEANSPP_MAX_TRIALS\s+16\b", header) and B.KMEANSPP_MAX_TRIALS == 16 == P.MAX_TRIALS
    decl = re.search(r"int\s+tsvgp_kmeanspp_f64\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(decl.split(",")) == len(B._PROTOTYPES["tsvgp_kmeanspp_f64"][1]) == 15
    assert "(13) k-means++ seeding" in header


def test_sizing_helpers():
    lib = pkg()._backend.lib()
    for D in range(1, 33):
        rows = lib.tsvgp_kmeanspp_rows(D)
        assert rows == lib.tsvgp_kmeans_assign_rows(D) and rows % 256 == 0 and rows // 256 <= 4
        assert lib.tsvgp_kmeanspp_work(1, D, 1) == 1 and lib.tsvgp_kmeanspp_work(rows, D, 16) == 16
        assert lib.tsvgp_kmeanspp_work(rows + 1, D, 5) == 10
    assert lib.tsvgp_kmeanspp_rows(0) == -1 and lib.tsvgp_kmeanspp_rows(33) == -1
    for bad in ((0, 4, 2), (10, 0, 2), (10, 33, 2), (10, 4, 0), (10, 4, 17), (lib.tsvgp_kmeanspp_rows(8) * (2 ** 31 - 1) + 1, 8, 2)):
        assert lib.tsvgp_kmeanspp_work(*bad) == -1, bad


def test_entry_rejects_bad_parameters_before_any_launch():
    """Every call below fails a parameter check, so nothing is launched and the host buffers are never read."""
    lib = pkg()._backend.lib()
    buf = (ctypes.c_double * 1024)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    assert ctypes.addressof(buf) % 16 == 0
    names = ("X", "il", "indices", "dist", "pot_hist", "cand", "cand_pot", "unif", "work")

    def call(N=100, M=4, L=3, D=2, seed=0, **ptrs):
        a = {k: ptrs.get(k, ptr) for k in names}
        return lib.tsvgp_kmeanspp_f64(a["X"], a["il"], seed, M, L, a["indices"], a["dist"], a["pot_hist"], a["cand"], a["cand_pot"],
                                      a["unif"], a["work"], N, D, None)

    for name in names:
        assert call(**{name: None}) == 1, name
        assert call(**{name: ctypes.c_void_p(ptr.value + 4)}) == 1, name  # doubles and int64: 8-byte boundaries
    for kw in (dict(N=0), dict(N=-5), dict(M=0), dict(M=-1), dict(M=101), dict(N=3, M=4), dict(L=0), dict(L=17), dict(L=-1),
               dict(D=0), dict(D=33), dict(D=-2)):
        assert call(**kw) == 1, kw


def test_argument_errors_need_no_gpu():
    import torch

    p = pkg()
    X = np.random.RandomState(0).randn(10, 2)
    for fn in (p.kmeanspp_seeds, lambda *a, **k: p.kmeans_inducing_points(*a, init="k-means++", **k)):
        for empty in (np.zeros((0, 2)), np.zeros((5, 0)), np.zeros(5), np.zeros((2, 3, 4))):
            with pytest.raises(ValueError, match="non-empty"):
                fn(empty, 4)
        with pytest.raises(ValueError, match="32"):
            fn(np.zeros((40, 33)), 4)
        for bad in (0, -3, 2.5, 11, True):
            with pytest.raises(ValueError, match="num_inducing"):
                fn(X, bad)
        for bad in (0.0, -1.0, float("nan"), [1.0, 0.0], [1.0, 1.0, 1.0]):
            with pytest.raises(ValueError, match="lengthscales"):
                fn(X, 4, lengthscales=bad)
        for bad in (0, 17, -1, 2.5, True):
            with pytest.raises(ValueError, match="n_local_trials"):
                fn(X, 4, n_local_trials=bad)
        for bad in (-1, 2 ** 63, 1.5, True):
            with pytest.raises(ValueError, match="seed"):
                fn(X, 4, seed=bad)
        k = p.SquaredExponential(variance=1.0, lengthscales=1.0)
        with pytest.raises(ValueError, match="SeparateIndependent"):
            fn(X, 4, lengthscales=p.SeparateIndependent([k, k]))
    km = p.kmeans_inducing_points
    with pytest.raises(ValueError, match="init"):
        km(X, 4, init="random")
    with pytest.raises(ValueError, match="init"):
        km(X, 4, init="kmeans++")
    # seed and n_local_trials belong to "k-means++" alone
    for init in ("first", X[:4], "random"):
        for kw in (dict(seed=0), dict(n_local_trials=2), dict(seed=3, n_local_trials=2)):
            with pytest.raises(ValueError, match="seed and n_local_trials"):
                km(X, 4, init=init, **kw)
    # a seeding made for another M
    z = torch.zeros((3, 2), dtype=torch.float64)
    sd = p.KMeansSeeding(Z=z, indices=torch.arange(3), dist=torch.zeros(10), potential=torch.zeros(()), potential_history=torch.zeros(3),
                         candidates=torch.zeros((3, 2), dtype=torch.int64), trial_potentials=torch.zeros((3, 2)),
                         uniforms=torch.zeros((3, 2)), seed=0, n_local_trials=2)
    with pytest.raises(ValueError, match="init holds 3 rows"):
        km(X, 4, init=sd)
    with pytest.raises(ValueError, match="seed and n_local_trials"):
        km(X, 3, init=sd, seed=1)


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = pkg()
    X = np.zeros((10, 2)) + np.arange(10)[:, None]
    with pytest.raises(p.HipExtensionError):
        p.kmeanspp_seeds(X, 4)
    with pytest.raises(p.HipExtensionError):
        p.kmeans_inducing_points(X, 4, init="k-means++", seed=1)
