"""GPU checks of ``kmeanspp_seeds`` / ``tsvgp_kmeanspp_f64`` against the NumPy restatement (tests/kmeanspp_ref.py).

A random choice cannot be compared index by index with a reference that adds in another order, so every round is checked
TEACHER-FORCED: the reference is put into the state the device's own earlier choices define, and the device's next draws must
then be legal under the sampling rule within the derived rounding bound delta_r (kmeanspp_ref's docstring; nothing is tuned on
the device's output), its trial potentials within their bound, and everything the contract promises exactly (the uniforms, the
winner among the reported potentials, the history, the final distances, repeatability) is compared bit for bit.

Shapes: one row; M = N; the smallest sizes that cross a workgroup edge (rows + 1), a second edge with a ragged tail
(2 rows + 37), every compile-time dimension with and without padded columns (1, 2, 3, 8, 17, 32), both ends of L (1, 16).
"""
import math

import numpy as np
import pytest

from tests import kmeans_ref as R
from tests import kmeanspp_ref as P
from tests.helpers import pkg
from tests.test_gpu_kmeans import Guarded, bits, same_run, to_np

pytestmark = pytest.mark.gpu

LS3 = np.array([1.0, 0.7, 1.6])
SEED = 11
# (N, D, M, L, lengthscales): N as a number, or as (a, b) for a * rows + b with rows = tsvgp_kmeanspp_rows(D)
SHAPES = [(1, 1, 1, 1, None), (2, 1, 2, 1, None), (5, 2, 5, 3, None), (257, 3, 16, None, None), ((1, 1), 8, 8, 4, None),
          ((2, 37), 8, 12, None, None), (3000, 3, 12, None, LS3), (700, 17, 9, 16, None), (600, 32, 7, 2, None)]
IDS = ["N{}_D{}_M{}_L{}".format("{}rows+{}".format(*s[0]) if isinstance(s[0], tuple) else s[0], s[1], s[2], s[3]) for s in SHAPES]


def torch_():
    import torch

    return torch


def fields(sd):
    return dict(Z=sd.Z.cpu().numpy(), indices=sd.indices.cpu().numpy(), dist=sd.dist.cpu().numpy(), potential=np.asarray(float(sd.potential)),
                potential_history=sd.potential_history.cpu().numpy(), candidates=sd.candidates.cpu().numpy(),
                trial_potentials=sd.trial_potentials.cpu().numpy(), uniforms=sd.uniforms.cpu().numpy())


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


@pytest.fixture(scope="module")
def runs():
    """One problem and one device call per shape, shared read-only: {index: (X, lengthscales, M, L, KMeansSeeding, fields)}."""
    p = pkg()
    lib = p._backend.lib()
    out = {}
    for k, (N, D, M, L, ls) in enumerate(SHAPES):
        if isinstance(N, tuple):
            N = N[0] * lib.tsvgp_kmeanspp_rows(D) + N[1]
        X = R.blobs(0)[0] if N == 3000 else np.random.RandomState(500 + k).randn(N, D)
        sd = p.kmeanspp_seeds(X, M, lengthscales=ls, seed=SEED, n_local_trials=L)
        out[k] = (X, ls, M, P.default_trials(M) if L is None else L, sd, fields(sd))
    return out


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_uniforms_are_the_restatement_bit_for_bit(runs, k):
    X, ls, M, L, sd, f = runs[k]
    assert sd.n_local_trials == L and sd.seed == SEED and f["uniforms"].shape == (M, L) and f["candidates"].dtype == np.int64
    ref = P.uniforms(SEED, M, L)
    ref[0, 1:] = 0.0
    assert np.array_equal(bits(f["uniforms"]), bits(ref))
    assert np.all(f["candidates"][0, 1:] == -1) and np.all(np.isposinf(f["trial_potentials"][0, 1:]))
    assert tuple(sd.Z.shape) == (M, X.shape[1])
    assert np.array_equal(bits(f["Z"]), bits(X[f["indices"]]))


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_every_round_teacher_forced(runs, k):
    X, ls, M, L, sd, f = runs[k]
    N = X.shape[0]
    idx, hist, cand, cpot, unif = f["indices"], f["potential_history"], f["candidates"], f["trial_potentials"], f["uniforms"]
    assert np.all((idx >= 0) & (idx < N))
    # round 0: the first centre is a pure function of the uniform; its potential is the only trial
    assert idx[0] == cand[0, 0] == min(int(math.floor(unif[0, 0] * N)), N - 1)
    f0 = P.forced(X, ls, [], [idx[0]])
    assert abs(cpot[0, 0] - f0.trial[0]) <= f0.trial_bound[0] and bits(hist[:1])[0] == bits(cpot[0, :1])[0]
    worst_cdf = worst_pot = 0.0
    for r in range(1, M):
        fr = P.forced(X, ls, idx[:r], cand[r])
        for j in range(L):
            n, t = int(cand[r, j]), unif[r, j] * hist[r - 1]  # the device's own product, repeated bit for bit
            assert 0 <= n < N
            if fr.pot > 0.0:
                assert fr.mind[n] > 0.0, (r, j, "a row of zero mass was drawn")
                lo, hi = (fr.cum[n - 1] if n else 0.0), fr.cum[n]
                worst_cdf = max(worst_cdf, (lo - t) / fr.delta, (t - hi) / fr.delta)
                assert lo - fr.delta <= t <= hi + fr.delta, (r, j, n, lo, t, hi, fr.delta)
            else:
                assert n == N - 1 and hist[r - 1] == 0.0
            err = abs(cpot[r, j] - fr.trial[j])
            worst_pot = max(worst_pot, err / fr.trial_bound[j] if fr.trial_bound[j] > 0 else float(err > 0))
            assert err <= fr.trial_bound[j], (r, j, err, fr.trial_bound[j])
        js = int(np.argmin(cpot[r]))  # the lowest index of the minimum of the device's OWN reported potentials: exact
        assert idx[r] == cand[r, js]
        assert bits(hist[r:r + 1])[0] == bits(cpot[r, js:js + 1])[0]
    print(f"{IDS[k]}: inverse CDF off by at most {worst_cdf:.2e} delta outside its row, potentials by {worst_pot:.2e} of their bound")
    assert np.all(np.diff(hist) <= 0.0) and np.all(np.isfinite(hist))


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_final_distances_are_the_assignments(runs, k):
    torch = torch_()
    p = pkg()
    X, ls, M, L, sd, f = runs[k]
    engine = p.estep.EStepEngine(torch.float64, None)
    il = torch.as_tensor(P.inv_ls(X.shape[1], ls)).cuda()
    _, dist, _ = engine.kmeans_assign(torch.as_tensor(X).cuda(), sd.Z, il)
    assert np.array_equal(bits(dist.cpu().numpy()), bits(f["dist"]))
    fr = P.forced(X, ls, f["indices"], [])
    assert np.all(np.abs(f["dist"] - fr.mind) <= fr.e)
    assert sd.potential.dim() == 0 and bits(f["potential"].reshape(1))[0] == bits(f["potential_history"][-1:])[0]
    bound = math.fsum(fr.e) + P.gamma(X.shape[0]) * (fr.pot + math.fsum(fr.e))
    assert abs(float(f["potential"]) - fr.pot) <= bound
    if M == X.shape[0]:  # M = N on distinct rows: every row once, nothing left
        assert sorted(f["indices"].tolist()) == list(range(M)) and float(f["potential"]) == 0.0 and np.all(f["dist"] == 0.0)


def test_every_row_is_taken_once_when_m_is_n():
    X = np.random.RandomState(3).randn(130, 3)
    f = fields(pkg().kmeanspp_seeds(X, 130, seed=2, n_local_trials=2))
    assert sorted(f["indices"].tolist()) == list(range(130)) and float(f["potential"]) == 0.0
    assert np.all(f["potential_history"][:-1] > 0.0)


def test_duplicated_rows():
    """K = 7 distinct values, 200 copies of each over two workgroups.  M = K takes each value once; M = K + 3 completes with
    zeros: nothing is divided by the potential, nothing is NaN, nothing raises."""
    p = pkg()
    rs = np.random.RandomState(8)
    K = 7
    vals = rs.randn(K, 2)
    which = rs.permutation(np.repeat(np.arange(K), 200))
    X = vals[which]
    f = fields(p.kmeanspp_seeds(X, K, seed=5, n_local_trials=3))
    assert sorted(which[f["indices"]].tolist()) == list(range(K)) and float(f["potential"]) == 0.0 and np.all(f["dist"] == 0.0)
    g = fields(p.kmeanspp_seeds(X, K + 3, seed=5, n_local_trials=3))
    assert all(np.all(np.isfinite(g[k])) for k in ("Z", "dist", "potential_history", "uniforms")) and not np.isnan(g["trial_potentials"]).any()
    assert np.all(g["potential_history"][K - 1:] == 0.0) and np.all(g["potential_history"][:K - 1] > 0.0)
    assert np.all(g["candidates"][K:] == X.shape[0] - 1) and np.all(g["trial_potentials"][K:] == 0.0)
    assert sorted(set(which[g["indices"]].tolist())) == list(range(K))
    assert np.array_equal(g["indices"][:K], f["indices"])


def test_two_calls_agree_bit_for_bit_and_the_seed_matters(runs):
    p = pkg()
    for k in (5, 6):
        X, ls, M, L, sd, f = runs[k]
        again = fields(p.kmeanspp_seeds(X, M, lengthscales=ls, seed=SEED, n_local_trials=L))
        assert same_bits(f, again)
        other = fields(p.kmeanspp_seeds(X, M, lengthscales=ls, seed=SEED + 1, n_local_trials=L))
        assert not np.array_equal(other["indices"], f["indices"])


def test_entry_writes_inside_its_buffers():
    """The C entry on guarded buffers at a ragged three-workgroup shape: the outputs are those of the public function, no guard
    element is touched."""
    torch = torch_()
    p = pkg()
    lib = p._backend.lib()
    D, M, L = 8, 12, 4
    N = 2 * lib.tsvgp_kmeanspp_rows(D) + 37
    X = np.random.RandomState(505).randn(N, D)
    f64, i64 = torch.float64, torch.int64
    gx, gl = Guarded(N * D, f64, X), Guarded(D, f64, np.ones(D))
    idx, dist, hist = Guarded(M, i64), Guarded(N, f64), Guarded(M, f64)
    cand, cpot, unif = Guarded(M * L, i64), Guarded(M * L, f64), Guarded(M * L, f64)
    work = Guarded(int(lib.tsvgp_kmeanspp_work(N, D, L)), f64)
    st = lib.tsvgp_kmeanspp_f64(gx.ptr, gl.ptr, SEED, M, L, idx.ptr, dist.ptr, hist.ptr, cand.ptr, cpot.ptr, unif.ptr, work.ptr, N, D,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0
    for g in (gx, gl, idx, dist, hist, cand, cpot, unif, work):
        assert g.guards_intact()
    f = fields(p.kmeanspp_seeds(X, M, seed=SEED, n_local_trials=L))
    assert np.array_equal(idx.get(), f["indices"]) and np.array_equal(bits(dist.get()), bits(f["dist"]))
    assert np.array_equal(bits(hist.get()), bits(f["potential_history"])) and np.array_equal(cand.get().reshape(M, L), f["candidates"])
    assert np.array_equal(bits(cpot.get().reshape(M, L)), bits(f["trial_potentials"]))


def test_non_finite_rows_are_refused():
    p = pkg()
    X = np.random.RandomState(0).randn(50, 2)
    for bad in (float("nan"), float("inf")):
        Y = X.copy()
        Y[17, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            p.kmeanspp_seeds(Y, 4)
        with pytest.raises(ValueError, match="finite"):
            p.kmeans_inducing_points(Y, 4, init="k-means++")


@pytest.mark.parametrize("data,seed", [(1, 0), (2, 3)])
def test_public_function_runs_lloyd_from_the_seeds(data, seed):
    p = pkg()
    X = P.sorted_blobs(data)
    res = p.kmeans_inducing_points(X, 12, init="k-means++", seed=seed, lengthscales=LS3)  # (a ValueError without the feature)
    sd = res.seeding
    assert isinstance(sd, p.KMeansSeeding) and sd.seed == seed and sd.n_local_trials == 4 and tuple(sd.indices.shape) == (12,)
    ref = R.lloyd(X, 12, init=X[sd.indices.cpu().numpy()], lengthscales=LS3)
    same_run(res, ref, f"k-means++ seed {seed}")
    # the seeding alone gives the same seeds, and passed as init the same run, bit for bit
    alone = p.kmeanspp_seeds(X, 12, lengthscales=LS3, seed=seed)
    assert same_bits(fields(alone), fields(sd))
    again = p.kmeans_inducing_points(X, 12, init=alone, lengthscales=LS3)
    assert again.seeding is alone and (again.n_iter, again.converged) == (res.n_iter, res.converged)
    for a, b in zip(to_np(res), to_np(again)):
        assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))
    first = p.kmeans_inducing_points(X, 12, lengthscales=LS3)
    assert first.seeding is None
    print(f"blobs({data}): 'first' ends at {float(first.inertia):.0f}, k-means++ (seed {seed}) at {float(res.inertia):.0f}")
    assert float(res.inertia) < 0.5 * float(first.inertia)
    with pytest.raises(ValueError, match="init holds 12 rows"):
        p.kmeans_inducing_points(X, 11, init=alone, lengthscales=LS3)


def test_result_feeds_a_model():
    p = pkg()
    rng = np.random.RandomState(0)
    X = rng.randn(2000, 2)
    Y = np.sin(X @ rng.randn(2, 1)) + np.sqrt(0.1) * rng.randn(2000, 1)
    res = p.kmeans_inducing_points(X, 16, init="k-means++", seed=1, lengthscales=1.0)
    assert tuple(res.Z.shape) == (16, 2) and int(res.counts.sum()) == 2000
    model = p.t_SVGP(p.SquaredExponential(variance=1.0, lengthscales=1.0), p.Gaussian(0.1), res.Z)
    model.natgrad_step((X, Y), lr=0.8)
    assert np.isfinite(float(model.elbo((X, Y))))
    assert p.InducingPoints(res.seeding.Z).num_inducing == 16


def test_the_library_exports_the_entry():
    lib = pkg()._backend.lib()
    assert hasattr(lib, "tsvgp_kmeanspp_f64") and lib.tsvgp_kmeanspp_rows(8) == lib.tsvgp_kmeans_assign_rows(8)
