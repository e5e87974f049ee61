"""GPU checks of ``kmeans_inducing_points`` and its two C-ABI entries against the NumPy restatement (tests/kmeans_ref.py).

Labels are compared EXACTLY, on every row.  That is legitimate because each test first asserts, from the reference alone, that no
row's gap between its best and second-best centre is within the rounding bounds E of the two distances (kmeans_ref.dist2): the
bound is ~1e-14 relative, the smallest gap on these inputs ~1e-5.  Distances are held to E, the partial inertias to sum E, the
centroid sums to the worst case of any summation order (checked against exact rational arithmetic), and everything that is
promised bit for bit (ties, slices, repeated launches, empty clusters, untouched neighbours) is compared bit for bit.

Tiling the shapes are chosen around (asserted in test_tiling_is_what_the_shapes_assume): 1024 rows per workgroup for D <= 16,
512 beyond; centres in chunks of 128; compile-time dimensions 1, 2, 4, 8, 16, 32.
"""
from fractions import Fraction
import math

import numpy as np
import pytest

from tests import kmeans_ref as R
from tests.helpers import pkg

pytestmark = pytest.mark.gpu

G = 64  # guard elements in front of and behind every buffer
U = 2.0 ** -53
LS3 = np.array([1.0, 0.7, 1.6])

# (N, M, D): seven shapes from one row to several workgroups and chunks, then one row short of / exactly / one row past a workgroup and a centre chunk for both row
# counts, and every compile-time dimension with (3, 5, 13, 17, 20) and without (1, 2, 4, 8, 16, 32) padded columns
SHAPES = [(1, 1, 1), (63, 5, 2), (65, 129, 3), (1025, 513, 8), (300, 1000, 13), (2100, 641, 16), (700, 2049, 32),
          (1023, 127, 4), (1024, 128, 5), (1025, 129, 1), (2049, 257, 2), (511, 128, 17), (512, 127, 32), (513, 129, 20)]
IDS = ["N{}_M{}_D{}".format(*s) for s in SHAPES]


def problem(N, M, D):
    rs = np.random.RandomState(1000 + N + M)
    X, C = rs.randn(N, D), rs.randn(M, D)
    ls = (0.7 + rs.rand(D)) * np.sqrt(D)
    return X, C, 1.0 / ls


def torch_():
    import torch

    return torch


class Guarded:
    """A device buffer with G guard elements on both sides; ``fill`` (NaN, or -7 for integers) everywhere the caller puts no data."""

    def __init__(self, n, dtype, data=None):
        torch = torch_()
        self.n, self.fill = n, (float("nan") if dtype == torch.float64 else -7)
        self.buf = torch.full((n + 2 * G,), self.fill, dtype=dtype, device="cuda")
        if data is not None:
            self.buf[G:G + n] = torch.as_tensor(np.ascontiguousarray(data).reshape(-1), dtype=dtype).cuda()
        self.ptr = self.buf.data_ptr() + G * self.buf.element_size()

    def get(self):
        return self.buf[G:G + self.n].cpu().numpy()

    def guards_intact(self):
        torch = torch_()
        g = torch.cat([self.buf[:G], self.buf[G + self.n:]])
        return bool(torch.isnan(g).all()) if self.fill != -7 else bool((g == -7).all())


def launch_assign(X, C, il, a=0, b=None):
    """tsvgp_kmeans_assign_f64 on rows [a, b) of X through guarded buffers: (labels, dist, part), guards checked."""
    torch = torch_()
    lib = pkg()._backend.lib()
    N, D = X.shape
    b = N if b is None else b
    M = C.shape[0]
    gx, gc, gl = Guarded(N * D, torch.float64, X), Guarded(M * D, torch.float64, C), Guarded(D, torch.float64, il)
    n = b - a
    nparts = lib.tsvgp_kmeans_assign_parts(n, D)
    labels, dist, part = Guarded(n, torch.int32), Guarded(n, torch.float64), Guarded(nparts, torch.float64)
    st = lib.tsvgp_kmeans_assign_f64(gx.ptr + 8 * a * D, gc.ptr, gl.ptr, labels.ptr, dist.ptr, part.ptr, n, M, D,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0
    for g in (gx, gc, gl, labels, dist, part):
        assert g.guards_intact()
    return labels.get(), dist.get(), part.get()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def test_tiling_is_what_the_shapes_assume():
    lib = pkg()._backend.lib()
    assert lib.tsvgp_kmeans_assign_chunk() == 128
    assert [lib.tsvgp_kmeans_assign_rows(D) for D in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)] == [1024] * 8 + [512] * 2


@pytest.fixture(scope="module")
def assigned():
    """One reference and one launch per shape, shared read-only: {shape: (X, C, il, ref tuple, gpu tuple)}."""
    out = {}
    for shape in SHAPES:
        X, C, il = problem(*shape)
        out[shape] = (X, C, il, R.assign(X, C, il), launch_assign(X, C, il))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_assign_every_row(assigned, shape):
    N, M, D = shape
    X, C, il, (lab_ref, best, second, E), (lab, dist, part) = assigned[shape]
    rows = np.arange(N)
    if M > 1:
        # from the reference alone: no row is close enough to a tie for rounding to decide it, so no row is excused below
        second_arg = np.argmin(np.where(np.arange(M)[None, :] == lab_ref[:, None], np.inf, R.dist2(X, C, il)[0]), axis=1)
        margin = (second - best) - (E[rows, lab_ref] + E[rows, second_arg])
        print(f"{shape}: smallest relative gap {np.min((second - best) / best):.3e}, largest bound {np.max(E[rows, lab_ref] / best):.3e}")
        assert np.all(margin > 0)
    assert lab.dtype == np.int32 and np.array_equal(lab, lab_ref)
    err = np.abs(dist - best)
    print(f"{shape}: max |dist - ref| / E = {np.max(err / np.maximum(E[rows, lab_ref], 1e-300)):.3e}")
    assert np.all(err <= E[rows, lab_ref])
    # the per-workgroup partial sums: each one its rows' distances (any order: (n - 1) u sum), all of them the inertia within sum E
    lib = pkg()._backend.lib()
    wg = lib.tsvgp_kmeans_assign_rows(D)
    assert part.shape == (-(-N // wg),)
    for i, p in enumerate(part):
        seg = dist[i * wg:(i + 1) * wg]
        assert abs(p - math.fsum(seg)) <= len(seg) * U * math.fsum(seg)
    assert abs(math.fsum(part) - math.fsum(best)) <= math.fsum(E[rows, lab_ref])


def test_assign_exact_ties_go_to_the_lowest_index():
    """Centres 3, 7 and 130 (the next LDS chunk) hold the bits of centre 1 and some rows of X are centre 1: label 1, distance
    exactly 0 (with a contracted a - b the distance of identical rows would be the rounding error of b).  Every other row still
    matches the reference, whose argmin also takes the first of equal values."""
    N, M, D = 300, 140, 5
    X, C, il = problem(N, M, D)
    C[3] = C[7] = C[130] = C[1]
    on = [0, 17, 64, 299]
    X[on] = C[1]
    lab_ref, best, second, E = R.assign(X, C, il)
    lab, dist, part = launch_assign(X, C, il)
    assert np.all(lab[on] == 1) and np.all(bits(dist[on]) == 0)
    assert np.array_equal(lab, lab_ref) and not np.isin(lab, [3, 7, 130]).any()
    assert (lab == 1).sum() > len(on)  # rows that are merely nearest to the tied centres are there too
    assert np.all(np.abs(dist - best) <= E[np.arange(N), lab_ref])


def test_assign_rows_do_not_depend_on_the_launch(assigned):
    shape = (2100, 641, 16)
    X, C, il, _, (lab, dist, part) = assigned[shape]
    lab2, dist2, part2 = launch_assign(X, C, il)
    assert np.array_equal(lab, lab2) and np.array_equal(bits(dist), bits(dist2)) and np.array_equal(bits(part), bits(part2))
    for a, b in ((37, 1500), (1024, 2100), (2099, 2100), (0, 1)):
        ls, ds, _ = launch_assign(X, C, il, a, b)
        assert np.array_equal(ls, lab[a:b]) and np.array_equal(bits(ds), bits(dist[a:b])), (a, b)


# ------------------------------------------------------------------------------------------------ the update kernel
SIZES = [0, 1, 63, 64, 65, 5000, 0, 317]  # segment lengths ("the rest" = 317), an empty one first and one in the middle


def update_problem(D):
    rs = np.random.RandomState(77 + D)
    N, M = sum(SIZES), len(SIZES)
    X = rs.randn(N, D) + 0.3
    labels = rs.permutation(np.repeat(np.arange(M), SIZES))
    C_old = rs.randn(M, D)
    C_old[0, 0] = -0.0  # an empty cluster's centre is copied, not recomputed: the sign of a zero survives
    order = np.argsort(labels, kind="stable").astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    return X, labels, C_old, order, offsets


def launch_update(X, order, offsets, C_old):
    torch = torch_()
    lib = pkg()._backend.lib()
    N, D = X.shape
    M = C_old.shape[0]
    gx, go, gf = Guarded(N * D, torch.float64, X), Guarded(N, torch.int64, order), Guarded(M + 1, torch.int64, offsets)
    gc, out = Guarded(M * D, torch.float64, C_old), Guarded(M * D, torch.float64)
    st = lib.tsvgp_kmeans_update_f64(gx.ptr, go.ptr, gf.ptr, gc.ptr, out.ptr, N, M, D, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0
    for g in (gx, go, gf, gc, out):
        assert g.guards_intact()
    return out.get().reshape(M, D)


@pytest.mark.parametrize("D", [1, 3, 8, 32])
def test_update_means(D):
    X, labels, C_old, order, offsets = update_problem(D)
    C_new = launch_update(X, order, offsets, C_old)
    worst = 0.0
    for m, cnt in enumerate(SIZES):
        if cnt == 0:
            assert np.array_equal(bits(C_new[m]), bits(C_old[m]))
            continue
        rows = X[order[offsets[m]:offsets[m + 1]]]
        assert np.array_equal(np.sort(order[offsets[m]:offsets[m + 1]]), np.nonzero(labels == m)[0])
        for q in range(D):
            exact = sum(map(Fraction, rows[:, q].tolist())) / cnt
            ref = float(exact)
            bound = cnt * U * (np.abs(rows[:, q]).sum() / cnt) + U * abs(ref)  # any summation order, then the division
            err = abs(float(Fraction(float(C_new[m, q])) - exact))
            worst = max(worst, err / bound)
            assert err <= bound, (m, q, err, bound)
    print(f"D = {D}: largest error / bound = {worst:.3e}")
    # again: the same bits
    assert np.array_equal(bits(launch_update(X, order, offsets, C_old)), bits(C_new))


@pytest.mark.parametrize("D", [3, 32])
def test_update_bits_depend_on_the_own_segment_alone(D):
    """Permuting the rows of the OTHER clusters inside `order` leaves a cluster's bits alone; so does every other cluster's
    content: the 5000-row and the 65-row segment alone in a call of M = 2 give the bits they have among the eight."""
    X, labels, C_old, order, offsets = update_problem(D)
    C_new = launch_update(X, order, offsets, C_old)
    rs = np.random.RandomState(5)
    for keep in (4, 5, 7):
        order2 = order.copy()
        for m in range(len(SIZES)):
            if m != keep:
                seg = slice(offsets[m], offsets[m + 1])
                order2[seg] = rs.permutation(order2[seg])
        C2 = launch_update(X, order2, offsets, C_old)
        assert np.array_equal(bits(C2[keep]), bits(C_new[keep]))
    seg5, seg4 = order[offsets[5]:offsets[6]], order[offsets[4]:offsets[5]]
    rest = np.setdiff1d(np.arange(X.shape[0]), np.concatenate([seg5, seg4]))
    order3 = np.concatenate([seg5, seg4, rest]).astype(np.int64)  # (rows behind offsets[M] are in no segment)
    C3 = launch_update(X, order3, np.array([0, 5000, 5065], dtype=np.int64), C_old[:2])
    assert np.array_equal(bits(C3[0]), bits(C_new[5])) and np.array_equal(bits(C3[1]), bits(C_new[4]))


# ------------------------------------------------------------------------------------------------ the public function
def to_np(res):
    return (res.Z.cpu().numpy(), res.labels.cpu().numpy(), res.counts.cpu().numpy(), float(res.inertia),
            res.inertia_history.cpu().numpy())


def same_run(res, ref, what):
    """The device run against the restatement's: the same path (iterations, stop), identical labels and counts, Z and the
    inertias within 1e-12 relative.  The reference's own smallest gap says that rounding decided no label."""
    Z, labels, counts, inertia, hist = to_np(res)
    assert ref.min_gap >= 1e-9, f"{what}: the reference run has a near tie ({ref.min_gap:.2e}); labels cannot be compared exactly"
    assert (res.n_iter, res.converged) == (ref.n_iter, ref.converged), what
    assert labels.dtype == np.int64 and counts.dtype == np.int64
    assert np.array_equal(labels, ref.labels) and np.array_equal(counts, ref.counts), what
    zerr = np.max(np.abs(Z - ref.Z) / np.abs(ref.Z))
    herr = np.max(np.abs(hist - ref.inertia_history) / ref.inertia_history)
    print(f"{what}: n_iter {res.n_iter}, min gap {ref.min_gap:.2e}, min count {counts.min()}, Z rel {zerr:.2e}, inertia rel {herr:.2e}")
    assert Z.dtype == np.float64 and Z.shape == ref.Z.shape and zerr <= 1e-12
    assert hist.shape == (ref.n_iter,) and herr <= 1e-12
    assert abs(inertia - ref.inertia) <= 1e-12 * ref.inertia and res.inertia.dim() == 0


@pytest.fixture(scope="module")
def blob_runs():
    """(X, reference run, device run) for seeds 0, 1, 2, shared read-only."""
    out = []
    for seed in (0, 1, 2):
        X, _, _ = R.blobs(seed)
        out.append((X, R.lloyd(X, 12, lengthscales=LS3), pkg().kmeans_inducing_points(X, 12, lengthscales=LS3)))
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_public_function_follows_the_restatement(blob_runs, seed):
    X, ref, res = blob_runs[seed]
    assert ref.converged and ref.n_iter == (15, 21, 11)[seed] and ref.min_gap >= 1.4e-5 and ref.counts.min() >= 102
    same_run(res, ref, f"seed {seed}")
    assert np.all(np.diff(res.inertia_history.cpu().numpy()) <= 0)


def test_two_calls_agree_bit_for_bit(blob_runs):
    X, ref, res = blob_runs[1]
    again = pkg().kmeans_inducing_points(X, 12, lengthscales=LS3)
    for a, b in zip(to_np(res), to_np(again)):
        assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))
    assert (res.n_iter, res.converged) == (again.n_iter, again.converged)


def test_array_and_selection_inits(blob_runs):
    p = pkg()
    X, _, _ = blob_runs[0]
    init = X[np.random.RandomState(3).choice(3000, 12, replace=False)]
    same_run(p.kmeans_inducing_points(X, 12, init=init, lengthscales=LS3), R.lloyd(X, 12, init=init, lengthscales=LS3), "array init")
    kernel = p.SquaredExponential(variance=1.0, lengthscales=LS3)
    sel = p.select_inducing_points(X, kernel, 12)
    assert sel.count == 12
    Z0 = sel.Z.cpu().numpy()
    same_run(p.kmeans_inducing_points(X, 12, init=sel, lengthscales=LS3), R.lloyd(X, 12, init=Z0, lengthscales=LS3), "selection init")
    with pytest.raises(ValueError, match="init holds 12 rows"):
        p.kmeans_inducing_points(X, 11, init=sel, lengthscales=LS3)


def test_max_iter_one_and_tol_return_labels_of_the_returned_centres(blob_runs):
    p = pkg()
    X, _, _ = blob_runs[2]
    for kw in (dict(max_iter=1), dict(max_iter=3), dict(tol=0.05)):
        res = p.kmeans_inducing_points(X, 12, lengthscales=LS3, **kw)
        ref = R.lloyd(X, 12, lengthscales=LS3, **kw)
        same_run(res, ref, str(kw))
        Z, labels, counts, inertia, hist = to_np(res)
        lab, best, _, _ = R.assign(X, Z, 1.0 / LS3)  # the labels belong to the RETURNED Z (the extra assignment pass)
        assert np.array_equal(labels, lab) and np.array_equal(counts, np.bincount(lab, minlength=12))
        assert abs(inertia - best.sum()) <= 1e-12 * best.sum()
    assert not p.kmeans_inducing_points(X, 12, lengthscales=LS3, max_iter=1).converged


def test_a_centre_far_from_all_data_keeps_its_place(blob_runs):
    p = pkg()
    X, _, _ = blob_runs[0]
    init = X[:12].copy()
    init[4] = [1e3, -1e3, 1e3]
    res = p.kmeans_inducing_points(X, 12, init=init, lengthscales=LS3)
    same_run(res, R.lloyd(X, 12, init=init, lengthscales=LS3), "far centre")
    assert int(res.counts[4]) == 0 and np.array_equal(bits(res.Z[4].cpu().numpy()), bits(init[4]))
    assert not bool((res.labels == 4).any())


def test_lengthscales(blob_runs):
    p = pkg()
    X, _, _ = blob_runs[1]
    none, ones, scalar = (p.kmeans_inducing_points(X, 12, lengthscales=ls) for ls in (None, np.ones(3), 1.0))
    for other in (ones, scalar):
        for a, b in zip(to_np(none), to_np(other)):
            assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))
    # a column and its lengthscale scaled by 2 (exact in binary): the same scaled coordinates up to the rounding of x / l, so
    # the same labels; the centres' column scales with the data
    base = p.kmeans_inducing_points(X, 12, lengthscales=LS3)
    X2, ls2 = X.copy(), LS3.copy()
    X2[:, 1] *= 2.0
    ls2[1] *= 2.0
    res2 = p.kmeans_inducing_points(X2, 12, lengthscales=ls2)
    assert np.array_equal(res2.labels.cpu().numpy(), base.labels.cpu().numpy()) and res2.n_iter == base.n_iter
    Zb, Z2 = base.Z.cpu().numpy(), res2.Z.cpu().numpy()
    Zb[:, 1] *= 2.0
    assert np.array_equal(bits(Z2), bits(Zb))


def test_result_feeds_a_model():
    p = pkg()
    rng = np.random.RandomState(0)
    X = rng.randn(2000, 2)
    Y = np.sin(X @ rng.randn(2, 1)) + np.sqrt(0.1) * rng.randn(2000, 1)
    kernel = p.SquaredExponential(variance=1.0, lengthscales=1.0)
    res = p.kmeans_inducing_points(X, 16, lengthscales=1.0)
    assert tuple(res.Z.shape) == (16, 2) and int(res.counts.sum()) == 2000 and tuple(res.labels.shape) == (2000,)
    model = p.t_SVGP(kernel, p.Gaussian(0.1), res.Z)
    model.natgrad_step((X, Y), lr=0.8)
    assert np.isfinite(float(model.elbo((X, Y))))
    assert p.InducingPoints(res.Z).num_inducing == 16
