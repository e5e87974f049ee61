"""The blocked Cholesky family -- tsvgp_potrf_f64, tsvgp_potrf_solve_f64, tsvgp_potrf_inv_f64 -- through the C ABI against NumPy
fp64 LAPACK, with every argument the test's own: the five block-step forms (default, TSVGP_POTRF_SUBST, _DIAG_V1, _FUSE, the
inverse path), the three right-hand-side forms (none, dense, TSVGP_POTRF_RHS_UPPER), lda > M, gaps between the matrices of a
batch, rhs_rows != M, the Xt output, info for a defect in a batch member other than the first and at every pivot-group edge,
the accuracy of the inverse-based panels up to the condition number at which the models switch to substitution, and scale.

Sentinels: every buffer starts as NaN and the test writes only what the entry is documented to read -- the lower triangle of the
matrix (NaN stays in the strict upper triangle of the diagonal 128 x 128 tiles, which the kernels load and drop) and the
right-hand-side rows.  Afterwards the lower triangle holds the factor, the strict upper part of the diagonal tiles is exactly 0,
and the blocks above the diagonal, columns [M, lda) and the gap rows between the matrices are still NaN.

Tolerances on well-conditioned input (G G^T / M + 0.5 I, as tests/test_gpu_kernels.py::test_potrf) are that file's: factor 1e-12,
solved rows and inverse 1e-11, relative to the largest entry of the reference."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import POTRF_AUX_OFF, pkg, potrf_layout_cases, relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NB = 128
EPS = np.finfo(np.float64).eps
SUBST, RHS_UPPER, DIAG_V1, FUSE = 1, 2, 4, 16
STEP_FLAGS = [0, SUBST, DIAG_V1, FUSE]
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    from importlib import import_module

    assert (SUBST, RHS_UPPER, DIAG_V1, FUSE) == tuple(getattr(pkg()._backend, "POTRF_" + n) for n in ("SUBST", "RHS_UPPER", "DIAG_V1", "FUSE"))
    return import_module("t-svgp_amd.estep").EStepEngine(torch.float64, DEV)


@functools.lru_cache(maxsize=None)
def _spd(M, batch, seed=5):
    """test_potrf's matrices, a different draw per batch member, and their LAPACK factors (computed once, never written)."""
    rng = np.random.RandomState(seed + M)
    G = rng.randn(batch, M, M)
    A = G @ np.swapaxes(G, -1, -2) / M + 0.5 * np.eye(M)
    L = np.linalg.cholesky(A)
    A.setflags(write=False)
    L.setflags(write=False)
    return A, L


def _run(eng, entry, A, flags, lda, stride, rhs=None, off=0, check=True, aux_off=0):
    """One call of ``entry`` on NaN-filled buffers holding tril(A[b]) and the rows rhs[b] at A + b*stride; ``off``: doubles
    between the 16-byte boundary and A, ``aux_off``: the same for work, X, Xt and T.  Returns dict(rc, info, mats [batch, rows,
    lda], gaps [batch, stride - rows*lda], X, Xt)."""
    B = pkg()._backend
    batch, M = A.shape[0], A.shape[-1]
    rhs_rows = 0 if rhs is None else rhs.shape[1]
    rows = M + rhs_rows
    host = np.full(batch * stride, np.nan)
    lower = np.tril(np.ones((M, M), dtype=bool))
    for b in range(batch):
        v = host[b * stride:b * stride + rows * lda].reshape(rows, lda)
        v[:M, :M][lower] = A[b][lower]
        if rhs is not None:
            v[M:, :M] = rhs[b]
    buf = torch.full((batch * stride + off + 2,), NAN, dtype=torch.float64, device=DEV)
    assert buf.data_ptr() % 16 == 0
    a = buf[off:off + batch * stride]
    a.copy_(torch.from_numpy(host))
    info = torch.full((batch,), 77, dtype=torch.int32, device=DEV)
    aux = lambda n: torch.full((n + aux_off,), NAN, dtype=torch.float64, device=DEV)[aux_off:]
    work = aux(batch * NB * NB)
    X = Xt = None
    if entry == "potrf":
        rc = eng.lib.tsvgp_potrf_f64(a.data_ptr(), M, lda, batch, stride, info.data_ptr(), work.data_ptr(), flags, eng._stream())
    elif entry == "potrf_solve":
        rc = eng.lib.tsvgp_potrf_solve_f64(a.data_ptr(), M, lda, batch, stride, info.data_ptr(), work.data_ptr(), rhs_rows, flags,
                                           eng._stream())
    else:
        X, Xt, T = (aux(batch * M * M).view(batch, M, M) for _ in range(3))
        rc = eng.lib.tsvgp_potrf_inv_f64(a.data_ptr(), M, lda, batch, stride, info.data_ptr(), work.data_ptr(), X.data_ptr(),
                                         Xt.data_ptr(), T.data_ptr(), flags, eng._stream())
    if check:
        B.check(rc, "tsvgp_" + entry)
    torch.cuda.synchronize()
    out = a.cpu().numpy().reshape(batch, stride)
    assert np.isnan(buf[:off].cpu().numpy()).all() and np.isnan(buf[off + batch * stride:].cpu().numpy()).all()
    return dict(rc=rc, info=info.cpu().numpy(), mats=out[:, :rows * lda].reshape(batch, rows, lda), gaps=out[:, rows * lda:], X=X, Xt=Xt)


def _check_member(res, b, M, L_ref, R_ref=None, tol_L=1e-12, tol_R=1e-11):
    """Matrix b of a finished call: the factor, the solved rows, exact zeros and untouched sentinels."""
    mat = res["mats"][b]
    blk = np.kron(np.eye(M // NB), np.ones((NB, NB))).astype(bool)  # the diagonal 128 x 128 tiles
    above = np.kron(np.triu(np.ones((M // NB, M // NB)), 1), np.ones((NB, NB))).astype(bool)
    upper = np.triu(np.ones((M, M), dtype=bool), 1)
    Lk = mat[:M, :M]
    assert relerr(np.tril(Lk), L_ref) < tol_L
    assert np.all(Lk[blk & upper] == 0.0)  # the strict upper part of the diagonal tiles: written, as zeros
    assert np.isnan(Lk[above]).all()  # blocks above the diagonal: never touched
    assert np.isnan(mat[:, M:]).all()  # columns [M, lda)
    assert np.isnan(res["gaps"][b]).all()  # the rows between this matrix and the next
    if R_ref is not None:
        assert relerr(mat[M:, :M], R_ref) < tol_R


def _solve_ref(L, rhs):
    return np.linalg.solve(L, np.swapaxes(rhs, -1, -2)).swapaxes(-1, -2)  # B L^-T


# ------------------------------------------------------------------------------------------------ (a) layout x block step
@pytest.mark.parametrize("lda_extra", [2, 64])
@pytest.mark.parametrize("M", [128, 256, 384])
@pytest.mark.parametrize("entry,flags", [("potrf", f) for f in STEP_FLAGS] + [("potrf_inv", 0), ("potrf_inv", SUBST)])
def test_padded_rows_and_gapped_batches_under_every_block_step(eng, entry, flags, M, lda_extra):
    """lda > M and two spare rows behind every matrix of a batch of three, which no engine call ever passes: every kernel of the
    block step addresses rows by lda and matrices by stride, and writes nothing outside the block lower triangle.  For the inverse
    path also X = inv(L) against LAPACK, exact zeros above the diagonal of X and below that of Xt, and Xt = X^T bit for bit."""
    batch, lda = 3, M + lda_extra
    A, L = _spd(M, batch)
    res = _run(eng, entry, A, flags, lda, (M + 2) * lda)
    assert not res["info"].any()
    for b in range(batch):
        _check_member(res, b, M, L[b])
    if entry == "potrf_inv":
        X, Xt = res["X"], res["Xt"]
        assert torch.equal(Xt, X.transpose(-1, -2))
        Xn, Xtn = X.cpu().numpy(), Xt.cpu().numpy()
        assert relerr(Xn, np.linalg.inv(L)) < 1e-11
        assert np.all(np.triu(Xn, 1) == 0.0) and np.all(np.tril(Xtn, -1) == 0.0)


def test_twelve_block_steps(eng):
    """M = 1536: the longest chain of block steps any model here runs, in the plain engine layout."""
    M = 1536
    A, L = _spd(M, 1)
    res = _run(eng, "potrf", A, 0, M, M * M)
    assert not res["info"].any()
    _check_member(res, 0, M, L[0])


# ------------------------------------------------------------------------------------------------ (b) dense right-hand side
@pytest.mark.parametrize("M,rhs_rows", [(128, 128), (256, 128), (128, 384), (384, 256)])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("flags", STEP_FLAGS)
def test_dense_rows_ride_through_every_block_step(eng, flags, batch, M, rhs_rows):
    """tsvgp_potrf_solve_f64 without TSVGP_POTRF_RHS_UPPER -- t_VGP's whole solve, and with TSVGP_POTRF_DIAG_V1 in the environment
    the round-4 panels under it -- with fewer, as many and more rows than the matrix has: the rows come out as B L^-T."""
    lda = M + 2
    A, L = _spd(M, batch)
    rhs = np.random.RandomState(100 + M + rhs_rows).randn(batch, rhs_rows, M)
    res = _run(eng, "potrf_solve", A, flags, lda, (M + rhs_rows + 2) * lda, rhs=rhs)
    assert not res["info"].any()
    R = _solve_ref(L, rhs)
    for b in range(batch):
        _check_member(res, b, M, L[b], R[b])


# ------------------------------------------------------------------------------------------------ (c) block upper triangular rows
@pytest.mark.parametrize("M,rhs_rows", [(384, 128), (384, 256), (384, 384), (256, 256)])
@pytest.mark.parametrize("flags", [RHS_UPPER, RHS_UPPER | SUBST])
def test_rhs_upper_skips_only_products_with_zero_blocks(eng, flags, M, rhs_rows):
    """TSVGP_POTRF_RHS_UPPER with rhs_rows < M, where block step k carries min(rhs_rows, 128 (k + 1)) rows and the min bites
    before the last step.  The contract is exact zeros in row block i, column blocks < i; what the flag skips is then products
    with zero blocks (0 * x accumulated onto +0 is +0, and a tile minus such a product is the tile), so the buffer equals, bit
    for bit, the one the same call leaves without the flag."""
    batch, lda = 2, M + 2
    A, L = _spd(M, batch)
    rhs = np.random.RandomState(200 + M + rhs_rows).randn(batch, rhs_rows, M)
    for i in range(rhs_rows // NB):
        rhs[:, i * NB:(i + 1) * NB, :i * NB] = 0.0
    stride = (M + rhs_rows + 2) * lda
    res = _run(eng, "potrf_solve", A, flags, lda, stride, rhs=rhs)
    assert not res["info"].any()
    R = _solve_ref(L, rhs)
    for b in range(batch):
        _check_member(res, b, M, L[b], R[b])
    dense = _run(eng, "potrf_solve", A, flags & ~RHS_UPPER, lda, stride, rhs=rhs)
    assert np.array_equal(res["mats"], dense["mats"], equal_nan=True)
    for i in range(rhs_rows // NB):  # the skipped blocks are still the zeros they were
        assert np.all(res["mats"][:, M + i * NB:M + (i + 1) * NB, :i * NB] == 0.0)


# ------------------------------------------------------------------------------------------------ (d) info
def _first_bad_pivot(A):
    """Unblocked Cholesky of the lower triangle (the elimination LAPACK's dpotrf2 ends in): the 1-based index of the first pivot
    that is not > 0 -- NaN included -- or 0."""
    n = A.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0.0:
            return j + 1
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return 0


INFO_FORMS = [("potrf", f) for f in STEP_FLAGS] + [("potrf_inv", 0), ("potrf_solve", 0), ("potrf_solve", RHS_UPPER)]
DEFECTS = [("neg", c) for c in (1, 4, 5, 16, 17, 128, 129, 256)] + [("zero", 130), ("nan", 5), ("nan", 129), ("two", 70)]


@functools.lru_cache(maxsize=None)
def _defective(kind, c):
    """Member 1 of the M = 256 batch with its defect, and the index the reference elimination reports for it."""
    M = 256
    A, L = _spd(M, 3)
    bad = A[1].copy()
    if kind == "neg":  # pivot c of the elimination is A[c-1, c-1] - |L[c-1, :c-1]|^2 = L[c-1, c-1]^2: take twice that away
        bad[c - 1, c - 1] -= 2.0 * L[1, c - 1, c - 1] ** 2
    elif kind == "two":  # two defects in different blocks: the first one is reported
        for d in (c, 200):
            bad[d - 1, d - 1] -= 2.0 * L[1, d - 1, d - 1] ** 2
    elif kind == "nan":
        bad[c - 1, c - 1] = np.nan
    else:  # block diagonal with a 1 x 1 zero block: row c-1 of the factor is exactly 0 and so is the pivot
        bad[c - 1, :] = 0.0
        bad[:, c - 1] = 0.0
    expect = _first_bad_pivot(bad)
    assert expect == c  # (the test's own construction)
    bad.setflags(write=False)
    return bad, expect


@pytest.mark.parametrize("kind,c", DEFECTS)
@pytest.mark.parametrize("entry,flags", INFO_FORMS)
def test_info_is_lapacks_for_a_defect_in_the_middle_member(eng, entry, flags, kind, c):
    """The first pivot that is not positive, 1-based, as dpotrf reports it -- at both ends of a 4-column pivot group (4, 5), of a
    16-wide sub-block (16, 17), of a 128-wide block (128, 129, where the pivot has been through a trailing update) and of the
    matrix (1, 256); an exactly zero pivot; a NaN pivot; two defects -- in member 1 of 3, whose neighbours report 0 and come out
    right."""
    M, batch, lda = 256, 3, 258
    A, L = _spd(M, batch)
    bad, expect = _defective(kind, c)
    mats = np.stack([A[0], bad, A[2]])
    rhs = None
    if entry == "potrf_solve":
        rhs = np.random.RandomState(300).randn(batch, M, M)
        if flags & RHS_UPPER:
            rhs[:, NB:, :NB] = 0.0
    res = _run(eng, entry, mats, flags, lda, (M + (0 if rhs is None else M) + 2) * lda, rhs=rhs)
    assert res["info"].tolist() == [0, expect, 0]
    for b in (0, 2):
        _check_member(res, b, M, L[b], None if rhs is None else _solve_ref(L[b], rhs[b]))
    if entry == "potrf_inv":
        Xn = res["X"].cpu().numpy()
        assert relerr(Xn[[0, 2]], np.linalg.inv(L[[0, 2]])) < 1e-11


@pytest.mark.parametrize("entry", ["potrf", "potrf_solve", "potrf_inv"])
def test_accepted_neighbours_of_the_rejected_layouts_run(eng, entry):
    """tests/test_cabi.py holds that an odd lda, a misaligned A, an odd or overlapping stride are rejected; here the calls one
    argument away from them -- an even lda, A two doubles behind the boundary, an even stride, matrices that just touch -- return 0
    and factor.  One matrix with no rows takes any stride."""
    M = NB
    rhs_rows = M if entry == "potrf_solve" else 0
    rhs = np.random.RandomState(400).randn(2, rhs_rows, M) if rhs_rows else None
    A, L = _spd(M, 2)
    for name, ok, _ in potrf_layout_cases(M, rhs_rows):
        res = _run(eng, entry, A, 0, ok["lda"], ok["stride"], rhs=rhs, off=ok["off"], check=False)
        assert res["rc"] == 0, name
        assert not res["info"].any()
        for b in range(2):
            _check_member(res, b, M, L[b], None if rhs is None else _solve_ref(L[b], rhs[b]))
    if rhs_rows == 0:
        res = _run(eng, entry, A[:1], 0, M + 2, M * (M + 2) + 1, check=False)
        assert res["rc"] == 0 and not res["info"].any()
        _check_member(res, 0, M, L[0])
    # work, and X, Xt, T of the inverse path, two doubles behind the boundary (one double behind it is rejected); two block steps,
    # so that the panels read work and the inverse recursion goes through T
    M2 = 2 * NB
    A2, L2 = _spd(M2, 2)
    rhs2 = np.random.RandomState(401).randn(2, rhs_rows, M2) if rhs_rows else None
    for flags in (0, DIAG_V1):  # (the round-4 panel product is what reads work with 16-byte loads)
        res = _run(eng, entry, A2, flags, M2 + 2, (M2 + rhs_rows + 2) * (M2 + 2), rhs=rhs2, check=False, aux_off=POTRF_AUX_OFF[0])
        assert res["rc"] == 0 and not res["info"].any()
        for b in range(2):
            _check_member(res, b, M2, L2[b], None if rhs2 is None else _solve_ref(L2[b], rhs2[b]))
        if entry == "potrf_inv":
            assert torch.equal(res["Xt"], res["X"].transpose(-1, -2))
            assert relerr(res["X"].cpu().numpy(), np.linalg.inv(L2)) < 1e-11


def test_engine_copies_an_overwritable_view_that_is_off_the_16_byte_boundary(eng):
    """``EStepEngine.cholesky(overwrite=True)`` factors a contiguous caller's temporary in place; a contiguous [M, M] view at an odd
    element offset of its storage is not on the boundary the entry demands, so the engine factors a copy: the call succeeds, the
    factor is right and the view keeps its contents.  The same view one element further on IS factored in place."""
    M = 256
    A, L = _spd(M, 1)
    for off in (1, 2):
        store = torch.zeros(M * M + 2, dtype=torch.float64, device=DEV)
        view = store[off:off + M * M].view(M, M)
        view.copy_(torch.tensor(A[0]))
        assert view.is_contiguous() and view.data_ptr() % 16 == 8 * (off % 2)
        Lk, info = eng.cholesky(view, overwrite=True)
        torch.cuda.synchronize()
        assert int(info.abs().sum()) == 0
        assert relerr(Lk.cpu().numpy(), L[0]) < 1e-12
        assert torch.equal(view.cpu(), torch.tensor(A[0])) == (off == 1)


# ------------------------------------------------------------------------------------------------ (e) conditioning ladder
@functools.lru_cache(maxsize=None)
def _ladder(M, jitter):
    """SE kernel matrix on sorted 1-D points (the LEADING diagonal block is itself ill-conditioned), LAPACK's factor, and kappa =
    the largest 2-norm condition number of the factor's 128 x 128 diagonal blocks: what a panel multiplied by inv(L_kk) can lose."""
    x = np.sort(np.random.RandomState(3).rand(M)) * M / 40
    A = np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2) + jitter * np.eye(M)
    L = np.linalg.cholesky(A)
    kappa = max(np.linalg.cond(L[i:i + NB, i:i + NB]) for i in range(0, M, NB))
    rhs = np.random.RandomState(4).randn(1, NB, M)
    for a in (A, L, rhs):
        a.setflags(write=False)
    return A, L, kappa, rhs


def _exact(a):
    return np.asarray(a, dtype=np.longdouble)


LADDER = [(M, j) for M in (256, 384) for j in (1e-2, 1e-4, 1e-5, 1e-6)]


@pytest.mark.parametrize("M,jitter", LADDER)
@pytest.mark.parametrize("flags", STEP_FLAGS)
def test_backward_error_up_to_the_route_gate(eng, flags, M, jitter):
    """cond_2(A) = 9.4e3 .. 9.4e7, the range below and just above the 1e7 at which the models ask for substitution panels: the
    substitution panels stay at LAPACK's backward error (50 eps max|A|, the bound of the cond-1e14 test), the inverse-based block
    steps within eps * kappa * max|A|, the loss include/tsvgp_hip.h states for them (a NumPy emulation of 128-wide inverse-based
    panels measured <= 0.1 eps kappa: 10 x headroom).  The residual is formed in extended precision."""
    A, L_ref, kappa, _ = _ladder(M, jitter)
    res = _run(eng, "potrf", A[None], flags, M, M * M)
    assert not res["info"].any()
    Lk = _exact(np.tril(res["mats"][0][:, :M]))
    ratio = float(np.max(np.abs(Lk @ Lk.T - _exact(A)))) / (EPS * np.max(np.abs(A)))
    bound = 50.0 if flags & SUBST else max(50.0, kappa)
    print(f"potrf flags={flags} M={M} jitter={jitter:g} kappa={kappa:.3g}: backward error / (eps max|A|) = {ratio:.3g} (bound {bound:.3g})")
    assert ratio <= bound


@pytest.mark.parametrize("M,jitter", LADDER)
@pytest.mark.parametrize("flags", STEP_FLAGS)
def test_solved_rows_residual_up_to_the_route_gate(eng, flags, M, jitter):
    """128 dense rows through the same matrices, judged against the kernel's OWN factor: by substitution componentwise
    |R L^T - B| <= M eps |R| |L^T| (the gamma_M bound of a triangular solve), through the inverted diagonal blocks the same times
    max(1, kappa)."""
    A, _, kappa, rhs = _ladder(M, jitter)
    res = _run(eng, "potrf_solve", A[None], flags, M, (M + NB) * M, rhs=rhs)
    assert not res["info"].any()
    Lk, R = _exact(np.tril(res["mats"][0][:M, :M])), _exact(res["mats"][0][M:, :M])
    resid = np.abs(R @ Lk.T - _exact(rhs[0]))
    scale = np.abs(R) @ np.abs(Lk.T)
    ratio = float(np.max(resid / scale)) / EPS
    bound = M * (1.0 if flags & SUBST else max(1.0, kappa))
    print(f"potrf_solve flags={flags} M={M} jitter={jitter:g} kappa={kappa:.3g}: residual / (eps |R||L^T|) = {ratio:.3g} (bound {bound:.3g})")
    assert ratio <= bound


# ------------------------------------------------------------------------------------------------ (f) scale
@pytest.mark.parametrize("flags", [0, SUBST])
@pytest.mark.parametrize("e", [-40, 40])
def test_scale_far_from_one(eng, flags, e):
    """The kernel variance multiplies K_uu.  A power of two scales every intermediate exactly, so the factor of 2^e A is 2^(e/2)
    times the factor of A: the reciprocal square roots (hardware estimate + one third-order step) hold away from unit scale."""
    M, batch, lda = 256, 3, 258
    A, L = _spd(M, batch)
    res = _run(eng, "potrf", A * 2.0 ** e, flags, lda, (M + 2) * lda)
    assert not res["info"].any()
    for b in range(batch):
        _check_member(res, b, M, L[b] * 2.0 ** (e // 2))
