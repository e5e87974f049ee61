"""The exact-arithmetic probes of tests/npass_ref.py, checked without a GPU:

(a) the exactness condition (``absum`` below 2^24 / 2^53) for every case tests/test_gpu_npass_values.py parametrises over -- the case
    lists are imported from npass_ref.py by both files;
(b) the references against a row-by-row / einsum restatement and ``_moments_ref`` of tests/test_gpu_kernels.py on the smallest cases;
(c) the probes see what they are for: ten simulated kernel faults applied to the reference in NumPy, each of which the bit-for-bit
    comparison must notice in every case the fault applies to, in both dtypes.  Fault 10 (the one row with the smallest dyadic weight
    dropped) is also run through the earlier rule of tests/test_gpu_kernels.py, ``relerr < 50 tol``, which does not notice it: the
    gap this file closes.

A fault of the ``Tm`` read (1 - 4) applies to ``trmm`` and to the moments; where it applies: a strict diagonal bound only in the
triangular modes, a dropped chunk of a column tile behind the first only from two tiles on.  The moments cases with N = 1 carry one
4-sparse row, which touches four columns: they are there for the row tail, and only the faults of the counts (9) are asked of them.
"""
import numpy as np
import pytest

from tests import npass_ref as R
from tests.helpers import relerr

TILE = R.TILE
NP_DTYPES = {"f32": np.float32, "f64": np.float64}


def differs(fault, ref):
    """The bit-for-bit comparison of the GPU file sees the fault in both compute dtypes."""
    return all(R.first_difference(np.asarray(fault).astype(dt), np.asarray(ref).astype(dt)) is not None for dt in NP_DTYPES.values())


# ------------------------------------------------------------------------------------------------ faults of the Tm read (1 - 4)
def tm_read_faults(Tm, mode):
    """(name, rows I, replacement of Tm[I, :]) for faults 1 - 4 of one [Mp, Mp] operand."""
    Mp = Tm.shape[0]
    nt = Mp // TILE
    out = []
    if mode != R.DENSE:  # 1: j < i where j <= i is meant (or the mirror)
        out.append(("1 strict diagonal bound", np.arange(Mp), Tm - np.diag(np.diag(Tm))))
    for it in sorted({0, nt // 2, nt - 1}):  # 2: the last 16 columns of the diagonal k-tile
        I = np.arange(it * TILE, (it + 1) * TILE)
        rows = Tm[I].copy()
        rows[:, (it + 1) * TILE - 16:(it + 1) * TILE] = 0.0
        out.append((f"2 last 16 columns of the diagonal k-tile dropped, tile {it}", I, rows))
    if nt >= 2:  # 3: one 16-column chunk of a column tile behind the first
        I = np.arange(TILE, 2 * TILE)
        rows = Tm[I].copy()
        lo = Mp - 16 if mode == R.UPPER else 0  # (inside the range of tile 1 in every mode)
        rows[:, lo:lo + 16] = 0.0
        out.append(("3 one k-chunk dropped in tile 1", I, rows))
    for b in sorted({0, (Mp // 32) * 16 + 16 if Mp > 32 else 0, Mp - 16}):  # 4: one 16 x 16 diagonal block read transposed
        I = np.arange(b, b + 16)
        rows = Tm[I].copy()
        rows[:, b:b + 16] = Tm[b:b + 16, b:b + 16].T
        out.append((f"4 diagonal block at {b} read transposed", I, rows))
    return out


def swap_rows_xor8(x, r0):
    """5: rows n and n ^ 8 of the 16-row block at r0 swapped."""
    y = x.copy()
    idx = np.arange(r0, r0 + 16)
    y[idx] = x[idx ^ 8]
    return y


# ------------------------------------------------------------------------------------------------ trmm
@pytest.mark.parametrize("Mp,mode", R.TRMM_CASES)
def test_trmm_probes_are_exact_and_see_the_faults(Mp, mode):
    probes = [("placement", R.trmm_placement(Mp, mode))] + [(f"sum Np={Np}", R.trmm_sum(Mp, mode, Np)) for Np in R.TRMM_SUM_NP]
    for pname, c in probes:
        A, Tm, C = c["A"], c["Tm"], c["C"]
        assert c["absum"] < R.EXACT_LIMIT["f32"], (pname, c["absum"])  # (a): the fp32 limit is the tighter one
        assert np.all(Tm[R.tri_mask(Mp, mode) == 0] == 0)  # exactly zero outside the triangle: the header's contract
        assert np.array_equal(C.astype(np.float32).astype(np.float64), C)
        for name, I, rows in tm_read_faults(Tm, mode):
            Cf = C.copy()
            Cf[:, I] = A @ rows.T
            assert differs(Cf, C), (pname, name)
        for r0 in (0, A.shape[0] - 16):
            assert differs(swap_rows_xor8(C, r0), C), (pname, "5 rows n and n ^ 8 swapped", r0)
    if Mp == 1152:
        assert R.trmm_placement(Mp, mode)["Tm"].max() == 1152 * 1152  # the largest placement code, 1 327 104 < 2^24


def test_trmm_reference_restated():
    for mode in (R.LOWER, R.UPPER, R.DENSE):
        c = R.trmm_sum(128, mode, 256)
        rng = np.random.RandomState(1000 + 128 + 7 * mode + 256)
        A = rng.randint(-1, 2, (256, 128)).astype(np.float64)
        raw = rng.randint(-2, 3, (128, 128)).astype(np.float64)  # the unmasked draw: the ranges below do the masking
        C = np.zeros((256, 128))
        for i in range(128):
            js = {R.LOWER: range(0, i + 1), R.UPPER: range(i, 128), R.DENSE: range(128)}[mode]
            for j in js:
                C[:, i] += A[:, j] * raw[i, j]
        assert np.array_equal(A, c["A"]) and np.array_equal(C, c["C"])
        p = R.trmm_placement(128, mode)
        for i in range(128):
            for n in range(128):
                inside = {R.LOWER: n <= i, R.UPPER: n >= i, R.DENSE: True}[mode]
                assert p["C"][n, i] == (1 + i * 128 + n if inside else 0.0)


# ------------------------------------------------------------------------------------------------ moments
def check_moments_case(c, tm_faults):
    Mp, mode, P, N, Np = c["Mp"], c["mode"], c["P"], c["N"], c["Np"]
    for form in ("shared", "batched"):
        f = c[form]
        ref = f["ref"]
        assert f["absum"] < R.EXACT_LIMIT["f32"], (form, f["absum"])  # (a)
        var = ref["var"]
        assert (var == 0).any(), form  # an exact zero variance, which the header counts as non-positive
        if N >= 3:
            assert (var > 0).any() and (var < 0).any(), form
        if form == "batched":
            assert len(set(f["kdiag"])) == P
        # 9: the counts of non-positive variances
        nonpos = ref["nonpos"]
        bad_rows = np.zeros(Np, dtype=np.int64)
        bad_rows[:N] = np.sum(var < 0, axis=1)  # a var == 0 row is not counted
        assert not np.array_equal(bad_rows.reshape(-1, TILE).sum(axis=1), nonpos), (form, "9 var == 0 not counted")
        if N < Np:  # a row >= N of the last panel is counted
            over = nonpos.copy()
            over[-1] += 1
            assert not np.array_equal(over, nonpos)
        if Np > TILE and len(set(nonpos.tolist())) > 1:  # credited to the neighbouring block
            assert not np.array_equal(np.roll(nonpos, 1), nonpos), (form, "9 count credited to the neighbour")
        if not tm_faults:
            continue
        p = P - 1
        Ap = (f["A"][p] if form == "batched" else f["A"])[:N]
        kd = f["kdiag"][p] if form == "batched" else f["kdiag"]
        Tm = c["Tm"][p]
        for name, I, rows in tm_read_faults(Tm, mode):
            Cn, Cf = Ap @ Tm[I].T, Ap @ rows.T
            qf = ref["q"][:, p] - np.sum(Cn * Cn, axis=1) + np.sum(Cf * Cf, axis=1)
            assert differs(kd - qf, var[:, p]), (form, name)
        for r0 in (0, (N // 16 - 1) * 16):
            seen = [differs(swap_rows_xor8(ref[k][:N], r0), ref[k][:N]) for k in ("mean", "var", "g0")]
            assert any(seen), (form, "5 rows n and n ^ 8 swapped", r0)


@pytest.mark.parametrize("Mp,mode,P", R.MOMENTS_GRID)
def test_moments_grid_is_exact_and_sees_the_faults(Mp, mode, P):
    check_moments_case(R.moments_case(Mp, mode, P, R.grid_rows(Mp)), tm_faults=True)


@pytest.mark.parametrize("Mp,mode,P,N", R.MOMENTS_TAIL_CASES)
def test_moments_tails_are_exact_and_see_the_faults(Mp, mode, P, N):
    c = R.moments_case(Mp, mode, P, N)
    assert c["Np"] - N == {1: 127, 127: 1, 128: 0, 129: 127, 255: 1, 256: 0, 257: 127}[N]
    A = c["batched"]["A"][:, :N]
    assert (np.count_nonzero(A[:, :min(N, Mp)], axis=-1) == (1 if N >= Mp else 4)).all()  # 4-sparse rows only when N < Mp
    check_moments_case(c, tm_faults=N > 1)


@pytest.mark.parametrize("Mp,P", R.MEANONLY_CASES)
def test_mean_only_cases_are_exact(Mp, P):
    c = R.meanonly_case(Mp, P)
    assert c["absum"] < R.EXACT_LIMIT["f32"]
    assert differs(swap_rows_xor8(c["mean"], 16), c["mean"]) or differs(swap_rows_xor8(c["g0"], 16), c["g0"])


def test_wide_case_is_exact():
    A = R.wide_rows()
    assert R.WIDE_ABSUM < R.EXACT_LIMIT["f64"] and np.abs(A).sum(axis=1).max() == 4 and (np.abs(A).sum(axis=1)[:64] == 1).all()
    cols = np.argmax(A[:64], axis=1)
    assert len(set((cols // TILE).tolist())) == 64  # both sides of 32 tile edges


def test_moments_reference_restated():
    from tests.test_gpu_kernels import _moments_ref

    for mode in (R.LOWER, R.UPPER, R.DENSE):
        c = R.moments_case(128, mode, 3, R.grid_rows(128))
        f = c["shared"]
        mean, var = _moments_ref(f["A"][:c["N"]], c["Tm"], c["gamma"], f["kdiag"])
        assert np.array_equal(mean, f["ref"]["mean"]) and np.array_equal(var, f["ref"]["var"])
        q_unit = np.sum(c["Tm"] ** 2, axis=1).T  # rows 0 .. Mp - 1 are e_n: q_n is the column sum of squares over the triangle
        assert np.array_equal(f["kdiag"] - q_unit, f["ref"]["var"][:128]) and np.array_equal(c["gamma"], f["ref"]["mean"][:128])
        assert np.array_equal(f["ref"]["g0"][:c["N"]], 2 * (c["Y"] - mean)) and np.all(f["ref"]["g0"][c["N"]:] == 0)
        b = c["batched"]
        for p in range(3):
            mp_, vp_ = _moments_ref(b["A"][p][:c["N"]], c["Tm"][p:p + 1], c["gamma"][:, p:p + 1], b["kdiag"][p])
            assert np.array_equal(mp_[:, 0], b["ref"]["mean"][:, p]) and np.array_equal(vp_[:, 0], b["ref"]["var"][:, p])


# ------------------------------------------------------------------------------------------------ site sums
SITE_IDS = [f"Mp{Mp}-P{P}-Np{Np}" for Mp, P, Np, _ in R.SITE_CASES]


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("Mp,P,Np,nsplits", R.SITE_CASES, ids=SITE_IDS)
def test_site_cases_are_exact_and_see_the_faults(Mp, P, Np, nsplits, dt):
    c = R.site_case(Mp, P, Np, dt)
    esize = 8 if dt == "f64" else 4
    nt = Mp // TILE
    p = P - 1
    B, g0 = c["B"][0], c["g0"]
    if dt == "f64":
        assert c["E"] == 27  # down to 2^-26, the scale of the crop value -1e-8
    assert c["E"] >= 8
    for wname, w in c["sets"].items():
        assert w["absum"] < R.EXACT_LIMIT[dt], (wname, w["absum"])  # (a)
        g1 = w["g1"]
        assert not g1[-5:].any() and not g0[-5:].any() and (g1[:-5] < 0).all()
        acc2, acc1 = w["shared"]
        tile_sum = lambda rows, I, J: B[rows][:, I].T @ (g1[rows, p, None] * B[rows][:, J])
        # 6: the last chunk of a slice dropped / counted twice, on one tile of either partition
        ns = nsplits[len(nsplits) // 2]
        bounds, chunk = R.slice_bounds(Np, ns, esize, P)
        for part, (it, jt) in (("diag", (nt - 1, nt - 1)), ("off", (nt - 1, 0))):
            if part == "off" and nt < 2:
                continue
            I, J = np.arange(it * TILE, (it + 1) * TILE), np.arange(jt * TILE, (jt + 1) * TILE)
            live = [(lo, hi) for lo, hi in bounds[part] if hi > lo]
            for lo, hi in (live[0], live[-1]):
                D = tile_sum(np.arange(hi - chunk, hi), I, J)
                for sign in (-1.0, 1.0):
                    f2 = acc2.copy()
                    f2[p][np.ix_(I, J)] += sign * D
                    if part == "off":
                        f2[p][np.ix_(J, I)] += sign * D.T
                    assert R.first_difference(f2, acc2) is not None, (wname, "6", part, lo, hi, sign)
                    assert np.array_equal(f2[p], f2[p].T)  # (the symmetry check alone does not see it)
        # 7: the weights shifted by one row inside a chunk
        rows = np.arange(chunk)
        shifted = np.roll(g1[rows, p], -1) - g1[rows, p]
        f2 = acc2.copy()
        f2[p] += B[rows].T @ (shifted[:, None] * B[rows])
        assert R.first_difference(f2, acc2) is not None, (wname, "7 weights shifted by one row")
        # 8: one off-diagonal tile written transposed (and mirrored: still symmetric)
        if nt >= 2:
            I, J = np.arange((nt - 1) * TILE, nt * TILE), np.arange(TILE)
            f2 = acc2.copy()
            f2[p][np.ix_(I, J)] = acc2[p][np.ix_(I, J)].T
            f2[p][np.ix_(J, I)] = acc2[p][np.ix_(I, J)]
            assert np.array_equal(f2[p], f2[p].T) and R.first_difference(f2, acc2) is not None, (wname, "8 tile transposed")
        # the same on the per-latent operands
        b2, b1 = w["batched"]
        assert np.array_equal(b2[0], acc2[0]) and np.array_equal(b1[0], acc1[0])
        if P > 1:
            assert R.first_difference(b2[1], acc2[1]) is not None
    # 10: the ONE row with the smallest dyadic weight dropped
    w = c["sets"]["dyadic"]
    g1, (acc2, acc1) = w["g1"], w["shared"]
    n_small = int(np.argmax(g1[:, 0] == -2.0 ** -(c["E"] - 1)))
    assert g1[n_small, 0] == g1[:-5, 0].max() < 0
    f2 = acc2.copy()
    f2[0] -= g1[n_small, 0] * np.outer(B[n_small], B[n_small])
    assert R.first_difference(f2, acc2) is not None, "10 smallest-weight row dropped"
    # ... which the rule of tests/test_gpu_kernels.py::test_site_accum, relerr < 50 tol, cannot see.  In fp64 that holds from
    # max|acc2| > 4 * 2^-26 / 5e-10 = 119 on, which the Np = 4096 case reaches; the cases of a few hundred rows have sums of 20 to
    # 100, where 2^-26 is still (just) above 5e-10 relative
    old_tol = 50 * (1e-11 if dt == "f64" else 2e-5)
    if dt == "f32" or Np == 4096:
        assert relerr(f2, acc2) < old_tol, relerr(f2, acc2)
        assert np.array_equal(f2[0], f2[0].T)


def test_site_slice_lengths_cover_0_to_5_on_both_partitions():
    """Computed from the launcher's formulas (include/tsvgp_hip.h): slices of 0, 1, 2, 3, 4 and 5 chunks, a short last slice and empty
    trailing slices, on the diagonal and on the off-diagonal partition, in each of the three kernels' chunk sizes."""
    for esize, Pk in ((8, 1), (8, 9), (4, 1), (4, 9)):
        seen = {"off": set(), "diag": set()}
        short, empty = set(), set()
        for Mp, P, Np, nsplits in R.SITE_CASES:
            if Mp < 2 * TILE or (P <= 8) != (Pk <= 8):
                continue
            for ns in nsplits:
                for part, lens in R.slice_lengths(Np, ns, esize, P).items():
                    assert sum(lens) == Np // R.site_chunk(esize, P)
                    seen[part] |= set(lens)
                    nonempty = [x for x in lens if x]
                    if nonempty[-1] < nonempty[0]:
                        short.add(part)
                    if lens[-1] == 0:
                        empty.add(part)
        for part in ("off", "diag"):
            assert set(range(6)) <= seen[part], (esize, Pk, part, sorted(seen[part]))
        assert short == {"off", "diag"} and empty == {"off", "diag"}, (esize, Pk)
    assert any(Np == 4096 for _, _, Np, _ in R.SITE_CASES)
    assert {Mp for Mp, *_ in R.SITE_CASES} == {128, 256, 384, 1024} and {P for _, P, *_ in R.SITE_CASES} == {1, 3, 8, 9}


def test_site_reference_restated():
    c = R.site_case(128, 3, 128, "f64")
    for w in c["sets"].values():
        ref2 = np.einsum("nm,no,nl->lmo", c["B"][0], c["B"][0], w["g1"])
        ref1 = np.einsum("nm,nl->lm", c["B"][0], c["g0"])
        assert np.array_equal(ref2, w["shared"][0]) and np.array_equal(ref1, w["shared"][1])
        bat2 = np.einsum("lnm,lno,nl->lmo", c["B"], c["B"], w["g1"])
        assert np.array_equal(bat2, w["batched"][0])


def test_rounding_operands_are_graded():
    op = R.rounding_operands(128, R.LOWER, 3, np.float32)
    assert np.array_equal(op["A"].astype(np.float32).astype(np.float64), op["A"]) and not op["A"][:, 128 - 37:].any()
    assert not op["Tm"][:, 128 - 37:].any() and not op["Tm"][:, :, 128 - 37:].any() and not np.triu(op["Tm"][0], 1).any()
    assert op["g1"][26, 0] == -2.0 ** -26 and op["g1"][27, 0] == -1.0 and not op["g1"][op["N"]:].any()
    b = R.rounding_bounds(op, 2.0 ** -24)
    for ref, bound, absum in b.values():
        assert ref.shape == bound.shape == absum.shape and (bound >= 0).all()
