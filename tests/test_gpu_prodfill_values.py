"""``tsvgp_kernel_fill_prod_*`` entry by entry against the longdouble reference of tests/kernel_value_ref.py, no new constants.

The problem is ``product_kernel_ref.value_problem`` on the component lists of tests/test_gpu_sumfill_values.py (the geometry of
the two fills is shared, and so is the shape list): component c takes ``inv_ls[c]`` and its own kind, components 1.. with their
row times 1/16 (the inclusion condition, asserted on the CPU by tests/test_product_kernel_cpu.py).  Reference:
variance * prod_c ``reference(kind_c, ...)["K"]`` in longdouble.  Bound per entry, relative:

    sum_c rel_bound(kind_c, T, ref_c, D, factor=GPU_FACTOR)  +  C * u

(every component under its own derived bound; C - 1 multiplications of the running product and the one by the variance).
Entries whose reference is below 1e3 * tiny follow ``check_values``' absolute rule; at least 90 % are held to the relative one.
Outputs are NaN-filled before every call: the padding inside [Np, cols_pad] must be exact zeros and everything beyond it still
NaN."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import kernel_value_ref as R
from tests import product_kernel_ref as PR
from tests.helpers import pkg
from tests.test_gpu_sumfill_values import COL_TILE, DEV, DTYPES, GUARD, IDS, NAN, SPECS, _check_layout, _ru, _t

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _problem(C, dtype, N, M, D, x_is_z=False):
    return PR.value_problem(SPECS[C], R.np_type(dtype), N, M, D, x_is_z=x_is_z)


def _prod_fill(pr, dtype, N, M, D, ldk, offset=0, x_is_z=False):
    """One call into a NaN-filled [Np, ldk] view ``offset`` elements behind a 256-byte boundary; checks the guards."""
    B = pkg()._backend
    C = len(pr["kinds"])
    Np = _ru(N)
    flat = torch.full((GUARD + offset + Np * ldk + GUARD,), NAN, dtype=dtype, device=DEV)
    start = GUARD + offset
    out = flat[start:start + Np * ldk].view(Np, ldk)
    Zt, il = _t(pr["Z"], dtype), _t(pr["inv_ls"], dtype)
    Xt = Zt if x_is_z else _t(pr["X"], dtype)
    kinds = (ctypes.c_int * C)(*[R.KINDS[k] for k in pr["kinds"]])
    fn = getattr(B.lib(), f"tsvgp_kernel_fill_prod_{B.suffix(dtype)}")
    B.check(fn(kinds, Xt.data_ptr(), Zt.data_ptr(), il.data_ptr(), pr["variance"], out.data_ptr(), N, M, D, ldk, C,
               torch.cuda.current_stream(DEV).cuda_stream), "kernel_fill_prod")
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat[:start]).all()) and bool(torch.isnan(flat[start + Np * ldk:]).all())
    return out


def _check_values(pr, got, what, min_frac=0.9):
    """``check_values`` uses its ``variance`` argument for one thing only, the cap of the small entries: an entry whose reference
    is below 1e3 * tiny must satisfy 0 <= K <= 2e3 * tiny * variance, twice the largest reference the rule covers when the
    variance is 1 (the sum test passes the summed variance, 1.3 to 2.8).  The product of the components' variances is 0.104 at
    C = 4, where 2e3 * tiny * variance would lie BELOW references the rule itself covers (up to 1e3 * tiny).  What is passed here
    is therefore NOT the variance but the cap's scale, max(1, variance), so that the cap admits every reference it covers with
    the same factor of two; a deviation from how the sum test calls it, and the only one."""
    cap_scale = max(1.0, pr["variance"])
    worst, frac = R.check_values(got.double().cpu().numpy(), pr["ref"], pr["bound"], pr["T"], cap_scale, what)
    assert frac >= min_frac
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("D", [1, 3, 8, 16, 32])
def test_prod_fill_values(dtype, C, D):
    """N = 130: the 8-row workgroups, two row tiles and a ragged tail; M one past the column tile; D padded to 1, 4, 8, 16, 32;
    C * Dpad <= 32 keeps every component's Z columns in registers, beyond (D = 16 with C = 4, D = 32 with C = 2, 4) the row-chunk
    form reloads them.  Mixed kinds, components with zeroed columns."""
    N, M = 130, COL_TILE[dtype] + 1
    pr = _problem(C, dtype, N, M, D)
    out = _prod_fill(pr, dtype, N, M, D, _ru(M) + 4)
    _check_layout(out, N, M)
    _check_values(pr, out[:N, :M], f"prod fill C={C} D={D} {N} x {M}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,M", [(R.MIN_ROWS, R.K_SAME + 1), (65, 511), (129, 513), (1, 130), (130, 3)])
def test_prod_fill_small_and_ragged_shapes(dtype, N, M):
    """The smallest grid, rows one past a 64 and a 128 multiple, columns either side of the fp64 column tile, one row, three
    columns (a grid asked for below its minimum size is made at the minimum and cut).  The grid plants N_FAR = 2 rows far beyond
    underflow whatever N is: of the smallest grid's 12 rows they are more than a tenth, so there the relative rule must hold
    every other row, (N - N_FAR) / N of the entries.  N = 1 is row 0 of a grid made at MIN_ROWS: what fraction of ONE row is
    relative says nothing about the grid, so no fraction is asserted there (the values are checked all the same)."""
    C, D = 2, 3
    pr = _problem(C, dtype, N, M, D)
    out = _prod_fill(pr, dtype, N, M, D, _ru(M))
    _check_layout(out, N, M)
    _check_values(pr, out[:N, :M], f"prod fill {N} x {M}", min_frac=0.0 if N < R.MIN_ROWS else min(0.9, (N - R.N_FAR) / N - 1e-12))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C,D,M", [(2, 8, 130), (4, 32, 130), (2, 3, 1025)])
def test_prod_fill_on_the_production_row_path(dtype, C, D, M):
    """N > 4096: the 64-row workgroups of the N-sized operand.  N = 4166: the block of row 4160 has 6 valid rows and 58 zero rows,
    the last block none.  M = 1025: a third (fp64) / second (fp32) column tile with one live column."""
    N = 4096 + 70
    pr = _problem(C, dtype, N, M, D)
    out = _prod_fill(pr, dtype, N, M, D, _ru(M) + 4)
    assert _ru(N) == 4224
    _check_layout(out, N, M)
    _check_values(pr, out[:N, :M], f"prod fill 64-row blocks C={C} D={D} M={M}")


@pytest.mark.parametrize("layout", ["ldk = Mp + 2", "K 8 bytes off"])
@pytest.mark.parametrize("C,D", [(2, 8), (4, 16)])
def test_fp32_prod_fill_with_two_columns_per_thread(layout, C, D):
    """The fp32 fallback to 8-byte stores (an odd pair offset of K): the same entrywise bound, and the values of the four-column
    form bit for bit (packed arithmetic per column pair in both)."""
    dtype, N, M = torch.float32, 130, 513
    Mp = _ru(M)
    pr = _problem(C, dtype, N, M, D)
    wide = _prod_fill(pr, dtype, N, M, D, Mp + 4)
    ldk, off = (Mp + 2, 0) if layout == "ldk = Mp + 2" else (Mp + 4, 2)
    out = _prod_fill(pr, dtype, N, M, D, ldk, offset=off)
    assert (out.data_ptr() % 16 == 8) == (off == 2)
    _check_layout(out, N, M)
    _check_values(pr, out[:N, :M], f"fp32 prod fill, two columns, {layout}")
    assert torch.equal(out[:, :Mp], wide[:, :Mp])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C,D", [(2, 3), (4, 32)])
def test_prod_fill_kzz_is_symmetric_and_reproducible(dtype, C, D):
    """The K(Z, Z) call (X is Z, one pointer): values, exact symmetry, a diagonal of exactly variance * 1, two calls bit for bit."""
    M = 130
    pr = _problem(C, dtype, M, M, D, x_is_z=True)
    a = _prod_fill(pr, dtype, M, M, D, _ru(M), x_is_z=True)
    b = _prod_fill(pr, dtype, M, M, D, _ru(M), x_is_z=True)
    _check_layout(a, M, M)
    _check_values(pr, a[:M, :M], f"prod fill K(Z, Z) C={C} D={D}")
    assert torch.equal(a[:M, :M], a[:M, :M].t())
    assert torch.equal(a, b)
    assert bool((a[:M, :M].diagonal() == torch.tensor(pr["variance"], dtype=dtype, device=DEV)).all())


def _identity_pair(dtype, scale):
    """Product([SE(dims 0, 1), SE(dims 2)]) and the plain fill of the ARD SquaredExponential with the product variance on one cloud
    of the given scale: (both outputs, their [N, M] values in float64, X, Z, the ARD inv_ls, the product's two rows)."""
    B = pkg()._backend
    T = R.np_type(dtype)
    N, M, D = 130, 513, 3
    rng = np.random.RandomState(11)
    X = (rng.randn(N, D) * scale).astype(T).astype(np.float64)
    Z = (rng.randn(M, D) * scale).astype(T).astype(np.float64)
    il = (1.0 / np.array([0.9, 1.2, 1.5])).astype(T).astype(np.float64)
    rows = np.array([[il[0], il[1], 0.0], [0.0, 0.0, il[2]]])
    v0, v1 = R.c_variance(1.3, T), R.c_variance(0.7, T)
    variance = R.c_variance(v0 * v1, T)
    pr = dict(X=X, Z=Z, inv_ls=rows, kinds=["SquaredExponential", "SquaredExponential"], variance=variance)
    got = _prod_fill(pr, dtype, N, M, D, _ru(M))
    plain = torch.full((_ru(N), _ru(M)), NAN, dtype=dtype, device=DEV)
    Xt, Zt, ilt = _t(X, dtype), _t(Z, dtype), _t(il, dtype)
    B.check(getattr(B.lib(), f"tsvgp_kernel_fill_{B.suffix(dtype)}")(
        R.KINDS["SquaredExponential"], Xt.data_ptr(), Zt.data_ptr(), ilt.data_ptr(), variance, plain.data_ptr(), N, M, D, _ru(M),
        torch.cuda.current_stream(DEV).cuda_stream), "kernel_fill")
    torch.cuda.synchronize()
    assert torch.equal(got[N:], plain[N:]) and torch.equal(got[:, M:], plain[:, M:])
    g, p = got[:N, :M].double().cpu().numpy(), plain[:N, :M].double().cpu().numpy()
    assert p.min() >= 1e3 * R.TINY[T]
    return g, p, X, Z, il, rows


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_product_of_two_squared_exponentials_is_the_ard_squared_exponential(dtype):
    """Product([SE(dims 0, 1), SE(dims 2)]) against the plain fill of the ARD SquaredExponential with the product variance:
    relative difference <= 8 u (two exponentials of 2 ulp each, one multiply, and the plain fill's own 2: 7 u).  That count has no
    rounding of an exponent's ARGUMENT in it, and each of those is worth s / 2 ulp of the value: the two forms round their
    arguments differently (s_01 and s_2 apart, or one sum over three columns; D + 2 = 5 roundings each), so the inputs are one small
    cloud with s <= 0.2, asserted below, where those ten roundings come to 10 * 0.1 u = 1 u at the most -- the u that 8 leaves.
    The next test takes the wide range with the argument term written out.  Measured on an MI355X: 1.15 u (fp64), 2.22 u (fp32)."""
    T = R.np_type(dtype)
    g, p, X, Z, il, _ = _identity_pair(dtype, 0.05)
    assert float(np.max(np.sum(((X[:, None, :] - Z[None, :, :]) * il) ** 2, axis=-1))) <= 0.2
    worst = float(np.max(np.abs(g - p) / p)) / R.U[T]
    print(f"product of two SE against the ARD SE: worst relative difference {worst:.2f} u")
    assert worst <= 8.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_identity_over_a_wide_range_of_the_exponent(dtype):
    """The same identity where exp is far from 1 (a cloud of scale 0.8: s up to 27, values down to 1e-6).  Per entry the bound is
    the 8 u of the test above plus the argument terms of ``rel_bound`` for each of the three exponentials involved (the ARD one
    and the product's two): |k'/k| times ``ds_bound`` (the roundings of s: inputs scaled, difference, square, sum) and, in fp32,
    ``__expf``'s rounding of a * log2 e.  At s ~ 27 the two forms differ by 10 u in fp64 and 22 u in fp32 already in the CPU
    restatement with a correctly rounded exponential.  Measured on an MI355X: 23.3 u (fp64) and 21.6 u (fp32), 0.25 and 0.23 of
    the bound."""
    T = R.np_type(dtype)
    D = 3
    g, p, X, Z, il, rows = _identity_pair(dtype, 0.8)
    kind = "SquaredExponential"
    bound = np.full(p.shape, 8.0 * R.U[T])
    for inv in (il, rows[0], rows[1]):
        ref = R.reference(kind, X, Z, inv, 1.0)
        a = np.abs(ref["a"]).astype(np.float64)
        bound += R.log_slope(kind, a) * R.ds_bound(ref, T, D) + R.U[T] * R.arg_roundings(kind, T) * a
    s_max = float(np.max(R.reference(kind, X, Z, il, 1.0)["s"]))
    assert s_max >= 20.0
    ratio = np.abs(g - p) / p / bound
    print(f"identity over a wide range: s up to {s_max:.1f}, worst relative difference {float(np.max(np.abs(g - p) / p)) / R.U[T]:.2f} u, "
          f"worst difference / bound {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0
