"""``tsvgp_kernel_fill_sum_*`` entry by entry against the longdouble reference of tests/kernel_value_ref.py, no new constants.

``grid(kind, T, N, M, D, P=C)`` lays out C lengthscale sets in the geometry of component 0 (kind ``kind``); component c takes
``inv_ls[c]`` and its own kind.  Reference: sum_c ``reference(kind_c, ...)["K"]`` in longdouble.  Bound per entry, absolute:

    sum_c rel_bound(kind_c, T, ref_c, D, factor=GPU_FACTOR) * K_c  +  (C - 1) * u * sum_c K_c

(every component under its own derived bound, and one rounding of the running sum per addition).  Entries whose summed
reference is below 1e3 * tiny follow ``check_values``' absolute rule; at least 90 % are held to the relative one -- the grid's
guarantee for component 0, which the summed reference keeps (a sum is at least its first term).  Outputs are NaN-filled
before every call: the padding inside [Np, cols_pad] must be exact zeros and everything beyond it still NaN."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import kernel_value_ref as R
from tests.helpers import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
GUARD = 256
DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]
# components: (kind, variance, input columns whose inv_ls is zeroed -- an ``active_dims`` component; never component 0, whose
# scaling lays out the grid).  Columns beyond D - 1 are dropped, and a component keeps at least one column.
# Component 0 of a mixed sum is the SquaredExponential: ``rel_bound`` holds for a component while ITS exponent's argument a_c
# stays inside the type's normal range, which the grid guarantees for component 0 alone (a_0 <= A_MAX).  With a_0 = r^2 / 2 a
# Matern component has a_c = sqrt(3) r or sqrt(5) r <= max(a_0, 10), and a longer lengthscale or a dropped column only lowers
# a_c -- so every component stays inside the range.  (With a Matern first, a faster-decaying component reaches a_c > 87.3 in
# fp32 where the grid still has a_0 <= 84: ``__expf`` flushes there while (1 + a + a^2 / 3) exp(-a) is still 1e-36, a property
# of ``kernel_profile`` that the single-kernel grids never meet either.)
SPECS = {1: [("Matern52", 1.3, ())],
         2: [("SquaredExponential", 1.3, ()), ("Matern32", 0.8, (0, 1, 5))],
         4: [("SquaredExponential", 1.3, ()), ("Matern32", 0.8, (2,)), ("Matern52", 0.5, (0, 3, 4, 20)), ("SquaredExponential", 0.2, ())]}
COL_TILE = {torch.float64: 512, torch.float32: 1024}  # columns per workgroup: 2 x 256 threads, 4 x 256 in fp32


def _t(a, dtype):
    return torch.as_tensor(np.array(a), dtype=dtype, device=DEV).contiguous()


def _ru(n):
    return pkg()._backend.round_up(n)


@functools.lru_cache(maxsize=None)
def _problem(C, dtype, N, M, D):
    """The grid (made at the sizes ``grid`` needs, cut to [N] rows and [M] inducing rows), the component list and the reference."""
    T = R.np_type(dtype)
    spec = SPECS[C]
    g = R.grid(spec[0][0], T, max(N, R.MIN_ROWS), max(M, R.K_SAME + 1), D, P=C if C > 1 else None)
    X, Z = g["X"][:N], g["Z"][:M]
    il = np.array(g["inv_ls"], dtype=np.float64).reshape(C, D)
    for c, (_, _, off) in enumerate(spec):
        cols = [d for d in off if d < D]
        if len(cols) < D:
            il[c, cols] = 0.0
    kinds = [s[0] for s in spec]
    var = [R.c_variance(s[1], T) for s in spec]
    refs = [R.reference(kinds[c], X, Z, il[c], var[c]) for c in range(C)]
    Ksum = refs[0]["K"].copy()
    for r in refs[1:]:
        Ksum = Ksum + r["K"]
    absb = np.zeros(Ksum.shape)
    for c in range(C):
        absb += R.rel_bound(kinds[c], T, refs[c], D, factor=R.GPU_FACTOR) * refs[c]["K"].astype(np.float64)
    absb += (C - 1) * R.U[T] * Ksum.astype(np.float64)
    ref = dict(K=Ksum, a=refs[0]["a"])
    rel = R.relative_mask(ref, T)
    bound = absb / np.where(rel, Ksum, 1).astype(np.float64)  # relative to the summed reference, as check_values takes it
    for a in (X, Z, il):
        a.setflags(write=False)
    return dict(X=X, Z=Z, inv_ls=il, kinds=kinds, var=var, ref=ref, bound=bound, T=T)


def _sum_fill(pr, dtype, N, M, D, ldk, offset=0, x_is_z=False):
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
    var = ((ctypes.c_double if dtype == torch.float64 else ctypes.c_float) * C)(*pr["var"])
    fn = getattr(B.lib(), f"tsvgp_kernel_fill_sum_{B.suffix(dtype)}")
    B.check(fn(kinds, Xt.data_ptr(), Zt.data_ptr(), il.data_ptr(), var, out.data_ptr(), N, M, D, ldk, C,
               torch.cuda.current_stream(DEV).cuda_stream), "kernel_fill_sum")
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat[:start]).all()) and bool(torch.isnan(flat[start + Np * ldk:]).all())
    return out


def _check_layout(out, N, M):
    cols_pad = _ru(M)
    assert bool(torch.isfinite(out[:N, :M]).all())
    assert bool((out[N:, :cols_pad] == 0).all()) and bool((out[:N, M:cols_pad] == 0).all())
    assert not bool(torch.signbit(out[:, :cols_pad]).any())  # +0.0
    assert bool(torch.isnan(out[:, cols_pad:]).all())


def _check_values(pr, got, what, min_frac=0.9):
    worst, frac = R.check_values(got.double().cpu().numpy(), pr["ref"], pr["bound"], pr["T"], float(sum(pr["var"])), what)
    assert frac >= min_frac
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("D", [1, 3, 8, 16, 32])
def test_sum_fill_values(dtype, C, D):
    """N = 130: the 8-row workgroups, two row tiles and a ragged tail; M one past the column tile (a second workgroup column with one
    live column); D padded to 1, 4, 8, 16, 32; C * Dpad <= 32 keeps every component's Z columns in registers, beyond (D = 16 with
    C = 4, D = 32 with C = 2, 4) the row-chunk form reloads them.  Mixed kinds, components with zeroed columns."""
    N, M = 130, COL_TILE[dtype] + 1
    pr = _problem(C, dtype, N, M, D)
    out = _sum_fill(pr, dtype, N, M, D, _ru(M) + 4)
    _check_layout(out, N, M)
    _check_values(pr, out[:N, :M], f"sum fill C={C} D={D} {N} x {M}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,M", [(1, 3), (1, 130), (130, 3)])
def test_sum_fill_one_row_and_three_columns(dtype, N, M):
    C, D = 2, 3
    pr = _problem(C, dtype, N, M, D)
    out = _sum_fill(pr, dtype, N, M, D, _ru(M))
    _check_layout(out, N, M)
    _check_values(pr, out[:N, :M], f"sum fill {N} x {M}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C,D", [(2, 8), (4, 32)])
def test_sum_fill_on_the_production_row_path(dtype, C, D):
    """N > 4096: the 64-row workgroups of the N-sized operand.  N = 4166: the block of row 4160 has 6 valid rows and 58 zero rows,
    the last block none."""
    N, M = 4096 + 70, 130
    pr = _problem(C, dtype, N, M, D)
    out = _sum_fill(pr, dtype, N, M, D, _ru(M) + 4)
    assert _ru(N) == 4224
    _check_layout(out, N, M)
    _check_values(pr, out[:N, :M], f"sum fill 64-row blocks C={C} D={D}")


@pytest.mark.parametrize("layout", ["ldk = Mp + 2", "K 8 bytes off"])
@pytest.mark.parametrize("C,D", [(2, 8), (4, 16)])
def test_fp32_sum_fill_with_two_columns_per_thread(layout, C, D):
    """The fp32 fallback to 8-byte stores; the same entrywise bound, and the values of the four-column form bit for bit (packed
    arithmetic per column pair in both)."""
    dtype, N, M = torch.float32, 130, 513
    Mp = _ru(M)
    pr = _problem(C, dtype, N, M, D)
    wide = _sum_fill(pr, dtype, N, M, D, Mp + 4)
    ldk, off = (Mp + 2, 0) if layout == "ldk = Mp + 2" else (Mp + 4, 2)
    out = _sum_fill(pr, dtype, N, M, D, ldk, offset=off)
    assert (out.data_ptr() % 16 == 8) == (off == 2)
    _check_layout(out, N, M)
    _check_values(pr, out[:N, :M], f"fp32 sum fill, two columns, {layout}")
    assert torch.equal(out[:, :Mp], wide[:, :Mp])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C,D", [(2, 3), (4, 32)])
def test_sum_fill_kzz_is_symmetric_and_reproducible(dtype, C, D):
    """The K(Z, Z) call (X is Z, one pointer): values, exact symmetry, and two calls bit for bit."""
    M = 130
    pr0 = _problem(C, dtype, M, M, D)
    pr = dict(pr0, X=pr0["Z"])  # the reference of k(Z, Z)
    T = pr["T"]
    refs = [R.reference(pr["kinds"][c], pr["Z"], pr["Z"], pr["inv_ls"][c], pr["var"][c]) for c in range(C)]
    Ksum = sum(r["K"] for r in refs[1:]) + refs[0]["K"]
    absb = sum(R.rel_bound(pr["kinds"][c], T, refs[c], D, factor=R.GPU_FACTOR) * refs[c]["K"].astype(np.float64) for c in range(C))
    absb = absb + (C - 1) * R.U[T] * Ksum.astype(np.float64)
    pr["ref"] = dict(K=Ksum, a=refs[0]["a"])
    pr["bound"] = absb / np.where(R.relative_mask(pr["ref"], T), Ksum, 1).astype(np.float64)
    a = _sum_fill(pr, dtype, M, M, D, _ru(M), x_is_z=True)
    b = _sum_fill(pr, dtype, M, M, D, _ru(M), x_is_z=True)
    _check_layout(a, M, M)
    _check_values(pr, a[:M, :M], f"sum fill K(Z, Z) C={C} D={D}")
    assert torch.equal(a[:M, :M], a[:M, :M].t())
    assert torch.equal(a, b)
    assert bool((a[:M, :M].diagonal() > 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [3, 32])
def test_one_component_agrees_with_the_plain_fill(dtype, D):
    """C = 1 against ``tsvgp_kernel_fill_*`` on the same inputs: within the same entrywise bound of it (the two forms may contract
    and order differently); prints whether they agree bit for bit."""
    B = pkg()._backend
    N, M = 130, COL_TILE[dtype] + 1
    pr = _problem(1, dtype, N, M, D)
    got = _sum_fill(pr, dtype, N, M, D, _ru(M))
    plain = torch.full((_ru(N), _ru(M)), NAN, dtype=dtype, device=DEV)
    Xt, Zt, il = _t(pr["X"], dtype), _t(pr["Z"], dtype), _t(pr["inv_ls"][0], dtype)
    B.check(getattr(B.lib(), f"tsvgp_kernel_fill_{B.suffix(dtype)}")(
        R.KINDS[pr["kinds"][0]], Xt.data_ptr(), Zt.data_ptr(), il.data_ptr(), pr["var"][0], plain.data_ptr(), N, M, D, _ru(M),
        torch.cuda.current_stream(DEV).cuda_stream), "kernel_fill")
    torch.cuda.synchronize()
    print(f"C = 1, D = {D}: bit-equal to the plain fill: {torch.equal(got, plain)}")
    rel = R.relative_mask(pr["ref"], pr["T"])
    diff = np.abs(got[:N, :M].double().cpu().numpy() - plain[:N, :M].double().cpu().numpy())
    allowed = pr["bound"] * pr["ref"]["K"].astype(np.float64)
    assert np.all(diff[rel] <= allowed[rel])
    assert np.all(diff[~rel] <= 2e3 * R.TINY[pr["T"]] * pr["var"][0])
    assert torch.equal(got[N:], plain[N:]) and torch.equal(got[:, M:], plain[:, M:])
