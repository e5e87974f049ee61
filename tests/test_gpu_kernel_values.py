"""Kernel-matrix values entry by entry at every site that evaluates ``kernel_profile`` (csrc/tsvgp_device.h): the fill in all
its row, column and store paths, ``tsvgp_gram_to_kernel_*``, the epilogue of ``tsvgp_cov_*``, ``tsvgp_vgp_system_f64`` and
``tsvgp_greedy_select_f64``, against the longdouble reference of tests/kernel_value_ref.py under its derived relative bound
(flat constant doubled, ``GPU_FACTOR``) on its radial grid (a from 0 to the edge of the type's normal range, exact r = 0, both
sides of the Matern clamp, rows far beyond underflow).  Outputs are NaN-filled before every call: the padding inside
[Np, cols_pad] must be exactly zero and everything beyond it still NaN.  Every test prints its worst error / bound."""
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
GUARD = 256  # NaN elements in front of and behind every output
KIND_NAMES = list(R.KINDS)
DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]


def _t(a, dtype):
    return torch.as_tensor(np.array(a), dtype=dtype, device=DEV).contiguous()  # (a copy: the cached grids are read-only)


def _fn(name, dtype):
    B = pkg()._backend
    return getattr(B.lib(), f"{name}_{B.suffix(dtype)}")


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _ru(n):
    return pkg()._backend.round_up(n)


def _buffer(dtype, numel, offset=0):
    """A NaN-filled flat buffer and the element index at which the output starts (``offset`` elements behind a 256-byte boundary)."""
    flat = torch.full((GUARD + offset + numel + GUARD,), NAN, dtype=dtype, device=DEV)
    assert flat.data_ptr() % 256 == 0
    return flat, GUARD + offset


def _guards_untouched(flat, start, numel):
    return bool(torch.isnan(flat[:start]).all()) and bool(torch.isnan(flat[start + numel:]).all())


@functools.lru_cache(maxsize=None)
def _grid(kind, T, N, M, D, seed=0, pairwise=False, P=None):
    g = R.grid(kind, T, N, M, D, seed=seed, pairwise=pairwise, P=P)
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


def _fill(kind, dtype, g, N, M, D, ldk, offset=0):
    """One ``tsvgp_kernel_fill_*`` call into a NaN-filled [Np, ldk] view ``offset`` elements off the boundary; checks the guards."""
    B = pkg()._backend
    Np = _ru(N)
    flat, start = _buffer(dtype, Np * ldk, offset)
    out = flat[start:start + Np * ldk].view(Np, ldk)
    Xt, Zt, il = _t(g["X"], dtype), _t(g["Z"], dtype), _t(g["inv_ls"], dtype)
    B.check(_fn("tsvgp_kernel_fill", dtype)(R.KINDS[kind], Xt.data_ptr(), Zt.data_ptr(), il.data_ptr(), g["variance"], out.data_ptr(),
                                            N, M, D, ldk, _stream()), "kernel_fill")
    torch.cuda.synchronize()
    assert _guards_untouched(flat, start, Np * ldk)
    return out


def _check_layout(out, N, M, cols_pad=None):
    """Exact zeros in the padding of [Np, cols_pad], NaN in the columns behind cols_pad, finite values on [N, M]."""
    cols_pad = _ru(M) if cols_pad is None else cols_pad
    assert bool(torch.isfinite(out[:N, :M]).all())
    assert bool((out[N:, :cols_pad] == 0).all()) and bool((out[:N, M:cols_pad] == 0).all())
    assert not bool(torch.signbit(out[:, :cols_pad]).any())  # +0.0
    assert bool(torch.isnan(out[:, cols_pad:]).all())


def _check_rows(kind, dtype, g, got, rows, D, what):
    """``got`` [len(rows), M] against the reference of the grid's rows ``rows``; returns (worst error / bound, fraction relative)."""
    T = R.np_type(dtype)
    var = R.c_variance(g["variance"], T)
    ref = R.reference(kind, g["X"][rows], g["Z"], g["inv_ls"], var)
    bound = R.rel_bound(kind, T, ref, D, factor=R.GPU_FACTOR)
    return R.check_values(got.double().cpu().numpy(), ref, bound, T, var, what)


# --------------------------------------------------------------------------------------------------------------------- the fill
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("D", [1, 3, 8, 19, 32])
def test_fill_values_at_every_padded_dimension(dtype, kind, D):
    """(130, 130): the 8-row workgroups, two row tiles and a partial column group; D padded to 1, 4, 8, 32, 32 (fp32: four columns
    per thread up to 16, two at 32)."""
    N = M = 130
    g = _grid(kind, R.np_type(dtype), N, M, D)
    out = _fill(kind, dtype, g, N, M, D, _ru(M) + 4)
    _check_layout(out, N, M)
    worst, frac = _check_rows(kind, dtype, g, out[:N, :M], slice(0, N), D, f"fill {kind} D={D}")
    assert frac >= 0.9


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("N,M", [(4097, 130), (4096 + 70, 130), (129, 1025)])
def test_fill_values_on_the_production_row_path_and_past_the_first_column_tile(dtype, kind, N, M):
    """N > 4096: rows_pad = 4224 takes the 64-row workgroup every E-step runs.  N = 4097: the block of row 4096 has one valid row
    and 63 zero rows, the last block none; N = 4166: 6 valid rows.  M = 1025: the third 512-column tile in fp64, the second
    1024-column tile of the four-column fp32 kernel, both cut at cols_pad = 1152."""
    D = 8
    g = _grid(kind, R.np_type(dtype), N, M, D)
    out = _fill(kind, dtype, g, N, M, D, _ru(M) + 4)
    _check_layout(out, N, M)
    if N > 4096:
        assert _ru(N) == 4224
    worst, frac = _check_rows(kind, dtype, g, out[:N, :M], slice(0, N), D, f"fill {kind} {N} x {M}")
    assert frac >= 0.9


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("layout", ["ldk = Mp + 2", "K 8 bytes off", "strideK % 4 == 2"])
def test_fp32_fill_with_two_columns_per_thread(kind, layout):
    """The fp32 fallback to 8-byte stores: an ldk that is no multiple of 4, a K 8 bytes behind a 16-byte boundary, a batch whose
    stride is 2 modulo 4.  The same entrywise bound, and bit for bit the values of the four-column kernel on the same inputs
    (packed arithmetic per column pair in both)."""
    B = pkg()._backend
    dtype, T, N, M, D = torch.float32, np.float32, 130, 600, 8  # 600 columns: the second 512-column tile of the two-column kernel
    Np, Mp = _ru(N), _ru(M)
    g = _grid(kind, T, N, M, D)
    wide = _fill(kind, dtype, g, N, M, D, Mp + 4)  # four columns per thread
    if layout == "strideK % 4 == 2":
        P = 2
        gp = _grid(kind, T, N, M, D, P=P)
        Xt, Zt, il = _t(gp["X"], dtype), _t(gp["Z"], dtype), _t(gp["inv_ls"], dtype)
        var = [1.3, 0.8]
        outs = {}
        for name, ldk, stride in (("two", Mp, Np * Mp + 2), ("four", Mp, Np * Mp + 4)):
            assert stride % 4 == (2 if name == "two" else 0)
            flat, start = _buffer(dtype, P * stride)
            B.check(_fn("tsvgp_kernel_fill_batched", dtype)(R.KINDS[kind], Xt.data_ptr(), Zt.data_ptr(), il.data_ptr(),
                                                            (ctypes.c_float * P)(*var), flat[start:].data_ptr(), stride, N, M, D, ldk, P,
                                                            _stream()), "fill batched")
            torch.cuda.synchronize()
            assert _guards_untouched(flat, start, P * stride)
            body = flat[start:start + P * stride].view(P, stride)
            assert bool(torch.isnan(body[:, Np * ldk:]).all())  # the gap behind each latent
            outs[name] = body[:, :Np * ldk].reshape(P, Np, ldk)
        for p in range(P):
            gq = dict(gp, inv_ls=gp["inv_ls"][p], variance=var[p])
            _check_layout(outs["two"][p], N, M)
            _, frac = _check_rows(kind, dtype, gq, outs["two"][p][:N, :M], slice(0, N), D, f"fp32 two columns, {layout}, latent {p}")
            assert frac >= 0.9
        equal = torch.equal(outs["two"], outs["four"])
    else:
        ldk, off = (Mp + 2, 0) if layout == "ldk = Mp + 2" else (Mp + 4, 2)
        assert (ldk % 4 != 0) != (off % 4 != 0)
        out = _fill(kind, dtype, g, N, M, D, ldk, offset=off)
        assert (out.data_ptr() % 16 == 8) == (off == 2)
        _check_layout(out, N, M)
        _check_rows(kind, dtype, g, out[:N, :M], slice(0, N), D, f"fp32 two columns, {layout}")
        equal = torch.equal(out[:, :Mp], wide[:, :Mp])
    print(f"fp32 {kind} {layout}: two and four columns per thread bit-equal: {equal}")
    assert equal


NT_BLOCKS = [(0, 128), (4032, 4160), (65536 - 128, 65536)]


@pytest.mark.parametrize("dtype,wide_ldk", [(torch.float64, 1024), (torch.float32, 2048)], ids=IDS)
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_fill_non_temporal_store_path(dtype, wide_ldk, kind):
    """An output of exactly 512 MB (65536 rows, ldk 1024 / 2048 passed explicitly) takes the non-temporal stores: bit for bit the
    values of the cached path (ldk = 256) on [Np, cols_pad], NaN behind cols_pad; the ldk = 256 result against the reference on
    three row blocks (the first, around row 4096, the last)."""
    N, M, D = 65536, 130, 8
    g = _grid(kind, R.np_type(dtype), N, M, D)
    assert N * wide_ldk * torch.empty((), dtype=dtype).element_size() == 512 * 1024 * 1024
    small = _fill(kind, dtype, g, N, M, D, 256)
    _check_layout(small, N, M)
    for lo, hi in NT_BLOCKS:
        _check_rows(kind, dtype, g, small[lo:hi, :M], slice(lo, hi), D, f"fill {kind} rows [{lo}, {hi}) of 65536")
    wide = _fill(kind, dtype, g, N, M, D, wide_ldk)
    assert bool(torch.isnan(wide[:, 256:]).all())
    assert torch.equal(wide[:, :256], small)


def test_fill_non_temporal_store_path_batched():
    """Two latents of 256 MB each: P * rows_pad * ldk crosses 512 MB although one latent does not."""
    B = pkg()._backend
    kind, dtype, T, N, M, D, P = "Matern52", torch.float64, np.float64, 32768, 130, 8, 2
    g = _grid(kind, T, N, M, D, P=P)
    Xt, Zt, il = _t(g["X"], dtype), _t(g["Z"], dtype), _t(g["inv_ls"], dtype)
    var = [1.3, 0.8]
    outs = []
    for ldk in (256, 1024):
        stride = N * ldk
        assert (P * stride * 8 >= 512 * 1024 * 1024) == (ldk == 1024) and stride * 8 < 512 * 1024 * 1024
        flat, start = _buffer(dtype, P * stride)
        B.check(_fn("tsvgp_kernel_fill_batched", dtype)(R.KINDS[kind], Xt.data_ptr(), Zt.data_ptr(), il.data_ptr(),
                                                        (ctypes.c_double * P)(*var), flat[start:].data_ptr(), stride, N, M, D, ldk, P,
                                                        _stream()), "fill batched")
        torch.cuda.synchronize()
        assert _guards_untouched(flat, start, P * stride)
        outs.append(flat[start:start + P * stride].view(P, N, ldk))
    small, wide = outs
    assert bool(torch.isnan(wide[:, :, 256:]).all()) and torch.equal(wide[:, :, :256], small)
    for p in range(P):
        gq = dict(g, inv_ls=g["inv_ls"][p], variance=var[p])
        _check_layout(small[p], N, M)
        for lo, hi in [(0, 128), (N - 128, N)]:
            _check_rows(kind, dtype, gq, small[p][lo:hi, :M], slice(lo, hi), D, f"batched fill latent {p} rows [{lo}, {hi})")


# ------------------------------------------------------------------------------------------------------- tsvgp_gram_to_kernel_*
def _gram_case(kind, dtype, N, M, ldk, blocks):
    B = pkg()._backend
    T, D = R.np_type(dtype), 33
    g = _grid(kind, T, N, M, D, seed=2)
    var = R.c_variance(g["variance"], T)
    Np, cols_pad = _ru(N), _ru(M)
    Xs, Zs = _t(g["X"], dtype) * _t(g["inv_ls"], dtype), _t(g["Z"], dtype) * _t(g["inv_ls"], dtype)
    xx, zz = (Xs * Xs).sum(dim=1).contiguous(), (Zs * Zs).sum(dim=1).contiguous()
    flat, start = _buffer(dtype, Np * ldk)
    out = flat[start:start + Np * ldk].view(Np, ldk)
    out[:N, :M] = torch.mm(Xs, Zs.t())  # the Gram block from the BLAS library; the rest of the buffer stays NaN
    # the Z = X[:k] entries, where the expanded form comes out as rounding noise of either sign, are pushed to the negative side:
    # s = xx + zz - 2 G = -8 u (xx + zz) there, whatever the library's summation order gave
    k = torch.arange(R.K_SAME, device=DEV)
    out[k, k] = (xx[:R.K_SAME] + zz[:R.K_SAME]) * (0.5 * (1.0 + 8.0 * R.U[T]))
    G = out[:N, :M].cpu().numpy()
    B.check(_fn("tsvgp_gram_to_kernel", dtype)(R.KINDS[kind], out.data_ptr(), xx.data_ptr(), zz.data_ptr(), g["variance"], N, M, ldk,
                                               _stream()), "gram_to_kernel")
    torch.cuda.synchronize()
    assert _guards_untouched(flat, start, Np * ldk)
    _check_layout(out, N, M, cols_pad)
    xh, zh = xx.cpu().numpy(), zz.cpu().numpy()
    got = out[:N, :M].double().cpu().numpy()
    negative = 0
    for lo, hi in blocks:
        ref = R.reference_gram(kind, xh[lo:hi], zh, G[lo:hi], var)
        negative += int((ref["s"] < 0).sum())
        if lo == 0:
            assert np.all(np.diag(ref["s"])[:R.K_SAME] < 0)
        bound = R.rel_bound(kind, T, ref, None, factor=R.GPU_FACTOR)
        # (check_values wants K >= +0: a negative s gives variance * exp(+small) > variance under SE, the clamp under Matern)
        _, frac = R.check_values(got[lo:hi], ref, bound, T, var, f"gram_to_kernel {kind} rows [{lo}, {hi}) of {N}")
        assert frac >= 0.9 or lo > 0
    print(f"gram_to_kernel {kind}: {negative} entries with s < 0")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_gram_to_kernel_values(dtype, kind):
    """(130, 130, D = 33) through the entry's own C ABI with ldk > cols_pad; the Gram block comes from torch.mm on the device and
    is read back for the reference, so the elementwise kernel alone is under test.  Where s comes out negative -- made sure of on
    the Z = X[:k] entries -- the values are held to the profile at that s: variance * exp(+small) under SE, the clamp under Matern."""
    _gram_case(kind, dtype, 130, 130, 256 + 4, [(0, 130)])


def test_gram_to_kernel_second_launch():
    """N = 65600: rows go through grid.y in launches of 65535; the second launch has 129 grid rows of which 65 are valid and must
    read xx from row 65535 on."""
    N = 65600
    assert _ru(N) - 65535 == 129 and N - 65535 == 65
    _gram_case("Matern52", torch.float64, N, 100, 128, [(0, 128), (65535 - 63, N)])


# ----------------------------------------------------------------------------------------------- the sites that evaluate k(X, X)
def _pair_ref(kind, dtype, g, cols=None):
    T = R.np_type(dtype)
    var = R.c_variance(g["variance"], T)
    return var, R.reference(kind, g["X"], g["X"] if cols is None else g["X"][cols], g["inv_ls"], var)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("D", [1, 5, 32])
def test_cov_base_term_values(dtype, kind, D):
    """``tsvgp_cov_*`` with T = 0 and sign = -1: C is the base term variance * k(x_i, x_j).  N = 130: two diagonal tiles and one
    off-diagonal tile.  Entrywise bound, C == C^T bit for bit, the identity in the padding, NaN behind column Np."""
    B = pkg()._backend
    T, N, Mp = R.np_type(dtype), 130, 128
    Np, ldc = _ru(N), _ru(N) + 4
    g = _grid(kind, T, N, 0, D, seed=1, pairwise=True)
    Xt, il = _t(g["X"], dtype), _t(g["inv_ls"], dtype)
    tile = torch.zeros((Np, Mp), dtype=dtype, device=DEV)
    flat, start = _buffer(dtype, Np * ldc)
    C = flat[start:start + Np * ldc].view(Np, ldc)
    B.check(_fn("tsvgp_cov", dtype)(R.KINDS[kind], tile.data_ptr(), Xt.data_ptr(), il.data_ptr(), g["variance"], -1.0, C.data_ptr(), N, Np,
                                    Mp, D, ldc, 0, _stream()), "cov")
    torch.cuda.synchronize()
    assert _guards_untouched(flat, start, Np * ldc) and bool(torch.isnan(C[:, Np:]).all())
    Cs = C[:, :Np]
    assert torch.equal(Cs, Cs.t())
    eye = torch.eye(Np, dtype=dtype, device=DEV)
    assert torch.equal(Cs[N:], eye[N:]) and torch.equal(Cs[:, N:], eye[:, N:])
    var, ref = _pair_ref(kind, dtype, g)
    bound = R.rel_bound(kind, T, ref, D, factor=R.GPU_FACTOR)
    _, frac = R.check_values(Cs[:N, :N].double().cpu().numpy(), ref, bound, T, var, f"cov {kind} D={D}")
    assert frac >= 0.9


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("D", [1, 5, 32])
def test_vgp_system_kernel_values(kind, D):
    """``tsvgp_vgp_system_f64`` with lambda_2 = 1: s = 1, so rows [Np, 2 Np) are K~ = K + jitter I itself (the products with s are
    exact).  Entrywise bound off the diagonal, fl(variance + jitter) exactly ON it, zeros in the padding; the lower block triangle of
    B = I + K~ repeats the same kernel values bit for bit off the diagonal."""
    B = pkg()._backend
    dtype, T, N, jitter = torch.float64, np.float64, 130, 1e-6
    Np, lds = _ru(N), _ru(N) + 2
    g = _grid(kind, T, N, 0, D, seed=1, pairwise=True)
    Xt, il = _t(g["X"], dtype), _t(g["inv_ls"], dtype)
    l1 = _t(np.random.RandomState(3).randn(Np), dtype)
    l2 = torch.ones(Np, dtype=dtype, device=DEV)
    rows = 2 * Np + 128
    flat, start = _buffer(dtype, rows * lds)
    S = flat[start:start + rows * lds].view(rows, lds)
    B.check(B.lib().tsvgp_vgp_system_f64(R.KINDS[kind], Xt.data_ptr(), il.data_ptr(), g["variance"], jitter, l1.data_ptr(), l2.data_ptr(),
                                         S.data_ptr(), N, Np, D, lds, 0, _stream()), "vgp_system")
    torch.cuda.synchronize()
    assert _guards_untouched(flat, start, rows * lds) and bool(torch.isnan(S[:, Np:]).all())
    Rk = S[Np:2 * Np, :Np]
    assert bool((Rk[N:] == 0).all()) and bool((Rk[:, N:] == 0).all())
    var, ref = _pair_ref(kind, dtype, g)
    got = Rk[:N, :N].cpu().numpy()
    assert np.all(np.diag(got) == var + jitter)  # one rounded addition on the exact value variance * k(0)
    off = got.copy()
    np.fill_diagonal(off, var)
    bound = R.rel_bound(kind, T, ref, D, factor=R.GPU_FACTOR)
    _, frac = R.check_values(off, ref, bound, T, var, f"vgp_system {kind} D={D}")
    assert frac >= 0.9
    Bk = S[:Np, :Np].cpu().numpy()
    lower = np.tril(np.ones((N, N), bool), -1)
    assert np.array_equal(Bk[:N, :N][lower], got[lower])
    assert np.all(np.diag(Bk)[:N] == 1.0 + (var + jitter)) and np.all(np.diag(Bk)[N:] == 1.0)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("D", [1, 5, 32])
def test_greedy_select_first_factor_row(kind, D):
    """``tsvgp_greedy_select_f64`` with M = 1: the first pivot is row 0 and row 0 of C is k(X, x_0) / sqrt(variance).  The bound
    takes 2 u more for the square root and the division."""
    B = pkg()._backend
    dtype, T, N = torch.float64, np.float64, 130
    Np, ldc = _ru(N), _ru(N) + 2
    g = _grid(kind, T, N, 0, D, seed=1, pairwise=True)
    Xt, il = _t(g["X"], dtype), _t(g["inv_ls"], dtype)
    flat, start = _buffer(dtype, ldc)
    C = flat[start:start + ldc].view(1, ldc)
    d = torch.full((Np,), NAN, dtype=dtype, device=DEV)
    indices = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    pivots = torch.full((1,), NAN, dtype=dtype, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    work = torch.zeros((int(B.lib().tsvgp_greedy_select_work_bytes(N, 1)) + 7) // 8, dtype=torch.int64, device=DEV)
    B.check(B.lib().tsvgp_greedy_select_f64(R.KINDS[kind], Xt.data_ptr(), il.data_ptr(), g["variance"], 1e-12 * g["variance"], C.data_ptr(),
                                            ldc, d.data_ptr(), indices.data_ptr(), pivots.data_ptr(), count.data_ptr(), work.data_ptr(),
                                            N, 1, D, _stream()), "greedy_select")
    torch.cuda.synchronize()
    assert _guards_untouched(flat, start, ldc) and bool(torch.isnan(C[:, Np:]).all()) and bool((C[:, N:Np] == 0).all())
    assert int(count) == 1 and int(indices[0]) == 0 and float(pivots[0]) == g["variance"]
    var, ref = _pair_ref(kind, dtype, g, cols=slice(0, 1))
    ref["K"] = ref["K"] / np.sqrt(R.L(var))
    bound = R.rel_bound(kind, T, ref, D, factor=R.GPU_FACTOR, extra=2.0)
    _, frac = R.check_values(C[0, :N].cpu().numpy()[:, None], ref, bound, T, var, f"greedy {kind} D={D}")
    assert frac >= 0.9
