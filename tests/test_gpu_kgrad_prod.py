"""``tsvgp_kernel_grad_prod_f64/_f32`` (the M-step contraction of a Product kernel, all C parameter sets in one pass over U) called
directly through the C-ABI, every entry of every output against tests/kgrad_prod_ref.py (NumPy, fp64).

Shapes: the full cross D in {1, 2, 3, 4, 8, 16} x C in {1, 2, 3, 4} at N = 70, M = 5 -- every (Dpad, C) instantiation, both
column forms of the kernel (two columns per pass, and one where C * Dpad * sizeof(T) >= 256) -- and a list of larger cases with
N in {1, 63, 65, 1023, 1025, 2049} (the 64-row chunk, the 1024-row block and a third block) and M in {1, 2, 511, 513} (the lone
last column of a thread's pair, the second column tile).  From C = 2 on component 1 has input column 0 zeroed in ``inv_ls`` (an
``active_dims`` component): its dls there must be exactly 0.  Every other case runs with ldu beyond Mp, g0 / g1 as a column of an
[N, 3] array and beta with stride 2, NaN in every slot that must not be used.

Bound: |got - ref| <= c u A entry by entry with c = 512 C, A the sum of the absolute values of the entry's terms
(kgrad_prod_ref), u = 2^-53 / 2^-24: the derivation of tests/test_gpu_kgrad.py applied per component -- each of the C profile
arguments carries D + 2 roundings amplified by at most |s_c| / 2, a term gains two factors (a profile value and the running
product's rounding) per further component, accumulation is in fp64 for both types.

Measured on an MI355X, worst |got - ref| / (u A) over all shapes and outputs (bound: 512 C):
    fp64:  C = 1 18.3   C = 2 3.64   C = 3 5.31   C = 4 5.75
    fp32:  C = 1 9.47   C = 2 0.76   C = 3 1.06   C = 4 1.46       (C = 3 with the flushed component below: 35.7)
The C = 1 figures come from one case, N = 1, M = 513, D = 4 (Matern-5/2), where an entry of dZ is a single term: nothing
averages, and the far columns show the rounding of their profile argument in full (the other C = 1 cases: at most 1.2);
tests/test_gpu_kgrad.py, which measures at most 3.4, has no one-row case against many columns.  In the flushed-component case
the entries that are checked (A >= 1e-20) keep terms with s_1 up to 90, where the (D + 2) roundings of the argument are worth
s / 2 u each.  C = 1 against ``tsvgp_kernel_grad_*``: at most 2.77 (fp64), 0.75 (fp32).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import kgrad_prod_ref as PR
from tests.helpers import pkg
from tests.test_gpu_kgrad import DEV, DTYPE_IDS, DTYPES, GUARD, KIND_ID, UNIT, _dev, _host, _launch_fused, _padded_rows, _stream, _strided

pytestmark = pytest.mark.gpu

C_PER_COMPONENT = 512.0
KINDS = {1: ("matern52",), 2: ("se", "matern32"), 3: ("matern32", "se", "matern52"), 4: ("se", "matern32", "matern52", "se")}
VARIANCES = (1.3, 0.8, 0.5, 1.7)
# (N, M, D, C)
SHAPES = [(1, 1, 1, 1), (63, 2, 2, 2), (65, 511, 3, 4), (1023, 513, 4, 2), (1025, 2, 8, 4), (2049, 1, 16, 1), (65, 513, 16, 4),
          (1025, 511, 16, 2), (63, 513, 8, 3), (2049, 513, 2, 4), (65, 2, 16, 3), (1, 513, 4, 1), (130, 511, 1, 3)]

WORST = {}  # (dtype id, C) -> worst ratio seen in this session; printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for key in sorted(WORST):
        print(f"\nworst ratio product gradient {key[0]} C={key[1]}: {WORST[key]:.3f}", end="")
    print()


def _note(dtype, C, ratio):
    key = (DTYPE_IDS[DTYPES.index(dtype)], C)
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


@functools.lru_cache(maxsize=None)
def _inputs(N, M, D, C, seed):
    """Seeded fp64 host inputs (never written to).  Lengthscales in [0.7, 1.7] sqrt(D C) keep the product away from zero; the first
    rows of Z are rows of X (s = 0 exactly, the Matern clamp); U, g0, g1, beta of order 1, g1 of both signs."""
    rng = np.random.RandomState(seed)
    X, Z = rng.randn(N, D), rng.randn(M, D)
    k = min(N, M, 8)
    Z[:k] = X[:k]
    il = 1.0 / ((0.7 + rng.rand(C, D)) * np.sqrt(D * C))
    if C >= 2 and D >= 2:
        il[1, 0] = 0.0
    U, g0, g1, beta = rng.randn(N, M), rng.randn(N), rng.randn(N), rng.randn(M)
    for a in (X, Z, il, U, g0, g1, beta):
        a.setflags(write=False)
    return X, Z, il, U, g0, g1, beta


def _launch(dtype, kinds, X, Z, il, variance, U, g0, g1, beta, bstride, N, M, D):
    """One launch into fresh buffers of the documented sizes plus a guard tail, everything pre-filled with 7."""
    lib = pkg()._backend.lib()
    C = len(kinds)
    rows, Dp = int(lib.tsvgp_kernel_grad_rows()), int(lib.tsvgp_kernel_grad_dpad(D))
    Mp = (M + 127) // 128 * 128
    nrb, ncb = (N + rows - 1) // rows, (Mp + 511) // 512
    sizes = (nrb * Mp * Dp, nrb * ncb * C * Dp, nrb * ncb)
    bufs = [torch.full((n + GUARD,), 7.0, dtype=torch.float64, device=DEV) for n in sizes]
    fn = lib.tsvgp_kernel_grad_prod_f64 if dtype == torch.float64 else lib.tsvgp_kernel_grad_prod_f32
    assert g0.stride(0) == g1.stride(0)
    with torch.cuda.device(DEV):
        st = fn((ctypes.c_int * C)(*[KIND_ID[k] for k in kinds]), X.data_ptr(), Z.data_ptr(), il.data_ptr(), variance, U.data_ptr(),
                U.stride(0), g0.data_ptr(), g1.data_ptr(), g0.stride(0), beta.data_ptr(), bstride, N, M, D, C, bufs[0].data_ptr(),
                bufs[1].data_ptr(), bufs[2].data_ptr(), _stream())
    assert st == 0, f"tsvgp_kernel_grad_prod returned {st}"
    torch.cuda.synchronize(DEV)
    return bufs, sizes, (nrb, ncb, Mp, Dp)


def _operands(dtype, N, M, D, C, seed, strided):
    Xh, Zh, ilh, Uh, g0h, g1h, betah = _inputs(N, M, D, C, seed)
    Mp = (M + 127) // 128 * 128
    X, Z, il = _dev(Xh, dtype), _dev(Zh, dtype), _dev(ilh, dtype)
    if strided:  # ldu beyond Mp, g0 / g1 as column 1 of [N, 3] arrays, beta with stride 2: NaN wherever nothing may be used
        U = _padded_rows(Uh, dtype, Mp + 2, M, Mp)
        (_, g0), (_, g1) = _strided(g0h, dtype, 3, 1), _strided(g1h, dtype, 3, 1)
        (_, beta), bstride = _strided(betah, dtype, 2, 0), 2
    else:  # the engine's layout
        U = _padded_rows(Uh, dtype, Mp, M, Mp)
        g0, g1, beta, bstride = _dev(g0h, dtype), _dev(g1h, dtype), _dev(betah, dtype), 1
    return X, Z, il, U, g0, g1, beta, bstride


def _variances(dtype, C):
    """The components' variances and their product as the by-value argument holds it."""
    var = [float(torch.tensor(v, dtype=dtype)) for v in VARIANCES[:C]]
    prod = 1.0
    for v in var:
        prod *= v
    return var, float(torch.tensor(prod, dtype=dtype))


def _reference(kinds, var, variance, X, Z, il, U, g0, g1, beta, M):
    """The reference on the operands as the kernel sees them.  The kernel takes the ONE product of the variances; the reference is
    given component variances with that product (component 0 absorbs the product's rounding)."""
    rest = 1.0
    for v in var[1:]:
        rest *= v
    var = [variance / rest] + list(var[1:])
    return PR.fused(kinds, _host(X), _host(Z), _host(il), var, _host(U[:, :M]), _host(g0), _host(g1), _host(beta))


def _compare(what, dtype, C, got, ref):
    u, c_bound = UNIT[dtype], C_PER_COMPONENT * C
    worst, bad = 0.0, []
    for name, A in (("vsum", "A_vsum"), ("dls", "A_ls"), ("dZ", "A_Z")):
        err, bound = np.abs(got[name] - ref[name]), u * np.asarray(ref[A])
        live = bound > 0  # (a zeroed inv_ls column: no term at all, checked for an exact zero by the caller)
        assert np.all(err[~live] == 0) if np.ndim(err) else bool(live)
        ratio = float(np.max(err[live] / bound[live])) if np.ndim(err) else float(err / bound)
        worst = max(worst, ratio)
        print(f"{what}: {name} worst |got - ref| / (u A) = {ratio:.3f}")
        if ratio > c_bound:
            bad.append((name, ratio))
    _note(dtype, C, worst)
    assert not bad, f"{what}: beyond {c_bound:.0f} u A: {bad}"


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", range(len(SHAPES)), ids=[f"N{n}-M{m}-D{d}-C{c}" for n, m, d, c in SHAPES])
def test_every_entry_against_fp64_reference(case, dtype):
    N, M, D, C = SHAPES[case]
    _check_case(dtype, N, M, D, C, 5000 + case, case % 2 == 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 8, 16])
def test_every_compile_time_size_and_component_count(D, C, dtype):
    """The full cross D x C: every (Dpad, C) instantiation of the kernel, D = 3 with a padded dimension, at N = 70 (a full 64-row
    chunk and a ragged one) and M = 5 (the lone last column of a pair); layouts alternate."""
    _check_case(dtype, 70, 5, D, C, 8000 + 10 * D + C, (D + C) % 2 == 1)


def _check_case(dtype, N, M, D, C, seed, strided):
    kinds = KINDS[C]
    X, Z, il, U, g0, g1, beta, bstride = _operands(dtype, N, M, D, C, seed, strided)
    var, variance = _variances(dtype, C)
    args = (dtype, kinds, X, Z, il, variance, U, g0, g1, beta, bstride, N, M, D)
    bufs, sizes, (nrb, ncb, Mp, Dp) = _launch(*args)
    what = f"product gradient {DTYPE_IDS[DTYPES.index(dtype)]} N={N} M={M} D={D} C={C} {'strided' if strided else 'engine'} layout"
    for name, b, n in zip(("zpart", "lpart", "vpart"), bufs, sizes):
        assert bool(torch.isfinite(b[:n]).all()), f"{what}: {name} has a non-finite documented element"
        assert bool((b[n:] == 7.0).all()), f"{what}: {name} written beyond its documented extent"
    zpart, lpart = bufs[0][:sizes[0]].view(nrb, Mp, Dp), bufs[1][:sizes[1]].view(nrb, ncb, C, Dp)
    vpart = bufs[2][:sizes[2]].view(nrb, ncb)
    assert bool((zpart[:, M:, :] == 0).all()) and bool((zpart[:, :, D:] == 0).all()), f"{what}: zpart padding is not zero"
    assert bool((lpart[:, :, :, D:] == 0).all()), f"{what}: lpart padding is not zero"
    if C >= 2 and D >= 2:
        assert bool((lpart[:, :, 1, 0] == 0).all()), f"{what}: dls of a zeroed inv_ls column is not exactly zero"
    bufs2, _, _ = _launch(*args)
    for name, a, b in zip(("zpart", "lpart", "vpart"), bufs, bufs2):
        assert torch.equal(a, b), f"{what}: two runs differ in {name}"
    # summed as EStepEngine.kernel_grad_prod sums them
    got = dict(vsum=_host(vpart.sum()), dls=_host(lpart.sum(dim=(0, 1))[:, :D]), dZ=_host(zpart.sum(dim=0)[:M, :D]))
    ref = _reference(kinds, var, variance, X, Z, il, U, g0, g1, beta, M)
    _compare(what, dtype, C, got, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", ["se", "matern32", "matern52"])
@pytest.mark.parametrize("N,M,D", [(1025, 513, 3), (65, 2, 16)])
def test_one_component_agrees_with_the_single_kernel_contraction(N, M, D, kind, dtype):
    """C = 1 against ``tsvgp_kernel_grad_*`` on the same operands: entry by entry within the same c u A (the two kernels scale
    before and after the subtraction, so they need not agree bit for bit)."""
    X, Z, il, U, g0, g1, beta, bstride = _operands(dtype, N, M, D, 1, 6000 + N + D, False)
    variance = float(torch.tensor(1.3, dtype=dtype))
    bufs, sizes, (nrb, ncb, Mp, Dp) = _launch(dtype, (kind,), X, Z, il, variance, U, g0, g1, beta, bstride, N, M, D)
    pb, ps, _ = _launch_fused(dtype, kind, X, Z, il[0].contiguous(), variance, U, g0, g1, beta, bstride, N, M, D)
    ref = PR.fused((kind,), _host(X), _host(Z), _host(il), [variance], _host(U[:, :M]), _host(g0), _host(g1), _host(beta))
    u = UNIT[dtype]
    pairs = (("vsum", bufs[2][:sizes[2]].sum(), pb[2][:ps[2]].sum(), ref["A_vsum"]),
             ("dls", bufs[1][:sizes[1]].view(nrb, ncb, Dp).sum(dim=(0, 1))[:D], pb[1][:ps[1]].view(nrb, ncb, Dp).sum(dim=(0, 1))[:D], ref["A_ls"][0]),
             ("dZ", bufs[0][:sizes[0]].view(nrb, Mp, Dp).sum(dim=0)[:M, :D], pb[0][:ps[0]].view(nrb, Mp, Dp).sum(dim=0)[:M, :D], ref["A_Z"]))
    for name, a, b, A in pairs:
        ratio = float(np.max(np.abs(_host(a) - _host(b)) / (u * np.asarray(A))))
        print(f"C = 1 {kind} {DTYPE_IDS[DTYPES.index(dtype)]} N={N} M={M} D={D}: {name} |product form - single form| / (u A) = {ratio:.3f}")
        assert ratio <= C_PER_COMPONENT


def test_a_profile_flushed_to_zero_in_fp32_leaves_every_output_finite():
    """Component 1 is a squared exponential with lengthscale 0.05: exp(-s / 2) is below the smallest normal fp32 number on most
    entries and the kernel's exponential returns 0 there, not on all.  P_c comes from prefix and suffix products, so the other
    components' terms stay finite (a division of the full product by f_1 would be 0 / 0).  The entrywise bound is relative to A
    and knows nothing of underflow: a term below the smallest normal fp32 number is lost whole.  Such a term is at most
    tiny * 2 variance |V| |s_cd| inv_ls ~ 1e-35 here and there are N C = 390 of them per entry, 4e-33 in all, which c u A = 1e-4 A
    covers from A = 4e-29 on; the bound is checked on the entries with A >= 1e-20 and every entry must be finite."""
    dtype, N, M, D, C = torch.float32, 130, 130, 2, 3
    kinds = ("matern32", "se", "matern52")
    Xh, Zh, ilh, Uh, g0h, g1h, betah = _inputs(N, M, D, C, 7000)
    ilh = ilh.copy()
    ilh[1] = 1.0 / 0.05
    s1 = np.sum(((Xh[:, None, :] - Zh[None, :, :]) * ilh[1]) ** 2, axis=-1)
    flushed = -0.5 * s1 < np.log(np.finfo(np.float32).tiny) - 1.0
    assert 0.5 < flushed.mean() < 1.0 and (s1 < 20).sum() >= 8
    X, Z, il = _dev(Xh, dtype), _dev(Zh, dtype), _dev(ilh, dtype)
    U = _padded_rows(Uh, dtype, 128 * 2, M, 128 * 2)
    g0, g1, beta = _dev(g0h, dtype), _dev(g1h, dtype), _dev(betah, dtype)
    var, variance = _variances(dtype, C)
    bufs, sizes, (nrb, ncb, Mp, Dp) = _launch(dtype, kinds, X, Z, il, variance, U, g0, g1, beta, 1, N, M, D)
    for name, b, n in zip(("zpart", "lpart", "vpart"), bufs, sizes):
        assert bool(torch.isfinite(b[:n]).all()), f"{name} has a non-finite element"
    got = dict(vsum=_host(bufs[2][:sizes[2]].sum()), dls=_host(bufs[1][:sizes[1]].view(nrb, ncb, C, Dp).sum(dim=(0, 1))[:, :D]),
               dZ=_host(bufs[0][:sizes[0]].view(nrb, Mp, Dp).sum(dim=0)[:M, :D]))
    ref = _reference(kinds, var, variance, X, Z, il, U, g0, g1, beta, M)
    big = ref["A_Z"] >= 1e-20
    assert big.sum() >= 8 * D and ref["A_vsum"] >= 1e-20 and np.all(ref["A_ls"] >= 1e-20)
    print(f"flushed component: {int((~big).sum())} of {big.size} dZ entries have A below 1e-20")
    got["dZ"], ref["dZ"], ref["A_Z"] = got["dZ"][big], ref["dZ"][big], ref["A_Z"][big]
    _compare("product gradient f32 with a flushed component", dtype, C, got, ref)
