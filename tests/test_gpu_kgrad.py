"""The M-step gradient kernels called directly through the C-ABI, every entry of every output against tests/kgrad_ref.py (NumPy,
fp64): ``tsvgp_kernel_grad_f64/_f32`` (fused contraction, D <= 16), ``tsvgp_gram_to_gradw_f64/_f32`` (GEMM form, any D) and the
host finish of ``EStepEngine.kernel_grad`` / ``_kernel_grad_gemm``.  tests/test_gpu_mstep.py reaches them only through the
models, in fp64, at one column tile and D <= 8, against difference quotients good to ~1e-7.

Shapes: every edge of the kernels' tiling -- the 64-row chunk, the 1024-row block, the 512-column tile, the lone last column of
a thread's pair, every compile-time D (1, 2, 4, 8, 16) with and without padded dimensions; for the GEMM form a second x-block
(M = 513) and the second launch of the 65535-row loop (N = 65600).  Layouts: the engine's, and leading dimensions / element
strides beyond it with NaN in every slot that must not be addressed.  Buffers carry guard tails.

Bound: |got - ref| <= c u A entry by entry, A the sum of the absolute values of the entry's terms (kgrad_ref), u = 2^-53 / 2^-24,
c = 512 for both types: a term is a product of at most eight rounded factors; the profile's argument s carries D + 2 roundings,
amplified by at most |s| / 2 in exp, and terms with s > 40 are below 1e-8 of the sum; accumulation is in fp64 for both types (no
growth with N): about (D + 2) 20 + 16 <= 400 at D = 16.  For the GEMM form the cancellation in s = xx + zz - 2 G is bounded
separately (kgrad_ref.gemm_form).

Measured on an MI355X, worst |got - ref| / (u A) over all shapes and outputs (fused) and worst |W - ref| / bound, |dvar - ref| /
bound (GEMM form):
    fused      fp64: SE 2.75   Matern-3/2 3.39   Matern-5/2 3.19      fp32: SE 0.85   Matern-3/2 1.51   Matern-5/2 1.40
    GEMM W     fp64: SE 0.012  Matern-3/2 0.013  Matern-5/2 0.016     fp32: SE 0.011  Matern-3/2 0.405  Matern-5/2 0.025
    GEMM dvar  fp64: 0.002 (all three)                                fp32: 0.001 (all three)
(fp32 Matern-3/2 W: the nearly coincident rows, where the rounding of s decides f'.)  With c = 512 no case comes near the bound, and
at u = 2^-24 the bound is 3e-5: the exact-operand test below is what holds the profiles' constants in fp32 (worst measured there:
1.43 u, Matern-5/2 fp32 W).

Host finish: the project's own bounds: fp64 relerr <= 1e-8; fp32 atol 1e-4 + rtol 1e-3 max|ref|."""
import functools

import numpy as np
import pytest
import torch

from tests import kgrad_ref as R
from tests.helpers import pkg, relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KIND_ID = {"se": 0, "matern32": 2, "matern52": 3}
DTYPES = [torch.float64, torch.float32]
DTYPE_IDS = ["f64", "f32"]
UNIT = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}
C_BOUND = 512.0
GUARD = 64
VARIANCE = 1.3

WORST = {}  # (what, dtype id, kind) -> worst ratio seen in this session; printed when the module is done


@pytest.fixture(scope="module")
def engines():
    from importlib import import_module

    estep = import_module("t-svgp_amd.estep")
    return {dt: estep.EStepEngine(dt, DEV) for dt in DTYPES}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for key in sorted(WORST):
        print(f"\nworst ratio {key[0]} {key[1]} {key[2]}: {WORST[key]:.3f}", end="")
    print()


def _note(what, dtype, kind, ratio):
    key = (what, DTYPE_IDS[DTYPES.index(dtype)], kind)
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def _dev(a, dtype):
    return torch.tensor(np.array(a, dtype=np.float64), dtype=dtype, device=DEV)  # a copy: the shared inputs are read-only


def _host(t):
    return t.double().cpu().numpy()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _strided(values, dtype, width, col):
    """values [n] as column ``col`` of an [n, width] array whose other slots hold NaN; returns (array, view of the column)."""
    buf = torch.full((values.shape[0], width), float("nan"), dtype=dtype, device=DEV)
    buf[:, col] = _dev(values, dtype)
    return buf, buf[:, col]


def _padded_rows(values, dtype, ld, valid_cols, zero_cols):
    """values [n, valid_cols] in an [n, ld] array: zeros up to ``zero_cols`` (the padding the kernels may read), NaN beyond."""
    buf = torch.full((values.shape[0], ld), float("nan"), dtype=dtype, device=DEV)
    buf[:, :zero_cols] = 0.0
    buf[:, :valid_cols] = _dev(values, dtype)
    return buf


@functools.lru_cache(maxsize=None)
def _inputs(N, M, D, seed):
    """Seeded fp64 host inputs, shared by every kind and type (never written to).  Lengthscales in [0.7, 1.7] sqrt(D) keep the
    kernel values away from zero; the first rows of Z are rows of X (inducing points taken from the data: s = 0 exactly in the
    difference form, the Matern clamp); U, g0, g1, beta of order 1, g1 of both signs."""
    rng = np.random.RandomState(seed)
    X, Z = rng.randn(N, D), rng.randn(M, D)
    k = min(N, M, 8)
    Z[:k] = X[:k]
    ls = (0.7 + rng.rand(D)) * np.sqrt(D)
    U, g0, g1, beta = rng.randn(N, M), rng.randn(N), rng.randn(N), rng.randn(M)
    assert N == 1 or (g1.min() < 0 < g1.max())
    for a in (X, Z, ls, U, g0, g1, beta):
        a.setflags(write=False)
    return X, Z, ls, U, g0, g1, beta


# ------------------------------------------------------------------------------------------------ the fused kernel
FUSED_SHAPES = [(1, 1, 1), (63, 127, 2), (64, 128, 2), (65, 129, 3), (1023, 511, 4), (1024, 512, 5), (1025, 513, 8),
                (130, 1000, 13), (1100, 300, 16), (2100, 641, 9)]


def _launch_fused(dtype, kind, X, Z, il, variance, U, g0, g1, beta, bstride, N, M, D):
    """One launch into fresh buffers of the documented sizes plus a guard tail, everything pre-filled with 7."""
    lib = pkg()._backend.lib()
    rows, Dp = int(lib.tsvgp_kernel_grad_rows()), int(lib.tsvgp_kernel_grad_dpad(D))
    Mp = (M + 127) // 128 * 128
    nrb, ncb = (N + rows - 1) // rows, (Mp + 511) // 512
    sizes = (nrb * Mp * Dp, nrb * ncb * Dp, nrb * ncb)
    bufs = [torch.full((n + GUARD,), 7.0, dtype=torch.float64, device=DEV) for n in sizes]
    fn = lib.tsvgp_kernel_grad_f64 if dtype == torch.float64 else lib.tsvgp_kernel_grad_f32
    assert g0.stride(0) == g1.stride(0)
    with torch.cuda.device(DEV):
        st = fn(KIND_ID[kind], X.data_ptr(), Z.data_ptr(), il.data_ptr(), variance, U.data_ptr(), U.stride(0), g0.data_ptr(),
                g1.data_ptr(), g0.stride(0), beta.data_ptr(), bstride, N, M, D, bufs[0].data_ptr(), bufs[1].data_ptr(),
                bufs[2].data_ptr(), _stream())
    assert st == 0, f"tsvgp_kernel_grad returned {st}"
    torch.cuda.synchronize(DEV)
    return bufs, sizes, (nrb, ncb, Mp, Dp)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", range(len(FUSED_SHAPES)), ids=[f"N{n}-M{m}-D{d}" for n, m, d in FUSED_SHAPES])
def test_fused_kernel_every_entry_against_fp64_reference(case, kind, dtype):
    N, M, D = FUSED_SHAPES[case]
    Xh, Zh, ls, Uh, g0h, g1h, betah = _inputs(N, M, D, 1000 + case)
    Mp = (M + 127) // 128 * 128
    strided = case % 2 == 1
    X, Z, il = _dev(Xh, dtype), _dev(Zh, dtype), _dev(1.0 / ls, dtype)
    variance = float(torch.tensor(VARIANCE, dtype=dtype))  # what the by-value argument holds
    if strided:  # ldu beyond Mp, g0 / g1 as column 1 of [N, 3] arrays, beta with stride 2: NaN wherever nothing may be addressed
        U = _padded_rows(Uh, dtype, Mp + 2, M, Mp)
        (_, g0), (_, g1) = _strided(g0h, dtype, 3, 1), _strided(g1h, dtype, 3, 1)
        (betabuf, beta), bstride = _strided(betah, dtype, 2, 0), 2
    else:  # the engine's layout
        U = _padded_rows(Uh, dtype, Mp, M, Mp)
        g0, g1, beta, bstride = _dev(g0h, dtype), _dev(g1h, dtype), _dev(betah, dtype), 1
    args = (dtype, kind, X, Z, il, variance, U, g0, g1, beta, bstride, N, M, D)
    bufs, sizes, (nrb, ncb, Mp_, Dp) = _launch_fused(*args)
    assert Mp_ == Mp
    what = f"fused {kind} {DTYPE_IDS[DTYPES.index(dtype)]} N={N} M={M} D={D} {'strided' if strided else 'engine'} layout"
    for name, b, n in zip(("zpart", "lpart", "vpart"), bufs, sizes):
        assert bool(torch.isfinite(b[:n]).all()), f"{what}: {name} has a non-finite documented element"
        assert bool((b[n:] == 7.0).all()), f"{what}: {name} written beyond its documented extent"
    zpart, lpart, vpart = bufs[0][:sizes[0]].view(nrb, Mp, Dp), bufs[1][:sizes[1]].view(nrb, ncb, Dp), bufs[2][:sizes[2]].view(nrb, ncb)
    assert bool((zpart[:, M:, :] == 0).all()) and bool((zpart[:, :, D:] == 0).all()), f"{what}: zpart padding is not zero"
    assert bool((lpart[:, :, D:] == 0).all()), f"{what}: lpart padding is not zero"
    bufs2, _, _ = _launch_fused(*args)
    for name, a, b in zip(("zpart", "lpart", "vpart"), bufs, bufs2):
        assert torch.equal(a, b), f"{what}: two runs differ in {name}"
    # summed as EStepEngine.kernel_grad sums them
    got = dict(dvar=_host(vpart.sum()), dls=_host(lpart.sum(dim=(0, 1))[:D]), dZ=_host(zpart.sum(dim=0)[:M, :D]))
    # the reference sees the operands as the kernel does: rounded to the array type
    ref = R.fused(kind, _host(X), _host(Z), _host(il), variance, _host(U[:, :M]), _host(g0), _host(g1), _host(beta))
    u = UNIT[dtype]
    worst, bad = 0.0, []
    for name, A in (("dvar", "A_var"), ("dls", "A_ls"), ("dZ", "A_Z")):
        err, bound = np.abs(got[name] - ref[name]), u * np.asarray(ref[A])
        assert np.all(bound > 0)
        ratio = float(np.max(err / bound))
        worst = max(worst, ratio)
        print(f"{what}: {name} worst |got - ref| / (u A) = {ratio:.3f}")
        if not np.all(err <= C_BOUND * bound):
            idx = np.unravel_index(np.argmax(err / bound), np.shape(err)) if np.ndim(err) else ()
            bad.append((name, idx, ratio))
    _note("fused", dtype, kind, worst)
    assert not bad, f"{what}: beyond {C_BOUND:.0f} u A: {bad}"


# ------------------------------------------------------------------------------------------------ the GEMM-form kernel
GEMM_SHAPES = [(1, 1), (127, 129), (128, 130), (300, 513), (65600, 129)]
GEMM_D = 20


@functools.lru_cache(maxsize=None)
def _gemm_inputs(N, M):
    Xh, Zh, ls, Uh, g0h, g1h, betah = _inputs(N, M, GEMM_D, 2000 + N + M)
    Zh = Zh.copy()
    k, k8 = min(N, M, 4), min(N, M, 8)
    # the first 4 rows of Z equal X: xx, zz and G round to the same number, s = 0 (fp64: to an ulp).  The next 4 are 1e-5 away in relative
    # terms: s ~ 1e-10, far below the rounding of xx + zz - 2 G in fp32 (~1e-7), which then comes out with either sign
    Zh[k:k8] = Xh[k:k8] * (1.0 + 1e-5)
    xt, zt = Xh / ls, Zh / ls
    out = (xt @ zt.T, np.sum(xt * xt, axis=1), np.sum(zt * zt, axis=1), Uh, g0h, g1h, betah)
    for a in out:
        a.setflags(write=False)
    return out


def _launch_gemm(dtype, kind, Gh, xx, zz, variance, U, g0, g1, beta, bstride, N, M):
    """One launch on a fresh copy of G in a [rows_pad, cols_pad + 2] array pre-filled with 7, vpart pre-filled with NaN."""
    lib = pkg()._backend.lib()
    rows_pad, cols_pad = (N + 127) // 128 * 128, (M + 127) // 128 * 128
    G = torch.full((rows_pad, cols_pad + 2), 7.0, dtype=dtype, device=DEV)
    G[:N, :M] = Gh
    parts = int(lib.tsvgp_gram_to_gradw_parts(N, M))
    assert parts == rows_pad * ((cols_pad // 2 + 255) // 256)
    vpart = torch.full((parts + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    fn = lib.tsvgp_gram_to_gradw_f64 if dtype == torch.float64 else lib.tsvgp_gram_to_gradw_f32
    assert g0.stride(0) == g1.stride(0)
    with torch.cuda.device(DEV):
        st = fn(KIND_ID[kind], G.data_ptr(), xx.data_ptr(), zz.data_ptr(), variance, U.data_ptr(), U.stride(0), g0.data_ptr(),
                g1.data_ptr(), g0.stride(0), beta.data_ptr(), bstride, N, M, G.stride(0), vpart.data_ptr(), _stream())
    assert st == 0, f"tsvgp_gram_to_gradw returned {st}"
    torch.cuda.synchronize(DEV)
    return G, vpart, parts


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("N,M", GEMM_SHAPES)
def test_gemm_form_kernel_every_entry_against_fp64_reference(N, M, kind, dtype):
    Gh64, xxh, zzh, Uh, g0h, g1h, betah = _gemm_inputs(N, M)
    rows_pad, cols_pad = (N + 127) // 128 * 128, (M + 127) // 128 * 128
    gx = (cols_pad // 2 + 255) // 256
    variance = float(torch.tensor(VARIANCE, dtype=dtype))
    Gh, xx, zz = _dev(Gh64, dtype), _dev(xxh, dtype), _dev(zzh, dtype)  # formed in fp64, then rounded to the array type
    U = _padded_rows(Uh, dtype, cols_pad + 4, M, cols_pad)
    (_, g0), (_, g1) = _strided(g0h, dtype, 2, 1), _strided(g1h, dtype, 2, 1)
    _, beta = _strided(betah, dtype, 3, 2)
    args = (dtype, kind, Gh, xx, zz, variance, U, g0, g1, beta, 3, N, M)
    G, vpart, parts = _launch_gemm(*args)
    what = f"gemm form {kind} {DTYPE_IDS[DTYPES.index(dtype)]} N={N} M={M}"
    if min(N, M) >= 8:  # the point of the (nearly) coincident rows: s = 0 up to the rounding of G, xx, zz, of either sign
        s8 = _host(xx)[:8] + _host(zz)[:8] - 2.0 * np.diagonal(_host(Gh[:8, :8]))
        print(f"{what}: s at the coincident points {s8}")
        assert s8.min() <= 0  # at or below the Matern clamp
    assert bool((G[:, cols_pad:] == 7.0).all()), f"{what}: wrote beyond column cols_pad"
    assert bool((G[N:, :cols_pad] == 0).all()) and bool((G[:, M:cols_pad] == 0).all()), f"{what}: padding of W is not zero"
    assert bool(torch.isfinite(vpart[:parts]).all()), f"{what}: vpart has a non-finite documented element"
    assert bool((vpart[:parts].view(rows_pad, gx)[N:] == 0).all()), f"{what}: vpart of the rows beyond N is not zero"
    assert bool(torch.isnan(vpart[parts:]).all()), f"{what}: vpart written beyond its documented extent"
    G2, vpart2, _ = _launch_gemm(*args)
    assert torch.equal(G, G2) and torch.equal(vpart[:parts], vpart2[:parts]), f"{what}: two runs differ"
    W, dvar, W_bound, dvar_bound = R.gemm_form(kind, _host(Gh), _host(xx), _host(zz), variance, _host(U[:, :M]), _host(g0), _host(g1),
                                               _host(beta), N, M, u=UNIT[dtype], c=C_BOUND)
    err = np.abs(_host(G[:N, :M]) - W)
    assert np.all(W_bound > 0)
    ratio_w, ratio_v = float(np.max(err / W_bound)), abs(float(vpart[:parts].sum()) - dvar) / dvar_bound
    print(f"{what}: worst |W - ref| / bound = {ratio_w:.4f}, |dvar - ref| / bound = {ratio_v:.4f}")
    _note("gemm W/bound", dtype, kind, ratio_w)
    _note("gemm dvar/bound", dtype, kind, ratio_v)
    idx = np.unravel_index(np.argmax(err / W_bound), err.shape)
    assert np.all(err <= W_bound), f"{what}: W beyond its bound at {idx}: {ratio_w:.3f} of the bound"
    assert ratio_v <= 1.0, f"{what}: dvar {ratio_v:.3f} of its bound"


# ------------------------------------------------------------------------------------------------ exact operands
# c = 512 at u = 2^-24 is 3e-5: no relative error below that in a profile's constants can show in fp32 above.  Here every operand
# is a small dyadic number (D = 1, unit lengthscale and variance, |x - z| in {1/8, 1/4}, V = +-2, +-4 formed without rounding), so
# that s, r = sqrt(s), V and every product with V, s_d, variance are exact in either type and ONLY the profile rounds.  Counting
# its roundings for the worst case, Matern-5/2 f' = -(5/6)(1 + a) e^-a at a = sqrt(5) / 4: the constants sqrt(5), 5/6 (u each),
# a = sqrt(5) r, 1 + a, two products (u each), exp to one ulp (2 u), the error of a felt through (1 + a) e^-a by a^2 / (1 + a) =
# 0.2 (three times: constant, product, a square root that is not correctly rounded): at most 6.6 u per term; f, and the other two
# kinds, have fewer.  Every term of dZ has the same sign, so the bound is 8 u times the sum itself.
EXACT_C = 8.0


def _exact_problem():
    X = np.array([1.125, 1.25, 0.875, 0.75])[:, None]
    Z = np.array([1.0, 1.0])[:, None]
    g0, g1, beta = np.array([1.0, 2.0, -2.0, -1.0]), np.array([-0.5, -0.5, 0.5, 0.5]), np.array([1.0, 2.0])
    U = np.array([1.0, 2.0, 2.0, 1.0])[:, None] * np.array([1.0, 2.0])[None, :]
    V = g0[:, None] * beta[None, :] - 2.0 * g1[:, None] * U  # [+2, +4, -4, -2] x [1, 2]: dvar and dls do not cancel to zero
    sd = X - Z.T
    assert np.all(np.sign(V) == np.sign(sd)) and set(np.abs(V).ravel()) <= {2.0, 4.0, 8.0}
    return X, Z, U, g0, g1, beta, V, sd


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_both_kernels_on_exact_operands_where_only_the_profile_rounds(kind, dtype):
    Xh, Zh, Uh, g0h, g1h, betah, V, sd = _exact_problem()
    N, M = sd.shape
    f, df = R.profile_grad(kind, sd * sd)
    w = -2.0 * V * df
    u, tag = UNIT[dtype], DTYPE_IDS[DTYPES.index(dtype)]
    assert np.all(w * sd > 0)  # no cancellation in dZ: a relative error common to every f' shows in full
    # fused kernel
    X, Z, il = _dev(Xh, dtype), _dev(Zh, dtype), _dev(np.ones(1), dtype)
    U = _padded_rows(Uh, dtype, 128, M, 128)
    bufs, sizes, (nrb, ncb, Mp, Dp) = _launch_fused(dtype, kind, X, Z, il, 1.0, U, _dev(g0h, dtype), _dev(g1h, dtype),
                                                    _dev(betah, dtype), 1, N, M, 1)
    got = dict(dvar=float(bufs[2][:sizes[2]].sum()), dls=float(bufs[1][:sizes[1]].sum()), dZ=_host(bufs[0][:M]))
    for name, terms in (("dvar", V * f), ("dls", (w * sd * sd)), ("dZ", w * sd)):
        ref, A = (terms.sum(axis=0), np.abs(terms).sum(axis=0)) if name == "dZ" else (terms.sum(), np.abs(terms).sum())
        ratio = float(np.max(np.abs(got[name] - ref) / (u * A)))
        print(f"exact operands fused {kind} {tag}: {name} |got - ref| / (u sum|terms|) = {ratio:.3f}")
        _note("exact fused", dtype, kind, ratio)
        assert ratio <= EXACT_C, f"fused {kind} {tag} {name}: {ratio:.3f} u"
    # GEMM form: G = x z^T, xx = x^2, zz = z^2 and s = xx + zz - 2 G are exact as well
    Gh, xx, zz = _dev(Xh @ Zh.T, dtype), _dev((Xh * Xh)[:, 0], dtype), _dev((Zh * Zh)[:, 0], dtype)
    G, vpart, parts = _launch_gemm(dtype, kind, Gh, xx, zz, 1.0, U, _dev(g0h, dtype), _dev(g1h, dtype), _dev(betah, dtype), 1, N, M)
    ratio_w = float(np.max(np.abs(_host(G[:N, :M]) - w) / (u * np.abs(w))))
    ratio_v = abs(float(vpart[:parts].sum()) - (V * f).sum()) / (u * np.abs(V * f).sum())
    print(f"exact operands gemm form {kind} {tag}: |W - ref| / (u |W|) = {ratio_w:.3f}, dvar {ratio_v:.3f}")
    _note("exact gemm", dtype, kind, max(ratio_w, ratio_v))
    assert ratio_w <= EXACT_C and ratio_v <= EXACT_C, f"gemm form {kind} {tag}: W {ratio_w:.3f} u, dvar {ratio_v:.3f} u"


# ------------------------------------------------------------------------------------------------ the host finish
HOST_N, HOST_M = 700, 150


def _close(got, ref, dtype, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if dtype == torch.float64:
        e = relerr(got, ref)
        print(f"{what} fp64 relerr {e:.3e}")
        assert e <= 1e-8, f"{what}: relerr {e:.3e}"
    else:
        e, bound = float(np.max(np.abs(got - ref))), 1e-4 + 1e-3 * float(np.max(np.abs(ref)))
        print(f"{what} fp32 max abs err {e:.3e} (bound {bound:.3e})")
        assert e <= bound, f"{what}: max abs err {e:.3e} > {bound:.3e}"


def _engine_problem(eng, kind, D):
    """Operands in the engine's layout (U [Np, Mp] zero-padded, compute dtype) and the fp64 reference on what the kernels see."""
    p, dtype = pkg(), eng.dtype
    Xh, Zh, ls, Uh, g0h, g1h, betah = _inputs(HOST_N, HOST_M, D, 3000 + D)
    kernel = {"se": p.SquaredExponential, "matern32": p.Matern32, "matern52": p.Matern52}[kind](VARIANCE, np.array(ls))
    B = p._backend
    Np, Mp = B.round_up(HOST_N), B.round_up(HOST_M)
    X, Z = _dev(Xh, dtype), _dev(Zh, dtype)
    U = torch.zeros((Np, Mp), dtype=dtype, device=DEV)
    U[:HOST_N, :HOST_M] = _dev(Uh, dtype)
    g0, g1 = _dev(g0h, dtype), _dev(g1h, dtype)
    beta = _dev(betah, torch.float64)
    il = kernel.inv_lengthscales(D, dtype, torch.device(DEV))
    ref = R.fused(kind, _host(X), _host(Z), _host(il), float(torch.tensor(VARIANCE, dtype=dtype)), _host(U[:HOST_N, :HOST_M]),
                  _host(g0), _host(g1), _host(beta.to(dtype)))
    return (X, Z, kernel, U, g0, g1, beta), ref


def _check_triple(out, ref, dtype, what):
    dvar, dls, dZ = out
    assert tuple(dls.shape) == ref["dls"].shape and tuple(dZ.shape) == ref["dZ"].shape
    assert dvar.dtype == dls.dtype == dZ.dtype == torch.float64
    _close(_host(dvar), ref["dvar"], dtype, what + " dvar")
    _close(_host(dls), ref["dls"], dtype, what + " dls")
    _close(_host(dZ), ref["dZ"], dtype, what + " dZ")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_host_finish_fused_and_gemm_paths_agree_at_d16(engines, kind, dtype):
    eng = engines[dtype]
    args, ref = _engine_problem(eng, kind, 16)
    fused = eng.kernel_grad(*args)
    gemm = eng._kernel_grad_gemm(*args)
    _check_triple(fused, ref, dtype, f"{kind} D=16 fused path")
    _check_triple(gemm, ref, dtype, f"{kind} D=16 GEMM path")
    for name, a, b in zip(("dvar", "dls", "dZ"), gemm, fused):
        _close(_host(a), _host(b), dtype, f"{kind} D=16 GEMM path vs fused path {name}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("D", [17, 40])
def test_host_finish_gemm_path_beyond_d16(engines, D, kind, dtype):
    eng = engines[dtype]
    args, ref = _engine_problem(eng, kind, D)
    _check_triple(eng.kernel_grad(*args), ref, dtype, f"{kind} D={D} kernel_grad")
