"""``tsvgp_moments_vjp_f64/_f32`` called directly through the C-ABI, every entry of dX against tests/predict_vjp_ref.py (NumPy,
fp64) on operands rounded to the array type.  tests/test_gpu_predict_grad.py reaches the kernel only through the models.

Shapes: every edge of the kernel's tiling.  With R = tsvgp_moments_vjp_rows(D) rows per workgroup (256 up to D = 8, 128 up to 16, 32
beyond) and C = 128 (fp64) / 256 (fp32) columns per lane sweep: N in {1, R - 1, R, R + 1, 2 R + 3}, M in {1, odd M and M = 2 mod 4 (one, two
or three last columns of a lane's vector), C - 1, C, C + 1}, an M beyond one LDS stage of z~ (tsvgp_moments_vjp_stage_*(D)) for every stage size
that fits below 1100 columns, and every compile-time D with and without padded dimensions.  Layouts: the engine's, and leading
dimensions / element strides beyond it; NaN in every slot that must not be addressed, U's columns >= M included; guard rows
behind dX.

Bound: |got - ref| <= 512 u A entry by entry, A the sum of the absolute values of the entry's terms (predict_vjp_ref), u = 2^-53 /
2^-24 -- the constant and the derivation of tests/test_gpu_kgrad.py: a dX term has the factors of a dZ term (at most eight rounded
factors; the profile's argument carries D + 2 roundings amplified by at most |s| / 2 in exp; terms with s > 40 are below 1e-8 of
the sum) and the accumulation is in fp64 for both types.  The exact-operand case (D = 1, dyadic operands: only the profile rounds)
holds the profiles' constants in fp32 with that file's 8 u.

Measured on an MI355X, worst |got - ref| / (u A) over all shapes, and worst |got - ref| / (u sum|terms|) on the exact operands:
    dX     fp64: SE 2.69   Matern-3/2 3.07   Matern-5/2 2.64      fp32: SE 1.57   Matern-3/2 2.42   Matern-5/2 2.36
    exact  fp64: 0.00 (all three)                                 fp32: SE 0.34   Matern-3/2 0.13   Matern-5/2 1.43
"""
import functools

import numpy as np
import pytest
import torch

from tests import predict_vjp_ref as R
from tests.helpers import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KIND_ID = {"se": 0, "matern32": 2, "matern52": 3}
DTYPES = [torch.float64, torch.float32]
DTYPE_IDS = ["f64", "f32"]
UNIT = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}
SWEEP = {torch.float64: 128, torch.float32: 256}
C_BOUND = 512.0
EXACT_C = 8.0
GUARD = 5  # rows behind dX
VARIANCE = 1.3

WORST = {}


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
    """values [n] as column ``col`` of an [n, width] array whose other slots hold NaN; returns the view of the column."""
    buf = torch.full((values.shape[0], width), float("nan"), dtype=dtype, device=DEV)
    buf[:, col] = _dev(values, dtype)
    return buf[:, col]


def _u_rows(values, dtype, ld):
    """values [n, M] in an [n, ld] array with NaN in every column >= M: the kernel reads none of them."""
    buf = torch.full((values.shape[0], ld), float("nan"), dtype=dtype, device=DEV)
    buf[:, :values.shape[1]] = _dev(values, dtype)
    return buf


@functools.lru_cache(maxsize=None)
def _inputs(N, M, D, seed):
    """Seeded fp64 host inputs, shared by every kind and type (never written to): the recipe of tests/test_gpu_kgrad.py.
    Lengthscales in [0.7, 1.7] sqrt(D); the first rows of Z are rows of X (s = 0 exactly, the Matern clamp); U, cm, cv, beta of
    order 1, cv of both signs."""
    rng = np.random.RandomState(seed)
    X, Z = rng.randn(N, D), rng.randn(M, D)
    k = min(N, M, 8)
    Z[:k] = X[:k]
    ls = (0.7 + rng.rand(D)) * np.sqrt(D)
    U, cm, cv, beta = rng.randn(N, M), rng.randn(N), rng.randn(N), rng.randn(M)
    assert N == 1 or (cv.min() < 0 < cv.max())
    for a in (X, Z, ls, U, cm, cv, beta):
        a.setflags(write=False)
    return X, Z, ls, U, cm, cv, beta


def _call(dtype, kind, X, Z, il, variance, U, cm, cv, beta, bstride, N, M, D, dX, accumulate=0):
    lib = pkg()._backend.lib()
    fn = lib.tsvgp_moments_vjp_f64 if dtype == torch.float64 else lib.tsvgp_moments_vjp_f32
    assert cm.stride(0) == cv.stride(0) or N == 1
    assert U.shape[0] >= N and U.shape[1] >= M and dX.dtype == torch.float64 and dX.is_contiguous() and dX.shape[0] >= N
    with torch.cuda.device(DEV):
        st = fn(KIND_ID[kind], X.data_ptr(), Z.data_ptr(), il.data_ptr(), variance, U.data_ptr(), U.stride(0), cm.data_ptr(),
                cv.data_ptr(), max(cm.stride(0), 1), beta.data_ptr(), bstride, N, M, D, dX.data_ptr(), accumulate, _stream())
    assert st == 0, f"tsvgp_moments_vjp returned {st}"
    torch.cuda.synchronize(DEV)
    return dX


def _rows(D):
    return int(pkg()._backend.lib().tsvgp_moments_vjp_rows(D))


def _stage(dtype, D):
    lib = pkg()._backend.lib()
    return int((lib.tsvgp_moments_vjp_stage_f64 if dtype == torch.float64 else lib.tsvgp_moments_vjp_stage_f32)(D))


def _shapes(dtype):
    """(N, M, D): see the module docstring.  R and the stage come from the library, C from the header."""
    C = SWEEP[dtype]
    r = {D: _rows(D) for D in (1, 2, 3, 4, 5, 8, 13, 16, 17, 32)}
    shapes = [(1, 1, 1), (r[2] - 1, 7, 2), (r[3], C - 1, 3), (r[4] + 1, C, 4), (2 * r[5] + 3, C + 1, 5), (r[8] + 1, 2 * C + 3, 8),
              (2 * r[13] + 3, 62, 13), (r[16] - 1, C + 1, 16), (2 * r[17] + 3, C - 1, 17), (r[32] + 1, 33, 32)]
    # beyond one LDS stage of z~, for every stage size below 1100 columns: one column, and a lone column, into the next stage
    for D in (8, 16, 32):
        st = _stage(dtype, D)
        if st + 3 <= 1100:
            shapes.append((r[D] + 2, st + (1 if D == 8 else 3), D))
    shapes.append((70, 2 * _stage(dtype, 32) + 5, 29))  # three stages
    assert all(n <= 2100 and m <= 1100 for n, m, _ in shapes)
    return shapes


N_SHAPES = 14


def _case(dtype, case):
    shapes = _shapes(dtype)
    assert len(shapes) == N_SHAPES, len(shapes)
    return shapes[case]


def _operands(dtype, N, M, D, seed, strided):
    Xh, Zh, ls, Uh, cmh, cvh, betah = _inputs(N, M, D, seed)
    Mp = (M + 127) // 128 * 128
    X, Z, il = _dev(Xh, dtype), _dev(Zh, dtype), _dev(1.0 / ls, dtype)
    variance = float(torch.tensor(VARIANCE, dtype=dtype))  # what the by-value argument holds
    if strided:  # ldu beyond Mp, cm / cv as column 1 of [N, 3] arrays, beta with stride 2: NaN wherever nothing may be addressed
        U = _u_rows(Uh, dtype, Mp + 4)
        cm, cv = _strided(cmh, dtype, 3, 1), _strided(cvh, dtype, 3, 1)
        beta, bstride = _strided(betah, dtype, 2, 0), 2
    else:  # the engine's layout (its padding holds zeros; NaN here: columns >= M are not read either way)
        U = _u_rows(Uh, dtype, Mp)
        cm, cv, beta, bstride = _dev(cmh, dtype), _dev(cvh, dtype), _dev(betah, dtype), 1
    return (X, Z, il, variance, U, cm, cv, beta, bstride, N, M, D)


def _fresh(N, D, fill=7.0):
    return torch.full((N + GUARD, D), fill, dtype=torch.float64, device=DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", range(N_SHAPES))
def test_every_entry_against_fp64_reference(case, kind, dtype):
    N, M, D = _case(dtype, case)
    strided = case % 2 == 1
    ops = _operands(dtype, N, M, D, 4000 + case, strided)
    X, Z, il, variance, U, cm, cv, beta, bstride = ops[:9]
    what = f"{kind} {DTYPE_IDS[DTYPES.index(dtype)]} N={N} M={M} D={D} {'strided' if strided else 'engine'} layout"
    dX = _call(dtype, kind, *ops, _fresh(N, D))
    assert bool(torch.isfinite(dX[:N]).all()), f"{what}: a non-finite entry (something beyond M or N was read)"
    assert bool((dX[N:] == 7.0).all()), f"{what}: rows >= N were written"
    again = _call(dtype, kind, *ops, _fresh(N, D, -3.0))
    assert torch.equal(dX[:N], again[:N]), f"{what}: two launches differ"
    # accumulate = 1 onto a known array: bit for bit the write followed by an addition
    known = torch.linspace(-2.0, 3.0, (N + GUARD) * D, dtype=torch.float64, device=DEV).reshape(N + GUARD, D).contiguous()
    acc = _call(dtype, kind, *ops, known.clone(), accumulate=1)
    assert torch.equal(acc[:N], known[:N] + dX[:N]), f"{what}: accumulate = 1 is not write-then-add"
    assert torch.equal(acc[N:], known[N:]), f"{what}: accumulate = 1 touched rows >= N"
    # the reference sees the operands as the kernel does: rounded to the array type
    ref, A = R.vjp(kind, _host(X), _host(Z), _host(il), variance, _host(U[:, :M]), _host(cm), _host(cv), _host(beta))
    err, bound = np.abs(_host(dX[:N]) - ref), UNIT[dtype] * A
    assert np.all(bound > 0)
    ratio = float(np.max(err / bound))
    print(f"{what}: worst |got - ref| / (u A) = {ratio:.3f}")
    _note("dX", dtype, kind, ratio)
    idx = np.unravel_index(np.argmax(err / bound), err.shape)
    assert np.all(err <= C_BOUND * bound), f"{what}: beyond {C_BOUND:.0f} u A at {idx}: {ratio:.3f}"
    k = min(N, M, 8)  # the inputs did hold rows that are inducing points (s = 0 exactly, the Matern clamp), rounded alike
    assert np.array_equal(_host(X[:k]), _host(Z[:k]))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("D,M", [(1, 5), (2, 70), (3, 130), (8, 600), (16, 259), (32, 40)])
def test_a_row_has_the_same_bits_alone_and_anywhere_in_a_batch(D, M, kind, dtype):
    """dX[n] depends on row n's own operands alone: evaluated as a batch of one, and as row 0, 1, 2, 3 (every place of a pass of
    four, two or one rows: D = 1, 2 carry four), R + 1 and the last of a batch of 2 R + 2 other rows, it has the same bits."""
    Rr = _rows(D)
    N = 2 * Rr + 2
    Xh, Zh, ls, Uh, cmh, cvh, betah = _inputs(N, M, D, 5000 + D)
    rng = np.random.RandomState(77 + D)
    x, u, gm, gv = rng.randn(1, D), rng.randn(1, M), rng.randn(1), rng.randn(1)
    Z, il, beta = _dev(Zh, dtype), _dev(1.0 / ls, dtype), _dev(betah, dtype)
    variance = float(torch.tensor(VARIANCE, dtype=dtype))
    Mp = (M + 127) // 128 * 128
    alone = _call(dtype, kind, _dev(x, dtype), Z, il, variance, _u_rows(u, dtype, Mp), _dev(gm, dtype), _dev(gv, dtype), beta, 1, 1, M, D,
                  _fresh(1, D))[:1]
    assert bool(torch.isfinite(alone).all())
    for at in (0, 1, 2, 3, Rr + 1, N - 1):
        Xb, Ub, cmb, cvb = Xh.copy(), Uh.copy(), cmh.copy(), cvh.copy()
        Xb[at], Ub[at], cmb[at], cvb[at] = x[0], u[0], gm[0], gv[0]
        got = _call(dtype, kind, _dev(Xb, dtype), Z, il, variance, _u_rows(Ub, dtype, Mp), _dev(cmb, dtype), _dev(cvb, dtype), beta, 1, N,
                    M, D, _fresh(N, D))
        assert torch.equal(got[at:at + 1], alone), f"{kind} D={D} M={M}: row at {at} differs from the row alone"


def _exact_problem():
    """tests/test_gpu_kgrad.py's: D = 1, unit lengthscale and variance, |x - z| in {1/8, 1/4}, V = +-2, +-4, +-8 formed without
    rounding, the sign of V that of s_d: s, V and every product with them are exact in either type and only the profile rounds."""
    X = np.array([1.125, 1.25, 0.875, 0.75])[:, None]
    Z = np.array([1.0, 1.0])[:, None]
    cm, cv, beta = np.array([1.0, 2.0, -2.0, -1.0]), np.array([-0.5, -0.5, 0.5, 0.5]), np.array([1.0, 2.0])
    U = np.array([1.0, 2.0, 2.0, 1.0])[:, None] * np.array([1.0, 2.0])[None, :]
    V = cm[:, None] * beta[None, :] - 2.0 * cv[:, None] * U
    sd = X - Z.T
    assert np.all(np.sign(V) == np.sign(sd)) and set(np.abs(V).ravel()) <= {2.0, 4.0, 8.0}
    return X, Z, U, cm, cv, beta, V, sd


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_exact_operands_where_only_the_profile_rounds(kind, dtype):
    """Every term of a row has the same sign, so a relative error common to every f' shows in full: bound 8 u sum|terms| (the
    count of the profile's roundings in tests/test_gpu_kgrad.py: at most 6.6 u per term)."""
    Xh, Zh, Uh, cmh, cvh, betah, V, sd = _exact_problem()
    N, M = sd.shape
    _, df = R.profile_grad(kind, sd * sd)
    terms = 2.0 * V * df * sd
    assert np.all(terms < 0)
    u, tag = UNIT[dtype], DTYPE_IDS[DTYPES.index(dtype)]
    dX = _call(dtype, kind, _dev(Xh, dtype), _dev(Zh, dtype), _dev(np.ones(1), dtype), 1.0, _u_rows(Uh, dtype, 128), _dev(cmh, dtype),
               _dev(cvh, dtype), _dev(betah, dtype), 1, N, M, 1, _fresh(N, 1))
    ref, A = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    ratio = float(np.max(np.abs(_host(dX[:N, 0]) - ref) / (u * A)))
    print(f"exact operands {kind} {tag}: |got - ref| / (u sum|terms|) = {ratio:.3f}")
    _note("exact", dtype, kind, ratio)
    assert ratio <= EXACT_C, f"{kind} {tag}: {ratio:.3f} u"


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_engine_methods_against_the_reference(dtype):
    """``EStepEngine.moments_vjp`` (the engine's layout, accumulate) and ``predict_vjp`` (fill, GEMM, one launch per latent, shared
    and per-latent kernels) against the restatement with K and U formed in fp64: fp64 relerr <= 1e-8, fp32 atol 1e-4 + rtol 1e-3
    max|ref|."""
    from importlib import import_module

    p = pkg()
    eng = import_module("t-svgp_amd.estep").EStepEngine(dtype, DEV)
    N, M, D, P = 300, 150, 5, 2
    rng = np.random.RandomState(9)
    Xh, Zh = rng.randn(N, D), rng.randn(M, D)
    Zh[:8] = Xh[:8]
    beta, cm, cv = rng.randn(M, P), rng.randn(N, P), rng.randn(N, P)
    Rm = rng.randn(P, M, M) / M
    Q = Rm @ Rm.transpose(0, 2, 1)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64, device=DEV)

    def close(got, ref, what):
        got = _host(got)
        if dtype == torch.float64:
            e = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
            print(f"{what} fp64 relerr {e:.3e}")
            assert e <= 1e-8, f"{what}: relerr {e:.3e}"
        else:
            e, bound = float(np.max(np.abs(got - ref))), 1e-4 + 1e-3 * float(np.max(np.abs(ref)))
            print(f"{what} fp32 max abs err {e:.3e} (bound {bound:.3e})")
            assert e <= bound, f"{what}: {e:.3e} > {bound:.3e}"

    for name, kinds in (("shared", ["matern52"]), ("separate", ["se", "matern32"])):
        cls = {"se": p.SquaredExponential, "matern32": p.Matern32, "matern52": p.Matern52}
        ks = [cls[k](VARIANCE + 0.2 * i, (0.9 + 0.3 * i) * np.sqrt(D) * (1.0 + 0.1 * np.arange(D))) for i, k in enumerate(kinds)]
        kernel = ks[0] if len(ks) == 1 else p.SeparateIndependent(ks)
        ref = np.zeros((N, D))
        for q in range(P):
            k = ks[q if len(ks) > 1 else 0]
            il = 1.0 / k.lengthscales.numpy()
            g, _ = R.predict_vjp(kinds[q if len(ks) > 1 else 0], Xh, Zh, il, k.variance.item(), beta[:, q:q + 1], Q[q:q + 1], cm[:, q:q + 1],
                                 cv[:, q:q + 1])
            ref += g
        got = eng.predict_vjp(t64(Xh), t64(Zh), kernel, t64(beta), t64(Q), t64(cm), t64(cv))
        assert got.dtype == torch.float64 and tuple(got.shape) == (N, D)
        close(got, ref, f"predict_vjp {name}")
        assert torch.equal(got, eng.predict_vjp(t64(Xh), t64(Zh), list(ks), t64(beta), t64(Q), t64(cm), t64(cv)))  # a list of kernels
    # mean alone
    k0 = p.SquaredExponential(VARIANCE, np.sqrt(D))
    ref0, _ = R.predict_vjp("se", Xh, Zh, np.full(D, 1.0 / np.sqrt(D)), VARIANCE, beta, Q, cm, np.zeros_like(cv))
    close(eng.predict_vjp(t64(Xh), t64(Zh), k0, t64(beta), t64(Q), t64(cm)), ref0, "predict_vjp mean alone")
    with pytest.raises(ValueError, match="32"):
        eng.predict_vjp(torch.zeros((4, 33), device=DEV), torch.zeros((3, 33), device=DEV), k0, torch.zeros((3, 1)), torch.zeros((1, 3, 3)),
                        torch.zeros((4, 1)))
