"""The many-latent (P > 8) kernel paths against NumPy fp64, entry by entry through the C ABI.

Softmax(C) and MultiClass(C) run with P = C = 10 latents (up to TSVGP_MAX_BATCH = 32).  Above eight latents ``site_accum()`` leaves
syrk1_kernel (fp64) / syrk1f_kernel (fp32) for the generic ``syrk_kernel<T>`` (16-row chunks in both types, its own staging and
ring); the latent-batched entries (``tsvgp_*_batched_*``, the SeparateIndependent path) loop or grid over P.  Every case here calls
the entry directly on device operands and compares with NumPy fp64 computed from those operands cast to fp64, so an fp32 case
measures the kernel and not the rounding of its inputs.

Tolerances are those of tests/test_gpu_kernels.py: ``tol`` = 1e-11 (fp64) / 2e-5 (fp32), times 10 for the fill, 20 for trmm and the
moments, 50 for the site sums; likelihood gradients rtol = atol = 1e-10 (fp64) / 1e-5 (fp32).

Strided operands and outputs live in NaN-filled buffers with a gap behind every latent's slice: a read past a slice poisons the
result, a write past it destroys a NaN; both are asserted.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests.helpers import pkg, relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [(torch.float64, 1e-11), (torch.float32, 2e-5)]
NAN = float("nan")
KDIAG = 2.5


@pytest.fixture(scope="module")
def engines():
    from importlib import import_module

    estep = import_module("t-svgp_amd.estep")
    return {dt: estep.EStepEngine(dt, DEV) for dt, _ in DTYPES}


@pytest.fixture(scope="module")
def cache():
    """Operands and references shared between the cases of this module (freed with it)."""
    store = {}
    yield store
    store.clear()


def _cached(cache, key, make):
    if key not in cache:
        cache[key] = make()
    return cache[key]


def _t(a, dtype):
    return torch.as_tensor(a, dtype=dtype, device=DEV).contiguous()


def _h(x):
    """A device tensor as the fp64 NumPy array of the values the kernel reads."""
    return x.double().cpu().numpy()


def _gapped(src, gap):
    """src [P, ...] -> (flat NaN-filled buffer holding slice p at p * stride, stride); ``gap`` NaN elements follow every slice."""
    P, n = src.shape[0], src[0].numel()
    stride = n + gap
    flat = torch.full((P * stride,), NAN, dtype=src.dtype, device=DEV)
    flat.view(P, stride)[:, :n] = src.reshape(P, n)
    return flat, stride


def _slices(flat, P, stride, shape):
    """(the P slices [P, *shape] as a copy, the gap elements [P, gap])."""
    n = int(np.prod(shape))
    v = flat[:P * stride].view(P, stride)
    return v[:, :n].reshape((P,) + tuple(shape)).clone(), v[:, n:]


def _tri(x, mode):
    return torch.tril(x) if mode == 0 else torch.triu(x) if mode == 1 else x


def _randn(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


# ---------------------------------------------------------------------------------------------------------------------
# 1. site sums above eight latents: syrk_kernel<T>
# ---------------------------------------------------------------------------------------------------------------------
def _site_inputs(Np, Mp, P, dtype, seed=4):
    rng = np.random.RandomState(seed)
    Bm = rng.randn(Np, Mp)
    g0 = rng.randn(Np, P)
    g1 = -rng.rand(Np, P) - 0.1
    g0[-5:] = 0
    g1[-5:] = 0
    return _t(Bm, dtype), _t(g0, dtype), _t(g1, dtype)


def _site_ref(Bd, g0d, g1d):
    """acc2[l] = sum_n g1[n, l] b_n b_n^T, acc1[l] = sum_n g0[n, l] b_n (the einsums of test_site_accum as matrix products);
    Bd [Np, Mp] shared or [P, Np, Mp] per latent."""
    P = g0d.shape[1]
    per = (lambda p: Bd[p]) if Bd.ndim == 3 else (lambda p: Bd)
    ref2 = np.stack([(per(p) * g1d[:, p:p + 1]).T @ per(p) for p in range(P)])
    ref1 = np.stack([g0d[:, p] @ per(p) for p in range(P)])
    return ref2, ref1


def _site_call(eng, Bt, g0t, g1t, Np, Mp, P, nsplit, strideB=None):
    """One launch on NaN-filled outputs.  strideB None: tsvgp_site_accum_*; else the batched entry."""
    B = pkg()._backend
    nbytes = int(eng._fn("tsvgp_site_accum_work_bytes")(Mp, P, nsplit))
    assert nbytes > 0
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    acc2 = torch.full((P, Mp, Mp), NAN, dtype=torch.float64, device=DEV)
    acc1 = torch.full((P, Mp), NAN, dtype=torch.float64, device=DEV)
    if strideB is None:
        st = eng._fn("tsvgp_site_accum")(Bt.data_ptr(), g0t.data_ptr(), g1t.data_ptr(), acc2.data_ptr(), acc1.data_ptr(),
                                         work.data_ptr(), Np, Mp, P, nsplit, eng._stream())
    else:
        st = eng._fn("tsvgp_site_accum_batched")(Bt.data_ptr(), strideB, g0t.data_ptr(), g1t.data_ptr(), acc2.data_ptr(),
                                                 acc1.data_ptr(), work.data_ptr(), Np, Mp, P, nsplit, eng._stream())
    B.check(st, "site_accum")
    torch.cuda.synchronize()
    return acc2, acc1


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("Np,Mp,P,nsplit", [(128, 128, 9, 1),  # one tile, no off-diagonal work, one slice of 8 chunks
                                            (2048, 128, 16, 1),  # 128 chunks in one slice: the ring runs long
                                            (640, 384, 10, 3),  # three tiles, 40 chunks over 3 slices: uneven, the last one short
                                            (1152, 1024, 10, 5),  # the 36 lower tiles of the multiclass shape, 72 chunks over 5 slices
                                            (256, 256, 32, 2),  # TSVGP_MAX_BATCH
                                            (384, 256, 9, 7)])  # an odd chunk count per slice: the single-step tail of the paired loop
def test_site_accum_above_eight_latents(engines, dtype, tol, Np, Mp, P, nsplit):
    eng = engines[dtype]
    assert P > 8  # syrk_kernel<T>, not syrk1_kernel / syrk1f_kernel
    Bt, g0t, g1t = _site_inputs(Np, Mp, P, dtype)
    acc2, acc1 = _site_call(eng, Bt, g0t, g1t, Np, Mp, P, nsplit)
    ref2, ref1 = _site_ref(_h(Bt), _h(g0t), _h(g1t))
    a2 = acc2.cpu().numpy()
    e2, e1 = relerr(a2, ref2), relerr(acc1.cpu().numpy(), ref1)
    print(f"site_accum {dtype} Np={Np} Mp={Mp} P={P} nsplit={nsplit}: acc2 {e2:.2e} acc1 {e1:.2e} (bound {tol * 50:.1e})")
    assert np.isfinite(a2).all()
    assert e2 < tol * 50
    assert e1 < tol * 50
    # every latent on its own, so that a small latent cannot hide behind a large one
    for p in range(P):
        assert relerr(a2[p], ref2[p]) < tol * 50, p
    assert np.array_equal(a2, np.swapaxes(a2, -1, -2))  # exactly symmetric
    acc2b, acc1b = _site_call(eng, Bt, g0t, g1t, Np, Mp, P, nsplit)  # fixed-order reduction: bitwise reproducible
    assert torch.equal(acc2, acc2b) and torch.equal(acc1, acc1b)


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_site_accum_across_the_kernel_switch(engines, dtype, tol):
    """P = 9 (syrk_kernel<T>) and P = 8 on the first eight columns of the same weights (syrk1_kernel / syrk1f_kernel): latents
    0-7 of both runs against the reference under the rule, and against each other within twice the rule (two kernels, two
    summation orders, each within the rule of the same reference)."""
    eng = engines[dtype]
    Np, Mp, nsplit = 384, 256, 3
    Bt, g0t, g1t = _site_inputs(Np, Mp, 9, dtype, seed=9)
    g0e, g1e = g0t[:, :8].contiguous(), g1t[:, :8].contiguous()
    a9, b9 = _site_call(eng, Bt, g0t, g1t, Np, Mp, 9, nsplit)
    a8, b8 = _site_call(eng, Bt, g0e, g1e, Np, Mp, 8, nsplit)
    ref2, ref1 = _site_ref(_h(Bt), _h(g0t), _h(g1t))
    a9, b9, a8, b8 = (x.cpu().numpy() for x in (a9, b9, a8, b8))
    assert relerr(a9, ref2) < tol * 50 and relerr(b9, ref1) < tol * 50
    assert relerr(a8, ref2[:8]) < tol * 50 and relerr(b8, ref1[:8]) < tol * 50
    for p in range(8):
        assert relerr(a9[p], ref2[p]) < tol * 50 and relerr(a8[p], ref2[p]) < tol * 50, p
        assert relerr(a9[p], a8[p]) < 2 * tol * 50 and relerr(b9[p], b8[p]) < 2 * tol * 50, p


# ---------------------------------------------------------------------------------------------------------------------
# 2. tsvgp_site_accum_batched_*: one operand per latent
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("Mp", [128, 384])
@pytest.mark.parametrize("P", [2, 8, 9, 10])
def test_site_accum_batched(engines, dtype, tol, P, Mp):
    eng = engines[dtype]
    Np, nsplit = 384, 3
    rng = np.random.RandomState(21)
    Bsrc = _t(rng.randn(P, Np, Mp), dtype)
    g0 = rng.randn(Np, P)
    g1 = -rng.rand(Np, P) - 0.1
    g0[-5:] = 0
    g1[-5:] = 0
    g0t, g1t = _t(g0, dtype), _t(g1, dtype)
    flat, strideB = _gapped(Bsrc, 2 * Mp)
    assert strideB == Np * Mp + 2 * Mp
    acc2, acc1 = _site_call(eng, flat, g0t, g1t, Np, Mp, P, nsplit, strideB=strideB)
    ref2, ref1 = _site_ref(_h(Bsrc), _h(g0t), _h(g1t))
    a2, a1 = acc2.cpu().numpy(), acc1.cpu().numpy()
    assert np.isfinite(a2).all() and np.isfinite(a1).all()  # nothing was read from a gap
    for p in range(P):
        assert relerr(a2[p], ref2[p]) < tol * 50 and relerr(a1[p], ref1[p]) < tol * 50, p
    assert np.array_equal(a2, np.swapaxes(a2, -1, -2))
    # strideB = 0 through the batched entry is tsvgp_site_accum_*: bit for bit
    s2, s1 = _site_call(eng, Bsrc[0], g0t, g1t, Np, Mp, P, nsplit, strideB=0)
    u2, u1 = _site_call(eng, Bsrc[0], g0t, g1t, Np, Mp, P, nsplit)
    assert torch.equal(s2, u2) and torch.equal(s1, u1)
    r2, r1 = _site_ref(_h(Bsrc[0]), _h(g0t), _h(g1t))
    assert relerr(s2.cpu().numpy(), r2) < tol * 50 and relerr(s1.cpu().numpy(), r1) < tol * 50
    # a stride that takes latent 1 off the 16-byte boundary is an invalid argument
    work = torch.empty(int(eng._fn("tsvgp_site_accum_work_bytes")(Mp, P, nsplit)), dtype=torch.uint8, device=DEV)
    assert eng._fn("tsvgp_site_accum_batched")(flat.data_ptr(), Np * Mp + 1, g0t.data_ptr(), g1t.data_ptr(), acc2.data_ptr(),
                                               acc1.data_ptr(), work.data_ptr(), Np, Mp, P, nsplit, eng._stream()) == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 3. tsvgp_moments_* with one shared operand, P up to 33
# ---------------------------------------------------------------------------------------------------------------------
PMAX_SHARED = 33
LIK_IDS = {"none": 0, "gaussian": 1, "bernoulli": 2}


def _shared_base(cache, dtype, M):
    """Tm [33, M, M] dense with entries N(0, 1 / M) (so q = |Tm a|^2 ~ |a|^2 ~ 1 < kdiag), gamma [M, 33]: on the device."""
    def make():
        return _t(_randn((PMAX_SHARED, M, M), 30 + M, 1.0 / np.sqrt(M)), dtype), _t(_randn((M, PMAX_SHARED), 31 + M), dtype)
    return _cached(cache, ("shared_base", dtype, M), make)


def _shared_rows(cache, dtype, N, M):
    def make():
        Np = pkg()._backend.round_up(N)
        A = torch.zeros((Np, M), dtype=torch.float64)
        A[:N] = _randn((N, M), 32 + N + M, 1.0 / np.sqrt(M))
        Yg = _randn((N, PMAX_SHARED), 33 + N)
        Yb = (_randn((N, PMAX_SHARED), 34 + N) > 0).to(torch.float64)
        return _t(A, dtype), {"none": _t(Yg, dtype), "gaussian": _t(Yg, dtype), "bernoulli": _t(Yb, dtype)}
    return _cached(cache, ("shared_rows", dtype, N, M), make)


def _shared_ref(cache, dtype, N, M, mode):
    """(mean, var) [N, 33] in NumPy fp64 from the device operands, once per (type, shape, triangle)."""
    def make():
        Tm, gamma = _shared_base(cache, dtype, M)
        A, _ = _shared_rows(cache, dtype, N, M)
        Ah, Th = _h(A)[:N], _h(_tri(Tm, mode))
        q = np.stack([np.sum((Ah @ Th[p].T) ** 2, axis=-1) for p in range(PMAX_SHARED)], axis=1)
        mref, vref = Ah @ _h(gamma), KDIAG - q
        mref.setflags(write=False)
        vref.setflags(write=False)
        return mref, vref
    return _cached(cache, ("shared_ref", dtype, N, M, mode), make)


def _check_lik_outputs(lik, dtype, N, mean, var, g0, g1, vep, Yh):
    """g0 / g1 / ve against the oracle's likelihood at the kernel's own moments, as test_moments_and_likelihood_map.

    The ve sum is held to 1e-9 relative, as there.  (In that test the check never runs at these sizes: its Tm makes most variances
    negative.)  The kernel evaluates ve at its fp64 (mean, var) BEFORE it rounds them to the array type for output, the oracle
    here sees the rounded outputs; in fp64 they are the same numbers, in fp32 each differs by up to u = 2^-24 relative, which moves
    the sum by at most sum_rows (|d ve / d mean| |mean| + |d ve / d var| |var|) u to first order -- that term, from the oracle's
    own derivatives, is added to the fp32 bound (P = 9, N = 129, M = 128, lower form, Bernoulli: 2.4e-5 measured, 7.6e-5 allowed by that term, 1.7e-6 by the 1e-9 alone)."""
    mu_k, var_k = _h(mean), _h(var)
    olik = O.Gaussian(variance=0.3) if lik == "gaussian" else O.Bernoulli()
    r0, r1 = olik.variational_expectations_grads(mu_k, var_k, Yh)
    ve_round = 0.0 if dtype == torch.float64 else 2.0 ** -24 * float(np.sum(np.abs(r0 * mu_k) + np.abs(r1 * var_k)))
    r1 = np.minimum(r1, -1e-8)
    k0, k1 = _h(g0), _h(g1)
    ltol = 1e-10 if dtype == torch.float64 else 1e-5
    np.testing.assert_allclose(k0[:N], r0, rtol=ltol, atol=ltol)
    np.testing.assert_allclose(k1[:N], r1, rtol=ltol, atol=ltol)
    assert np.all(k0[N:] == 0) and np.all(k1[N:] == 0)
    ve_ref = np.sum(olik.variational_expectations(mu_k, var_k, Yh))
    err_ve, tol_ve = abs(float(vep.sum()) - ve_ref), 1e-9 * max(1.0, abs(ve_ref)) + ve_round
    assert err_ve < tol_ve, (err_ve, tol_ve)


def _moment_outputs(dtype, N, Np, P):
    return dict(mean=torch.full((N, P), NAN, dtype=dtype, device=DEV), var=torch.full((N, P), NAN, dtype=dtype, device=DEV),
                g0=torch.full((Np, P), NAN, dtype=dtype, device=DEV), g1=torch.full((Np, P), NAN, dtype=dtype, device=DEV),
                vep=torch.zeros(Np // 128, dtype=torch.float64, device=DEV), npp=torch.zeros(Np // 128, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("lik", ["none", "gaussian", "bernoulli"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("N,M", [(129, 128), (300, 384), (150, 1024)])
@pytest.mark.parametrize("P", [9, 10, 32, 33])  # 33: legal with a uniform kdiag (beyond TSVGP_MAX_BATCH)
def test_moments_shared_operand(engines, cache, dtype, tol, lik, mode, N, M, P):
    eng = engines[dtype]
    B = pkg()._backend
    Np = B.round_up(N)
    Tm33, gamma33 = _shared_base(cache, dtype, M)
    A, Ys = _shared_rows(cache, dtype, N, M)
    mref, vref = (r[:, :P] for r in _shared_ref(cache, dtype, N, M, mode))
    assert vref.min() >= 0.1 * KDIAG  # every row goes through the likelihood map, none is masked out
    Tm = _tri(Tm33[:P], mode).contiguous()
    gamma, Y = gamma33[:, :P].contiguous(), Ys[lik][:, :P].contiguous()
    o = _moment_outputs(dtype, N, Np, P)
    B.check(eng._fn("tsvgp_moments")(A.data_ptr(), Tm.data_ptr(), gamma.data_ptr(), Y.data_ptr(), KDIAG, LIK_IDS[lik], 0.3,
                                     o["mean"].data_ptr(), o["var"].data_ptr(), o["g0"].data_ptr(), o["g1"].data_ptr(),
                                     o["vep"].data_ptr(), o["npp"].data_ptr(), N, Np, M, P, mode, eng._stream()), "moments")
    torch.cuda.synchronize()
    assert relerr(o["mean"].cpu().numpy(), mref) < tol * 20
    assert np.max(np.abs(_h(o["var"]) - vref)) < tol * 20 * KDIAG
    assert int(o["npp"].sum()) == 0
    if lik != "none":
        _check_lik_outputs(lik, dtype, N, o["mean"], o["var"], o["g0"], o["g1"], o["vep"], _h(Y))


@pytest.mark.parametrize("dtype,P,accepted", [(torch.float64, 16, True), (torch.float64, 17, False), (torch.float32, 32, True)])
def test_moments_mean_only_at_the_lds_limit(engines, cache, dtype, P, accepted):
    """TSVGP_LIK_MEANONLY keeps gamma [P][Mp] in LDS: Mp P sizeof(T) <= 128 KiB.  At Mp = 1024 that is P = 16 in fp64 (exactly
    128 KiB) and P = 32 in fp32; fp64 P = 17 is refused."""
    eng = engines[dtype]
    B = pkg()._backend
    tol = dict(DTYPES)[dtype]
    N, M = 150, 1024
    Np = B.round_up(N)
    _, gamma33 = _shared_base(cache, dtype, M)
    A, Ys = _shared_rows(cache, dtype, N, M)
    gamma, Y = gamma33[:, :P].contiguous(), Ys["gaussian"][:, :P].contiguous()
    o = _moment_outputs(dtype, N, Np, P)
    st = eng._fn("tsvgp_moments")(A.data_ptr(), None, gamma.data_ptr(), Y.data_ptr(), KDIAG, B.LIK_GAUSSIAN | B.LIK_MEANONLY, 0.3,
                                  o["mean"].data_ptr(), None, o["g0"].data_ptr(), o["g1"].data_ptr(), o["vep"].data_ptr(),
                                  o["npp"].data_ptr(), N, Np, M, P, 1, eng._stream())
    torch.cuda.synchronize()
    assert (M * P * A.element_size() <= 128 * 1024) == accepted
    if not accepted:
        assert st == 1
        return
    B.check(st, "moments (mean only)")
    mref = _h(A)[:N] @ _h(gamma)
    assert relerr(o["mean"].cpu().numpy(), mref) < tol * 20
    assert int(o["npp"].sum()) == 0 and torch.isnan(o["vep"]).all()
    mu = _h(o["mean"])
    ltol = 1e-12 if dtype == torch.float64 else 1e-5
    np.testing.assert_allclose(_h(o["g0"])[:N], (_h(Y) - mu) / 0.3, rtol=ltol, atol=ltol)
    np.testing.assert_allclose(_h(o["g1"])[:N], -0.5 / 0.3, rtol=ltol)
    assert np.all(_h(o["g0"])[N:] == 0) and np.all(_h(o["g1"])[N:] == 0)


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_moments_batched_rejects_more_than_max_batch(engines, cache, dtype, tol):
    """P = 33 is legal in tsvgp_moments_* (one kdiag for all) and an invalid argument in the batched entry (one per latent)."""
    eng = engines[dtype]
    B = pkg()._backend
    N, M, P = 129, 128, 33
    assert P == B.MAX_BATCH + 1
    Np = B.round_up(N)
    Tm33, gamma33 = _shared_base(cache, dtype, M)
    A, Ys = _shared_rows(cache, dtype, N, M)
    o = _moment_outputs(dtype, N, Np, P)
    held = {nlat: (gamma33[:, :nlat].contiguous(), Ys["gaussian"][:, :nlat].contiguous()) for nlat in (32, 33)}
    call = lambda nlat: eng._fn("tsvgp_moments_batched")(
        A.data_ptr(), 0, Tm33.data_ptr(), held[nlat][0].data_ptr(), held[nlat][1].data_ptr(),
        (ctypes.c_double * P)(*([KDIAG] * P)), B.LIK_GAUSSIAN, 0.3, o["mean"].data_ptr(), o["var"].data_ptr(), o["g0"].data_ptr(),
        o["g1"].data_ptr(), o["vep"].data_ptr(), o["npp"].data_ptr(), N, Np, M, nlat, 2, eng._stream())
    assert call(33) == 1
    assert call(32) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 4. tsvgp_moments_batched_*: one operand and one prior variance per latent
# ---------------------------------------------------------------------------------------------------------------------
PMAX_BATCHED = 32
KD = [2.0 + 0.05 * p for p in range(PMAX_BATCHED)]  # all different


def _batched_problem(cache, dtype, N, Mp, mode):
    def make():
        Np = pkg()._backend.round_up(N)
        A = torch.zeros((PMAX_BATCHED, Np, Mp), dtype=torch.float64)
        A[:, :N] = _randn((PMAX_BATCHED, N, Mp), 40 + N + Mp, 1.0 / np.sqrt(Mp))
        Asrc = _t(A, dtype)
        Tm = _tri(_t(_randn((PMAX_BATCHED, Mp, Mp), 41 + Mp, 0.8 / np.sqrt(Mp)), dtype), mode).contiguous()  # q ~ 0.64 |a|^2 < kd
        gamma = _t(_randn((Mp, PMAX_BATCHED), 42 + Mp), dtype)
        Yg = _t(_randn((N, PMAX_BATCHED), 43 + N), dtype)
        Yb = _t((_randn((N, PMAX_BATCHED), 44 + N) > 0).to(torch.float64), dtype)
        flat, stride = _gapped(Asrc, 2 * Mp)
        Ah, Th = _h(Asrc)[:, :N], _h(Tm)
        q = np.stack([np.sum((Ah[p] @ Th[p].T) ** 2, axis=-1) for p in range(PMAX_BATCHED)], axis=1)
        vref = np.asarray(KD)[None, :] - q
        mref = np.einsum("pnj,jp->np", Ah, _h(gamma))
        return dict(flat=flat, stride=stride, Asrc=Asrc, Tm=Tm, gamma=gamma, Y={"gaussian": Yg, "bernoulli": Yb}, mref=mref, vref=vref)
    return _cached(cache, ("batched", dtype, N, Mp, mode), make)


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("lik", ["gaussian", "bernoulli"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("N", [129, 333])
@pytest.mark.parametrize("Mp", [128, 384])
@pytest.mark.parametrize("P", [2, 9, 10, 32])
def test_moments_batched(engines, cache, dtype, tol, lik, mode, N, Mp, P):
    eng = engines[dtype]
    B = pkg()._backend
    Np = B.round_up(N)
    w = _batched_problem(cache, dtype, N, Mp, mode)
    mref, vref, kd = w["mref"][:, :P], w["vref"][:, :P], KD[:P]
    assert np.all(vref >= 0.1 * np.asarray(kd)[None, :])  # every row goes through the likelihood map
    assert w["stride"] == Np * Mp + 2 * Mp
    Tm, gamma, Y = w["Tm"][:P], w["gamma"][:, :P].contiguous(), w["Y"][lik][:, :P].contiguous()
    o = _moment_outputs(dtype, N, Np, P)
    B.check(eng._fn("tsvgp_moments_batched")(w["flat"].data_ptr(), w["stride"], Tm.data_ptr(), gamma.data_ptr(), Y.data_ptr(),
                                             (ctypes.c_double * P)(*kd), LIK_IDS[lik], 0.3, o["mean"].data_ptr(), o["var"].data_ptr(),
                                             o["g0"].data_ptr(), o["g1"].data_ptr(), o["vep"].data_ptr(), o["npp"].data_ptr(), N, Np, Mp, P,
                                             mode, eng._stream()), "moments batched")
    torch.cuda.synchronize()
    mean, var = o["mean"].cpu().numpy(), _h(o["var"])
    assert np.isfinite(mean).all() and np.isfinite(var).all()  # nothing was read from a gap
    assert relerr(mean, mref) < tol * 20
    assert np.max(np.abs(var - vref)) < tol * 20 * max(kd)
    for p in range(P):  # each latent on its own operand and its own prior variance
        assert relerr(mean[:, p], mref[:, p]) < tol * 20 and np.max(np.abs(var[:, p] - vref[:, p])) < tol * 20 * kd[p], p
    assert int(o["npp"].sum()) == 0
    _check_lik_outputs(lik, dtype, N, o["mean"], o["var"], o["g0"], o["g1"], o["vep"], _h(Y))


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_moments_batched_shared_operand_is_the_unbatched_entry(engines, cache, dtype, tol, mode):
    """strideA = 0 with one prior variance for all: bit for bit what tsvgp_moments_* gives."""
    eng = engines[dtype]
    B = pkg()._backend
    N, Mp, P = 333, 384, 10
    Np = B.round_up(N)
    w = _batched_problem(cache, dtype, N, Mp, mode)
    A = w["Asrc"][3]
    Tm, gamma, Y = w["Tm"][:P], w["gamma"][:, :P].contiguous(), w["Y"]["gaussian"][:, :P].contiguous()
    ob, ou = _moment_outputs(dtype, N, Np, P), _moment_outputs(dtype, N, Np, P)
    tail = lambda o: (B.LIK_GAUSSIAN, 0.3, o["mean"].data_ptr(), o["var"].data_ptr(), o["g0"].data_ptr(), o["g1"].data_ptr(),
                      o["vep"].data_ptr(), o["npp"].data_ptr(), N, Np, Mp, P, mode, eng._stream())
    B.check(eng._fn("tsvgp_moments_batched")(A.data_ptr(), 0, Tm.data_ptr(), gamma.data_ptr(), Y.data_ptr(),
                                             (ctypes.c_double * P)(*([KDIAG] * P)), *tail(ob)), "moments batched")
    B.check(eng._fn("tsvgp_moments")(A.data_ptr(), Tm.data_ptr(), gamma.data_ptr(), Y.data_ptr(), KDIAG, *tail(ou)), "moments")
    torch.cuda.synchronize()
    for k in ob:
        assert torch.equal(ob[k], ou[k]), k
    assert torch.isfinite(ob["mean"]).all() and torch.isfinite(ob["g1"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. tsvgp_kernel_fill_batched_*
# ---------------------------------------------------------------------------------------------------------------------
KINDS = [("SquaredExponential", 0), ("Matern32", 2), ("Matern52", 3)]


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("name,kind", KINDS)
@pytest.mark.parametrize("D", [1, 8, 19, 32])  # padded to 1, 8, 32, 32; with 2, 4, 16 below
@pytest.mark.parametrize("P", [1, 10, 32])
@pytest.mark.parametrize("N,M", [(129, 513), (64, 1024), (300, 200)])  # M = 513 crosses the 512-column fill tile
def test_kernel_fill_batched_many_latents(engines, dtype, tol, name, kind, D, P, N, M):
    _fill_case(engines[dtype], dtype, tol, name, kind, D, P, N, M)


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("name,kind", KINDS)
@pytest.mark.parametrize("D", [2, 3, 16])  # the compile-time paddings 2, 4 and 16 that D = 1, 8, 19, 32 leave out
def test_kernel_fill_batched_remaining_paddings(engines, dtype, tol, name, kind, D):
    _fill_case(engines[dtype], dtype, tol, name, kind, D, 10, 129, 513)


def _fill_case(eng, dtype, tol, name, kind, D, P, N, M):
    B = pkg()._backend
    rng = np.random.RandomState(50 + D + P)
    X, Z = rng.randn(N, D) / np.sqrt(D), rng.randn(M, D) / np.sqrt(D)  # r^2 of order one at every D
    Z[:4] = X[:4]  # r = 0 entries in every latent
    ls = 0.7 + rng.rand(P, D)
    var = [0.5 + 0.07 * p for p in range(P)]
    Np, Mp = B.round_up(N), B.round_up(M)
    Xt, Zt, il = _t(X, dtype), _t(Z, dtype), _t(1.0 / ls, dtype)
    stride = Np * Mp + 2 * Mp
    flat = torch.full((P * stride,), NAN, dtype=dtype, device=DEV)
    ctype = ctypes.c_double if dtype == torch.float64 else ctypes.c_float
    B.check(eng._fn("tsvgp_kernel_fill_batched")(kind, Xt.data_ptr(), Zt.data_ptr(), il.data_ptr(), (ctype * P)(*var), flat.data_ptr(),
                                                 stride, N, M, D, Mp, P, eng._stream()), "fill batched")
    torch.cuda.synchronize()
    Kt, gaps = _slices(flat, P, stride, (Np, Mp))
    assert torch.isnan(gaps).all()  # nothing was written behind a latent's slice
    K = _h(Kt)
    assert np.isfinite(K).all()
    Xh, Zh, lsh = _h(Xt), _h(Zt), 1.0 / _h(il)
    for p in range(P):
        var_p = float(ctype(var[p]).value)  # the scalar as the kernel receives it
        ref = getattr(O, name)(variance=var_p, lengthscales=lsh[p]).K(Xh, Zh)
        assert relerr(K[p, :N, :M], ref) < tol * 10, p
        assert np.all(K[p, N:, :] == 0) and np.all(K[p, :, M:] == 0), p  # the padding inside a slice is exactly zero
        assert abs(K[p, 0, 0] - var_p) <= tol * 10 * var_p  # r = 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. tsvgp_trmm_batched_*
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("Np,Mp,P", [(128, 128, 10), (256, 640, 9), (128, 1024, 10)])
def test_trmm_batched_many_latents(engines, dtype, tol, mode, Np, Mp, P):
    eng = engines[dtype]
    B = pkg()._backend
    fn = eng._fn("tsvgp_trmm_batched")
    Asrc = _t(_randn((P, Np, Mp), 60 + Mp), dtype)
    Tt = _tri(_t(_randn((P, Mp, Mp), 61 + Mp), dtype), mode).contiguous()  # zero outside the intended triangle
    Ah, Th = _h(Asrc), _h(Tt)
    ref = np.stack([Ah[p] @ Th[p].T for p in range(P)])
    Aflat, strideA = _gapped(Asrc, 2 * Mp)
    strideC = Np * Mp + 4 * Mp  # another gap than A's
    Cflat = torch.full((P * strideC,), NAN, dtype=dtype, device=DEV)
    B.check(fn(Aflat.data_ptr(), strideA, Tt.data_ptr(), Mp * Mp, Cflat.data_ptr(), strideC, Np, Mp, mode, P, eng._stream()), "trmm")
    torch.cuda.synchronize()
    C, gaps = _slices(Cflat, P, strideC, (Np, Mp))
    assert torch.isnan(gaps).all() and torch.isfinite(C).all()
    Ch = C.cpu().numpy()
    for p in range(P):
        assert relerr(Ch[p], ref[p]) < tol * 20, p
    # one shared operand for all latents
    Cflat.fill_(NAN)
    B.check(fn(Asrc[P - 1].data_ptr(), 0, Tt.data_ptr(), Mp * Mp, Cflat.data_ptr(), strideC, Np, Mp, mode, P, eng._stream()), "trmm")
    torch.cuda.synchronize()
    C2, gaps = _slices(Cflat, P, strideC, (Np, Mp))
    assert torch.isnan(gaps).all() and torch.isfinite(C2).all()
    C2h = C2.cpu().numpy()
    for p in range(P):
        assert relerr(C2h[p], Ah[P - 1] @ Th[p].T) < tol * 20, p
    # the in-place upper form
    if mode == 1 and P == 10:
        B.check(fn(Aflat.data_ptr(), strideA, Tt.data_ptr(), Mp * Mp, Aflat.data_ptr(), strideA, Np, Mp, mode, P, eng._stream()), "trmm")
        torch.cuda.synchronize()
        C3, gaps = _slices(Aflat, P, strideA, (Np, Mp))
        assert torch.isnan(gaps).all() and torch.isfinite(C3).all()
        C3h = C3.cpu().numpy()
        for p in range(P):
            assert relerr(C3h[p], ref[p]) < tol * 20, p
    elif mode != 1:  # refused for the lower and dense forms
        assert fn(Aflat.data_ptr(), strideA, Tt.data_ptr(), Mp * Mp, Aflat.data_ptr(), strideA, Np, Mp, mode, P, eng._stream()) == 1


# ---------------------------------------------------------------------------------------------------------------------
# 7. M x M helpers no test named: tsvgp_sym_pack_f64, tsvgp_sym_unpack_f64, tsvgp_step_status_f64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3, 10])
@pytest.mark.parametrize("M", [1, 33, 200, 1024])
def test_sym_pack_and_unpack(engines, M, P):
    """The packed lower triangles against the index gather acc2[:, i, j] over tril_indices (what distributed.pack_stats does
    without an engine), from a source with lda > M and a matrix stride beyond lda * M; the unpack mirrors them back."""
    eng = engines[torch.float64]
    lib = eng.lib
    lda, tri = M + 3, M * (M + 1) // 2
    stride = lda * M + 5
    src = torch.full((P * stride,), NAN, dtype=torch.float64, device=DEV)
    view = src.view(P, stride)[:, :lda * M].view(P, M, lda)[:, :, :M]
    view[:] = _t(_randn((P, M, M), 70 + M), torch.float64)  # not symmetric: the pack reads the lower triangle only
    acc2 = view.clone()
    packed = torch.full((P * tri + 7,), NAN, dtype=torch.float64, device=DEV)
    assert lib.tsvgp_sym_pack_f64(src.data_ptr(), lda, stride, M, P, packed.data_ptr(), eng._stream()) == 0
    torch.cuda.synchronize()
    i, j = torch.tril_indices(M, M, device=DEV)
    want = acc2[:, i, j].reshape(-1)
    assert torch.equal(packed[:P * tri], want)
    assert torch.isnan(packed[P * tri:]).all()
    dst = torch.full((P * stride,), NAN, dtype=torch.float64, device=DEV)
    assert lib.tsvgp_sym_unpack_f64(packed.data_ptr(), dst.data_ptr(), lda, stride, M, P, eng._stream()) == 0
    torch.cuda.synchronize()
    full = dst.view(P, stride)[:, :lda * M].view(P, M, lda)
    got = full[:, :, :M]
    low = torch.tril(acc2)
    mirrored = low + torch.tril(acc2, -1).transpose(-1, -2)
    assert torch.equal(got, got.transpose(-1, -2))
    assert torch.equal(got, mirrored)
    assert torch.isnan(full[:, :, M:]).all() and torch.isnan(dst.view(P, stride)[:, lda * M:]).all()  # nothing outside M x M


def test_step_status(engines):
    """flags = (sum |info_a|, nonpos[0], sum |info_b|) against the torch fallback of t_SVGP._status_flags (a model whose engine has no
    ``step_status``): all zero, one non-zero info at the first, middle and last position of either list, negative infos, empty
    lists (NULL, 0), and nonpos passed through unchanged."""
    eng = engines[torch.float64]
    lib = eng.lib
    t_SVGP = pkg().t_SVGP
    stub = types.SimpleNamespace(_get_engine=lambda: object(), device=torch.device(DEV))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)

    def kernel_flags(a, b, nonpos):
        flags = torch.full((3,), NAN, dtype=torch.float64, device=DEV)
        st = lib.tsvgp_step_status_f64(None if a is None else a.data_ptr(), 0 if a is None else a.numel(),
                                       None if b is None else b.data_ptr(), 0 if b is None else b.numel(),
                                       None if nonpos is None else nonpos.data_ptr(), flags.data_ptr(), eng._stream())
        assert st == 0
        torch.cuda.synchronize()
        return flags

    n = 11
    cases = [([0] * n, [0] * n)]
    for pos in (0, n // 2, n - 1):
        one = [0] * n
        one[pos] = 37
        cases += [(one, [0] * n), ([0] * n, one)]
    cases += [([0, -3, 0, 5, -7], [-2, 0, 0]), ([-1], [-(2 ** 31) + 1, 2 ** 31 - 1])]
    for k, (a, b) in enumerate(cases):
        nonpos = torch.tensor(float(3 * k) + 0.5, dtype=torch.float64, device=DEV)  # passed through as it is, no rounding
        at, bt = i32(a), i32(b)
        got = kernel_flags(at, bt, nonpos.reshape(1))
        # the fallback takes lists of info tensors, as the models collect them: split the lists in two
        want = t_SVGP._status_flags(stub, {"infos": [at[:1], at[1:]] if len(a) > 1 else [at]}, nonpos, [bt[:1], bt[1:]])
        assert torch.equal(got, want), (a, b)
        assert got.tolist() == [float(sum(abs(v) for v in a)), 3 * k + 0.5, float(sum(abs(v) for v in b))]
    # empty lists: NULL, 0
    nonpos = torch.tensor([4.0], dtype=torch.float64, device=DEV)
    at = i32([0, -6, 2])
    assert kernel_flags(None, None, nonpos).tolist() == [0.0, 4.0, 0.0]
    assert kernel_flags(at, None, nonpos).tolist() == [8.0, 4.0, 0.0]
    assert kernel_flags(None, at, nonpos).tolist() == [0.0, 4.0, 8.0]
    assert torch.equal(kernel_flags(at, None, nonpos), t_SVGP._status_flags(stub, {"infos": [at]}, nonpos[0], ()))
    assert kernel_flags(at, at, None).tolist() == [8.0, 0.0, 8.0]  # nonpos NULL: 0
    # a count without its list is an invalid argument
    flags = torch.zeros(3, dtype=torch.float64, device=DEV)
    assert lib.tsvgp_step_status_f64(None, 2, None, 0, nonpos.data_ptr(), flags.data_ptr(), eng._stream()) == 1
    assert lib.tsvgp_step_status_f64(None, 0, None, 2, nonpos.data_ptr(), flags.data_ptr(), eng._stream()) == 1
