"""The two forms of the site sums through the C ABI and through the models.

* CONSTANT WEIGHT (``tsvgp_site_accum_cw_*`` and ``_cw_batched_*``): g1[n, p] = c[p] on every row, the kernels sum b b^T unweighted and
  the reduction scales once.  On the integer operands of tests/npass_ref.py with c = -2^-k every product and sum is exact, so the entry
  equals the general one (given g1 = c on every row) and NumPy bit for bit, for every slice count, and acc1 -- the same code in both forms
  -- is bit-identical.  With c = -5 (not a power of two) the two forms round differently and agree within the bound of rounding analysis
  (npass_ref.rounding_bounds, the rounding family of tests/test_gpu_npass_values.py; no tolerance of this file's own).
* GENERAL FORM, diagonal tiles: the row-block operands are the column-block fragments already in registers; exact on the dyadic weights,
  within the same bound on graded random operands.
* PADDING: the operand's rows >= N are zero, so whatever g0 / g1 hold there changes nothing -- in either form.
* MODELS: a Gaussian likelihood takes the constant-weight entry (``EStepEngine.site_sum_calls``) and matches the oracle at the tolerance of
  tests/test_gpu_model.py; a Bernoulli likelihood takes the general one.

Shapes: Mp = 128 (one diagonal tile), 256 (the first off-diagonal tile), 384; P = 1, 3; Np and the slice counts of npass_ref.SITE_CASES, which
reach slices of 0, 1, 2, 3 and 5 chunks on both partitions (asserted below).
"""
import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests import npass_ref as R
from tests.helpers import pkg, relerr, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f64": (torch.float64, np.float64, 8), "f32": (torch.float32, np.float32, 4)}
DTYPES = pytest.mark.parametrize("dt", ["f64", "f32"])
CASES = [c for c in R.SITE_CASES if c[0] in (128, 256, 384) and c[1] in (1, 3) and c[2] <= 640]
IDS = [f"Mp{Mp}-P{P}-Np{Np}" for Mp, P, Np, _ in CASES]
GUARD = 64
_ENGINES = {}


def _engine(dt):
    if dt not in _ENGINES:
        _ENGINES[dt] = pkg().estep.EStepEngine(DT[dt][0], DEV)
    return _ENGINES[dt]


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV).contiguous()


def _guarded(numel, dtype, fill):
    full = torch.full((numel + GUARD,), fill, dtype=dtype, device=DEV)
    full[numel:] = 77
    return full


def _launch(eng, form, Bm, strideB, g0, weights, Np, Mp, P, nsplit, what):
    """One launch of the general (``weights`` = g1 [Np, P]) or the constant-weight (``weights`` = c [P], fp64) entry; acc2 [P, Mp, Mp] and
    acc1 [P, Mp] out of NaN-filled allocations whose 64 trailing elements (and those of ``work``) have to be left alone."""
    nbytes = int(eng._fn("tsvgp_site_accum_work_bytes")(Mp, P, nsplit))
    work = _guarded(nbytes, torch.uint8, 0x3C)
    acc2, acc1 = _guarded(P * Mp * Mp, torch.float64, float("nan")), _guarded(P * Mp, torch.float64, float("nan"))
    name = "tsvgp_site_accum" + ("_cw" if form == "cw" else "") + ("" if strideB is None else "_batched")
    operand = (Bm.data_ptr(),) if strideB is None else (Bm.data_ptr(), strideB)
    st = eng._fn(name)(*operand, g0.data_ptr(), weights.data_ptr(), acc2.data_ptr(), acc1.data_ptr(), work.data_ptr(), Np, Mp, P,
                       nsplit, eng._stream())
    pkg()._backend.check(st, what)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device fault: nothing more is launched on this device from here
        pytest.exit(f"{what}: {e}", returncode=3)
    for nm, buf, n in (("acc2", acc2, P * Mp * Mp), ("acc1", acc1, P * Mp), ("work", work, nbytes)):
        assert bool((buf[n:] == 77).all()), f"{what}: the {GUARD} elements behind {nm} were written"
    return acc2[:P * Mp * Mp].reshape(P, Mp, Mp), acc1[:P * Mp].reshape(P, Mp)


def _bits(x):
    return x.contiguous().view(torch.int64)


def _same(got, ref, what):
    """Bit for bit (integer views: -0.0 and +0.0 differ); ``ref`` a device tensor or a NumPy array of exactly representable values."""
    if not torch.is_tensor(ref):
        ref = torch.as_tensor(np.ascontiguousarray(ref), dtype=torch.float64, device=DEV).reshape(got.shape)
    if not torch.equal(_bits(got), _bits(ref)):
        raise AssertionError(f"{what}: {R.first_difference(got.cpu().numpy(), ref.cpu().numpy())}")


def test_the_cases_reach_slices_of_0_to_5_chunks_on_both_partitions():
    for esize in (8, 4):
        seen = {"off": set(), "diag": set()}
        for Mp, P, Np, nsplits in CASES:
            for ns in nsplits:
                for part, lens in R.slice_lengths(Np, ns, esize, P).items():
                    seen[part] |= set(lens)
        assert {0, 1, 2, 3, 5} <= seen["off"] and {0, 1, 2, 3, 5} <= seen["diag"], (esize, seen)
    assert {c[0] for c in CASES} == {128, 256, 384} and {c[1] for c in CASES} == {1, 3}


@DTYPES
@pytest.mark.parametrize("Mp,P,Np,nsplits", CASES, ids=IDS)
def test_constant_weight_equals_general_and_numpy_bit_for_bit(Mp, P, Np, nsplits, dt):
    """c[p] = -2^-(3 + p) on the integer operands: every partial sum in any order is exact (|sum| <= 4 Np < 2^24 before the scale),
    so the constant-weight entry, the general entry with g1 = c on EVERY row and NumPy give the same bits; so do all slice counts;
    acc2 is symmetric; acc1 of the two entries is identical.  Shared and per-latent operands."""
    tdt = DT[dt][0]
    eng = _engine(dt)
    c = R.site_case(Mp, P, Np, dt)
    cp = -(2.0 ** -(3.0 + np.arange(P)))
    g1 = np.broadcast_to(cp, (Np, P)).copy()
    assert 4.0 * Np < R.EXACT_LIMIT[dt]
    g0d, g1d, cd = _dev(c["g0"], tdt), _dev(g1, tdt), _dev(cp, torch.float64)
    stride = Np * Mp + 64
    Bg = torch.full((P * stride,), float("nan"), dtype=tdt, device=DEV)
    for p in range(P):
        Bg[p * stride:p * stride + Np * Mp] = _dev(c["B"][p], tdt).reshape(-1)
    for name, Bm, sB, ref, some in (("shared", _dev(c["B"][0], tdt), None, R.site_sums(c["B"][0], c["g0"], g1), nsplits),
                                    ("batched", Bg, stride, R.site_sums(c["B"], c["g0"], g1), (nsplits[0], nsplits[-1]))):
        first = None
        for ns in some:
            what = f"{name} Mp={Mp} P={P} Np={Np} nsplit={ns} {dt}"
            cw2, cw1 = _launch(eng, "cw", Bm, sB, g0d, cd, Np, Mp, P, ns, what + " cw")
            ge2, ge1 = _launch(eng, "general", Bm, sB, g0d, g1d, Np, Mp, P, ns, what + " general")
            _same(cw2, ge2, what + ": acc2, constant weight against general")
            _same(cw1, ge1, what + ": acc1, constant weight against general")
            _same(cw2, ref[0], what + ": acc2 against NumPy")
            _same(cw1, ref[1], what + ": acc1 against NumPy")
            assert torch.equal(_bits(cw2), _bits(cw2.transpose(-1, -2))), what + ": acc2 is not symmetric"
            first = first or (cw2, cw1)
            _same(cw2, first[0], what + f": acc2 differs from nsplit={some[0]}")
            _same(cw1, first[1], what + f": acc1 differs from nsplit={some[0]}")


@DTYPES
@pytest.mark.parametrize("Mp,P,Np,nsplits", CASES, ids=IDS)
def test_general_form_stays_exact_on_the_dyadic_weights(Mp, P, Np, nsplits, dt):
    """g1 = -2^-(n mod E) per row (npass_ref.site_case): the weighted row-block fragments a diagonal tile now makes from its
    column-block registers give the reference bit for bit, for every slice count, shared and per-latent operands."""
    tdt = DT[dt][0]
    eng = _engine(dt)
    c = R.site_case(Mp, P, Np, dt)
    w = c["sets"]["dyadic"]
    g0d, g1d = _dev(c["g0"], tdt), _dev(w["g1"], tdt)
    Bg = _dev(c["B"], tdt)
    for ns in nsplits:
        what = f"general dyadic Mp={Mp} P={P} Np={Np} nsplit={ns} {dt}"
        acc2, acc1 = _launch(eng, "general", Bg[0], None, g0d, g1d, Np, Mp, P, ns, what)
        _same(acc2, w["shared"][0], what + " acc2")
        _same(acc1, w["shared"][1], what + " acc1")
        assert torch.equal(_bits(acc2), _bits(acc2.transpose(-1, -2))), what + ": acc2 is not symmetric"
    for ns in (nsplits[0], nsplits[-1]):
        what = f"general dyadic batched Mp={Mp} P={P} Np={Np} nsplit={ns} {dt}"
        acc2, acc1 = _launch(eng, "general", Bg, Np * Mp, g0d, g1d, Np, Mp, P, ns, what)
        _same(acc2, w["batched"][0], what + " acc2")
        _same(acc1, w["batched"][1], what + " acc1")


def _within(got, triple, what):
    ref, bound, absum = triple
    err = np.abs(got.double().cpu().numpy().reshape(ref.shape) - ref)
    live = absum > 0
    print(f"{what}: worst |got - ref| / bound = {float(np.max(err[live] / bound[live])):.2e}")
    over = err > bound
    assert not over.any(), f"{what}: {int(over.sum())} entries beyond the bound; first at {tuple(int(v) for v in np.argwhere(over)[0])}"


@DTYPES
@pytest.mark.parametrize("Mp,P", [(128, 1), (256, 3), (384, 3)])
def test_rounding_stays_within_the_derived_bound(Mp, P, dt):
    """Graded random operands (npass_ref.rounding_operands, N = 257): the general form with their weights g1 = -2^-(n mod 27), and both
    forms with g1 = -5 on every live row, entry by entry inside 2 (Np + 2) u sum |g1| |a_i| |a_j| of the float64 reference; with
    c = -5 the two forms also agree with each other inside that bound."""
    tdt, npdt, _ = DT[dt]
    eng = _engine(dt)
    u = 2.0 ** -53 if dt == "f64" else 2.0 ** -24
    op = R.rounding_operands(Mp, R.LOWER, P, npdt)
    Np = op["Np"]
    A, g0 = _dev(op["A"], tdt), _dev(op["g0"], tdt)
    bounds = R.rounding_bounds(op, u)
    five = dict(op)
    five["g1"] = np.zeros((Np, P))
    five["g1"][:op["N"]] = -5.0
    bounds5 = R.rounding_bounds(five, u)
    c5 = _dev(np.full(P, -5.0), torch.float64)
    for ns in (1, 3):
        what = f"rounding Mp={Mp} P={P} nsplit={ns} {dt}"
        acc2, acc1 = _launch(eng, "general", A, None, g0, _dev(op["g1"], tdt), Np, Mp, P, ns, what)
        _within(acc2, bounds["acc2"], what + " general acc2")
        _within(acc1, bounds["acc1"], what + " general acc1")
        ge2, ge1 = _launch(eng, "general", A, None, g0, _dev(five["g1"], tdt), Np, Mp, P, ns, what + " c=-5 general")
        cw2, cw1 = _launch(eng, "cw", A, None, g0, c5, Np, Mp, P, ns, what + " c=-5 cw")
        _within(ge2, bounds5["acc2"], what + " c=-5 general acc2")
        _within(cw2, bounds5["acc2"], what + " c=-5 constant weight acc2")
        _within(cw2, (ge2.cpu().numpy(), bounds5["acc2"][1], bounds5["acc2"][2]), what + " c=-5 constant weight against general")
        _same(cw1, ge1, what + " c=-5: acc1, constant weight against general")


@DTYPES
def test_padding_rows_need_no_zero_weight(dt):
    """N = Np - 37 live rows, the operand's rows >= N zero (as its producers leave them): g0 and g1 may hold anything finite there --
    both forms return the bits they return with zeros."""
    tdt = DT[dt][0]
    eng = _engine(dt)
    Mp, P, Np = 256, 3, 384
    N = Np - 37
    c = R.site_case(Mp, P, Np, dt)
    B = c["B"][0].copy()
    B[N:] = 0.0
    cp = -(2.0 ** -(2.0 + np.arange(P)))
    clean0, clean1 = c["g0"].copy(), np.broadcast_to(cp, (Np, P)).copy()
    clean0[N:], clean1[N:] = 0.0, 0.0
    dirty0, dirty1 = clean0.copy(), clean1.copy()
    dirty0[N:], dirty1[N:] = 12345.0, -777.0
    Bd, cd = _dev(B, tdt), _dev(cp, torch.float64)
    ref = R.site_sums(B, clean0, clean1)
    for ns in (1, 5):
        what = f"padding nsplit={ns} {dt}"
        for form, w_clean, w_dirty in (("general", _dev(clean1, tdt), _dev(dirty1, tdt)), ("cw", cd, cd)):
            a2, a1 = _launch(eng, form, Bd, None, _dev(clean0, tdt), w_clean, Np, Mp, P, ns, f"{what} {form} clean")
            b2, b1 = _launch(eng, form, Bd, None, _dev(dirty0, tdt), w_dirty, Np, Mp, P, ns, f"{what} {form} dirty")
            _same(b2, a2, f"{what} {form}: acc2 moved with the padding rows' weights")
            _same(b1, a1, f"{what} {form}: acc1 moved with the padding rows' weights")
            _same(a2, ref[0], f"{what} {form}: acc2 against NumPy")
            _same(a1, ref[1], f"{what} {form}: acc1 against NumPy")


def test_constant_weight_entry_rejects_what_it_cannot_take():
    """More than eight latents (the generic kernel keeps the general form), a missing constant, a constant off its 8-byte boundary:
    TSVGP_EINVAL in front of any launch."""
    eng = _engine("f64")
    Np, Mp = 128, 128
    x = torch.zeros(Np * Mp, dtype=torch.float64, device=DEV)
    g = torch.zeros(Np * 9, dtype=torch.float64, device=DEV)
    out = torch.zeros(9 * Mp * Mp + 64, dtype=torch.float64, device=DEV)
    work = torch.zeros(int(eng._fn("tsvgp_site_accum_work_bytes")(Mp, 9, 1)), dtype=torch.uint8, device=DEV)
    call = lambda cptr, P: eng._fn("tsvgp_site_accum_cw")(x.data_ptr(), g.data_ptr(), cptr, out.data_ptr(), out.data_ptr(), work.data_ptr(),
                                                          Np, Mp, P, 1, eng._stream())
    assert call(g.data_ptr(), 9) == 1
    assert call(None, 1) == 1
    assert call(g.data_ptr() + 4, 1) == 1
    assert call(g.data_ptr(), 8) == 0
    torch.cuda.synchronize()


def _model_problem():
    X, Y, _ = synthetic(N=4099, M=130, D=4, P=1, lik="gaussian", seed=21)
    Z = np.random.RandomState(22).randn(130, 4) * 1.5  # spread inducing points: a well-conditioned K_uu
    return X, Y, Z


@pytest.mark.parametrize("projection", ["direct", "whitened"])
def test_gaussian_step_takes_the_constant_weight_entry_and_matches_the_oracle(projection):
    """One natgrad_step at N = 4099, M = 130 (two tiles of M, a partial last panel of N), P = 1: lambda_1 and Lambda_2 against the oracle
    at the fp64 tolerance of tests/test_gpu_model.py; the engine launched the constant-weight form once and the general form never."""
    p = pkg()
    X, Y, Z = _model_problem()
    hip = p.t_SVGP(p.SquaredExponential(1.0, 1.0), p.Gaussian(0.1), Z, projection=projection)
    ora = O.t_SVGP(O.SquaredExponential(1.0, 1.0), O.Gaussian(0.1), Z)
    hip.natgrad_step((X, Y), lr=0.8)
    ora.natgrad_step((X, Y), lr=0.8)
    assert hip._get_engine().site_sum_calls == {"general": 0, "constant_weight": 1}
    assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < 1e-8
    assert relerr(hip.lambda_2.cpu().numpy(), ora.lambda_2) < 1e-8


def test_white_gaussian_step_takes_the_constant_weight_entry_and_matches_the_oracle():
    p = pkg()
    X, Y, Z = _model_problem()
    mk = lambda mod: mod.t_SVGP_white(mod.SquaredExponential(1.0, 1.0), mod.Gaussian(0.1), Z, num_data=X.shape[0])
    hip, ora = mk(p), mk(O)
    hip.natgrad_step((X, Y), lr=0.8)
    ora.natgrad_step((X, Y), lr=0.8)
    calls = hip._get_engine().site_sum_calls
    assert calls["constant_weight"] >= 1 and calls["general"] == 0
    assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < 1e-8
    assert relerr(hip.lambda_2.numpy(), ora.lambda_2) < 1e-8


def test_bernoulli_step_takes_the_general_entry():
    p = pkg()
    X, Y, _ = synthetic(N=4099, M=130, D=4, P=1, lik="bernoulli", seed=21)
    Z = np.random.RandomState(22).randn(130, 4) * 1.5
    hip = p.t_SVGP(p.SquaredExponential(1.0, 1.0), p.Bernoulli(), Z)
    ora = O.t_SVGP(O.SquaredExponential(1.0, 1.0), O.Bernoulli(), Z)
    hip.natgrad_step((X, Y), lr=0.8)
    ora.natgrad_step((X, Y), lr=0.8)
    assert hip._get_engine().site_sum_calls == {"general": 1, "constant_weight": 0}
    assert relerr(hip.lambda_1.numpy(), ora.lambda_1) < 1e-8
    assert relerr(hip.lambda_2.cpu().numpy(), ora.lambda_2) < 1e-8
