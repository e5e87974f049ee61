"""The three N-pass MFMA products (``tsvgp_trmm_*``, ``tsvgp_moments_*``, ``tsvgp_site_accum_*`` and their ``_batched_`` forms)
through the C ABI, entry by entry:

* EXACT: the integer / dyadic operands of tests/npass_ref.py, on which every partial sum in any order is representable in the compute
  dtype (tests/test_npass_ref_cpu.py asserts that for every case below, and that the probes see the faults they are made for).  The
  kernel must equal NumPy bit for bit at every entry -- compared as integer views, so -0.0 and NaN count as differences -- whatever its
  chunk order, slice count or accumulation order.  A difference names the first (row, col) with got / expected.
* GUARD BANDS: every output of every launch below sits in an allocation with 64 more elements behind its documented extent, filled
  with a fixed bit pattern that has to be there afterwards (``mean`` / ``var`` behind [N, P], ``g0`` / ``g1`` behind [Np, P], the
  partials behind Np / 128, ``C``, ``acc2``, ``acc1``, and ``work`` behind ``work_bytes``).
* ROUNDING: graded random operands against the entrywise bounds of rounding analysis (npass_ref.rounding_bounds); the exact operands
  never round, so this family is what exercises the fp32 -> fp64 hand-over and the accumulation itself.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import npass_ref as R
from tests.helpers import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f64": (torch.float64, np.float64), "f32": (torch.float32, np.float32)}
DTYPES = pytest.mark.parametrize("dt", ["f64", "f32"])  # (innermost: the two dtypes of a case share one generated reference)
INT_VIEW = {8: torch.int64, 4: torch.int32, 1: torch.uint8}
GUARD = 64  # elements behind every output
PATTERN = {8: 0x7FF8DEADBEEF0001, 4: 0x7FC0BEEF, 1: 0xA5}
GAP = 64  # elements between the operands / outputs of consecutive latents in the NaN-gapped batched layouts
_ENGINES = {}


def _engine(dt):
    if dt not in _ENGINES:
        _ENGINES[dt] = pkg().estep.EStepEngine(DT[dt][0], DEV)
    return _ENGINES[dt]


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=DT[dt][0] if isinstance(dt, str) else dt, device=DEV).contiguous()


class Guarded:
    """``numel`` elements holding ``fill`` and GUARD elements of PATTERN behind them, in one allocation."""

    def __init__(self, numel, dtype, fill=float("nan")):
        self.n = int(numel)
        self.full = torch.empty(self.n + GUARD, dtype=dtype, device=DEV)
        self.body = self.full[:self.n]
        self.body.fill_(fill)
        self.bits = self.full.view(INT_VIEW[self.full.element_size()])
        self.pattern = PATTERN[self.full.element_size()]
        self.bits[self.n:] = self.pattern

    def ptr(self):
        return self.full.data_ptr()

    def intact(self):
        return bool((self.bits[self.n:] == self.pattern).all())


def _ptr(x):
    return None if x is None else (x.ptr() if isinstance(x, Guarded) else x.data_ptr())


def _check_guards(what, **guards):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device fault: nothing more is launched on this device from here
        pytest.exit(f"{what}: {e}", returncode=3)
    for name, g in guards.items():
        assert g is None or g.intact(), f"{what}: the {GUARD} elements behind {name} were written"


def _exact(got, ref, what):
    """``got`` (device tensor) equals ``ref`` (NumPy, any float dtype holding values exact in got's dtype) bit for bit."""
    ref_t = torch.as_tensor(np.ascontiguousarray(ref)).to(got.dtype).to(DEV).reshape(got.shape)
    view = INT_VIEW[got.element_size()]
    if torch.equal(got.contiguous().view(view), ref_t.view(view)):
        return
    raise AssertionError(f"{what}: {R.first_difference(got.cpu().numpy(), ref_t.cpu().numpy())}")


def _gapped(blocks, dt, stride):
    """[len(blocks) * stride] NaN with block b at b * stride."""
    buf = torch.full((len(blocks) * stride,), float("nan"), dtype=DT[dt][0], device=DEV)
    for b, x in enumerate(blocks):
        buf[b * stride:b * stride + x.size] = _dev(x, dt).reshape(-1)
    return buf


def _gaps_are_nan(buf, n, stride, used):
    return all(bool(torch.isnan(buf[b * stride + used:(b + 1) * stride]).all()) for b in range(n))


# ------------------------------------------------------------------------------------------------- trmm
def _trmm(eng, A, Tm, C, Np, Mp, mode):
    pkg()._backend.check(eng._fn("tsvgp_trmm")(_ptr(A), _ptr(Tm), _ptr(C), Np, Mp, mode, eng._stream()), "trmm")


def _trmm_batched(eng, A, sA, Tm, sT, C, sC, Np, Mp, mode, batch):
    pkg()._backend.check(eng._fn("tsvgp_trmm_batched")(_ptr(A), sA, _ptr(Tm), sT, _ptr(C), sC, Np, Mp, mode, batch, eng._stream()),
                         "trmm_batched")


@DTYPES
@pytest.mark.parametrize("Mp,mode", R.TRMM_CASES)
def test_trmm_exact(Mp, mode, dt):
    """Placement probe (every Tm[i, j] of the triangle read back by value, +0.0 elsewhere) and sum probes at Np = 256, 384, through
    both entries; the upper form in place; batch = 3 on NaN-gapped strides and with a shared operand."""
    eng = _engine(dt)
    tdt = DT[dt][0]
    probes = [("placement", R.trmm_placement(Mp, mode))] + [(f"sum Np={Np}", R.trmm_sum(Mp, mode, Np)) for Np in R.TRMM_SUM_NP]
    for pname, c in probes:
        what = f"trmm {pname} Mp={Mp} mode={mode} {dt}"
        Np = c["A"].shape[0]
        A, Tm = _dev(c["A"], dt), _dev(c["Tm"], dt)
        C = Guarded(Np * Mp, tdt)
        _trmm(eng, A, Tm, C, Np, Mp, mode)
        _check_guards(what, C=C)
        _exact(C.body.reshape(Np, Mp), c["C"], what)
        Cb = Guarded(Np * Mp, tdt)
        _trmm_batched(eng, A, 0, Tm, 0, Cb, Np * Mp, Np, Mp, mode, 1)
        _check_guards(what + " batched entry", C=Cb)
        _exact(Cb.body.reshape(Np, Mp), c["C"], what + " batched entry")
        if mode == R.UPPER:  # in place: bit-identical to out of place
            Ci = Guarded(Np * Mp, tdt)
            Ci.body.copy_(A.reshape(-1))
            _trmm(eng, Ci, Tm, Ci, Np, Mp, mode)
            _check_guards(what + " in place", C=Ci)
            _exact(Ci.body.reshape(Np, Mp), c["C"], what + " in place")
    # batch = 3: latent b reads A with its rows rolled by 17 b and Tm with the sign (1, -1, 1)[b]
    c = R.trmm_sum(Mp, mode, R.TRMM_SUM_NP[0])
    Np, batch, stride = R.TRMM_SUM_NP[0], 3, R.TRMM_SUM_NP[0] * Mp + GAP
    signs = (1.0, -1.0, 1.0)
    As = [np.roll(c["A"], 17 * b, axis=0) for b in range(batch)]
    Tms = _dev(np.stack([R.pz(s * c["Tm"]) for s in signs]), dt)
    refs = [R.pz(s * np.roll(c["C"], 17 * b, axis=0)) for b, s in enumerate(signs)]
    Ag = _gapped(As, dt, stride)
    Cg = Guarded(batch * stride, tdt)
    _trmm_batched(eng, Ag, stride, Tms, Mp * Mp, Cg, stride, Np, Mp, mode, batch)
    what = f"trmm_batched gapped Mp={Mp} mode={mode} {dt}"
    _check_guards(what, C=Cg)
    for b in range(batch):
        _exact(Cg.body[b * stride:b * stride + Np * Mp].reshape(Np, Mp), refs[b], f"{what} latent {b}")
    assert _gaps_are_nan(Cg.body, batch, stride, Np * Mp) and _gaps_are_nan(Ag, batch, stride, Np * Mp), what
    # strideA = 0: one operand shared by the three latents
    Cs = Guarded(batch * stride, tdt)
    _trmm_batched(eng, _dev(c["A"], dt), 0, Tms, Mp * Mp, Cs, stride, Np, Mp, mode, batch)
    what = f"trmm_batched shared operand Mp={Mp} mode={mode} {dt}"
    _check_guards(what, C=Cs)
    for b, s in enumerate(signs):
        _exact(Cs.body[b * stride:b * stride + Np * Mp].reshape(Np, Mp), R.pz(s * c["C"]), f"{what} latent {b}")
    assert _gaps_are_nan(Cs.body, batch, stride, Np * Mp), what


# ------------------------------------------------------------------------------------------------- moments
def _moments(eng, dt, A, strideA, Tm, gamma, Y, kdiag, lik, N, Np, Mp, P, mode, what, want_var=True):
    """One launch of tsvgp_moments_* (strideA None) or tsvgp_moments_batched_* into guarded outputs."""
    B = pkg()._backend
    tdt = DT[dt][0]
    fused = (lik & 0xFF) != B.LIK_NONE
    mean, var = Guarded(N * P, tdt), (Guarded(N * P, tdt) if want_var else None)
    g0, g1 = (Guarded(Np * P, tdt), Guarded(Np * P, tdt)) if fused else (None, None)
    ve, bad = Guarded(Np // 128, torch.float64), Guarded(Np // 128, torch.int32, fill=7)
    tail = (lik, 0.5, _ptr(mean), _ptr(var), _ptr(g0), _ptr(g1), _ptr(ve), _ptr(bad), N, Np, Mp, P, mode, eng._stream())
    if strideA is None:
        st = eng._fn("tsvgp_moments")(_ptr(A), _ptr(Tm), _ptr(gamma), _ptr(Y), float(kdiag), *tail)
    else:
        st = eng._fn("tsvgp_moments_batched")(_ptr(A), strideA, _ptr(Tm), _ptr(gamma), _ptr(Y), (ctypes.c_double * P)(*kdiag), *tail)
    B.check(st, what)
    _check_guards(what, mean=mean, var=var, g0=g0, g1=g1, ve_partial=ve, nonpos_partial=bad)
    shape = lambda g, rows: None if g is None else g.body.reshape(rows, P)
    return dict(mean=shape(mean, N), var=shape(var, N), g0=shape(g0, Np), g1=shape(g1, Np), ve=ve.body, nonpos=bad.body)


def _moments_exact(c, dt):
    B = pkg()._backend
    eng = _engine(dt)
    N, Np, Mp, P, mode = c["N"], c["Np"], c["Mp"], c["P"], c["mode"]
    Tm, gamma, Y = _dev(c["Tm"], dt), _dev(c["gamma"], dt), _dev(c["Y"], dt)
    stride = Np * Mp + GAP
    for form in ("shared", "batched"):
        f = c[form]
        if form == "shared":
            A, sA = _dev(f["A"], dt), None
        else:
            A, sA = _gapped(list(f["A"]), dt, stride), stride
        for lik in (B.LIK_NONE, B.LIK_GAUSSIAN):
            what = f"moments {form} lik={lik} Mp={Mp} mode={mode} P={P} N={N} {dt}"
            out = _moments(eng, dt, A, sA, Tm, gamma, Y if lik else None, f["kdiag"], lik, N, Np, Mp, P, mode, what)
            ref = f["ref"]
            _exact(out["mean"], ref["mean"], what + " mean")
            _exact(out["var"], ref["var"], what + " var")
            _exact(out["nonpos"], ref["nonpos"], what + " nonpos_partial")
            if lik:
                _exact(out["g0"], ref["g0"], what + " g0")
                _exact(out["g1"], ref["g1"], what + " g1")
        if form == "batched":
            assert _gaps_are_nan(A, P, stride, Np * Mp)


@DTYPES
@pytest.mark.parametrize("Mp,mode,P", R.MOMENTS_GRID)
def test_moments_exact(Mp, mode, P, dt):
    """1 to 9 column tiles in the three modes: unit rows (q_n = a column's sum of squares over the triangle, mean_n = gamma[n]) and
    4-sparse rows, a 37-row last panel, var > 0, < 0 and == 0; the shared-operand and the per-latent entry, with and without the
    Gaussian map (g0 = 2 (y - mean), g1 = -1, rows >= N +0.0)."""
    _moments_exact(R.moments_case(Mp, mode, P, R.grid_rows(Mp)), dt)


@DTYPES
@pytest.mark.parametrize("Mp,mode,P,N", R.MOMENTS_TAIL_CASES)
def test_moments_row_tails_exact(Mp, mode, P, N, dt):
    """Tails of 127, 1 and 0 (N = Np) rows behind 0, 1 and 2 full panels."""
    _moments_exact(R.moments_case(Mp, mode, P, N), dt)


@DTYPES
@pytest.mark.parametrize("Mp,P", R.MEANONLY_CASES)
def test_mean_only_exact(Mp, P, dt):
    B = pkg()._backend
    eng = _engine(dt)
    c = R.meanonly_case(Mp, P)
    A, gamma, Y = _dev(c["A"], dt), _dev(c["gamma"], dt), _dev(c["Y"], dt)
    for lik in (B.LIK_NONE, B.LIK_GAUSSIAN):
        what = f"mean only lik={lik} Mp={Mp} P={P} {dt}"
        out = _moments(eng, dt, A, None, None, gamma, Y if lik else None, 1.0, lik | B.LIK_MEANONLY, c["N"], c["Np"], Mp, P, 1, what,
                       want_var=False)
        _exact(out["mean"], c["mean"], what + " mean")
        _exact(out["nonpos"], np.zeros(c["Np"] // 128, dtype=np.int32), what + " nonpos_partial")
        if lik:
            _exact(out["g0"], c["g0"], what + " g0")
            _exact(out["g1"], c["g1"], what + " g1")


@pytest.fixture(scope="module")
def wide_problem():
    """Integer operands at Mp = 8320, Tm drawn on the device (554 MB in fp64): where gamma no longer fits panel1_kernel's dynamic LDS
    and the launcher takes the triangular panel_kernel arms."""
    M, N = R.WIDE_M, R.WIDE_N
    g = torch.Generator(device=DEV).manual_seed(23)
    Tm = torch.randint(-1, 2, (M, M), generator=g, device=DEV, dtype=torch.int8)
    rng = np.random.RandomState(23)
    A = np.zeros((128, M))
    A[:N] = R.wide_rows()
    return dict(A=A, Tm=Tm, Tm_h=Tm.cpu().numpy(), gamma=rng.randint(-3, 4, (M, 1)).astype(np.float64),
                Y=rng.randint(-5, 6, (N, 1)).astype(np.float64))


@pytest.mark.parametrize("mode", [R.LOWER, R.UPPER])
def test_moments_exact_beyond_the_gamma_lds_limit(wide_problem, mode):
    B = pkg()._backend
    w = wide_problem
    M, N, Np = R.WIDE_M, R.WIDE_N, 128
    assert M * 8 > 64 * 1024
    tri = torch.tril if mode == R.LOWER else torch.triu
    Tm = tri(w["Tm"]).to(torch.float64).reshape(1, M, M)
    Tm_h = (np.tril if mode == R.LOWER else np.triu)(w["Tm_h"]).astype(np.float64)[None]
    q = R.moments_values(w["A"], Tm_h, w["gamma"], 0.0, None, N)["q"]
    kdiag = R.pick_kdiag(q, 1, 2)
    ref = R.moments_values(w["A"], Tm_h, w["gamma"], kdiag, w["Y"], N)
    assert (ref["var"] == 0).any() and (ref["var"] > 0).any() and (ref["var"] < 0).any() and kdiag <= M
    what = f"moments Mp={M} mode={mode}"
    out = _moments(_engine("f64"), "f64", _dev(w["A"], "f64"), None, Tm, _dev(w["gamma"], "f64"), _dev(w["Y"], "f64"), kdiag,
                   B.LIK_GAUSSIAN, N, Np, M, 1, mode, what)
    for k in ("mean", "var", "g0", "g1", "nonpos"):
        _exact(out[k], ref[k], f"{what} {k}")


# ------------------------------------------------------------------------------------------------- site sums
def _site_accum(eng, dt, Bm, strideB, g0, g1, Np, Mp, P, nsplit, what):
    Bk = pkg()._backend
    nbytes = int(eng._fn("tsvgp_site_accum_work_bytes")(Mp, P, nsplit))
    assert nbytes > 0 and nbytes % 16 == 0
    work = Guarded(nbytes, torch.uint8, fill=0x3C)
    acc2, acc1 = Guarded(P * Mp * Mp, torch.float64), Guarded(P * Mp, torch.float64)
    tail = (_ptr(g0), _ptr(g1), _ptr(acc2), _ptr(acc1), _ptr(work), Np, Mp, P, nsplit, eng._stream())
    if strideB is None:
        st = eng._fn("tsvgp_site_accum")(_ptr(Bm), *tail)
    else:
        st = eng._fn("tsvgp_site_accum_batched")(_ptr(Bm), strideB, *tail)
    Bk.check(st, what)
    _check_guards(what, acc2=acc2, acc1=acc1, work=work)
    return acc2.body.reshape(P, Mp, Mp), acc1.body.reshape(P, Mp)


@DTYPES
@pytest.mark.parametrize("Mp,P,Np,nsplits", R.SITE_CASES, ids=[f"Mp{Mp}-P{P}-Np{Np}" for Mp, P, Np, _ in R.SITE_CASES])
def test_site_accum_exact(Mp, P, Np, nsplits, dt):
    """1, 3, 6 and 36 lower tiles; syrk1_kernel / syrk1f_kernel (P <= 8) and syrk_kernel<T> (P = 9); slice counts that give slices of
    0 to 5 chunks on either partition (test_site_slice_lengths_cover_0_to_5_on_both_partitions computes them); integer and dyadic
    weights (down to 2^-26 in fp64).  acc2 and acc1 equal the reference, hence each other across nsplit, bit for bit."""
    eng = _engine(dt)
    c = R.site_case(Mp, P, Np, dt)
    Bs, g0 = _dev(c["B"][0], dt), _dev(c["g0"], dt)
    stride = Np * Mp + GAP
    Bg = _gapped(list(c["B"]), dt, stride)
    for wname, w in c["sets"].items():
        g1 = _dev(w["g1"], dt)
        assert np.array_equal(g1.double().cpu().numpy(), w["g1"])  # the dyadic weights are exact in the compute dtype
        first = None
        for ns in nsplits:
            what = f"site_accum {wname} Mp={Mp} P={P} Np={Np} nsplit={ns} {dt}"
            acc2, acc1 = _site_accum(eng, dt, Bs, None, g0, g1, Np, Mp, P, ns, what)
            _exact(acc2, w["shared"][0], what + " acc2")
            _exact(acc1, w["shared"][1], what + " acc1")
            assert torch.equal(acc2, acc2.transpose(-1, -2)), what + ": acc2 is not symmetric"
            first = first or (acc2, acc1)
            view = lambda x: x.contiguous().view(torch.int64)
            assert torch.equal(view(acc2), view(first[0])) and torch.equal(view(acc1), view(first[1])), what + f": differs from nsplit={nsplits[0]}"
        for ns in (nsplits[0], nsplits[-1]):
            what = f"site_accum_batched {wname} Mp={Mp} P={P} Np={Np} nsplit={ns} {dt}"
            acc2, acc1 = _site_accum(eng, dt, Bg, stride, g0, g1, Np, Mp, P, ns, what)
            _exact(acc2, w["batched"][0], what + " acc2")
            _exact(acc1, w["batched"][1], what + " acc1")
            assert torch.equal(acc2, acc2.transpose(-1, -2)), what + ": acc2 is not symmetric"
    assert _gaps_are_nan(Bg, P, stride, Np * Mp)


def test_site_slice_lengths_cover_0_to_5_on_both_partitions():
    """The coverage the cases above are chosen for, from the launcher's formulas (the CPU file asserts the same list)."""
    for esize, Pk in ((8, 1), (8, 9), (4, 1), (4, 9)):
        seen = {"off": set(), "diag": set()}
        for Mp, P, Np, nsplits in R.SITE_CASES:
            if Mp >= 256 and (P <= 8) == (Pk <= 8):
                for ns in nsplits:
                    for part, lens in R.slice_lengths(Np, ns, esize, P).items():
                        seen[part] |= set(lens)
        assert set(range(6)) <= seen["off"] and set(range(6)) <= seen["diag"], (esize, Pk, seen)
    # the work size the slices are laid out in, from the header's formula
    for dt, esize in (("f64", 8), ("f32", 4)):
        for Mp, P, ns in ((128, 1, 1), (384, 3, 5), (1024, 9, 3)):
            nt = Mp // 128
            nd = R.site_ns_diag(ns, esize)
            want = P * ((nt * (nt - 1) // 2 * ns + nt * nd) * 128 * 128 + nd * Mp) * esize
            assert int(_engine(dt)._fn("tsvgp_site_accum_work_bytes")(Mp, P, ns)) == want


# ------------------------------------------------------------------------------------------------- rounding family
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for (kernel, dt), r in sorted(WORST.items()):
        print(f"\nrounding family, worst |got - ref| / (u absum): {kernel} {dt}: {r:.3f}", end="")
    print()


def _within(got, triple, u, key, what):
    ref, bound, absum = triple
    err = np.abs(got.double().cpu().numpy().reshape(ref.shape) - ref)
    live = absum > 0
    ratio = float(np.max(err[live] / (u * absum[live]))) if live.any() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"{what}: worst |got - ref| / (u absum) = {ratio:.3f}, worst |got - ref| / bound = {float(np.max(err[live] / bound[live])):.2e}")
    over = err > bound
    assert not over.any(), f"{what}: {int(over.sum())} entries beyond the bound; first at {tuple(int(v) for v in np.argwhere(over)[0])}"


@DTYPES
@pytest.mark.parametrize("Mp,mode,P", R.ROUNDING_CASES)
def test_rounding_within_the_derived_bounds(Mp, mode, P, dt):
    """Graded randn operands (rows of A / B scaled by 2^-(n mod 24), rows of Tm by 2^-(i mod 16), g1 = -2^-(n mod 27), 37 dead
    columns), N = 257, entry by entry against 2 (K + 1) u s_i and its kin; the reference is float64."""
    B = pkg()._backend
    eng = _engine(dt)
    tdt, npdt = DT[dt]
    u = 2.0 ** -53 if dt == "f64" else 2.0 ** -24
    op = R.rounding_operands(Mp, mode, P, npdt)
    bounds = R.rounding_bounds(op, u)
    N, Np = op["N"], op["Np"]
    A, Tm, gamma = _dev(op["A"], dt), _dev(op["Tm"], dt), _dev(op["gamma"], dt)
    what = f"rounding Mp={Mp} mode={mode} P={P} {dt}"
    C = Guarded(P * Np * Mp, tdt)
    _trmm_batched(eng, A, 0, Tm, Mp * Mp, C, Np * Mp, Np, Mp, mode, P)
    _check_guards(what, C=C)
    _within(C.body, bounds["C"], u, ("trmm", dt), what + " C")
    out = _moments(eng, dt, A, None, Tm, gamma, None, op["kdiag"], B.LIK_NONE, N, Np, Mp, P, mode, what)
    _within(out["mean"], bounds["mean"], u, ("moments mean", dt), what + " mean")
    _within(out["var"], bounds["var"], u, ("moments var", dt), what + " var")
    if mode == R.LOWER:  # (the site sums do not read Tm)
        for ns in (1, 3):
            acc2, acc1 = _site_accum(eng, dt, A, None, _dev(op["g0"], dt), _dev(op["g1"], dt), Np, Mp, P, ns, what)
            _within(acc2, bounds["acc2"], u, ("site_accum acc2", dt), what + f" acc2 nsplit={ns}")
            _within(acc1, bounds["acc1"], u, ("site_accum acc1", dt), what + f" acc1 nsplit={ns}")
