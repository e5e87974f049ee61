"""The likelihood maps of ``csrc/tsvgp_likmap.hip`` that came after the Gaussian / Bernoulli pair -- StudentT, Poisson, Gamma /
Exponential (``tsvgp_lik_map_scalar_*``), Ordinal (``tsvgp_lik_map_ordinal_*``), the heteroskedastic Gaussian
(``tsvgp_lik_map_hetero_*``), MultiClass / RobustMax (``tsvgp_lik_map_robustmax_*``) and Softmax with explicit draws
(``tsvgp_lik_map_softmax_*``) -- entry by entry over the whole (m, v) range the Gaussian / Bernoulli maps are held at
(tests/test_gpu_gauss_bern_map.py): m in [-12, 12], v in [1e-8, 100], in f64 and f32, with the crop and without.

Inputs, parameter sets, restatements and bounds: tests/likmap_range_ref.py (the grid of tests/bernoulli_ref.py, 15 714 rows in 123
blocks of 128 with a 98-row tail; column c rolled by 4999 c rows).  The restatements are held to mpmath at 50 digits on the fixture
rows by tests/test_likmap_range_cpu.py, within a quarter of every bound used here.  Bounds per entry, on the values the kernel
read (fp32 arrays: the fp32-rounded inputs held in fp64):
    fp64   g0, g1, ve   1e-10 (1 + |ref|)          Ordinal g1: + 4 C u64 A (``likmap_range_ref.ordinal_amplification``, C = 1.5)
           dparam       1e-10 sum |terms| + 2^-1022
    fp32   g0, g1       the fp64 bound + 2^-23 |ref| + 2^-149   (fp64 arithmetic, one rounding on the way out; ve, dparam stay fp64)
ve and dparam per 128-row block against the block's own rows under the sum of the rows' bounds.  With the crop the expected g1 is
min(ref, -1e-8).  Every case also checks: rows N .. Np exactly zero, nonpos_partial block by block, a second launch bit for bit,
the column maps on column 1 of [N, 3] buffers (NaN in the other input columns, a sentinel in the other output columns) and
through ``EStepEngine.lik_map`` on all three columns, and one launch with planted bad rows in blocks 0 and 7 (v <= 0, a
non-finite mean, a target outside the support, a label that is no integer in range): those blocks count the rows the kernel
comment says it counts, the rows it says it poisons are NaN, every other entry and partial is bit for bit the clean launch's.

Worst observed error / bound on an MI355X over the parameter sets, the direct call and the engine, with the crop and without (each
case prints its own):
    map         fp64: g0       g1       ve / block  dparam / block   |  fp32: g0     g1
    StudentT          1.0e-4   5.9e-3   5.3e-6      5.9e-6           |        0.48   0.49
    Poisson           1.4e-4   3.4e-6   9.3e-6      -                |        0.50   0.50
    Gamma             1.3e-5   3.4e-6   7.2e-6      1.9e-5           |        0.50   0.50
    Ordinal           1.1e-3   0.11     6.7e-6      6.0e-3           |        0.50   0.50
    hetero            1.5e-4   4.3e-3   1.4e-4      -                |        0.49   0.50
    RobustMax         3.6e-4   0.15     5.1e-4      -                |        0.49   0.48
    Softmax           1.8e-5   0.085    4.5e-6      -                |        0.49   0.50
(fp32: one rounding of an fp64 result is 2^-24 |ref| of the 2^-23 |ref| granted; ve and dparam are fp64 under either type).

Scratch mutants of tsvgp_likmap.hip, each built beside the product and never committed (first failing assertion here | the tests
that existed before this module and reach the mutated code):
    1  ordinal_node without the side switch (flip = false)     ``_check``: g1, ratio 13 at K = 2, sigma = 0.7 (fp64), 1.4 (fp32) |
       test_gpu_ordinal_gamma.py::test_map_entry_by_entry fails at N = 127 only, in fp64 only (1.66e-8 against its 1e-8)
    2  the StudentT accumulators a0, a1 held in float         ``_check``: g0, ratio 1775 (fp64), 24 (fp32) | test_gpu_scalar_lik.py fails
       in fp64 (2.6e-8 .. 1e-7 against 1e-8, and the model tests on top); every fp32 case there passes
    3  GH_W[9] dropped from the StudentT loop                  SURVIVES: the weight is 1.26e-13 and |l'| <= (nu + 1) / (2 sqrt(nu) s) = 22,
       |l''| <= 560 at the smallest scale, so g0 moves by 5.5e-12 and g1 by w z^2 |l''| = 4e-9 on |g1| = 280, both under
       1e-10 (1 + |ref|) | test_gpu_scalar_lik.py passes too
    4  RobustMax: a clipped unlabelled class returns the unclipped derivative   ``_check``: g1, ratio 2e13 | test_gpu_robustmax.py passes.
       (It survived the first version of this module as well: with the clipped class a grid step or more from the labelled mean
       every cdf saturates and the derivative is zero with or without the clip.  Every second planted row now carries the
       labelled mean.)
    5  hetero T1 formed with ep + em                           ``_check``: g1, ratio 1e10 | test_gpu_hetero.py fails too (28 of 32)
    6  lik_map_scalar_kernel writes ve_partial[blockIdx.x ^ 1]  ``_check``: ve per block, ratio 1.3e9 | test_gpu_scalar_lik.py and
       test_gpu_ordinal_gamma.py fail at N >= 129 in fp64 (their fp32 cases compare the sum over the blocks and pass)
"""
import functools

import numpy as np
import pytest
import torch

from tests import likmap_range_ref as L
from tests.helpers import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"f64": torch.float64, "f32": torch.float32}
SENTINEL = 7.0
COL = 1  # the column of the [N, 3] buffers the direct calls of the column maps run on
_ENGINES = {}


def _engine(dtype):
    if dtype not in _ENGINES:
        _ENGINES[dtype] = pkg().estep.EStepEngine(dtype, DEV)
    return _ENGINES[dtype]


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV).contiguous()


def _h(t):
    return t.double().cpu().numpy()


def _blocks(x, N):
    """Sums over the rows of every 128-row block of x [N] or [N, ...] (all columns)."""
    return np.add.reduceat(np.asarray(x, np.float64).reshape(N, -1).sum(axis=1), np.arange(0, N, 128))


@functools.lru_cache(maxsize=None)
def _reference(name, par, kind):
    """Inputs, restatement and bounds of one parameter set and array type, computed once for the crop variants and the engine."""
    mean, var, Y = L.inputs(name, par, kind)
    eps = L.softmax_eps(par, kind) if name == "softmax" else None
    ref = L.restate(name, par, mean, var, Y, eps)
    ref.update(L.bounds(ref, kind))
    if name not in L.COLUMN_MAPS:
        ref["ve"], ref["bve"] = ref["ve"].reshape(len(mean), 1), ref["bve"].reshape(len(mean), 1)
    for a in ref.values():
        if a is not None:
            a.setflags(write=False)
    return mean, var, Y, eps, ref


def _ratio(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((err == 0) & (bound == 0), 0.0, err / bound)
    assert not np.isnan(r).any()
    return float(np.max(r))


def _check(tag, ref, cols, k0, k1, vep, dpp, npp, N, crop):
    """g0, g1 [Np, len(cols)] against columns ``cols`` of the reference entry by entry, the rows past N, ve / dparam / nonpos per block."""
    r1 = np.minimum(ref["g1"][:, cols], -1e-8) if crop else ref["g1"][:, cols]
    e0 = _ratio(np.abs(k0[:N] - ref["g0"][:, cols]), ref["b0"][:, cols])
    e1 = _ratio(np.abs(k1[:N] - r1), ref["b1"][:, cols])
    vcols = cols if ref["ve"].shape[1] > 1 else [0]
    ev = _ratio(np.abs(vep - _blocks(ref["ve"][:, vcols], N)), _blocks(ref["bve"][:, vcols], N))
    line = f"{tag}: worst error / bound  g0 {e0:.2e}  g1 {e1:.2e}  ve per block {ev:.2e}"
    ed = None
    if dpp is not None:
        ed = _ratio(np.abs(dpp - _blocks(ref["dparam"][:, cols], N)), _blocks(ref["bdp"][:, cols], N))
        line += f"  dparam per block {ed:.2e}"
    print(line)
    assert e0 < 1.0, tag
    assert e1 < 1.0, tag
    assert ev < 1.0, tag
    assert ed is None or ed < 1.0, tag
    assert np.all(k0[N:] == 0) and np.all(k1[N:] == 0), tag
    assert len(vep) == len(npp) == (N + 127) // 128, tag
    assert not npp.any(), tag


def _check_planted(tag, clean, planted, N, plants, col=None):
    """``clean`` / ``planted``: (g0, g1 [Np, P], ve_partial, dparam_partial or None, nonpos_partial).  ``plants``: (row, counted,
    poisoned) of the planted rows, in two blocks."""
    nb = (N + 127) // 128
    rows = [r for r, _, _ in plants]
    keep = np.ones(N, bool)
    keep[rows] = False
    for a, b in zip(clean[:2], planted[:2]):
        assert np.array_equal(a[:N][keep], b[:N][keep], equal_nan=True), tag
        assert np.array_equal(a[N:], b[N:], equal_nan=True), tag
    want = np.zeros(nb, np.int64)
    hit = np.zeros(nb, bool)
    for r, counted, poisoned in plants:
        want[r // 128] += counted
        hit[r // 128] = True
        if poisoned:
            sel = slice(None) if col is None else col
            assert np.isnan(planted[0][r, sel]).all() and np.isnan(planted[1][r, sel]).all(), (tag, r)
            assert np.isnan(planted[2][r // 128]), (tag, r)
    assert hit.sum() == 2, tag
    assert np.array_equal(planted[4] - clean[4], want), (tag, planted[4] - clean[4])
    for a, b in zip(clean[2:4], planted[2:4]):
        if a is not None:
            assert np.array_equal(a[~hit], b[~hit], equal_nan=True), tag


# ------------------------------------------------------------------------------------------------- the column maps: C-ABI
def _lik_id(name):
    B = pkg()._backend
    return dict(studentt=B.LIK_STUDENT_T, poisson=B.LIK_POISSON, gamma=B.LIK_GAMMA, ordinal=B.LIK_ORDINAL, hetero=B.LIK_HETERO,
                robustmax=B.LIK_MULTICLASS, softmax=B.LIK_SOFTMAX)[name]


def _wants_dparam(name, par):
    return name in ("studentt", "ordinal") or (name == "gamma" and par[1])


def _column_call(name, par, dtype, crop, bufs, N, want_dparam):
    """One launch on column COL of the [N, 3] buffers ``bufs`` (mean, var, Y): g0, g1 [Np, 3] (doubles), the three partials."""
    B = pkg()._backend
    lib = B.lib()
    Np = B.round_up(N)
    nb = Np // 128
    P = L.P_COLUMNS
    g0 = torch.full((Np, P), SENTINEL, dtype=dtype, device=DEV)
    g1 = torch.full((Np, P), SENTINEL, dtype=dtype, device=DEV)
    ve = torch.full((nb,), float("nan"), dtype=torch.float64, device=DEV)
    dpar = torch.full((nb,), float("nan"), dtype=torch.float64, device=DEV)
    bad = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
    sfx = "f64" if dtype == torch.float64 else "f32"
    off = COL * g0.element_size()
    ins = [b.data_ptr() + off for b in bufs]
    flag = _lik_id(name) | (0 if crop else B.LIK_NOCROP)
    stream = torch.cuda.current_stream().cuda_stream
    dp = dpar.data_ptr() if want_dparam else None
    if name == "ordinal":
        edges = torch.as_tensor(L.EDGES[par[0]], dtype=torch.float64, device=DEV)
        st = getattr(lib, f"tsvgp_lik_map_ordinal_{sfx}")(*ins, P, flag, edges.data_ptr(), len(L.EDGES[par[0]]), float(par[1]),
                                                          g0.data_ptr() + off, g1.data_ptr() + off, P, ve.data_ptr(), dp,
                                                          bad.data_ptr(), N, Np, stream)
    else:
        p0, p1 = (par[0], par[1]) if name == "studentt" else (par[0], 0.0)
        st = getattr(lib, f"tsvgp_lik_map_scalar_{sfx}")(*ins, P, flag, float(p0), float(p1), g0.data_ptr() + off, g1.data_ptr() + off,
                                                         P, ve.data_ptr(), dp, bad.data_ptr(), N, Np, stream)
    assert st == 0
    torch.cuda.synchronize()
    return _h(g0), _h(g1), ve.cpu().numpy(), (dpar.cpu().numpy() if want_dparam else None), bad.cpu().numpy().astype(np.int64)


def _column_bufs(mean, var, Y, dtype):
    """[N, 3] device buffers that hold column COL of the inputs and NaN in the two columns the launch must not read."""
    out = []
    for a in (mean, var, Y):
        buf = torch.full(a.shape, float("nan"), dtype=dtype, device=DEV)
        buf[:, COL] = _t(a[:, COL], dtype)
        out.append(buf)
    return out


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# rows 5 and 77 lie in block 0, row 899 in block 7: (row, field, value, counted, poisoned)
def _column_plants(name, par):
    if name == "ordinal":  # a label that is no integer in [0, K): counted, and ve, g0, g1 of the row are NaN
        return [(5, "var", 0.0, 1, False), (77, "Y", 1.5, 1, True), (899, "Y", float(par[0]), 1, True), (900, "mean", float("inf"), 1, False)]
    if name == "gamma":  # a target outside the support: counted, its ve is NaN
        return [(5, "var", 0.0, 1, False), (77, "Y", -2.0, 1, None), (899, "mean", float("nan"), 1, False), (900, "Y", float("nan"), 1, None)]
    return [(5, "var", 0.0, 1, False), (77, "var", -0.5, 1, False), (899, "mean", float("nan"), 1, False), (900, "mean", float("-inf"), 1, False)]


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "nocrop"])
@pytest.mark.parametrize("kind", ["f64", "f32"])
@pytest.mark.parametrize("name", L.COLUMN_MAPS)
def test_column_map(name, kind, crop):
    dtype = DTYPES[kind]
    for par in L.CASES[name]:
        mean, var, Y, _, ref = _reference(name, par, kind)
        N = len(mean)
        tag = f"{name} {par} {kind} {'crop' if crop else 'nocrop'} column {COL} of 3"
        bufs = _column_bufs(mean, var, Y, dtype)
        want = _wants_dparam(name, par)
        out = _column_call(name, par, dtype, crop, bufs, N, want)
        k0, k1, vep, dpp, npp = out
        _check(tag, ref, [COL], k0[:, [COL]], k1[:, [COL]], vep, dpp, npp, N, crop)
        other = [c for c in range(L.P_COLUMNS) if c != COL]
        assert np.all(k0[:, other] == SENTINEL) and np.all(k1[:, other] == SENTINEL), tag  # neither read (NaN) nor written
        assert _same(out, _column_call(name, par, dtype, crop, bufs, N, want)), tag
        if name == "ordinal":  # both sides of the crop are there
            g1c = ref["g1"][:, COL]
            assert (g1c - ref["b1"][:, COL] > -1e-8).sum() > 100 and (g1c + ref["b1"][:, COL] < -1e-8).sum() > 100, tag
    # planted bad rows, on the last parameter set
    plants = _column_plants(name, par)
    pb = [b.clone() for b in bufs]
    for r, field, value, _, _ in plants:
        pb[("mean", "var", "Y").index(field)][r, COL] = value
    bad = _column_call(name, par, dtype, crop, pb, N, want)
    _check_planted(tag + " planted", out, bad, N, [(r, c, p is True) for r, _, _, c, p in plants], col=COL)
    if name == "gamma":
        assert np.isnan(bad[2][0]) and np.isnan(bad[2][7]), tag  # ve of a target outside the support is NaN


def test_gamma_log_zero_in_the_shape_derivative():
    """Shape exactly 1 with dparam requested and a single y = 0 row (a legal Exponential target): the derivative contains log 0,
    so that block's dparam partial is -inf; the row is not counted, and every other partial and entry is bit for bit what the
    launch without that row gave."""
    for kind, dtype in DTYPES.items():
        mean, var, Y = L.inputs("gamma", (0.5, True), kind)  # (all targets positive)
        N, row = len(mean), 128 * 50 + 17
        bufs = _column_bufs(mean, var, Y, dtype)
        clean = _column_call("gamma", (1.0, True), dtype, True, bufs, N, True)
        assert np.isfinite(clean[3]).all() and not clean[4].any()
        bufs[2][row, COL] = 0.0
        out = _column_call("gamma", (1.0, True), dtype, True, bufs, N, True)
        assert out[3][50] == -np.inf and not out[4].any(), kind
        keep = np.ones(N, bool)
        keep[row] = False
        blk = np.arange(len(out[2])) != 50
        assert np.array_equal(out[0][:N][keep], clean[0][:N][keep]) and np.array_equal(out[1][:N][keep], clean[1][:N][keep])
        assert np.array_equal(out[2][blk], clean[2][blk]) and np.array_equal(out[3][blk], clean[3][blk])
        m_row = mean[row, COL]
        assert out[0][row, COL] == -1.0 and out[1][row, COL] == float(np.float32(-1e-8) if kind == "f32" else -1e-8)  # e = 0: g0 = -a, g1 cropped
        assert abs((out[2][50] - clean[2][50]) - (Y[row, COL] * np.exp(-m_row + 0.5 * var[row, COL]))) <= 1e-10 * (1 + abs(clean[2][50]))


# --------------------------------------------------------------------------------- the column maps: EStepEngine.lik_map
class _OrdinalParam:
    """What ``EStepEngine.lik_map`` reads of an Ordinal likelihood: the fp64 edges on the device and sigma."""

    def __init__(self, edges, sigma):
        self._edges, self.sigma = torch.as_tensor(edges, dtype=torch.float64, device=DEV), torch.tensor(float(sigma), dtype=torch.float64)

    def device_edges(self, device):
        return self._edges


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "nocrop"])
@pytest.mark.parametrize("kind", ["f64", "f32"])
@pytest.mark.parametrize("name", L.COLUMN_MAPS)
def test_column_map_through_the_engine(name, kind, crop):
    """Y [N, 3]: one launch per column, partials [3, Np / 128]."""
    B = pkg()._backend
    dtype = DTYPES[kind]
    eng = _engine(dtype)
    for par in L.CASES[name]:
        mean, var, Y, _, ref = _reference(name, par, kind)
        N, Np, P = len(mean), B.round_up(len(mean)), L.P_COLUMNS
        nb = Np // 128
        tag = f"{name} {par} {kind} {'crop' if crop else 'nocrop'} engine"
        if name == "ordinal":
            lik_param = _OrdinalParam(L.EDGES[par[0]], par[1])
        elif name == "gamma":
            lik_param = (par[0], 0.0) if par[1] else (1.0, 0.0, False)
        else:
            lik_param = (par[0], par[1] if name == "studentt" else 0.0)
        out = dict(g0=torch.full((Np, P), float("nan"), dtype=dtype, device=DEV), g1=torch.full((Np, P), float("nan"), dtype=dtype, device=DEV),
                   ve_partial=torch.full((P, nb), float("nan"), dtype=torch.float64, device=DEV),
                   nonpos_partial=torch.full((P, nb), -7, dtype=torch.int32, device=DEV))
        res = eng.lik_map(_t(mean, dtype), _t(var, dtype), _t(Y, dtype), _lik_id(name) | (0 if crop else B.LIK_NOCROP), lik_param, N, Np, **out)
        torch.cuda.synchronize()
        k0, k1 = _h(out["g0"]), _h(out["g1"])
        vep, npp = out["ve_partial"].cpu().numpy(), out["nonpos_partial"].cpu().numpy().astype(np.int64)
        want = _wants_dparam(name, par)
        assert (res.dparam is not None) == want, tag
        dpp = eng._get("scalar_dparam_partial", (P, nb), torch.float64).cpu().numpy() if want else None
        for c in range(P):
            _check(f"{tag} column {c}", ref, [c], k0[:, [c]], k1[:, [c]], vep[c], None if dpp is None else dpp[c], npp[c], N, crop)
        if want:
            assert abs(float(res.dparam) - dpp.sum()) <= 1e-12 * np.abs(dpp).sum(), tag  # the sum over the columns and blocks


# ---------------------------------------------------------------------------------------------------------- the coupled maps
def _coupled_call(name, par, dtype, crop, mean_t, var_t, Y_t, eps_t, N):
    B = pkg()._backend
    lib = B.lib()
    Np = B.round_up(N)
    nb = Np // 128
    C = mean_t.shape[1]
    g0 = torch.full((Np, C), float("nan"), dtype=dtype, device=DEV)
    g1 = torch.full((Np, C), float("nan"), dtype=dtype, device=DEV)
    ve = torch.full((nb,), float("nan"), dtype=torch.float64, device=DEV)
    bad = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
    sfx = "f64" if dtype == torch.float64 else "f32"
    flag = _lik_id(name) | (0 if crop else B.LIK_NOCROP)
    stream = torch.cuda.current_stream().cuda_stream
    ins = (mean_t.data_ptr(), var_t.data_ptr(), Y_t.data_ptr())
    outs = (g0.data_ptr(), g1.data_ptr(), ve.data_ptr(), bad.data_ptr())
    if name == "hetero":
        st = getattr(lib, f"tsvgp_lik_map_hetero_{sfx}")(*ins, flag, *outs, N, Np, stream)
    elif name == "robustmax":
        st = getattr(lib, f"tsvgp_lik_map_robustmax_{sfx}")(*ins, flag, C, L.ROBUSTMAX_EPS, *outs, N, Np, stream)
    else:
        st = getattr(lib, f"tsvgp_lik_map_softmax_{sfx}")(*ins, flag, C, int(par[1]), None, 0, eps_t.data_ptr(), *outs, N, Np, stream)
    assert st == 0
    torch.cuda.synchronize()
    return _h(g0), _h(g1), ve.cpu().numpy(), None, bad.cpu().numpy().astype(np.int64)


def _coupled_plants(name, par):
    """(row, field, column, value, counted, poisoned): what each kernel comment says it counts (hetero: a variance <= 0 of either
    latent; RobustMax: a row with a variance <= 0 or a non-finite mean; Softmax: every variance <= 0) and poisons (a label that
    is no integer in [0, C): ve, g0, g1 of the row NaN, not counted)."""
    if name == "hetero":
        return [(5, "var", 0, 0.0, 1, False), (77, "var", 1, -0.5, 1, False), (899, "var", 0, -1e-3, 1, False)]
    C = par[0]
    mean_row = (900, "mean", C - 1, float("nan"), 1, False) if name == "robustmax" else (900, "var", C - 1, -1.0, 1, False)
    return [(5, "var", 0, 0.0, 1, False), (77, "Y", 0, 1.5, 0, True), (899, "Y", 0, float(C), 0, True), mean_row]


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "nocrop"])
@pytest.mark.parametrize("kind", ["f64", "f32"])
@pytest.mark.parametrize("name", ["hetero", "robustmax", "softmax"])
def test_coupled_map(name, kind, crop):
    dtype = DTYPES[kind]
    for par in L.CASES[name]:
        mean, var, Y, eps, ref = _reference(name, par, kind)
        N, C = mean.shape
        tag = f"{name} {par} {kind} {'crop' if crop else 'nocrop'}"
        ts = [_t(a, dtype) for a in (mean, var, Y)]
        eps_t = None if eps is None else _t(eps, dtype)
        out = _coupled_call(name, par, dtype, crop, *ts, eps_t, N)
        _check(tag, ref, list(range(C)), *out, N, crop)
        assert _same(out, _coupled_call(name, par, dtype, crop, *ts, eps_t, N)), tag
        if name == "robustmax":  # a clipped variance: that derivative is exactly zero before the crop
            lab = Y[:, 0].astype(int)
            tiny = var < 10 * L.TINY_VAR
            assert tiny[np.arange(N), lab].sum() > 100 and (tiny.sum() - tiny[np.arange(N), lab].sum()) > 100, tag
            want = float(np.float32(-1e-8)) if kind == "f32" else -1e-8
            assert np.all(out[1][:N][tiny] == (want if crop else 0.0)), tag
        if name != "softmax" or par[1] in (1, 100):
            plants = _coupled_plants(name, par)
            pt = [t.clone() for t in ts]
            for r, field, c, value, _, _ in plants:
                pt[("mean", "var", "Y").index(field)][r, c] = value
            bad = _coupled_call(name, par, dtype, crop, *pt, eps_t, N)
            _check_planted(tag + " planted", out, bad, N, [(r, k, p) for r, _, _, _, k, p in plants])
