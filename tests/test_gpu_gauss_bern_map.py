"""The Gaussian and Bernoulli gradient maps (mean, var, y) -> (g0, g1, ve) at every one of their six sites in
``csrc/`` (``lik_eval`` of ``tsvgp_device.h``; the sites are in ``tsvgp_kernels.hip``, ``tsvgp_likmap.hip`` and ``tsvgp_vgp.hip``), entry by entry against the oracle over the whole range a fit feeds them:

    panel1_kernel epilogue     tsvgp_moments_*, mode 0 / 1                  test_moments_epilogue
    panel_kernel epilogue      tsvgp_moments_*, mode 2                      test_moments_epilogue
    lik_map_kernel             tsvgp_lik_map_*                              test_lik_map
    diag_site_step_kernel      tsvgp_diag_site_step_*                       test_diag_site_step
    vgp_rows_kernel            tsvgp_vgp_rows_f64                           test_vgp_rows
    mean_lik_kernel            tsvgp_moments_* with TSVGP_LIK_MEANONLY      test_mean_only

Inputs: the grid of tests/bernoulli_ref.py -- m in [-12, 12] (97 points) x v in [1e-8, 100] (8 per decade) x both classes, 15 714
rows in 123 blocks of 128 whose ve alternates between about -300 and about -2, the last block with a 98-row tail -- directly
where the entry takes (mean, var), and through designed operands (A[n, 0] = m_n, A[n, 1] = sqrt(kdiag - v_n), Tm = e_1 e_1^T,
gamma = e_0) where the kernel forms them itself, in two launches kdiag = 2.5 (v from 1e-8 in fp64, from 1e-3 in fp32: an fp32 q
resolves 2.4e-7 there) and kdiag = 100 (v from 1).  Gaussian: noise variances 1e-6, 0.3 and 1e7, residuals y - m up to 1e3.

Reference: ``oracle.Bernoulli`` / ``oracle.Gaussian`` in fp64 on the (mean, var) the kernel consumed or returned.  Bounds:
    g0, ve      base (1 + |ref|),  base = 1e-10 (fp64) / 1e-5 (fp32); ve per block against the block's own rows
    g1          base (1 + |ref|) + 4 C u S / (2 sd)      (tests/bernoulli_ref.py: ``g1_bound``; S = 0 for the Gaussian map)
    sites       base (1 + |ref|) + the step's own propagation of the two bounds above
with u the unit roundoff of the type the quadrature runs in and C the constant tests/test_bernoulli_ref_cpu.py measures on the
NumPy restatement of bern_sums_f against the oracle (C_G1 = 11.6), never on the device.  In every case:
rows at or past N of g0 / g1 exactly zero, nonpos_partial block by block, and one more launch with three planted v <= 0 in two
blocks: those blocks count them, every other entry and partial is bit for bit what the clean launch gave.

Worst observed error / bound on an MI355X (each case prints its own), Bernoulli | Gaussian:
    lik_map            fp64: g0 1.3e-4, g1 0.14, ve 5e-6 | g0, g1 exact, ve 7e-6       fp32: g0 0.029, g1 0.23, ve 5e-3 | g0 3e-3, g1 1.5e-3
    moments epilogue   fp64: g0 1.7e-4, g1 0.09, ve 5e-6 | g0, g1 exact, ve 5e-6       fp32: g0 0.028, g1 0.05, ve 8e-3 | g0 3e-3, g1 1.5e-3
    mean only          fp64: g0, g1 exact                                             fp32: g0 3e-3, g1 1.5e-3
    diag_site_step     fp64: lambda_1 0.08, lambda_2 0.09 | 1.6e-6, 1e-6              fp32: lambda_1 0.23, lambda_2 0.22 | 1.6e-6, 1e-6
    vgp_rows           fp64: lambda_1 0.08, lambda_2 0.10, ve 3e-6, E_q log t 4e-6 | lambda_1 2e-6, ve 4e-6, E_q log t 4e-6

Scratch mutants of the kernel source, each built beside the product and never committed (first failing assertion here | the
tests that existed before this module and reach the mutated code):
    1  lik_map_kernel writes ve_partial[blockIdx.x ^ 1]      ``_check_map``: ve per block, ratio 6e10 | pass (white model, entry, sharded)
    2  bern_point_f forms 1 - p in fp32                      ``_check_map``: g0, ratio 2.1 (every fp32 Bernoulli case) | pass
    3  GH_X[7] times (1 + 1e-6)                              SURVIVES: the node's weight is 6.1e-8 and |l'| <= 2 under the 1e-3 jitter,
       so the sums move by at most 7e-13 sd, under 1e-10 for every sd <= 10 | test_site_step_kernel_against_numpy fails at its
       1e-12 (3.3e-12), and the hetero / robustmax map tests, which read the same table, fail by orders of magnitude
    4  diag_site_step_kernel reads mean of row n + 1 for skh == 1   test_diag_site_step: lambda bounds, ratio 4e7 | test_gpu_sites.py fails too
"""
import functools

import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests import bernoulli_ref as R
from tests.helpers import pkg, relerr
from tests.sites_ref import t_SVGP_sites

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# dtype, the tolerance of tests/test_gpu_kernels.py for products, base of the map bounds, unit roundoff and C of the quadrature
TYPES = {"f64": (torch.float64, 1e-11, 1e-10, R.U64, R.C_G1), "f32": (torch.float32, 2e-5, 1e-5, R.U32, R.C_G1)}
NOISES = (1e-6, 0.3, 1e7)
RESIDUALS = np.array([0.0, 1e-3, -1.0, 30.0, -1e3, 0.25, 1e3, -7.0])
SCALE_T = (1.0, 0.5, 0.75)    # Tm[p][1, 1]: var_p = kdiag - SCALE_T[p]^2 (kdiag - v)
SCALE_G = (1.0, -0.5, 0.25)   # gamma[0, p]: mean_p = SCALE_G[p] m
PLANT = ((5, 0), (77, -1), (128 * 7 + 3, 0))  # (row, column) of the planted v <= 0: two in block 0, one in block 7
_ENGINES = {}


def _engine(dtype):
    if dtype not in _ENGINES:
        _ENGINES[dtype] = pkg().estep.EStepEngine(dtype, DEV)
    return _ENGINES[dtype]


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV).contiguous()


def _h(t):
    return t.double().cpu().numpy()


def _columns(x, P):
    """[N, P]: column p holds the grid rolled by 4999 p rows, so that an n * P + p slip lands on another grid point."""
    return np.stack([np.roll(x, -4999 * p) for p in range(P)], axis=1)


def _targets(lik, m, y, P):
    """Y [N, P]: the classes, or mean + a residual from RESIDUALS (another one in every row and column)."""
    if lik == "bernoulli":
        return _columns(y, P)
    n = np.arange(len(m))
    return m + RESIDUALS[(n[:, None] + 3 * np.arange(P)[None, :]) % len(RESIDUALS)]


def _blocks(x, N):
    """Sums over the rows of every 128-row block (and over the columns) of x [N, ...]."""
    return np.add.reduceat(np.asarray(x).reshape(N, -1).sum(axis=1), np.arange(0, N, 128))


def _reference(kind, lik, noise, mean, var, Y):
    """The oracle on fp64 (mean, var, Y) of any one shape: g0, g1 (not cropped), ve per entry and the three bounds."""
    base, u, c = TYPES[kind][2:]
    if lik == "bernoulli":
        g0, g1, ve = R.oracle_entries(mean, var, Y)
        b1 = R.g1_bound(g1, mean, var, Y, base, u, c)
    else:
        ol = O.Gaussian(variance=noise)
        g0, g1 = ol.variational_expectations_grads(mean, var, Y)
        ve = ol.variational_expectations(mean[..., None], var[..., None], Y[..., None])
        b1 = base * (1 + np.abs(g1))
    return dict(g0=g0, g1=g1, ve=ve, b0=base * (1 + np.abs(g0)), b1=b1, bve=base * (1 + np.abs(ve)))


@functools.lru_cache(maxsize=None)
def _direct_inputs(kind, lik, P):
    """The whole grid as the entries that take (mean, var) see it: fp64 copies of the values of type ``kind``, read-only."""
    m, v, y = R.grid()
    T = np.float64 if kind == "f64" else np.float32
    out = tuple(a.astype(T).astype(np.float64) for a in (_columns(m, P), _columns(v, P), _targets(lik, _columns(m, P), y, P)))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _direct_reference(kind, mapkind, lik, noise, P):
    """The oracle on ``_direct_inputs`` under the bounds of ``mapkind``: computed once for all the cases that share it."""
    ref = _reference(mapkind, lik, noise, *_direct_inputs(kind, lik, P))
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _check_map(tag, ref, k0, k1, vep, npp, var, N, crop):
    """g0, g1 [Np, P] entry by entry, the rows past N, ve_partial and nonpos_partial block by block.  Returns the worst ratios."""
    r1 = np.minimum(ref["g1"], -1e-8) if crop else ref["g1"]
    e0 = float(np.max(np.abs(k0[:N] - ref["g0"]) / ref["b0"]))
    e1 = float(np.max(np.abs(k1[:N] - r1) / ref["b1"]))
    ev = float(np.max(np.abs(vep - _blocks(ref["ve"], N)) / _blocks(ref["bve"], N)))
    print(f"{tag}: worst error / bound  g0 {e0:.2e}  g1 {e1:.2e}  ve per block {ev:.2e}")
    assert e0 < 1.0, tag
    assert e1 < 1.0, tag
    assert ev < 1.0, tag
    assert np.all(k0[N:] == 0) and np.all(k1[N:] == 0), tag
    assert len(vep) == len(npp) == (N + 127) // 128
    assert np.array_equal(npp, _blocks(var <= 0, N)), tag
    return e0, e1, ev


def _planted_blocks(N, P, entries):
    want = np.zeros((N + 127) // 128, dtype=np.int64)
    for r, _ in entries:
        want[r // 128] += 1
    return want


def _check_planted(tag, clean, planted, N, rows, nonpos_clean, nonpos_planted, want_extra, block_partials):
    """``clean`` / ``planted``: lists of per-row arrays [>= N, ...]; every row outside ``rows`` bit for bit the same.  The partials in
    ``block_partials`` (pairs of per-block arrays): the same outside the planted blocks."""
    keep = np.ones(N, bool)
    keep[list(rows)] = False
    for a, b in zip(clean, planted):
        assert np.array_equal(a[:N][keep], b[:N][keep], equal_nan=True), tag
        assert np.array_equal(a[N:], b[N:], equal_nan=True), tag
    assert np.array_equal(nonpos_planted - nonpos_clean, want_extra), tag
    other = want_extra == 0
    assert other.sum() == len(want_extra) - 2
    for a, b in block_partials:
        assert np.array_equal(a[other], b[other], equal_nan=True), tag


# ---------------------------------------------------------------------------------------------------- (a) lik_map_kernel
@pytest.mark.parametrize("crop", [True, False], ids=["crop", "nocrop"])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("lik", ["bernoulli", "gaussian"])
@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_lik_map(kind, lik, P, crop):
    B = pkg()._backend
    dtype = TYPES[kind][0]
    eng = _engine(dtype)
    mean, var, Y = _direct_inputs(kind, lik, P)
    N, Np = len(mean), B.round_up(len(mean))
    nb = Np // 128
    mean_t, var_t, Y_t = _t(mean, dtype), _t(var, dtype), _t(Y, dtype)
    lik_id = (B.LIK_BERNOULLI if lik == "bernoulli" else B.LIK_GAUSSIAN) | (0 if crop else B.LIK_NOCROP)

    def run(var_in, noise):
        out = dict(g0=torch.full((Np, P), float("nan"), dtype=dtype, device=DEV), g1=torch.full((Np, P), float("nan"), dtype=dtype, device=DEV),
                   ve_partial=torch.full((nb,), float("nan"), dtype=torch.float64, device=DEV),
                   nonpos_partial=torch.full((nb,), -7, dtype=torch.int32, device=DEV))
        eng.lik_map(mean_t, var_in, Y_t, lik_id, noise, N, Np, **out)
        torch.cuda.synchronize()
        return _h(out["g0"]), _h(out["g1"]), out["ve_partial"].cpu().numpy(), out["nonpos_partial"].cpu().numpy().astype(np.int64)

    for noise in (NOISES if lik == "gaussian" else (0.0,)):
        tag = f"lik_map {kind} {lik} P={P} {'crop' if crop else 'nocrop'} noise={noise:g}"
        ref = _direct_reference(kind, kind, lik, noise, P)
        k0, k1, vep, npp = run(var_t, noise)
        _check_map(tag, ref, k0, k1, vep, npp, var, N, crop)
        if lik == "bernoulli":  # both sides of the crop, and the crop itself exactly
            above, below = ref["g1"] - ref["b1"] > -1e-8, ref["g1"] + ref["b1"] < -1e-8
            assert above.sum() > 1000 and below.sum() > 1000
            floor = -1e-8 if kind == "f64" else float(np.float32(-1e-8))  # the crop value as the output type holds it
            assert np.all(k1[:N][above] == floor) if crop else np.all(k1[:N][above] > -1e-8)
            assert np.all(k1[:N][below] < -1e-8)
    # three planted v <= 0 (0, -0.5, -1e-3) in blocks 0 and 7
    entries = [(r, c % P) for r, c in PLANT]
    var_p = var_t.clone()
    for (r, c), bad in zip(entries, (0.0, -0.5, -1e-3)):
        var_p[r, c] = bad
    p0, p1, vep_p, npp_p = run(var_p, noise)
    _check_planted(tag, (k0, k1), (p0, p1), N, [r for r, _ in entries], npp, npp_p, _planted_blocks(N, P, entries), [(vep, vep_p)])


# ------------------------------------------------------------------------------------- (b) the fused epilogues of the moments
def _moments_operands(kind, kdiag, P):
    """(m, v, y) of the sub-grid kdiag - q resolves in the type, A [Np, 128], Tm [P, 128, 128], gamma [128, P]."""
    B = pkg()._backend
    lo, hi = ((1e-8 if kind == "f64" else 1e-3), 2.4) if kdiag == 2.5 else (1.0, 100.0)
    m, v, y = R.grid(lo, hi)
    N, Np = len(m), B.round_up(len(m))
    A = np.zeros((Np, 128))
    A[:N, 0], A[:N, 1] = m, np.sqrt(kdiag - v)
    Tm, gamma = np.zeros((P, 128, 128)), np.zeros((128, P))
    for p in range(P):
        Tm[p, 1, 1], gamma[0, p] = SCALE_T[p], SCALE_G[p]
    return m, v, y, N, Np, A, Tm, gamma


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["lower", "upper", "dense"])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("lik", ["bernoulli", "gaussian"])
@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_moments_epilogue(kind, lik, P, mode):
    B = pkg()._backend
    dtype, tol = TYPES[kind][:2]
    eng = _engine(dtype)
    lik_id = B.LIK_BERNOULLI if lik == "bernoulli" else B.LIK_GAUSSIAN
    for kdiag in (2.5, 100.0):
        m, v, y, N, Np, A, Tm, gamma = _moments_operands(kind, kdiag, P)
        nb = Np // 128
        A_t, Tm_t, g_t = _t(A, dtype), _t(Tm, dtype), _t(gamma, dtype)
        Y_t = _t(_targets(lik, m[:, None] * np.array(SCALE_G[:P]), y, P), dtype)
        Y = _h(Y_t)

        def run(A_in, noise):
            mean = torch.full((N, P), float("nan"), dtype=dtype, device=DEV)
            var = torch.full((N, P), float("nan"), dtype=dtype, device=DEV)
            g0 = torch.full((Np, P), float("nan"), dtype=dtype, device=DEV)
            g1 = torch.full((Np, P), float("nan"), dtype=dtype, device=DEV)
            vep = torch.full((nb,), float("nan"), dtype=torch.float64, device=DEV)
            npp = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
            B.check(eng._fn("tsvgp_moments")(A_in.data_ptr(), Tm_t.data_ptr(), g_t.data_ptr(), Y_t.data_ptr(), kdiag, lik_id, noise,
                                             mean.data_ptr(), var.data_ptr(), g0.data_ptr(), g1.data_ptr(), vep.data_ptr(),
                                             npp.data_ptr(), N, Np, 128, P, mode, eng._stream()), "moments")
            torch.cuda.synchronize()
            return _h(mean), _h(var), _h(g0), _h(g1), vep.cpu().numpy(), npp.cpu().numpy().astype(np.int64)

        Ah, Th, gh = _h(A_t)[:N], _h(Tm_t), _h(g_t)
        mref = Ah @ gh
        Cq = np.einsum("nj,pij->pni", Ah, Th)
        vref = kdiag - np.sum(Cq * Cq, axis=-1).T
        for noise in (NOISES if lik == "gaussian" else (0.0,)):
            tag = f"moments {kind} {lik} P={P} mode={mode} kdiag={kdiag:g} noise={noise:g}"
            mean, var, k0, k1, vep, npp = run(A_t, noise)
            assert relerr(mean, mref) < tol * 20, tag
            assert np.max(np.abs(var - vref)) < tol * 20 * kdiag, tag
            assert np.all(var > 0), tag
            _check_map(tag, _reference(kind, lik, noise, mean, var, Y), k0, k1, vep, npp, var, N, True)
        if kdiag != 2.5:
            continue
        # three planted rows with q = 1.21 kdiag (v < 0 under the first latent; a larger, positive v under the others)
        rows = [r for r, _ in PLANT]
        A_p = A_t.clone()
        A_p[rows, 1] = float(np.sqrt(1.21 * kdiag))
        out_p = run(A_p, noise)
        assert np.all(out_p[1][rows, 0] < -0.5) and np.all(out_p[1][rows, 1:] > 0), tag
        _check_planted(tag, (mean, var, k0, k1), out_p[:4], N, rows, npp, out_p[5],
                       _planted_blocks(N, P, [(r, 0) for r in rows]), [(vep, out_p[4])])


# ------------------------------------------------------------------------------------------------------ (c) mean_lik_kernel
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_mean_only(kind, P):
    """TSVGP_LIK_MEANONLY: the Gaussian g0, g1 on the mean grid (v = 0 inside the kernel), NaN ve partials, no bad rows."""
    B = pkg()._backend
    dtype, tol = TYPES[kind][:2]
    eng = _engine(dtype)
    m, v, y, N, Np, A, Tm, gamma = _moments_operands(kind, 100.0, P)
    nb = Np // 128
    A_t, g_t = _t(A, dtype), _t(gamma, dtype)
    Y_t = _t(_targets("gaussian", m[:, None] * np.array(SCALE_G[:P]), y, P), dtype)
    Y, mref = _h(Y_t), _h(A_t)[:N] @ _h(g_t)
    for noise in NOISES:
        tag = f"mean only {kind} P={P} noise={noise:g}"
        mean = torch.full((N, P), float("nan"), dtype=dtype, device=DEV)
        g0 = torch.full((Np, P), float("nan"), dtype=dtype, device=DEV)
        g1 = torch.full((Np, P), float("nan"), dtype=dtype, device=DEV)
        vep = torch.zeros(nb, dtype=torch.float64, device=DEV)
        npp = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
        B.check(eng._fn("tsvgp_moments")(A_t.data_ptr(), None, g_t.data_ptr(), Y_t.data_ptr(), 100.0, B.LIK_GAUSSIAN | B.LIK_MEANONLY, noise,
                                         mean.data_ptr(), None, g0.data_ptr(), g1.data_ptr(), vep.data_ptr(), npp.data_ptr(), N, Np, 128,
                                         P, 1, eng._stream()), "moments (mean only)")
        torch.cuda.synchronize()
        mean, k0, k1 = _h(mean), _h(g0), _h(g1)
        assert relerr(mean, mref) < tol * 20, tag
        ref = _reference(kind, "gaussian", noise, mean, np.zeros_like(mean), Y)
        e0 = float(np.max(np.abs(k0[:N] - ref["g0"]) / ref["b0"]))
        e1 = float(np.max(np.abs(k1[:N] - np.minimum(ref["g1"], -1e-8)) / ref["b1"]))
        print(f"{tag}: worst error / bound  g0 {e0:.2e}  g1 {e1:.2e}")
        assert e0 < 1.0 and e1 < 1.0, tag
        assert np.all(k0[N:] == 0) and np.all(k1[N:] == 0), tag
        assert torch.isnan(vep).all() and np.all(npp.cpu().numpy() == 0), tag


# ------------------------------------------------------------------------------------------------ (d) diag_site_step_kernel
@pytest.mark.parametrize("floor", [False, True], ids=["clear", "floor"])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("lik", ["bernoulli", "gaussian"])
@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_diag_site_step(kind, lik, P, floor):
    """The sites after one step against sites_ref's ``site_update`` on the oracle's g0, g1.  Bounds: the update is linear in
    (g0, g1) -- lambda_1' = (1 - lr) lambda_1 + lr (g0 - 2 g1 m), lambda_2' = max((1 - lr) lambda_2 - 2 lr g1, 2e-8) -- so
    |d lambda_1'| <= lr (b0 + 2 |m| b1) and |d lambda_2'| <= 2 lr b1 (the floor is 1-Lipschitz), plus base (1 + |ref|) for the
    update's own rounding.  ``floor``: half of the rows carry lambda_2 in [-2e-7, 1.2e-7], which puts the value under the crop
    on either side of -1e-8 wherever g1 is small (Bernoulli: the saturated rows; Gaussian: noise 1e7, g1 = -5e-8)."""
    B = pkg()._backend
    dtype = TYPES[kind][0]
    # the Gaussian map runs in fp64 under either type and its g0, g1 go into the fp64 sites without a rounding to T: fp64 bounds
    mapkind = "f64" if lik == "gaussian" else kind
    base = TYPES[mapkind][2]
    eng = _engine(dtype)
    mean, var, Y = _direct_inputs(kind, lik, P)
    N, Np, lr = len(mean), B.round_up(len(mean)), 0.6
    nb = Np // 128
    mean_t, var_t, Y_t = _t(mean, dtype), _t(var, dtype), _t(Y, dtype)
    rng = np.random.RandomState(11)
    l1, l2 = rng.randn(N, P), 0.5 + rng.rand(N, P)
    small = rng.rand(N, P) < 0.5
    if floor:
        l2 = np.where(small, rng.uniform(-2e-7, 1.2e-7, (N, P)), l2)
    lik_id = B.LIK_BERNOULLI if lik == "bernoulli" else B.LIK_GAUSSIAN
    sentinel = 7.0

    def run(var_in, noise):
        s1 = torch.full((Np, P), sentinel, dtype=torch.float64, device=DEV)
        s2 = s1.clone()
        s1[:N], s2[:N] = torch.as_tensor(l1), torch.as_tensor(l2)
        copies = [torch.full((Np, P), sentinel, dtype=dtype, device=DEV) for _ in range(2)] if kind == "f32" else []
        vep = torch.full((nb,), float("nan"), dtype=torch.float64, device=DEV)
        npp = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
        B.check(eng._fn("tsvgp_diag_site_step")(mean_t.data_ptr(), var_in.data_ptr(), Y_t.data_ptr(), lik_id, noise, lr, s1.data_ptr(),
                                                s2.data_ptr(), *[c.data_ptr() for c in copies], vep.data_ptr(), npp.data_ptr(), N, Np, P,
                                                eng._stream()), "diag_site_step")
        torch.cuda.synchronize()
        return s1.cpu().numpy(), s2.cpu().numpy(), vep.cpu().numpy(), npp.cpu().numpy().astype(np.int64), [_h(c) for c in copies]

    for noise in (NOISES if lik == "gaussian" else (0.0,)):
        tag = f"diag_site_step {kind} {lik} P={P} {'floor' if floor else 'clear'} noise={noise:g}"
        ref = _direct_reference(kind, mapkind, lik, noise, P)
        n1, n2 = t_SVGP_sites.site_update(l1, l2, mean, ref["g0"], ref["g1"], lr)
        b_l1 = base * (1 + np.abs(n1)) + lr * (ref["b0"] + 2 * np.abs(mean) * ref["b1"])
        b_l2 = base * (1 + np.abs(n2)) + 2 * lr * ref["b1"]
        k1, k2, vep, npp, copies = run(var_t, noise)
        e1, e2 = float(np.max(np.abs(k1[:N] - n1) / b_l1)), float(np.max(np.abs(k2[:N] - n2) / b_l2))
        ev = float(np.max(np.abs(vep - _blocks(ref["ve"], N)) / _blocks(ref["bve"], N)))
        print(f"{tag}: worst error / bound  lambda_1 {e1:.2e}  lambda_2 {e2:.2e}  ve per block {ev:.2e}")
        assert e1 < 1.0 and e2 < 1.0 and ev < 1.0, tag
        assert np.all(k1[N:] == sentinel) and np.all(k2[N:] == sentinel), tag  # rows at or past N are not touched
        assert np.all(npp == 0), tag
        under = (1 - lr) * (-0.5 * l2) + lr * ref["g1"]  # the value under the crop
        hi, lo = under - lr * ref["b1"] > -1e-8, under + lr * ref["b1"] < -1e-8
        assert np.all(k2[:N][hi] == 2e-8) and np.all(k2[:N][lo] > 2e-8), tag
        if floor and (lik == "bernoulli" or noise == 1e7):  # (g1 = -1 / (2 noise) of the other two noises is far below the crop)
            assert (hi & small).sum() > 500 and (lo & small).sum() > 500, tag
        for c, k in zip(copies, (k1, k2)):  # the fp32 copies of the new sites
            assert np.array_equal(c[:N], k[:N].astype(np.float32).astype(np.float64)) and np.all(c[N:] == sentinel), tag
    entries = [(r, c % P) for r, c in PLANT]
    var_p = var_t.clone()
    for (r, c), bad in zip(entries, (0.0, -0.5, -1e-3)):
        var_p[r, c] = bad
    out_p = run(var_p, noise)
    _check_planted(tag, [k1, k2] + copies, list(out_p[:2]) + out_p[4], N, [r for r, _ in entries], npp, out_p[3],
                   _planted_blocks(N, P, entries), [(vep, out_p[2])])


# ------------------------------------------------------------------------------------------------------ (e) vgp_rows_kernel
@pytest.mark.parametrize("lik", ["bernoulli", "gaussian"])
def test_vgp_rows(lik):
    """The grid through C and z: C[n, 0] = m_n / s, z = s e_0 (s = 1e3, so that the mean's column takes at most 1.44e-4 of q),
    C[n, 1] = sqrt(kdiag - v_n - C[n, 0]^2); K = 128, ldc = K + 2 with NaN in the two columns the kernel must not read.  New
    sites (beta = 0.5, never floored: lambda' = (1 - beta) lambda + beta (g0 - 2 g1 m | -2 g1)) under the propagated bounds of
    test_diag_site_step; ve and E_q log t = -1/2 lambda_2 ((lambda_1 / lambda_2 - m)^2 + v) of the old sites per block."""
    B = pkg()._backend
    kind, dtype, base = "f64", torch.float64, 1e-10
    eng = _engine(dtype)
    K, ldc, s, beta = 128, 130, 1e3, 0.5
    lik_id = B.LIK_BERNOULLI if lik == "bernoulli" else B.LIK_GAUSSIAN
    for kdiag in (2.5, 100.0):
        m, v, y = R.grid(*((1e-8, 2.4) if kdiag == 2.5 else (1.0, 80.0)))  # (v <= kdiag - C[n, 0]^2: the grid's 100 is out)
        N, Np = len(m), B.round_up(len(m))
        nb = Np // 128
        C = np.full((Np, ldc), np.nan)
        C[:, :K] = 0.0
        C[:N, 0] = m / s
        C[:N, 1] = np.sqrt(kdiag - v - C[:N, 0] ** 2)
        z = np.zeros(K)
        z[0] = s
        rng = np.random.RandomState(13)
        l1, l2 = rng.randn(Np), 0.1 + rng.rand(Np)
        Y = _targets(lik, m[:, None], y, 1)[:, 0]
        C_t, z_t, Y_t = _t(C, dtype), _t(z, dtype), _t(Y, dtype)

        def run(C_in, noise):
            l1t, l2t = _t(l1, dtype), _t(l2, dtype)
            mean = torch.full((N,), float("nan"), dtype=dtype, device=DEV)
            var = torch.full((N,), float("nan"), dtype=dtype, device=DEV)
            vep = torch.full((nb,), float("nan"), dtype=dtype, device=DEV)
            eqp = torch.full((nb,), float("nan"), dtype=dtype, device=DEV)
            npp = torch.full((nb,), -7, dtype=torch.int32, device=DEV)
            B.check(eng.lib.tsvgp_vgp_rows_f64(C_in.data_ptr(), ldc, z_t.data_ptr(), Y_t.data_ptr(), l1t.data_ptr(), l2t.data_ptr(), kdiag,
                                               lik_id, noise, beta, mean.data_ptr(), var.data_ptr(), vep.data_ptr(), eqp.data_ptr(),
                                               npp.data_ptr(), N, Np, K, eng._stream()), "vgp_rows")
            torch.cuda.synchronize()
            return [a.cpu().numpy() for a in (mean, var, l1t, l2t, vep, eqp)] + [npp.cpu().numpy().astype(np.int64)]

        mref, vref = C[:N, :K] @ z, kdiag - np.sum(C[:N, :K] ** 2, axis=1)
        for noise in (NOISES if lik == "gaussian" else (0.0,)):
            tag = f"vgp_rows {lik} kdiag={kdiag:g} noise={noise:g}"
            mean, var, k1, k2, vep, eqp, npp = run(C_t, noise)
            assert relerr(mean, mref) < 2e-10 and np.max(np.abs(var - vref)) < 2e-10 * kdiag, tag
            assert np.all(var > 0), tag
            ref = _reference(kind, lik, noise, mean, var, Y)
            n1 = (1 - beta) * l1[:N] + beta * (ref["g0"] - 2 * ref["g1"] * mean)
            n2 = (1 - beta) * l2[:N] + beta * (-2 * ref["g1"])
            b_l1 = base * (1 + np.abs(n1)) + beta * (ref["b0"] + 2 * np.abs(mean) * ref["b1"])
            b_l2 = base * (1 + np.abs(n2)) + 2 * beta * ref["b1"]
            eqt = -0.5 * l2[:N] * ((l1[:N] / l2[:N] - mean) ** 2 + var)
            e1, e2 = float(np.max(np.abs(k1[:N] - n1) / b_l1)), float(np.max(np.abs(k2[:N] - n2) / b_l2))
            ev = float(np.max(np.abs(vep - _blocks(ref["ve"], N)) / _blocks(ref["bve"], N)))
            eq = float(np.max(np.abs(eqp - _blocks(eqt, N)) / _blocks(base * (1 + np.abs(eqt)), N)))
            print(f"{tag}: worst error / bound  lambda_1 {e1:.2e}  lambda_2 {e2:.2e}  ve per block {ev:.2e}  E_q log t per block {eq:.2e}")
            assert e1 < 1.0 and e2 < 1.0 and ev < 1.0 and eq < 1.0, tag
            assert np.array_equal(k1[N:], l1[N:]) and np.array_equal(k2[N:], l2[N:]), tag  # rows at or past N are not touched
            assert np.all(npp == 0), tag
        if kdiag != 2.5:
            continue
        rows = [r for r, _ in PLANT]
        C_p = C_t.clone()
        C_p[rows, 1] = float(np.sqrt(1.21 * kdiag))
        out_p = run(C_p, noise)
        assert np.all(out_p[1][rows] < -0.5), tag
        _check_planted(tag, (mean, var, k1, k2), out_p[:4], N, rows, npp, out_p[6], _planted_blocks(N, 1, [(r, 0) for r in rows]),
                       [(vep, out_p[4]), (eqp, out_p[5])])
