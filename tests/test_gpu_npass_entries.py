"""The single launch sites of the two N-sized kernels of a pass: ``EStepEngine.moments`` (``tsvgp_moments_*`` /
``tsvgp_moments_batched_*``) and ``EStepEngine._site_sums`` (``tsvgp_site_accum_*`` / ``tsvgp_site_accum_batched_*``).

(a) ``moments`` returns bit for bit what the matching C-ABI symbol writes into fresh buffers -- both compute dtypes, both triangles,
    a full row tile and a second tile with two live rows, one and two column tiles, the shared operand (P = 1, 2) and the per-latent
    one (P = 2, 3), Gaussian and Bernoulli fused, the no-likelihood form of the mapped pass, with and without ``mean_only``;
(b) ``_site_sums`` likewise against the site-sum symbols with the slice count the engine chose, after the symbol itself has been
    seen to repeat bit for bit on one input;
(c) the launches of whole model calls, by name in launch order, against the sequences the commit before the entries existed made
    for the same calls (``SEQUENCES``: recorded there, never from the code under test).
The same kernel on the same input: every comparison is of bit patterns (a NaN ve partial of ``mean_only`` included), no tolerance.
"""
import numpy as np
import pytest
import torch

from tests.helpers import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
_ENGINES = {}


def _engine(dtype):
    if dtype not in _ENGINES:
        _ENGINES[dtype] = pkg().estep.EStepEngine(dtype, DEV)
    return _ENGINES[dtype]


def _same(a, b):
    """Equal bit for bit (NaN = NaN, -0 != 0)."""
    bits = {8: torch.int64, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def _operands(dtype, N, M, P, batched, seed):
    """A [Np, Mp] or [P, Np, Mp], Tm [P, Mp, Mp], gam [Mp, P] (padding zero), kdiag, Gaussian and Bernoulli targets [N, P].
    |a_n|^2 <= 1 and |Tm_p|_F^2 <= 1/4, so |Tm_p a_n|^2 <= 1/4 < kdiag: every predictive variance is positive."""
    B = pkg()._backend
    rng = np.random.RandomState(seed)
    Np, Mp = B.round_up(N), B.round_up(M)
    lead = (P,) if batched else ()
    A = np.zeros(lead + (Np, Mp))
    A[..., :N, :M] = rng.uniform(-1.0, 1.0, lead + (N, M)) / np.sqrt(M)
    Tm = np.zeros((P, Mp, Mp))
    Tm[:, :M, :M] = rng.uniform(-1.0, 1.0, (P, M, M)) * 0.5 / M
    gam = np.zeros((Mp, P))
    gam[:M] = rng.randn(M, P)
    t = lambda a: torch.as_tensor(a, dtype=dtype, device=DEV).contiguous()
    kdiag = [1.0 + 0.25 * p for p in range(P)] if batched else 1.0
    return t(A), t(Tm), t(gam), kdiag, t(rng.randn(N, P)), t((rng.rand(N, P) > 0.5).astype(np.float64))


def _outputs(dtype, N, Np, P, want_mean, want_var, want_g):
    full = lambda rows: torch.full((rows, P), 7.0, dtype=dtype, device=DEV)
    return dict(mean=full(N) if want_mean else None, var=full(N) if want_var else None, g0=full(Np) if want_g else None,
                g1=full(Np) if want_g else None)


def _direct_moments(eng, A, Tm, gam, kdiag, Y, flags, lik_param, N, mode, out):
    """The C-ABI symbol on fresh partial buffers holding the sentinel: (ve_partial, nonpos_partial)."""
    import ctypes

    Np, Mp = A.shape[-2:]
    P = gam.shape[1]
    ve = torch.full((Np // 128,), 7.0, dtype=torch.float64, device=DEV)
    bad = torch.full((Np // 128,), 7, dtype=torch.int32, device=DEV)
    ptr = lambda x: None if x is None else x.data_ptr()
    tail = (flags, lik_param, ptr(out["mean"]), ptr(out["var"]), ptr(out["g0"]), ptr(out["g1"]), ve.data_ptr(), bad.data_ptr(),
            N, Np, Mp, P, mode, torch.cuda.current_stream().cuda_stream)
    if A.dim() == 3:
        st = eng._fn("tsvgp_moments_batched")(A.data_ptr(), Np * Mp, Tm.data_ptr(), gam.data_ptr(), ptr(Y),
                                              (ctypes.c_double * P)(*kdiag), *tail)
    else:
        st = eng._fn("tsvgp_moments")(A.data_ptr(), Tm.data_ptr(), gam.data_ptr(), ptr(Y), kdiag, *tail)
    assert st == 0
    return ve, bad


@pytest.mark.parametrize("M", [128, 130])
@pytest.mark.parametrize("N", [128, 130])
@pytest.mark.parametrize("mode", ["upper", "lower"])
@DTYPES
def test_moments_is_the_cabi_bit_for_bit(dtype, mode, N, M):
    B = pkg()._backend
    eng = _engine(dtype)
    tri = B.TRI_UPPER if mode == "upper" else B.TRI_LOWER
    Np = B.round_up(N)
    for batched, P in ((False, 1), (False, 2), (True, 2), (True, 3)):
        A, Tm, gam, kdiag, Yg, Yb = _operands(dtype, N, M, P, batched, seed=N + M + P)
        # (lik_id, lik_param handed to the entry, Y, mean_only, the caller wants mean / var)
        cases = [(B.LIK_GAUSSIAN, 0.3, Yg, False, True), (B.LIK_GAUSSIAN, 0.3, Yg, True, True), (B.LIK_GAUSSIAN, 0.3, Yg, False, False),
                 (B.LIK_BERNOULLI, 0.0, Yb, False, True),
                 # the mapped pass's form: no Y, no g0 / g1, and a likelihood parameter the launch must not see
                 (B.LIK_NONE, 0.3, None, False, True), (B.LIK_NONE, 0.3, None, True, True)]
        for lik_id, lik_param, Y, mean_only, want in cases:
            fused = lik_id != B.LIK_NONE
            mine = _outputs(dtype, N, Np, P, want, want and not mean_only, fused)
            ref = _outputs(dtype, N, Np, P, want, want and not mean_only, fused)
            eng._get("ve_partial", (Np // 128,), torch.float64).fill_(7.0)  # what the direct call's fresh buffers hold
            eng._get("nonpos_partial", (Np // 128,), torch.int32).fill_(7)
            ve, bad = eng.moments(A, Tm, gam, kdiag, N, tri, lik_id=lik_id, lik_param=lik_param, mean_only=mean_only, Y=Y, **mine)
            ve_ref, bad_ref = _direct_moments(eng, A, Tm, gam, kdiag, Y, lik_id | (B.LIK_MEANONLY if mean_only else 0),
                                              lik_param if fused else 0.0, N, tri, ref)
            torch.cuda.synchronize()
            what = f"batched={batched} P={P} lik={lik_id} mean_only={mean_only} moments={want}"
            assert ve is eng._buf["ve_partial"] and bad is eng._buf["nonpos_partial"], what
            assert _same(ve, ve_ref) and _same(bad, bad_ref), what
            assert not bad.any(), what  # every variance is positive (and every mean finite under mean_only)
            for k in mine:
                assert (mine[k] is None) == (ref[k] is None) and (mine[k] is None or _same(mine[k], ref[k])), (what, k)
            if want:
                assert torch.isfinite(mine["mean"]).all() and (mean_only or (mine["var"] > 0).all()), what
            if fused:
                assert not mine["g0"][N:].any() and not mine["g1"][N:].any(), what  # the rows at or past N come back zero
                assert torch.isfinite(mine["g0"]).all() and torch.isfinite(mine["g1"]).all(), what


# ------------------------------------------------------------------------------------------------- site sums
def _site_inputs(dtype, N, M, P, batched, seed):
    B = pkg()._backend
    A = _operands(dtype, N, M, P, batched, seed)[0]
    rng = np.random.RandomState(seed + 1)
    Np = B.round_up(N)
    g0, g1 = np.zeros((Np, P)), np.zeros((Np, P))
    g0[:N], g1[:N] = rng.randn(N, P), -rng.uniform(0.1, 2.0, (N, P))
    t = lambda a: torch.as_tensor(a, dtype=dtype, device=DEV).contiguous()
    return A, t(g0), t(g1)


def _direct_site_sums(eng, A, g0, g1, P, nsplit):
    """The C-ABI symbol on fresh buffers holding a sentinel: (acc2 [P, Mp, Mp], acc1 [P, Mp])."""
    Np, Mp = A.shape[-2:]
    work = torch.empty(int(eng._fn("tsvgp_site_accum_work_bytes")(Mp, P, nsplit)), dtype=torch.uint8, device=DEV)
    acc2 = torch.full((P, Mp, Mp), 7.0, dtype=torch.float64, device=DEV)
    acc1 = torch.full((P, Mp), 7.0, dtype=torch.float64, device=DEV)
    tail = (g0.data_ptr(), g1.data_ptr(), acc2.data_ptr(), acc1.data_ptr(), work.data_ptr(), Np, Mp, P, nsplit,
            torch.cuda.current_stream().cuda_stream)
    if A.dim() == 3:
        st = eng._fn("tsvgp_site_accum_batched")(A.data_ptr(), Np * Mp, *tail)
    else:
        st = eng._fn("tsvgp_site_accum")(A.data_ptr(), *tail)
    assert st == 0
    return acc2, acc1


# (dtype, N, nsplit): slice counts that survive the engine's clamp Np / chunk rows (8 in fp64, 4 in fp32 at Np = 128)
SITE_CASES = [(torch.float64, 128, 1), (torch.float64, 130, 1), (torch.float64, 130, 2), (torch.float32, 128, 1), (torch.float32, 130, 1)]
SITE_FORMS = ((False, 1), (False, 2), (True, 2), (True, 3))


@pytest.mark.parametrize("M", [128, 130])
@pytest.mark.parametrize("dtype,N,nsplit", SITE_CASES, ids=[f"{'f64' if d == torch.float64 else 'f32'}-N{n}-ns{s}" for d, n, s in SITE_CASES])
def test_site_accum_symbol_repeats_bit_for_bit(dtype, N, nsplit, M):
    """What (b) rests on: two calls of the symbol on one input agree in every bit (fixed-order reduction, no atomics)."""
    eng = _engine(dtype)
    for batched, P in SITE_FORMS:
        A, g0, g1 = _site_inputs(dtype, N, M, P, batched, seed=N + M + P)
        a2, a1 = _direct_site_sums(eng, A, g0, g1, P, nsplit)
        b2, b1 = _direct_site_sums(eng, A, g0, g1, P, nsplit)
        torch.cuda.synchronize()
        assert _same(a2, b2) and _same(a1, b1), f"batched={batched} P={P}"


@pytest.mark.parametrize("M", [128, 130])
@pytest.mark.parametrize("dtype,N,nsplit", SITE_CASES, ids=[f"{'f64' if d == torch.float64 else 'f32'}-N{n}-ns{s}" for d, n, s in SITE_CASES])
def test_site_sums_is_the_cabi_bit_for_bit(dtype, N, nsplit, M):
    eng = _engine(dtype)
    eng.nsplit_override = nsplit
    try:
        for batched, P in SITE_FORMS:
            A, g0, g1 = _site_inputs(dtype, N, M, P, batched, seed=N + M + P)
            acc2, acc1 = eng._site_sums(A, g0, g1, P, M)
            ref2, ref1 = _direct_site_sums(eng, A, g0, g1, P, eng.nsplit_override)
            torch.cuda.synchronize()
            what = f"batched={batched} P={P}"
            assert acc2.shape == (P, M, M) and acc1.shape == (P, M), what
            assert _same(acc2, ref2[:, :M, :M]) and _same(acc1, ref1[:, :M]), what
            assert torch.isfinite(acc2).all() and torch.isfinite(acc1).all() and acc2.abs().sum() > 0, what
    finally:
        eng.nsplit_override = None


# ------------------------------------------------------------------------------------------------- launches of whole calls
SEQ_CASES = ["tsvgp-gaussian", "tsvgp-bernoulli", "hetero-separate-batched", "hetero-separate-per-latent", "white-single-product",
             "white-two-product", "sites", "full_cov"]


def launch_sequence(case):
    """{call: [[kernel name, launches], ...] in the order of each name's first launch} of the calls of ``case`` at N = 130, M = 16,
    D = 2 (``profile_summary`` keeps the launch order)."""
    p = pkg()
    rng = np.random.RandomState(7)
    N, M, D = 130, 16, 2
    X = rng.randn(N, D)
    Z = X[:M].copy()
    Yg, Yb = rng.randn(N, 1), (rng.rand(N, 1) > 0.5).astype(np.float64)
    se = lambda: p.SquaredExponential(1.0, 0.8)
    out = {}

    def record(eng, name, call):
        eng.profile = {}
        call()
        out[name] = [[k, v[0]] for k, v in eng.profile_summary().items()]

    if case in ("tsvgp-gaussian", "tsvgp-bernoulli", "full_cov"):
        gauss = case != "tsvgp-bernoulli"
        m = p.t_SVGP(se(), p.Gaussian(variance=0.3) if gauss else p.Bernoulli(), Z, device=DEV)
        data = (X, Yg if gauss else Yb)
        if case == "full_cov":
            m.natgrad_step(data, lr=0.5)
            record(m._get_engine(), "predict_f(full_cov=True)", lambda: m.predict_f(X, full_cov=True))
        else:
            record(m._get_engine(), "natgrad_step", lambda: m.natgrad_step(data, lr=0.5))
            record(m._get_engine(), "elbo", lambda: m.elbo(data))
    elif case.startswith("hetero"):
        kernel = p.SeparateIndependent([p.SquaredExponential(1.0, 0.8 + 0.1 * i) for i in range(2)])
        m = p.t_SVGP(kernel, p.HeteroskedasticTFPConditional(), p.SharedIndependentInducingVariables(Z), num_latent_gps=2, device=DEV)
        eng = m._get_engine()
        eng.batch_separate = case.endswith("batched")
        record(eng, "natgrad_step", lambda: m.natgrad_step((X, Yg), lr=0.5))
        assert eng.last_batched == case.endswith("batched")
    elif case.startswith("white"):
        m = p.t_SVGP_white(se(), p.Gaussian(variance=0.3), Z, num_data=N, device=DEV, projection="whitened")
        m._two_product = case == "white-two-product"
        record(m._get_engine(), "natgrad_step", lambda: m.natgrad_step((X, Yg), lr=0.5))
        assert m._two_product == (case == "white-two-product")
    else:
        m = p.t_SVGP_sites((X, Yg), se(), p.Gaussian(variance=0.3), Z, device=DEV)
        record(m._get_engine(), "natgrad_step", lambda: m.natgrad_step(lr=0.5))
    return out


# Recorded by ``launch_sequence`` on the commit before ``EStepEngine.moments`` existed.  A difference is a fault of the code, not of this table.
SEQUENCES = {
    "tsvgp-gaussian": {
        "natgrad_step": [["tsvgp_se_fill(Kuu)", 2], ["tsvgp_potrf", 3], ["tsvgp_se_fill", 1], ["tsvgp_moments", 1], ["tsvgp_site_accum", 1]],
        "elbo": [["tsvgp_se_fill(Kuu)", 1], ["tsvgp_potrf", 1], ["tsvgp_se_fill", 1], ["tsvgp_moments", 1]],
    },
    "tsvgp-bernoulli": {
        "natgrad_step": [["tsvgp_se_fill(Kuu)", 2], ["tsvgp_potrf", 3], ["tsvgp_se_fill", 1], ["tsvgp_moments", 1], ["tsvgp_site_accum", 1]],
        "elbo": [["tsvgp_se_fill(Kuu)", 1], ["tsvgp_potrf", 1], ["tsvgp_se_fill", 1], ["tsvgp_moments", 1]],
    },
    "hetero-separate-batched": {
        "natgrad_step": [["tsvgp_se_fill(Kuu)", 4], ["tsvgp_potrf", 4], ["tsvgp_se_fill", 1], ["tsvgp_moments", 1], ["tsvgp_lik_map_hetero", 1], ["tsvgp_site_accum", 1]],
    },
    "hetero-separate-per-latent": {
        "natgrad_step": [["tsvgp_se_fill(Kuu)", 4], ["tsvgp_potrf", 4], ["tsvgp_se_fill", 4], ["tsvgp_moments", 2], ["tsvgp_lik_map_hetero", 1], ["tsvgp_site_accum", 2]],
    },
    "white-single-product": {
        "natgrad_step": [["tsvgp_se_fill(Kuu)", 2], ["tsvgp_potrf", 3], ["tsvgp_se_fill", 1], ["tsvgp_trmm", 1], ["tsvgp_moments", 1], ["tsvgp_site_accum", 1]],
    },
    "white-two-product": {
        "natgrad_step": [["tsvgp_se_fill(Kuu)", 2], ["tsvgp_potrf", 2], ["tsvgp_se_fill", 1], ["tsvgp_trmm", 1], ["tsvgp_moments", 1], ["tsvgp_lik_map", 1], ["tsvgp_site_accum", 1]],
    },
    "sites": {
        "natgrad_step": [["tsvgp_se_fill", 1], ["tsvgp_site_accum", 1], ["tsvgp_se_fill(Kuu)", 2], ["tsvgp_potrf", 3], ["tsvgp_trmm", 1], ["tsvgp_moments", 1], ["tsvgp_diag_site_step", 1]],
    },
    "full_cov": {
        "predict_f(full_cov=True)": [["tsvgp_se_fill(Kuu)", 1], ["tsvgp_potrf", 1], ["tsvgp_se_fill", 1], ["tsvgp_trmm", 1], ["tsvgp_cov", 1]],
    },
}


@pytest.mark.parametrize("case", SEQ_CASES)
def test_launch_sequences_are_the_parents(case):
    assert launch_sequence(case) == SEQUENCES[case]
