"""``EStepEngine.lik_map``, the one host entry in front of the five C-ABI likelihood maps (``tsvgp_lik_map*``):

(a) for every likelihood id, both compute dtypes, a full row tile and a second tile with two live rows, with and without the
    LIK_NOCROP bit, the entry returns bit for bit what the matching C-ABI symbol writes into fresh buffers: the same kernel on the
    same inputs, so ``torch.equal`` and no tolerance;
(b) the launches of one ``natgrad_step`` and one ``elbo`` of ``t_SVGP`` under every likelihood, by name, against the counts the
    commit before the entry existed made for the same calls (``COUNTS``: recorded there, never from the code under test);
(c) the StudentT scale gradient travels in the result, so a Poisson pass on an engine that just ran a StudentT one carries none.
"""
import numpy as np
import pytest
import torch

from tests.helpers import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ["gaussian", "bernoulli", "hetero", "softmax3", "softmax5", "multiclass", "student", "poisson"]
_ENGINES = {}


def _engine(dtype):
    if dtype not in _ENGINES:
        _ENGINES[dtype] = pkg().estep.EStepEngine(dtype, DEV)
    return _ENGINES[dtype]


def _likelihood(kind):
    """(likelihood object, number of latents P, number of target columns)."""
    p = pkg()
    if kind == "gaussian":
        return p.Gaussian(variance=0.3), 2, 2
    if kind == "bernoulli":
        return p.Bernoulli(), 2, 2
    if kind == "hetero":
        return p.HeteroskedasticTFPConditional(), 2, 1
    if kind.startswith("softmax"):
        lik = p.Softmax(int(kind[-1]), seed=3)
        lik.num_monte_carlo_points = 8
        lik.row_offset = 5
        return lik, lik.latent_dim, 1
    if kind == "multiclass":
        return p.MultiClass(3), 3, 1
    if kind == "student":
        return p.StudentT(scale=0.7, df=3.0), 2, 2
    return p.Poisson(binsize=0.5), 2, 2


def _targets(kind, rng, N, P, cols):
    if kind in ("gaussian", "hetero", "student"):
        return rng.randn(N, cols)
    if kind == "bernoulli":
        return (rng.rand(N, cols) > 0.5).astype(np.float64)
    if kind == "poisson":
        return rng.choice([0.0, 1.0, 7.0], (N, cols))
    return rng.randint(0, P, (N, cols)).astype(np.float64)  # class labels


def _direct(kind, lik, lik_id, mean, var, Y, N, Np, state, stream):
    """The C-ABI symbol of ``kind`` on fresh buffers holding a sentinel: (g0, g1, ve_partial, nonpos_partial, dparam_partial)."""
    B = pkg()._backend
    lib = B.lib()
    T, P, nblk = mean.dtype, mean.shape[1], Np // 128
    sfx = B.suffix(T)
    fn = lambda name: getattr(lib, f"{name}_{sfx}")
    scalar = kind in ("student", "poisson")
    g0 = torch.full((Np, P), 7.0, dtype=T, device=DEV)
    g1 = torch.full((Np, P), 7.0, dtype=T, device=DEV)
    ve = torch.full((P, nblk) if scalar else (nblk,), 7.0, dtype=torch.float64, device=DEV)
    bad = torch.full((P, nblk) if scalar else (nblk,), 7, dtype=torch.int32, device=DEV)
    dpar = torch.full((P, nblk), 7.0, dtype=torch.float64, device=DEV) if kind == "student" else None
    m, v, y = mean.data_ptr(), var.data_ptr(), Y.data_ptr()
    outs = (g0.data_ptr(), g1.data_ptr(), ve.data_ptr(), bad.data_ptr())
    if kind in ("gaussian", "bernoulli"):
        st = fn("tsvgp_lik_map")(m, v, y, lik_id, float(lik.lik_param), *outs, N, Np, P, stream)
    elif kind == "hetero":
        st = fn("tsvgp_lik_map_hetero")(m, v, y, lik_id, *outs, N, Np, stream)
    elif kind.startswith("softmax"):
        st = fn("tsvgp_lik_map_softmax")(m, v, y, lik_id, P, int(lik.num_monte_carlo_points), state.data_ptr(), int(lik.row_offset),
                                         None, *outs, N, Np, stream)
    elif kind == "multiclass":
        st = fn("tsvgp_lik_map_robustmax")(m, v, y, lik_id, P, float(lik.epsilon), *outs, N, Np, stream)
    else:
        p0, p1 = lik.lik_param
        st, esz = 0, mean.element_size()
        for c in range(P):  # one launch per column, each with its own run of the partials
            st |= fn("tsvgp_lik_map_scalar")(m + c * esz, v + c * esz, y + c * esz, P, lik_id, p0, p1, outs[0] + c * esz,
                                             outs[1] + c * esz, P, ve[c].data_ptr(), None if dpar is None else dpar[c].data_ptr(),
                                             bad[c].data_ptr(), N, Np, stream)
    assert st == 0
    return g0, g1, ve, bad, dpar


@pytest.mark.parametrize("nocrop", [False, True], ids=["crop", "nocrop"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("N", [128, 130])
@pytest.mark.parametrize("kind", KINDS)
def test_entry_is_the_cabi_bit_for_bit(kind, N, dtype, nocrop):
    B = pkg()._backend
    eng = _engine(dtype)
    lik, P, cols = _likelihood(kind)
    rng = np.random.RandomState(N + len(kind))
    t = lambda a: torch.as_tensor(a, dtype=dtype, device=DEV).contiguous()
    mean, var, Y = t(rng.randn(N, P)), t(rng.uniform(0.05, 2.0, (N, P))), t(_targets(kind, rng, N, P, cols))
    Np = B.round_up(N)
    lik_id = lik.lik_id | (B.LIK_NOCROP if nocrop else 0)
    softmax = kind.startswith("softmax")
    state = lik.rng_state(DEV).clone() if softmax else None  # the [seed, draw] words in front of the entry's call
    draw0 = lik.draw if softmax else None

    res = eng.lik_map(mean, var, Y, lik_id, lik.lik_param, N, Np)
    g0, g1, ve, bad, dpar = _direct(kind, lik, lik_id, mean, var, Y, N, Np, state, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    assert torch.equal(res.g0, g0) and torch.equal(res.g1, g1)
    assert torch.equal(res.ve_partial, ve) and torch.equal(res.nonpos_partial, bad)
    assert not res.g0[N:].any() and not res.g1[N:].any()  # the rows at or past N come back zero
    assert torch.isfinite(res.g0).all() and torch.isfinite(res.g1).all() and not res.nonpos_partial.any()
    if softmax:  # one evaluation consumed one draw, on the host and in the device words
        assert lik.draw == draw0 + 1
        assert lik.rng_state(DEV).tolist() == [int(state[0]), int(state[1]) + 1]
    if kind == "student":
        assert res.dparam is not None and res.dparam.dim() == 0 and torch.equal(res.dparam, dpar.sum())
    else:
        assert res.dparam is None


def test_caller_owned_fp64_buffers_on_an_fp32_engine():
    """What ``lik_grads`` does: fp64 operands and fp64 output / partial buffers of the caller's, whatever the engine computes in."""
    B = pkg()._backend
    eng = _engine(torch.float32)
    lik, P, cols = _likelihood("bernoulli")
    N, Np = 130, 256
    rng = np.random.RandomState(1)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=DEV).contiguous()
    mean, var, Y = t(rng.randn(N, P)), t(rng.uniform(0.05, 2.0, (N, P))), t(_targets("bernoulli", rng, N, P, cols))
    own = dict(g0=torch.full((Np, P), 3.0, dtype=torch.float64, device=DEV), g1=torch.full((Np, P), 3.0, dtype=torch.float64, device=DEV),
               ve_partial=torch.full((2,), 3.0, dtype=torch.float64, device=DEV),
               nonpos_partial=torch.full((2,), 3, dtype=torch.int32, device=DEV))
    lik_id = lik.lik_id | B.LIK_NOCROP
    res = eng.lik_map(mean, var, Y, lik_id, lik.lik_param, N, Np, **own)
    assert all(getattr(res, k) is own[k] for k in own)
    g0, g1, ve, bad, _ = _direct("bernoulli", lik, lik_id, mean, var, Y, N, Np, None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(res.g0, g0) and torch.equal(res.g1, g1) and torch.equal(res.ve_partial, ve) and torch.equal(res.nonpos_partial, bad)


# ------------------------------------------------------------------------------------------------- launches per step
def _model(kind, separate=False):
    p = pkg()
    lik, P, cols = _likelihood(kind)
    if kind in ("gaussian", "bernoulli"):
        P = cols = 1
    rng = np.random.RandomState(7)
    N, M, D = 130, 16, 2
    X = rng.randn(N, D)
    Y = _targets(kind, rng, N, P, cols)
    Z = X[:M].copy()
    if separate:
        kernel = p.SeparateIndependent([p.SquaredExponential(1.0, 0.8 + 0.1 * i) for i in range(P)])
        Z = p.SharedIndependentInducingVariables(Z)
    else:
        kernel = p.SquaredExponential(1.0, 0.8)
    return p.t_SVGP(kernel, lik, Z, num_latent_gps=P, device=DEV), X, Y


def step_counts(kind, separate=False):
    """{call: {kernel name: launches}} of one ``natgrad_step`` (and, on a shared kernel, one ``elbo``) at N = 130, M = 16, D = 2."""
    m, X, Y = _model(kind, separate)
    eng = m._get_engine()
    eng.profile = {}
    out = {}
    m.natgrad_step((X, Y), lr=0.5)
    out["natgrad_step"] = {k: v[0] for k, v in sorted(eng.profile_summary().items())}
    if separate:
        assert eng.last_batched
    else:
        m.elbo((X, Y))
        out["elbo"] = {k: v[0] for k, v in sorted(eng.profile_summary().items())}
    return out


COUNT_CASES = [(k, False) for k in KINDS if k != "softmax5"] + [("hetero", True)]
# Recorded by ``step_counts`` on the commit before ``lik_map`` existed.  A number that differs is a fault of the code, not of this table.
COUNTS = {
    ("gaussian", False): {
        "natgrad_step": {"tsvgp_moments": 1, "tsvgp_potrf": 3, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 2, "tsvgp_site_accum": 1},
        "elbo": {"tsvgp_moments": 1, "tsvgp_potrf": 1, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 1},
    },
    ("bernoulli", False): {
        "natgrad_step": {"tsvgp_moments": 1, "tsvgp_potrf": 3, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 2, "tsvgp_site_accum": 1},
        "elbo": {"tsvgp_moments": 1, "tsvgp_potrf": 1, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 1},
    },
    ("hetero", False): {
        "natgrad_step": {"tsvgp_lik_map_hetero": 1, "tsvgp_moments": 1, "tsvgp_potrf": 3, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 2, "tsvgp_site_accum": 1},
        "elbo": {"tsvgp_lik_map_hetero": 1, "tsvgp_moments": 1, "tsvgp_potrf": 1, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 1},
    },
    ("softmax3", False): {
        "natgrad_step": {"tsvgp_lik_map_softmax": 1, "tsvgp_moments": 1, "tsvgp_potrf": 3, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 2, "tsvgp_site_accum": 1},
        "elbo": {"tsvgp_lik_map_softmax": 1, "tsvgp_moments": 1, "tsvgp_potrf": 1, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 1},
    },
    ("multiclass", False): {
        "natgrad_step": {"tsvgp_lik_map_robustmax": 1, "tsvgp_moments": 1, "tsvgp_potrf": 3, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 2, "tsvgp_site_accum": 1},
        "elbo": {"tsvgp_lik_map_robustmax": 1, "tsvgp_moments": 1, "tsvgp_potrf": 1, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 1},
    },
    ("student", False): {
        "natgrad_step": {"tsvgp_lik_map_scalar": 2, "tsvgp_moments": 1, "tsvgp_potrf": 3, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 2, "tsvgp_site_accum": 1},
        "elbo": {"tsvgp_lik_map_scalar": 2, "tsvgp_moments": 1, "tsvgp_potrf": 1, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 1},
    },
    ("poisson", False): {
        "natgrad_step": {"tsvgp_lik_map_scalar": 2, "tsvgp_moments": 1, "tsvgp_potrf": 3, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 2, "tsvgp_site_accum": 1},
        "elbo": {"tsvgp_lik_map_scalar": 2, "tsvgp_moments": 1, "tsvgp_potrf": 1, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 1},
    },
    ("hetero", True): {
        "natgrad_step": {"tsvgp_lik_map_hetero": 1, "tsvgp_moments": 1, "tsvgp_potrf": 4, "tsvgp_se_fill": 1, "tsvgp_se_fill(Kuu)": 4, "tsvgp_site_accum": 1},
    },
}


@pytest.mark.parametrize("kind,separate", COUNT_CASES, ids=[f"{k}{'-separate' if s else ''}" for k, s in COUNT_CASES])
def test_launch_counts_are_the_parents(kind, separate):
    got = step_counts(kind, separate)
    assert got == COUNTS[(kind, separate)]


# ------------------------------------------------------------------------------------------------- no stale dparam
def test_no_stale_dparam_after_a_student_t_pass():
    ms, X, Ys = _model("student")
    mp, _, Yp = _model("poisson")
    eng = ms._get_engine()
    mp._engine = eng  # the same engine under both models
    seen = []
    run = eng.run

    def recording_run(*a, **kw):
        st = run(*a, **kw)
        seen.append((kw.get("lik_id", 0) & 0xFF, st.dparam))
        return st

    eng.run = recording_run
    _, grads = ms.elbo_and_grads((X, Ys))
    assert "likelihood_scale" in grads
    B = pkg()._backend
    assert any(lik == B.LIK_STUDENT_T and d is not None for lik, d in seen)
    del seen[:]
    mp.elbo((X, Yp))
    assert [lik for lik, _ in seen] == [B.LIK_POISSON] and seen[0][1] is None
