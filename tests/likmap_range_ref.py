"""The shared inputs, restatement calls and bounds of the range tests of the maps of ``csrc/tsvgp_likmap.hip`` that came after
the Gaussian / Bernoulli pair: StudentT, Poisson, Gamma / Exponential, Ordinal (one latent per target column), the heteroskedastic
Gaussian, MultiClass / RobustMax and Softmax (coupled latents).  tests/test_likmap_range_cpu.py holds the restatements to the
mpmath fixtures of tests/golden/likmaps/ (tests/golden/likmaps/make_golden.py), tests/test_gpu_likmap_range.py the kernels to the
restatements.

Grid: ``bernoulli_ref.grid()`` as it is -- 97 means on [-12, 12] x v log-spaced 8 per decade in [1e-8, 100], 15 714 rows in 123
blocks of 128 with a 98-row tail.  Column c of a map over several latents takes the grid rolled by 4999 c rows (``columns``).

``CASES[map]``      the parameter sets of a map.
``inputs``          (mean, var, Y) of a parameter set as arrays of type ``kind`` hold them (fp64 copies, read-only).
``restate``         the NumPy restatement (tests/scalar_lik_ref.py, ordinal_gamma_ref.py, hetero_ref.py, robustmax_ref.py,
                    softmax_ref.py) on such inputs: g0, g1 (not cropped), ve and, where the map has one, the parameter derivative
                    ``dparam`` with ``dmag``, the sum of the magnitudes of its terms.
``bounds``          per entry: base (1 + |ref|) with base = 1e-10 in fp64 (the base of test_gpu_gauss_bern_map.TYPES) for g0, g1
                    and ve, base * dmag + 2^-1022 for dparam (Ordinal and RobustMax g1: plus 4 C u64 A); for fp32 arrays bound64 + 2^-23 |ref| + 2^-149: these kernels compute in fp64
                    and round each output once (2^-24 |ref|), the factor 2 is for the double rounding of a result that already
                    carries the fp64 error, the last term is the smallest fp32 subnormal.  ve and dparam never pass through the
                    array type (fp64 partials): their bounds are the fp64 ones for either kind.
``fixture_rows``    the thinned grid of a fixture: every corner of (m, v), the rows the map's own edges need, every ``stride``-th
                    row.

tests/test_likmap_range_cpu.py measures every restatement on its fixture rows (``C_FLAT`` below is the record).  The flat term
carries every output but the Ordinal g1, where the restatement alone takes 0.29 of it (K = 256, sigma = 0.7, m = 0, v = 1e-8: a
bin 0.067 sigma wide), and the RobustMax g1, where it takes 0.58 (C = 2, a clipped class at the labelled mean, v_y = 1e-8: summands
of size 3e6 that cancel to zero); those two bounds have the term 4 C u A of ``ordinal_amplification`` / ``robustmax_amplification``
with C = ``C_G1_ORDINAL`` / ``C_G1_ROBUSTMAX``.  Three
restatements were ill-conditioned where the earlier tests never looked and are not used here as they stood: the literal 20 x 20
grid of hetero_ref.py (``separated`` there takes its place), the RobustMax argument (m_y + z s_y) - m_c at s_c = 1e-5 (now
(m_y - m_c) + z s_y in robustmax_ref.py), and a parameter sum whose terms underflow (the floor of ``bdp``).
"""
import functools
import os

import numpy as np
from scipy.special import digamma, erfc

from tests import bernoulli_ref as R
from tests.hetero_ref import HeteroskedasticTFPConditional
from tests.ordinal_gamma_ref import FLOOR, JIT, Gamma, Ordinal, _times_density
from tests.robustmax_ref import MultiClass
from tests.scalar_lik_ref import Poisson, StudentT, _nodes
from tests.softmax_ref import Softmax, normals

BASE64 = 1e-10
DBL_MIN = 2.0 ** -1022  # a term of a parameter sum under the smallest fp64 normal is flushed: the floor of that bound
C_G1_ORDINAL = 1.5  # measured 1.445 (tests/test_likmap_range_cpu.py prints it)
C_G1_ROBUSTMAX = 1.9  # measured 1.859 (the same test), on ``robustmax_amplification``
AMP_ROWS = 0.01 * BASE64 / (4.0 * R.U64)  # C is measured over the rows whose amplification term reaches 1% of the flat base
ROLL = 4999
RESIDUALS = np.array([0.0, 0.05, -1.0, 30.0, -1e3, 0.25, 1e3, -7.0])
COUNTS = np.array([0.0, 1.0, 7.0, 1000.0])
GAMMA_Y = np.logspace(-3.0, 3.0, 13)
EDGES = {2: np.array([0.0]), 5: np.array([-1.5, -0.4, 0.3, 1.7]), 256: np.linspace(-6.0, 6.0, 255)}  # test_gpu_ordinal_gamma.EDGES
ROBUSTMAX_EPS = 1e-3
TINY_VAR = 1e-12  # the planted RobustMax variances: under the clip at 1e-10 (unlabelled class) and at 2 v < 1e-10 (labelled)
SOFTMAX_SEED, SOFTMAX_EVERY = 5, 12
HETERO_F32_VMAX = 10.0  # the noise latent's largest variance under fp32 arrays (``inputs``)
COLUMN_MAPS = ("studentt", "poisson", "gamma", "ordinal")
P_COLUMNS = 3

CASES = {
    "studentt": [(0.05, 2.5), (0.7, 3.0), (20.0, 30.0)],  # (scale, df)
    "poisson": [(0.01,), (0.5,), (10.0,)],  # binsize
    # (shape, dparam requested): at shape 1 without dparam, the Exponential arm, y = 0 goes in every 16th row
    "gamma": [(0.5, True), (1.0, False), (7.5, True)],
    "ordinal": [(K, s) for K in (2, 5, 256) for s in (0.05, 0.7, 3.0)],  # (bins, sigma)
    "hetero": [()],
    "robustmax": [(2,), (3,), (10,)],  # classes; epsilon 1e-3
    "softmax": [(C, S) for C in (2, 3, 5, 10, 32) for S in (1, 7, 64, 100)],  # (classes, samples): templates Q = 1, 1, 2, 4, 8
}
# Measured by tests/test_likmap_range_cpu.py on the restatements against the mpmath fixtures, never on the device: the worst
# |restatement - mpmath| / bound64 per map and output.  All are under the quarter that test asks for.
C_FLAT = {
    "studentt": dict(g0=2.5e-4, g1=1.3e-2, ve=4.6e-5, dparam=6.6e-5),
    "poisson": dict(g0=2.1e-5, g1=1.8e-5, ve=1.1e-4, dparam=0.0),
    "gamma": dict(g0=3.8e-5, g1=3.8e-5, ve=3.8e-5, dparam=2.3e-6),
    "ordinal": dict(g0=7.3e-5, g1=4.0e-2, ve=1.9e-5, dparam=8.6e-3),  # (g1: under the bound with the amplification term)
    "hetero": dict(g0=1.1e-4, g1=1.5e-2, ve=1.1e-4, dparam=0.0),
    "robustmax": dict(g0=1.2e-5, g1=9.6e-2, ve=2.8e-5, dparam=0.0),  # (g1: with its amplification term)
    "softmax": dict(g0=9.0e-6, g1=7.6e-4, ve=8.4e-6, dparam=0.0),
}


def columns(x, P):
    """[N, P]: column p holds the grid rolled by 4999 p rows, so that a row / column slip lands on another grid point."""
    return np.stack([np.roll(x, -ROLL * p) for p in range(P)], axis=1)


def _corners(m, v, means):
    gv = R.grid()[1]
    return np.flatnonzero(np.isin(m, means) & ((v == gv.min()) | (v == gv.max())))


def _cycle(values, N, P):
    n = np.arange(N)
    return np.asarray(values)[(n[:, None] + 3 * np.arange(P)[None, :]) % len(values)]


def _as_kind(kind, *arrays):
    T = np.float64 if kind == "f64" else np.float32
    out = tuple(np.ascontiguousarray(a).astype(T).astype(np.float64) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def inputs(name, par, kind="f64"):
    """(mean, var, Y): [N, 3] each for the column maps, [N, C] and Y [N, 1] for the coupled ones."""
    gm, gv, _ = R.grid()
    N = len(gm)
    if name in COLUMN_MAPS:
        m, v = columns(gm, P_COLUMNS), columns(gv, P_COLUMNS)
        if name == "studentt":
            y = m + par[0] * _cycle(RESIDUALS, N, P_COLUMNS)
        elif name == "poisson":
            y = _cycle(COUNTS, N, P_COLUMNS)
        elif name == "gamma":
            y = _cycle(GAMMA_Y, N, P_COLUMNS).copy()
            if par == (1.0, False):
                y[::16] = 0.0
        else:
            y = _cycle(np.arange(par[0], dtype=np.float64), N, P_COLUMNS)
        return _as_kind(kind, m, v, y)
    if name == "hetero":
        if kind == "f64":
            m1, v1 = np.roll(gm, -ROLL), np.roll(gv, -ROLL)
        else:  # exp(-2 f1) leaves the fp32 range beyond: the grid's variances up to HETERO_F32_VMAX, repeated over the N rows
            sm, sv, _ = R.grid(1e-8, HETERO_F32_VMAX)
            m1, v1 = np.resize(np.roll(sm, -ROLL), N), np.resize(np.roll(sv, -ROLL), N)
        y = gm + _cycle(RESIDUALS, N, 1)[:, 0] * np.exp(m1)
        return _as_kind(kind, np.stack([gm, m1], axis=1), np.stack([gv, v1], axis=1), y[:, None])
    if name == "robustmax":
        C = par[0]
        m, v = columns(gm, C), columns(gv, C).copy()
        n = np.arange(N)
        y = n % C
        other, own = n[5::37], n[11::41]
        v[other, (y[other] + 1) % C] = TINY_VAR
        v[own, y[own]] = TINY_VAR
        # every second row with a clipped unlabelled class gives that class the labelled mean: d = z s_y / 1e-5 is then moderate
        # at the grid's small v_y, the node terms do not vanish and the UNCLIPPED derivative would be of size 1 / 1e-10 (with
        # the means a grid step or more apart every cdf saturates and the derivative is zero with or without the clip)
        m = m.copy()
        m[other[::2], (y[other[::2]] + 1) % C] = m[other[::2], y[other[::2]]]
        return _as_kind(kind, m, v, y[:, None].astype(np.float64))
    if name == "softmax":
        C = par[0]
        keep = np.unique(np.concatenate([np.arange(0, N, SOFTMAX_EVERY), _corners(gm, gv, (-12.0, 12.0))]))  # every 12th row + corners
        m, v = columns(gm, C)[keep], columns(gv, C)[keep]
        return _as_kind(kind, m, v, (np.arange(len(m)) % C)[:, None].astype(np.float64))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _softmax_eps_all(C, kind):
    N = len(inputs("softmax", (C, 1))[0])
    return _as_kind(kind, normals(SOFTMAX_SEED, 0, np.arange(N), max(S for _, S in CASES["softmax"]), C))[0]


def softmax_eps(par, kind="f64"):
    """epsilon [S, N, C] of ``softmax_ref.normals`` (seed 5, draw 0, rows 0 .. N - 1) as an array of type ``kind`` holds it (the
    draw of sample s does not depend on S: the first S samples of the largest count)."""
    return _softmax_eps_all(par[0], kind)[:par[1]]


def _ordinal_dmag(lik, Fmu, Fvar, Y):
    f, w, _, _ = _nodes(Fmu, Fvar)
    a, b, s = lik._ab(f, np.asarray(Y, np.float64)[..., None])
    mag = (1 - 2 * JIT) * (np.abs(_times_density(a)) + np.abs(_times_density(b))) / (s * (lik._phi(a, b) + FLOOR))
    return np.sum(w * mag, axis=-1)


def ordinal_amplification(lik, Fmu, Fvar, Y):
    """A of the Ordinal g1 = sum_i w_i l'(f_i) z_i / (2 sd): what one unit of relative rounding costs.  The summands cancel down to
    O(sd) (``bernoulli_ref.amplification``: S / (2 sd), S = sum_i w_i |l'(f_i)| |z_i|), and the arguments a = (edge - f) / sigma
    carry the rounding of edge - m, u (|m| + |edge|), into l' through l'' = (d l / d sigma) / sigma - l'^2:
        A = sum_i w_i |z_i| (|l'(f_i)| kappa_i + L2(f_i) (|m| + |edge|)) / (2 sd),
        L2 = (1 - 2e-3) (|a N(a)| + |b N(b)|) / (sigma^2 q) + l'^2,   kappa = ((1 - 2e-3) (Q_1 + Q_2) / 2 + 1e-6) / q >= 1,
    |edge| the larger finite edge of the row's bin and kappa the condition of q = phi + 1e-6 as the difference of the two erfc
    values Q_1, Q_2 it is formed from (a narrow bin near the mean: two values of size 1/2 whose difference is the bin's mass)."""
    Fmu, Y = np.asarray(Fmu, np.float64), np.asarray(Y, np.float64)
    f, w, z, sd = _nodes(Fmu, Fvar)
    a, b, s = lik._ab(f, Y[..., None])
    q = lik._phi(a, b) + FLOOR
    flip = b > 0.0
    hi, lw = np.where(flip, -b, a), np.where(flip, -a, b)
    kappa = (0.5 * (1 - 2 * JIT) * (erfc(-hi / np.sqrt(2.0)) + erfc(-lw / np.sqrt(2.0))) + FLOOR) / q
    dl = np.abs(lik.dlog_prob_df(f, Y[..., None])) * kappa
    l2 = (1 - 2 * JIT) * (np.abs(_times_density(a)) + np.abs(_times_density(b))) / (s * s * q) + (dl / kappa) ** 2
    k = Y.astype(np.int64)
    up, lo = lik._up[k], lik._lo[k]
    edge = np.maximum(np.where(np.isfinite(up), np.abs(up), 0.0), np.where(np.isfinite(lo), np.abs(lo), 0.0))
    return np.sum(w * np.abs(z) * (dl + l2 * (np.abs(Fmu) + edge)[..., None]), axis=-1) / (2.0 * sd)


def robustmax_amplification(lik, Fmu, Fvar, Y):
    """A [N, C] of the RobustMax g1: the sums of the magnitudes of the summands of
        c != y:  g1_c = -kappa sum_i w_i P_i r_ci d_ci / (2 v_c),        c == y:  g1_y = kappa sum_i w_i P_i (sum_c r_ci / s_c) z_i / (2 s_y)
    (0 where the clip makes the derivative zero).  Both sums cancel: with m_c = m_y the arguments d = z s_y / s_c are odd in z and
    w P r nearly even, so the summands, of size kappa r / (s_c s_y), leave a value near zero -- exactly zero for C = 2, where
    P r = (1 - 2e-4) N(d).  A flat bound on the value says nothing about what their rounding leaves."""
    mu, var = np.asarray(Fmu, np.float64), np.asarray(Fvar, np.float64)
    N, C = mu.shape
    rows, k = np.arange(N), np.asarray(Y, np.float64).reshape(-1).astype(np.int64)
    z, w = np.concatenate([R.GH_X, -R.GH_X]), np.concatenate([R.GH_W, R.GH_W])
    kappa = np.log(1.0 - lik.epsilon) - np.log(lik.eps_k1)
    other = np.arange(C)[None, :] != k[:, None]
    mu_y, v_y = mu[rows, k], var[rows, k]
    clip_y, clip_c = 2.0 * v_y < 1e-10, var < 1e-10
    s_y = np.sqrt(np.where(clip_y, 0.5e-10, v_y))
    v_c = np.where(clip_c, 1e-10, var)
    s_c = np.sqrt(v_c)
    A = np.zeros((N, C))
    for i in range(20):
        d = ((mu_y[:, None] - mu) + (z[i] * s_y)[:, None]) / s_c
        cdf = 0.5 * erfc(-d / np.sqrt(2.0)) * (1.0 - 2e-4) + 1e-4
        r = (1.0 - 2e-4) * np.exp(-0.5 * d * d) / np.sqrt(2.0 * np.pi) / cdf
        wP = w[i] * np.prod(np.where(other, cdf, 1.0), axis=1)
        A += np.where(other & ~clip_c, kappa * wP[:, None] * r * np.abs(d) / (2.0 * v_c), 0.0)
        t = kappa * wP * np.sum(np.where(other, r / s_c, 0.0), axis=1)
        A[rows, k] += np.where(clip_y, 0.0, t * abs(z[i]) / (2.0 * s_y))
    return A


def restate(name, par, mean, var, Y, eps=None):
    """The restatement on fp64 (mean, var, Y) of the shapes of ``inputs`` (or any rows of them): a dict of g0, g1 (not cropped),
    ve [rows] (the coupled maps: one per row), dparam and dmag [rows, ...] or None."""
    mean, var, Y = (np.asarray(a, np.float64) for a in (mean, var, Y))
    dparam = dmag = amp = None
    with np.errstate(all="ignore"):
        if name == "studentt":
            lik = StudentT(*par)
            g0, g1 = lik.variational_expectations_grads(mean, var, Y)
            ve = lik.variational_expectations(mean, var, Y)
            dparam = lik.variational_expectations_dscale(mean, var, Y)
            f, w, _, _ = _nodes(mean, var)
            u = ((Y[..., None] - f) / lik.scale) ** 2 / lik.df
            dmag = np.sum(w * ((lik.df + 1.0) * u / (1.0 + u) + 1.0), axis=-1) / lik.scale
        elif name == "poisson":
            lik = Poisson(*par)
            g0, g1 = lik.variational_expectations_grads(mean, var, Y)
            ve = lik.variational_expectations(mean, var, Y)
        elif name == "gamma":
            lik = Gamma(par[0])
            g0, g1 = lik.variational_expectations_grads(mean, var, Y)
            ve = lik.variational_expectations(mean, var, Y)
            if par[1]:
                dparam = lik.variational_expectations_dshape(mean, var, Y)
                dmag = np.abs(mean) + abs(digamma(par[0])) + np.abs(np.log(Y))
        elif name == "ordinal":
            lik = Ordinal(EDGES[par[0]], par[1])
            g0, g1 = lik.variational_expectations_grads(mean, var, Y)
            ve = lik.variational_expectations(mean, var, Y)
            dparam = lik.variational_expectations_dsigma(mean, var, Y)
            dmag = _ordinal_dmag(lik, mean, var, Y)
            amp = ordinal_amplification(lik, mean, var, Y)
        elif name == "hetero":
            g0, g1, ve = HeteroskedasticTFPConditional().separated(mean, var, Y)  # (not the literal 20 x 20 grid: see there)
        elif name == "robustmax":
            lik = MultiClass(par[0], ROBUSTMAX_EPS)
            g0, g1 = lik.variational_expectations_grads(mean, var, Y)
            ve = lik.variational_expectations(mean, var, Y)
            amp = robustmax_amplification(lik, mean, var, Y)
        elif name == "softmax":
            lik = Softmax(par[0])
            g0, g1 = lik.variational_expectations_grads(mean, var, Y, epsilon=eps)
            ve = lik.variational_expectations(mean, var, Y, epsilon=eps)
        else:
            raise KeyError(name)
    return dict(g0=g0, g1=g1, ve=ve, dparam=dparam, dmag=dmag, amp=amp)


def bounds(ref, kind="f64"):
    """b0, b1, bve, bdp (None without a parameter derivative) for the entries of ``restate``'s dict."""
    flat = lambda x: BASE64 * (1.0 + np.abs(x))
    wide = (lambda x: flat(x) + 2.0 ** -23 * np.abs(x) + 2.0 ** -149) if kind == "f32" else flat
    b1 = wide(ref["g1"])
    if ref.get("amp") is not None:
        b1 = b1 + 4.0 * (C_G1_ORDINAL if ref["dparam"] is not None else C_G1_ROBUSTMAX) * R.U64 * ref["amp"]
    return dict(b0=wide(ref["g0"]), b1=b1, bve=flat(ref["ve"]),
                bdp=None if ref["dparam"] is None else BASE64 * ref["dmag"] + DBL_MIN)


def fixture_rows(name, par, count):
    """About ``count`` rows of ``inputs(name, par)``: the twelve rows at m in {-12, 0, 12} x v in {1e-8, 100} (both classes of
    the grid), the rows the map's own edges need, and every stride-th row of the rest."""
    mean, var, Y = inputs(name, par)
    N = len(mean)
    m0, v0 = mean[:, 0], var[:, 0]
    vmin, vmax = R.grid()[1].min(), R.grid()[1].max()
    corner = _corners(m0, v0, (-12.0, 0.0, 12.0))
    extra = []
    y0 = Y[:, 0]
    if name in ("poisson", "gamma", "ordinal", "robustmax", "softmax"):  # the smallest and the largest target at a corner of v
        for t in (y0.min(), y0.max()):
            for vv in (vmin, vmax):
                extra.append(np.flatnonzero((y0 == t) & (v0 == vv))[:1 if name == "softmax" else 2])
    if name == "studentt":  # the largest residuals of either sign and the zero one
        r = np.round((y0 - m0) / par[0], 6)
        for t in (0.0, 1e3, -1e3):
            for vv in (vmin, vmax):
                extra.append(np.flatnonzero((r == t) & (v0 == vv))[:2])
    if name == "gamma" and par == (1.0, False):
        extra.append(np.flatnonzero(y0 == 0.0)[:8])
    if name == "ordinal":  # bottom, interior, top and far-tail bins (all edges 17 sigma or more from the mean)
        K, sigma = par
        e = EDGES[K]
        near = np.min(np.abs(e[None, :] - m0[:, None]), axis=1)
        extra += [np.flatnonzero(y0 == 0)[:4], np.flatnonzero(y0 == K - 1)[:4], np.flatnonzero(near >= 17 * sigma)[:6],
                  np.flatnonzero((near < sigma) & (v0 < 1e-6))[:6], np.flatnonzero((near < sigma) & (v0 > 10))[:4]]
        if K > 2:
            extra.append(np.flatnonzero((y0 > 0) & (y0 < K - 1))[:4])
    if name == "robustmax":  # both planted clips
        extra += [np.flatnonzero(np.any(var == TINY_VAR, axis=1) & (var[np.arange(N), Y[:, 0].astype(int)] != TINY_VAR))[:8],
                  np.flatnonzero(var[np.arange(N), Y[:, 0].astype(int)] == TINY_VAR)[:8]]
    if name == "robustmax":  # a clipped class at the labelled mean under the labelled latent's smallest variances: sums that cancel
        lab = Y[:, 0].astype(int)
        c = (lab + 1) % par[0]
        same = (var[np.arange(N), c] == TINY_VAR) & (mean[np.arange(N), c] == mean[np.arange(N), lab])
        extra.append(np.flatnonzero(same & (var[np.arange(N), lab] < 1e-6))[:12])
    if name == "hetero":  # the corners of the noise latent too
        m1, v1 = mean[:, 1], var[:, 1]
        extra.append(np.flatnonzero(np.isin(m1, (-12.0, 12.0)) & ((v1 == v1.min()) | (v1 == v1.max()))))
    fixed = np.unique(np.concatenate([corner] + extra))
    assert len(fixed) < count, (name, par, len(fixed))
    stride = N // (count - len(fixed)) + 1
    rest = np.setdiff1d(np.arange(stride // 2, N, stride), fixed)
    spare = np.setdiff1d(np.arange(stride // 2 + 1, N, stride), fixed)  # (a thinned row that was a fixed one already)
    rows = np.unique(np.concatenate([fixed, rest, spare[:count - len(fixed) - len(rest)]]))
    assert len(rows) == count, (name, par, len(rows))
    return rows


def fixture(name):
    """[(par, dict)] of tests/golden/likmaps/<name>.npz: rows, mean, var, Y, g0, g1, ve and dparam (or None) per parameter set."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "likmaps", name + ".npz"))
    out = []
    for i, par in enumerate(CASES[name]):
        got = {k: (z[f"{k}_{i}"] if f"{k}_{i}" in z.files else None) for k in ("rows", "mean", "var", "Y", "g0", "g1", "ve", "dparam")}
        for k in ("rows", "mean", "var", "Y"):  # Softmax: the inputs stand with the first sample count of a class count
            if got[k] is None:
                got[k] = out[-1][1][k]
        assert np.array_equal(z[f"params_{i}"], [float(x) for x in par]), (name, par)
        out.append((par, got))
    return out
