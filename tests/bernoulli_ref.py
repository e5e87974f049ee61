"""NumPy restatements of the Bernoulli (probit) Gauss-Hermite map of ``csrc/tsvgp_device.h`` and the input grid the
Gaussian / Bernoulli map tests share (tests/test_bernoulli_ref_cpu.py, tests/test_gpu_gauss_bern_map.py).

``bern_sums_f32``  the kernel's ``bern_sums_f`` in ``np.float32`` arithmetic: the node and weight tables of GH_XF / GH_WF, the
                   operation order of ``bern_point_f`` (the class probability from erfc of the SIGNED argument, never 1 - p), the
                   two five-pair partial sums the two threads of a row form, their sum in fp64 and g1 = a1 / (2 sd) in fp64 with
                   the fp64 sd.  erfc / exp / log are the correctly rounded fp32 values (evaluated in fp64 on the fp32 argument,
                   rounded once); the device's are not correctly rounded, and its compiler may contract a * b + c: the factor 4
                   of ``g1_bound`` is there for both.
``bern_sums_f64``  the kernel's ``bern_sums`` (fp64: p from erf, q = 1 - p), same node order and split.
``amplification``  S(m, v, y) / (2 sd),  S = sum_i w_i |l'(f_i)| |z_i|  over the 20 nodes: what one unit of relative rounding of
                   the summands of a1 = sum_i w_i l'(f_i) z_i costs in g1 = a1 / (2 sd).  The sum cancels down to O(sd) for
                   small sd while its summands do not, so the error of g1 grows as u / sd: a flat tolerance is the wrong rule.
``C_G1``           max |g1_restated - g1_oracle| / (u * amplification) of ``bern_sums_f32`` (u = 2^-24) on the grid below, measured
                   by tests/test_bernoulli_ref_cpu.py against ``oracle.Bernoulli``, never from the kernel: the constant of
                   ``g1_bound`` for BOTH types.  ``C_G1_F64`` is the same figure for ``bern_sums_f64`` (u = 2^-53), kept as a
                   record: it is larger (q = 1 - p keeps up to ten bits fewer of p, in the oracle's sums as well), but in fp64
                   4 C_G1 u S / (2 sd) <= 5.1e-11 on this grid, so the flat term 1e-10 (1 + |ref|) carries the bound there.
``grid``           (m, v, y): 97 means on [-12, 12] x the log-spaced variances (8 per decade) inside [vmin, vmax] x both classes,
                   in an order that alternates 128-row blocks of rows on the wrong side of the boundary (ve down to log 1e-3)
                   with blocks on the right side (ve near 0), cut so that the last block has a partial tail.
"""
import functools

import numpy as np
from scipy.special import erf, erfc

from oracle import tsvgp_oracle as O

U32, U64 = 2.0 ** -24, 2.0 ** -53
C_G1 = 11.6      # measured 11.54 (tests/test_bernoulli_ref_cpu.py prints it)
C_G1_F64 = 108.0  # measured 107.3; not used by any bound
G1_ROWS = 1e-6 / U32  # the constants are measured over rows with amplification > 1e-6 / 2^-24 = 16.8 (u32 * amplification > 1e-6)

# positive nodes of the 20-point rule times sqrt(2), weights / sqrt(pi): the digits of GH_X / GH_W in the kernel source
GH_X = np.array([3.46964157081355917e-01, 1.04294534880275114e+00, 1.74524732081412703e+00, 2.45866361117236787e+00,
                 3.18901481655339003e+00, 3.94396735065731630e+00, 4.73458133404605519e+00, 5.57873880589320148e+00,
                 6.51059015701365507e+00, 7.61904854167975909e+00])
GH_W = np.array([2.60793063449554885e-01, 1.61739333983999978e-01, 6.15063720639768968e-02, 1.39978374471010220e-02,
                 1.83010313108049002e-03, 1.28826279961929280e-04, 4.40212109023085101e-06, 6.12749025998292797e-08,
                 2.48206236231517553e-10, 1.25780067243792340e-13])
GH_XF = np.array([3.46964157e-01, 1.04294535e+00, 1.74524732e+00, 2.45866361e+00, 3.18901482e+00,
                  3.94396735e+00, 4.73458133e+00, 5.57873881e+00, 6.51059016e+00, 7.61904854e+00], np.float32)
GH_WF = np.array([2.60793063e-01, 1.61739334e-01, 6.15063721e-02, 1.39978374e-02, 1.83010313e-03,
                  1.28826280e-04, 4.40212109e-06, 6.12749026e-08, 2.48206236e-10, 1.25780067e-13], np.float32)

_f32 = np.float32


def _r32(fn, x):
    """The correctly rounded fp32 value of ``fn`` at the fp32 argument x."""
    return fn(x.astype(np.float64)).astype(np.float32)


def _bern_point_f32(f, y1, one_minus_p=False):
    jit = _f32(1e-3)
    c = _f32(1.0) - _f32(2.0) * jit
    if one_minus_p:  # NOT the kernel: the form its comment warns of, for tests/test_bernoulli_ref_cpu.py
        p1 = _f32(0.5) * _r32(erfc, -f * _f32(0.70710678)) * c + jit
        pp = np.where(y1, p1, _f32(1.0) - p1)
    else:
        pp = _f32(0.5) * _r32(erfc, np.where(y1, -f, f) * _f32(0.70710678)) * c + jit
    dp = (c * _f32(0.39894228)) * _r32(np.exp, _f32(-0.5) * f * f)
    return _r32(np.log, pp), np.where(y1, dp, -dp) / pp


def bern_sums_f32(m, v, y, one_minus_p=False):
    """(g0, g1, ve) of ``bern_sums_t<float>`` and the epilogue around it, for arrays of fp64-held (mean, var) and y in {0, 1}."""
    m64, v64 = np.asarray(m, np.float64), np.asarray(v, np.float64)
    y1 = np.asarray(y) == 1
    sd64 = np.sqrt(v64)
    mf, sd = m64.astype(np.float32), sd64.astype(np.float32)
    tot = [np.zeros(m64.shape), np.zeros(m64.shape), np.zeros(m64.shape)]
    for half in (0, 1):  # the two threads of a row: node pairs [0, 5) and [5, 10)
        a0, a1, av = (np.zeros(m64.shape, np.float32) for _ in range(3))
        for i in range(5 * half, 5 * half + 5):
            z, w = GH_XF[i], GH_WF[i]
            lp, dl = _bern_point_f32(mf + sd * z, y1, one_minus_p)
            av = av + w * lp
            a0 = a0 + w * dl
            a1 = a1 + w * dl * z
            lp, dl = _bern_point_f32(mf - sd * z, y1, one_minus_p)
            av = av + w * lp
            a0 = a0 + w * dl
            a1 = a1 - w * dl * z
        for s, a in zip(tot, (a0, a1, av)):
            s += a.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return tot[0], tot[1] / (2.0 * sd64), tot[2]


def _bern_point_f64(f, y1):
    jit = 1e-3
    p = 0.5 * (1.0 + erf(f * 0.70710678118654752440)) * (1.0 - 2.0 * jit) + jit
    dp = (1.0 - 2.0 * jit) * 0.39894228040143267794 * np.exp(-0.5 * f * f)
    q = 1.0 - p
    return np.log(np.where(y1, p, q)), np.where(y1, dp / p, -dp / q)


def bern_sums_f64(m, v, y):
    """(g0, g1, ve) of ``bern_sums`` (fp64) and the epilogue around it."""
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    y1 = np.asarray(y) == 1
    sd = np.sqrt(v)
    tot = [np.zeros(m.shape), np.zeros(m.shape), np.zeros(m.shape)]
    for half in (0, 1):
        a0, a1, av = (np.zeros(m.shape) for _ in range(3))
        for i in range(5 * half, 5 * half + 5):
            z, w = GH_X[i], GH_W[i]
            lp, dl = _bern_point_f64(m + sd * z, y1)
            av = av + w * lp
            a0 = a0 + w * dl
            a1 = a1 + w * dl * z
            lp, dl = _bern_point_f64(m - sd * z, y1)
            av = av + w * lp
            a0 = a0 + w * dl
            a1 = a1 - w * dl * z
        for s, a in zip(tot, (a0, a1, av)):
            s += a
    with np.errstate(divide="ignore", invalid="ignore"):
        return tot[0], tot[1] / (2.0 * sd), tot[2]


def amplification(m, v, y):
    """S / (2 sd) with S = sum_i w_i |l'(f_i)| |z_i| over the 20 nodes, l' = oracle.Bernoulli._dlogp."""
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    z, w = O.gh_points_and_weights(20)
    sd = np.sqrt(v)
    dl = O.Bernoulli()._dlogp(m[..., None] + sd[..., None] * z, np.asarray(y)[..., None])
    return np.sum(w * np.abs(dl) * np.abs(z), axis=-1) / (2.0 * sd)


def g1_bound(ref, m, v, y, base, u, c_g1=C_G1):
    """base (1 + |ref|) + 4 C_G1 u S / (2 sd): the bound on |g1 - ref| of a quadrature run with unit roundoff u."""
    return base * (1.0 + np.abs(ref)) + 4.0 * c_g1 * u * amplification(m, v, y)


def oracle_entries(m, v, y):
    """(g0, g1, ve) of ``oracle.Bernoulli`` entry by entry (any shape)."""
    m, v, y = (np.asarray(a, np.float64) for a in (m, v, y))
    lik = O.Bernoulli()
    g0, g1 = lik.variational_expectations_grads(m, v, y)
    return g0, g1, lik.variational_expectations(m[..., None], v[..., None], y[..., None])


V_PER_DECADE = 8


@functools.lru_cache(maxsize=None)
def grid(vmin=1e-8, vmax=100.0):
    """(m, v, y) [N] fp64, read-only.  The variances are those of the full 81-point grid on [1e-8, 100] that lie in [vmin, vmax]."""
    mg = np.linspace(-12.0, 12.0, 97)
    vg = 10.0 ** (np.arange(-8 * V_PER_DECADE, 2 * V_PER_DECADE + 1) / V_PER_DECADE)
    vg = vg[(vg >= vmin * (1 - 1e-12)) & (vg <= vmax * (1 + 1e-12))]
    y, m, v = (a.ravel() for a in np.meshgrid([0.0, 1.0], mg, vg, indexing="ij"))
    wrong = (2.0 * y - 1.0) * m < 0  # the mean on the other side of the boundary than the label: ve far below zero
    idx = [np.flatnonzero(wrong), np.flatnonzero(~wrong)]
    order, pos, side = [], [0, 0], 0
    while pos[0] < len(idx[0]) or pos[1] < len(idx[1]):  # 128 rows of one side, then 128 of the other
        if pos[side] < len(idx[side]):
            order.append(idx[side][pos[side]:pos[side] + 128])
            pos[side] += 128
        side ^= 1
    order = np.concatenate(order)
    if len(order) % 128 == 0:
        order = order[:-30]
    out = tuple(a[order].copy() for a in (m, v, y))
    for a in out:
        a.setflags(write=False)
    return out
