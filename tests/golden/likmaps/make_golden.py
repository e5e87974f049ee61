"""Writes tests/golden/likmaps/<map>.npz: the likelihood maps of csrc/tsvgp_likmap.hip evaluated in mpmath at 50 digits on a
thinned version of the grid of tests/likmap_range_ref.py, as the kernel comments define the operations -- for the quadrature maps
the 20-point Gauss-Hermite sum and the derivative OF THAT SUM, with the node and weight digits of tests/bernoulli_ref.py (GH_X,
GH_W), not the integral.  Nothing here is shared with the NumPy restatements but the inputs.  tests/test_likmap_range_cpu.py
compares the restatements with these files; no test imports mpmath.

Every file holds, for parameter set i of ``likmap_range_ref.CASES[map]``: params_i, rows_i [R] (row numbers of
``likmap_range_ref.inputs``), mean_i, var_i, Y_i (the inputs of those rows), g0_i, g1_i (not cropped), ve_i and, where the map has
one, dparam_i, all fp64 but the rows (Softmax: the inputs of a class count stand with its first sample count only).  The zip
members are stored with a fixed date, so a second run reproduces the files bit for bit.

Run from the repository root (a few minutes):  python tests/golden/likmaps/make_golden.py [map ...]
"""
import io
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from tests import likmap_range_ref as L  # noqa: E402
from tests.bernoulli_ref import GH_W, GH_X  # noqa: E402

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))
Z = [mp.mpf(float(x)) for x in GH_X] + [-mp.mpf(float(x)) for x in GH_X]  # the kernel's doubles, taken exactly
W = [mp.mpf(float(w)) for w in GH_W] * 2
ROWS = {"studentt": 250, "poisson": 250, "gamma": 250, "ordinal": 100, "hetero": 300, "robustmax": 100, "softmax": 16}
SQRT2, SQRT2PI = mp.sqrt(2), mp.sqrt(2 * mp.pi)
F = mp.mpf


def density(x):
    return mp.exp(-x * x / 2) / SQRT2PI


def tail(x):
    """Q(x) = 1 - Phi(x)."""
    return mp.erfc(x / SQRT2) / 2


def gh(m, v, point):
    """sum_i w_i point(f_i) over the 20 nodes f_i = m + sqrt(v) z_i, for a point function that returns a tuple; z with it."""
    sd = mp.sqrt(v)
    acc = None
    for z, w in zip(Z, W):
        val = point(m + sd * z, z)
        acc = [w * x for x in val] if acc is None else [a + w * x for a, x in zip(acc, val)]
    return acc, sd


def studentt(par, m, v, y):
    s, nu = F(par[0]), F(par[1])
    c0 = mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2) - mp.log(nu * mp.pi) / 2 - mp.log(s)

    def point(f, z):
        r = (y - f) / s
        u = r * r / nu
        dl = (nu + 1) * r / (s * nu * (1 + u))
        return c0 - (nu + 1) / 2 * mp.log1p(u), dl, dl * z, ((nu + 1) * u / (1 + u) - 1) / s

    (ve, a0, a1, ds), sd = gh(m, v, point)
    return a0, a1 / (2 * sd), ve, ds


def poisson(par, m, v, y):
    b = F(par[0])
    e = b * mp.exp(m + v / 2)
    return y - e, -e / 2, y * (m + mp.log(b)) - e - mp.loggamma(y + 1), None


def gamma(par, m, v, y):
    a = F(par[0])
    e = y * mp.exp(-m + v / 2)
    ve = -a * m - mp.loggamma(a) - e
    if a != 1:
        ve += (a - 1) * mp.log(y)
    return -a + e, -e / 2, ve, (-m - mp.digamma(a) + mp.log(y)) if par[1] else None


def ordinal(par, m, v, y):
    K, sigma = int(par[0]), F(par[1])
    edges = [F(float(e)) for e in L.EDGES[K]]
    k = int(y)
    up = None if k == K - 1 else edges[k]
    lo = None if k == 0 else edges[k - 1]
    c = 1 - F(2) / 1000

    def point(f, z):
        a = None if up is None else (up - f) / sigma
        b = None if lo is None else (lo - f) / sigma
        if b is not None and b > 0:  # Phi(a) - Phi(b) = Q(b) - Q(a): exact either way, this side keeps the digits
            mass = tail(b) - (0 if a is None else tail(a))
        else:
            mass = (1 if a is None else tail(-a)) - (0 if b is None else tail(-b))
        q = c * mass + F(1) / 1000000
        na, nb = (0 if a is None else density(a)), (0 if b is None else density(b))
        dl = -c * (na - nb) / (sigma * q)
        ds = -c * ((0 if a is None else a * na) - (0 if b is None else b * nb)) / (sigma * q)
        return mp.log(q), dl, dl * z, ds

    (ve, a0, a1, ds), sd = gh(m, v, point)
    return a0, a1 / (2 * sd), ve, ds


def hetero(par, m, v, y):
    m0, m1, v0, v1 = m[0], m[1], v[0], v[1]
    s1 = mp.sqrt(v1)
    W0 = sum(W)
    Q2 = sum(w * z * z for z, w in zip(Z, W))
    S1 = sum(w * mp.exp(-2 * (m1 + s1 * z)) for z, w in zip(Z, W))
    T1 = sum(w * z * mp.exp(-2 * (m1 + s1 * z)) for z, w in zip(Z, W))
    r = y - m0
    S0 = W0 * r * r + Q2 * v0
    ve = -mp.log(2 * mp.pi) / 2 * W0 * W0 - W0 * W0 * m1 - S0 * S1 / 2
    return [W0 * r * S1, S0 * S1 - W0 * W0], [-Q2 * S1 / 2, S0 * T1 / (2 * s1)], ve, None


def robustmax(par, m, v, y):
    C, k = int(par[0]), int(y)
    eps = F(L.ROBUSTMAX_EPS)
    clip, jit = F(1) / 10 ** 10, F(1) / 10 ** 4
    log_hit, log_miss = mp.log(1 - eps), mp.log(eps / (C - 1))
    kappa = log_hit - log_miss
    clip_y = 2 * v[k] < clip
    s_y = mp.sqrt(clip if clip_y else 2 * v[k]) / SQRT2  # X_i = m_y + z_i s_y
    clip_c = [v[c] < clip for c in range(C)]
    s = [mp.sqrt(clip if clip_c[c] else v[c]) for c in range(C)]
    others = [c for c in range(C) if c != k]
    p, g0, g1 = F(0), [F(0)] * C, [F(0)] * C
    for z, w in zip(Z, W):
        X = m[k] + z * s_y
        d = {c: (X - m[c]) / s[c] for c in others}
        cdf = {c: (1 - tail(d[c])) * (1 - 2 * jit) + jit for c in others}
        P = F(1)
        for c in others:
            P *= cdf[c]
        p += w * P
        tot = F(0)
        for c in others:
            r = (1 - 2 * jit) * density(d[c]) / cdf[c]
            g0[c] -= kappa * w * P * r / s[c]
            if not clip_c[c]:
                g1[c] -= kappa * w * P * r * d[c] / (2 * s[c] * s[c])
            tot += r / s[c]
        g0[k] += kappa * w * P * tot
        if not clip_y:
            g1[k] += kappa * w * P * tot * z / (2 * s_y)
    return g0, g1, p * log_hit + (1 - p) * log_miss, None


def softmax(par, m, v, y, eps):
    """eps [S][C] mpf."""
    C, S, k = int(par[0]), int(par[1]), int(y)
    sd = [mp.sqrt(x) for x in v]
    g0, g1, ve = [F(0)] * C, [F(0)] * C, F(0)
    for e in eps:
        f = [m[c] + sd[c] * e[c] for c in range(C)]
        mx = max(f)
        ex = [mp.exp(x - mx) for x in f]
        tot = sum(ex)
        ve += f[k] - mx - mp.log(tot)
        for c in range(C):
            d = (1 if c == k else 0) - ex[c] / tot
            g0[c] += d
            g1[c] += d * e[c]
    return [x / S for x in g0], [g1[c] / S / (2 * sd[c]) for c in range(C)], ve / S, None


POINT = dict(studentt=studentt, poisson=poisson, gamma=gamma, ordinal=ordinal, hetero=hetero, robustmax=robustmax, softmax=softmax)


def _mpf(a):
    a = np.asarray(a, np.float64)
    return F(float(a)) if a.ndim == 0 else [_mpf(x) for x in a]


def _f64(x):
    return [_f64(a) for a in x] if isinstance(x, (list, tuple)) else float(x)


def evaluate(name, par, rows):
    mean, var, Y = L.inputs(name, par)
    coupled = name not in L.COLUMN_MAPS
    eps = L.softmax_eps(par) if name == "softmax" else None
    out = dict(g0=[], g1=[], ve=[], dparam=[])
    for n in rows:
        m, v = (mean[n], var[n]) if coupled else (mean[n, 0], var[n, 0])
        args = (par, _mpf(m), _mpf(v), _mpf(Y[n, 0]))
        if eps is not None:
            args += (_mpf(eps[:, n, :]),)
        for key, val in zip(("g0", "g1", "ve", "dparam"), POINT[name](*args)):
            if val is not None:
                out[key].append(_f64(val))
    return {k: np.array(x, np.float64) for k, x in out.items() if x}


def save(path, arrays):
    """An .npz as np.savez writes it, members stored with a fixed date: the bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def build(name):
    per = []
    for par in L.CASES[name]:
        rows = L.fixture_rows(name, par, ROWS[name])
        mean, var, Y = L.inputs(name, par)
        coupled = name not in L.COLUMN_MAPS
        got = evaluate(name, par, rows)
        got.update(rows=rows.astype(np.int64), mean=mean[rows] if coupled else mean[rows, 0],
                   var=var[rows] if coupled else var[rows, 0], Y=Y[rows, 0], params=np.array([float(x) for x in par], np.float64))
        if name == "softmax" and par[1] != L.CASES[name][0][1]:  # the rows of a class count are those of its first sample count
            for key in ("rows", "mean", "var", "Y"):
                del got[key]
        per.append(got)
        print(f"{name} {par}: {len(rows)} rows", flush=True)
    arrays = {f"{k}_{i}": a for i, got in enumerate(per) for k, a in got.items()}  # shapes differ from set to set
    save(os.path.join(HERE, name + ".npz"), arrays)


if __name__ == "__main__":
    for name in (sys.argv[1:] or list(L.CASES)):
        build(name)
