"""The NumPy restatements the GPU range test compares the likelihood maps with (tests/likmap_range_ref.py: ``restate``), held to
the mpmath fixtures of tests/golden/likmaps/ (50 digits, tests/golden/likmaps/make_golden.py) on every fixture row: each is within
a QUARTER of the fp64 bound the GPU test grants the kernel, so three quarters of every bound are the kernel's own.  Also: the
fixtures' inputs lie on the shared grid and hold the corners and edge rows they were chosen for, and the fp32 sub-grid of the
heteroskedastic map keeps every reference output inside the fp32 range.

Each case prints its worst |restatement - mpmath| / bound per output; ``likmap_range_ref.C_FLAT`` records them.
"""
import numpy as np
import pytest

from tests import bernoulli_ref as R
from tests import likmap_range_ref as L

QUARTER = 0.25


def _ratio(err, bound):
    """max err / bound with 0 / 0 = 0 (an output that is exactly zero on both sides under a bound of zero)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert not np.isnan(err).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((err == 0) & (bound == 0), 0.0, err / bound)
    return float(np.max(r))


def _rows(name, par, fx):
    mean, var, Y = L.inputs(name, par)
    rows = fx["rows"]
    if name in L.COLUMN_MAPS:
        return mean[rows, 0], var[rows, 0], Y[rows, 0]
    return mean[rows], var[rows], Y[rows]


@pytest.mark.parametrize("name", list(L.CASES))
def test_restatement_within_a_quarter_of_the_bound_of_mpmath(name):
    worst = dict(g0=0.0, g1=0.0, ve=0.0, dparam=0.0)
    for par, fx in L.fixture(name):
        mean, var, Y = _rows(name, par, fx)
        eps = L.softmax_eps(par)[:, fx["rows"], :] if name == "softmax" else None
        ref = L.restate(name, par, mean, var, Y, eps)
        bnd = L.bounds(ref)
        line = []
        for key, b in (("g0", "b0"), ("g1", "b1"), ("ve", "bve"), ("dparam", "bdp")):
            if fx[key] is None:
                assert key == "dparam" and ref[key] is None
                continue
            assert np.all(np.isfinite(fx[key])), (name, par, key)
            r = _ratio(np.abs(ref[key] - fx[key]), bnd[b])
            worst[key] = max(worst[key], r)
            line.append(f"{key} {r:.2e}")
            assert r <= QUARTER, (name, par, key, r)
        print(f"{name} {par}: |restatement - mpmath| / bound  " + "  ".join(line))
    print(f"{name}: worst over the parameter sets  " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    rec = L.C_FLAT[name]
    for key, r in worst.items():  # the record beside the bounds is the measurement (to its two digits), not a guess
        assert r <= rec[key] <= max(2.0 * r, 1e-6), (name, key, r, rec[key])


@pytest.mark.parametrize("name,const,flat_alone", [("ordinal", "C_G1_ORDINAL", 0.29), ("robustmax", "C_G1_ROBUSTMAX", 0.58)])
def test_amplification_constants(name, const, flat_alone):
    """C_G1_*: max |g1 restated - g1 mpmath| / (u64 A) over the fixture rows whose amplification term reaches 1% of the flat
    base, measured here on the restatement (never on the device), as ``bernoulli_ref.C_G1`` is.  Without the term the flat bound
    does not carry these two: the restatement alone takes ``flat_alone`` of it (Ordinal: K = 256, sigma = 0.7, m = 0, v = 1e-8,
    bin 176; RobustMax: C = 2, m = (8.25, 8.25), v = (1e-12, 1e-8), label 1, where the value is zero and the summands 3e6)."""
    worst, flat, rows = 0.0, 0.0, 0
    for par, fx in L.fixture(name):
        ref = L.restate(name, par, fx["mean"], fx["var"], fx["Y"])
        err, A = np.abs(ref["g1"] - fx["g1"]), ref["amp"]
        sel = A > L.AMP_ROWS
        c = float(np.max(err[sel] / (R.U64 * A[sel]))) if sel.any() else 0.0
        f = float(np.max(err / (L.BASE64 * (1 + np.abs(ref["g1"])))))
        print(f"{name} {par}: {sel.sum()} rows, C = {c:.3f}, |restatement - mpmath| / flat bound {f:.2e}")
        worst, flat, rows = max(worst, c), max(flat, f), rows + int(sel.sum())
    print(f"{const} measured {worst:.3f} on {rows} rows")
    assert rows >= 5
    assert worst <= getattr(L, const) <= 1.1 * worst
    assert flat_alone - 0.01 < flat < flat_alone + 0.01 and flat > QUARTER  # the flat term alone leaves the kernel no three quarters


@pytest.mark.parametrize("name", list(L.CASES))
def test_fixture_inputs_lie_on_the_grid_and_hold_the_corners(name):
    gm, gv, _ = R.grid()
    assert len(gm) == 15714 and len(gm) % 128 == 98
    for par, fx in L.fixture(name):
        mean, var, Y = _rows(name, par, fx)
        assert np.array_equal(fx["mean"], mean) and np.array_equal(fx["var"], var) and np.array_equal(fx["Y"], Y.reshape(fx["Y"].shape))
        planted = var == L.TINY_VAR if name == "robustmax" else np.zeros(var.shape, bool)
        assert np.isin(mean, gm).all() and np.isin(var[~planted], gv).all()
        m0, v0 = (mean, var) if mean.ndim == 1 else (mean[:, 0], var[:, 0])
        for mc in (-12.0, 12.0):
            for vc in (gv.min(), gv.max()):
                assert np.any((m0 == mc) & (v0 == vc)), (name, par, mc, vc)
        y = Y.reshape(len(m0))
        full = L.inputs(name, par)[2][:, 0]
        if name != "hetero":  # (its targets follow the mean and the noise latent)
            ymin, ymax = (full.min(), full.max()) if name != "studentt" else (None, None)
            if name == "studentt":
                r = np.round((y - m0) / par[0], 6)
                assert {0.0, 1e3, -1e3} <= set(r.tolist())
            else:
                assert ymin in y and ymax in y, (name, par)
        if name == "gamma":
            assert (0.0 in y) == (par == (1.0, False)) and y.min() >= 0.0
        if name == "ordinal":
            K, sigma = par
            near = np.min(np.abs(L.EDGES[K][None, :] - m0[:, None]), axis=1)
            assert 0 in y and K - 1 in y and np.any(near < sigma)
            far = np.min(np.abs(L.EDGES[K][None, :] - gm[:, None]), axis=1).max() >= 17 * sigma  # (no mean is 17 * 3 from an edge)
            assert np.any(near >= 17 * sigma) == far and (far or sigma > 0.05)
            assert K == 2 or np.any((y > 0) & (y < K - 1))
        if name == "robustmax":
            lab = var[np.arange(len(y)), y.astype(int)]
            assert np.any(lab == L.TINY_VAR) and np.any(planted.any(axis=1) & (lab != L.TINY_VAR))
            ok = var[~planted]  # no variance within a factor 2 of either clip threshold
            assert not np.any((ok > 0.25e-10) & (ok < 2e-10))


def test_grid_inputs_of_every_case():
    """The whole inputs: the column roll, the cycles of the targets, the planted RobustMax variances and Exponential zeros."""
    gm, gv, _ = R.grid()
    N = len(gm)
    for name, cases in L.CASES.items():
        for par in cases:
            for kind in ("f64", "f32"):
                mean, var, Y = L.inputs(name, par, kind)
                assert not (mean.flags.writeable or var.flags.writeable or Y.flags.writeable)
                if kind == "f32":
                    for a in (mean, var, Y):
                        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
                    continue
                if name != "softmax":
                    assert len(mean) == N and (name == "robustmax" or np.array_equal(mean[:, 0], gm))
                    if name not in ("hetero", "robustmax"):  # (RobustMax moves planted means onto the labelled one)
                        assert np.array_equal(mean[:, 1], np.roll(gm, -L.ROLL))
                assert np.isin(mean, gm).all() and np.isin(var[var != L.TINY_VAR], gv).all()
    mean, var, Y = L.inputs("robustmax", (3,))
    lab = Y[:, 0].astype(int)
    moved = mean[:, 1] != np.roll(gm, -L.ROLL)
    assert 50 < moved.sum() < 250 and np.all(var[moved, 1] == L.TINY_VAR) and np.all(mean[moved, 1] == mean[moved, lab[moved]])
    y = L.inputs("ordinal", (256, 0.7))[2]
    assert set(np.unique(y[:, 1]).tolist()) == set(range(256))
    y = L.inputs("gamma", (1.0, False))[2]
    assert np.all(y[::16] == 0.0) and np.count_nonzero(y == 0.0) == 3 * len(y[::16])
    assert np.all(L.inputs("gamma", (7.5, True))[2] > 0)
    assert len(L.inputs("softmax", (32, 100))[0]) % 128 not in (0, 127)
    assert L.softmax_eps((3, 7)).shape == (7, len(L.inputs("softmax", (3, 7))[0]), 3)


def test_hetero_fp32_subgrid_stays_in_range():
    """fp32 arrays: the noise latent on the grid's variances up to 10 keeps every reference output below 1e37 in magnitude, and
    the full grid would not (exp(-2 f1) at v1 = 100): the restriction is the type's, not the kernel's."""
    mean, var, Y = L.inputs("hetero", (), "f32")
    gm, gv, _ = R.grid()
    assert np.isin(mean.astype(np.float32), gm.astype(np.float32)).all() and np.isin(var.astype(np.float32), gv.astype(np.float32)).all()
    assert var[:, 1].max() == float(np.float32(gv[gv <= L.HETERO_F32_VMAX * (1 + 1e-12)].max())) and var[:, 0].max() == 100.0
    ref = L.restate("hetero", (), mean, var, Y)
    worst = max(float(np.max(np.abs(ref[k]))) for k in ("g0", "g1", "ve"))
    print(f"hetero fp32 sub-grid: largest |reference output| {worst:.2e}")
    assert worst < 1e37
    full = L.restate("hetero", (), *L.inputs("hetero", (), "f64"))
    assert max(float(np.max(np.abs(full[k]))) for k in ("g0", "g1", "ve")) > 1e38
