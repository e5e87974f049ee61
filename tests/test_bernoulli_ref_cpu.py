"""The NumPy restatements of the Bernoulli quadrature (tests/bernoulli_ref.py) against ``oracle.Bernoulli`` on the grid of the
GPU map tests: m in [-12, 12] (97 points) x v in [1e-8, 100] (81 log-spaced points) x both classes.

What the GPU tests (tests/test_gpu_gauss_bern_map.py) take from here is the rule for g1,
    |g1 - oracle| <= base (1 + |oracle|) + 4 C u S / (2 sd),
and its constant C: the largest error of the restated arithmetic in units of u S / (2 sd), measured HERE against the oracle and
never on the device.  These tests hold the constants of the module to what the restatements measure, show that the restatements
themselves sit inside the flat bounds for g0 and ve and inside the g1 rule WITHOUT its factor 4 (which belongs to the device's
erfcf / expf / logf), and check the grid's own properties.
"""
import numpy as np
import pytest

from tests import bernoulli_ref as R

CASES = {"f32": (R.bern_sums_f32, R.U32, "C_G1", 1e-5), "f64": (R.bern_sums_f64, R.U64, "C_G1_F64", 1e-10)}


@pytest.fixture(scope="module")
def oracle():
    m, v, y = R.grid()
    out = R.oracle_entries(m, v, y) + (R.amplification(m, v, y),)
    for a in out:
        a.setflags(write=False)
    return out


def test_grid():
    m, v, y = R.grid()
    N = len(m)
    assert N == 97 * 81 * 2 == 15714 and N % 128 != 0 and N < 16384
    assert m.min() == -12.0 and m.max() == 12.0 and len(np.unique(m)) == 97
    assert np.isclose(v.min(), 1e-8, rtol=1e-12) and np.isclose(v.max(), 100.0, rtol=1e-12) and len(np.unique(v)) == 81
    assert set(np.unique(y)) == {0.0, 1.0}
    assert len({(a, b, c) for a, b, c in zip(m, v, y)}) == N  # every grid point once
    # neighbouring 128-row blocks carry very different ve: a partial written to the neighbouring block cannot hide
    ve = R.oracle_entries(m, v, y)[2]
    sums = np.array([ve[k:k + 128].sum() for k in range(0, N, 128)])
    assert np.all(np.abs(np.diff(sums))[:-1] > 50.0)  # (the two sides differ by 162 rows: the last full block and the tail share one)
    # the sub-grids of the fused kernels: the same variances, cut to what kdiag - q resolves
    for lo, hi in ((1e-8, 2.4), (1e-3, 2.4), (1.0, 100.0)):
        ms, vs, ys = R.grid(lo, hi)
        assert len(ms) % 128 != 0 and vs.min() >= lo * (1 - 1e-12) and vs.max() <= hi * (1 + 1e-12)
        assert set(np.unique(vs)) <= set(np.unique(v)) and len(np.unique(ms)) == 97 and set(np.unique(ys)) == {0.0, 1.0}


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_restatement_against_the_oracle(oracle, name):
    fn, u, cname, base = CASES[name]
    C = getattr(R, cname)
    m, v, y = R.grid()
    o0, o1, ove, amp = oracle
    g0, g1, ve = fn(m, v, y)
    e0 = np.max(np.abs(g0 - o0) / (1 + np.abs(o0)))
    ev = np.max(np.abs(ve - ove) / (1 + np.abs(ove)))
    rows = amp > R.G1_ROWS  # where u32 S / (2 sd) exceeds 1e-6: the same rows for both types
    c = np.max(np.abs(g1 - o1)[rows] / (u * amp[rows]))
    plain = np.max(np.abs(g1 - o1) / (base * (1 + np.abs(o1)) + R.C_G1 * u * amp))  # the GPU tests' rule without its factor 4
    print(f"{name}: g0 {e0:.2e} ve {ev:.2e} (flat bound {base:.0e}); c = {c:.2f} over {int(rows.sum())} rows ({cname} = {C}); "
          f"g1 / (base (1 + |ref|) + C_G1 u S / 2 sd) = {plain:.3f}")
    assert e0 < base and ev < base
    assert rows.sum() > 1000
    assert 0.9 * C < c <= C  # the module's constant IS the measured one
    assert C < 128  # a small constant: at most 7 bits (fp64: q = 1 - p gives up to 10 bits of p at q = 1e-3)
    assert plain < 1.0  # every grid row, without the factor 4 of the device's functions


def test_the_flat_fp32_tolerance_is_the_wrong_rule_for_g1(oracle):
    """The fp32 g1 error grows as 2^-24 / sd: a flat 1e-5 (1 + |ref|) fails below v = 1e-4 in correctly rounded fp32 arithmetic."""
    m, v, y = R.grid()
    err = np.abs(R.bern_sums_f32(m, v, y)[1] - oracle[1])
    flat = 1e-5 * (1 + np.abs(oracle[1]))
    assert np.all(err[v >= 1e-2] < flat[v >= 1e-2])
    assert np.any(err[v < 1e-4] > 4 * flat[v < 1e-4])


def test_one_minus_p_in_fp32_leaves_the_bound(oracle):
    """The hazard the kernel comments on: q = 1 - p formed in fp32 keeps four digits at p = 1 - 1e-3.  The restatement with that
    one change leaves the g0 bound of the GPU tests, so a 1 - p slipped back into bern_point_f cannot pass them."""
    m, v, y = R.grid()
    g0 = R.bern_sums_f32(m, v, y, one_minus_p=True)[0]
    worst = np.max(np.abs(g0 - oracle[0]) / (1 + np.abs(oracle[0])))
    print(f"1 - p in fp32: g0 error / (1 + |ref|) = {worst:.2e}")
    assert worst > 1e-5
