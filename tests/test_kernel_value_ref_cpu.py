"""CPU checks of tests/kernel_value_ref.py: the restated kernel arithmetic stays inside the derived bound against the longdouble
reference, the flat constants ``C_KIND`` are the ones measured here, every grid keeps at least 90 % of its entries under the
relative rule, the planted entries are where the module says, and the oracle's ``K()`` (GPflow's expanded form) agrees with the
reference entrywise -- so the two references of this suite cannot drift apart unnoticed."""
import functools

import numpy as np
import pytest

from oracle import tsvgp_oracle as O
from tests import kernel_value_ref as R

L = np.longdouble
TYPES = [np.float64, np.float32]
KIND_NAMES = list(R.KINDS)
FILL_D = [1, 3, 8, 19, 32]
PAIR_D = [1, 5, 32]
GRAM_D = 33


@functools.lru_cache(maxsize=None)
def _fill(kind, T, D, N=130, M=130):
    g = R.grid(kind, T, N, M, D)
    var = R.c_variance(g["variance"], T)
    return g, var, R.reference(kind, g["X"], g["Z"], g["inv_ls"], var)


@functools.lru_cache(maxsize=None)
def _pair(kind, T, D):
    g = R.grid(kind, T, 130, 0, D, seed=1, pairwise=True)
    var = R.c_variance(g["variance"], T)
    return g, var, R.reference(kind, g["X"], g["X"], g["inv_ls"], var)


def gram_inputs(g, T):
    """xx, zz, G of the D > 32 path in the type T from a grid: what torch computes on the device is replaced by NumPy here."""
    Xs, Zs = (g["X"] * g["inv_ls"]).astype(T), (g["Z"] * g["inv_ls"]).astype(T)
    return (Xs * Xs).sum(axis=1), (Zs * Zs).sum(axis=1), Xs @ Zs.T


@functools.lru_cache(maxsize=None)
def _gram(kind, T):
    g = R.grid(kind, T, 130, 130, GRAM_D, seed=2)
    var = R.c_variance(g["variance"], T)
    xx, zz, G = gram_inputs(g, T)
    return g, var, (xx, zz, G), R.reference_gram(kind, xx, zz, G, var)


def _cases(kind, T):
    """(name, D or None, restated values, reference) of every grid the GPU tests use at their base shape."""
    for D in FILL_D:
        g, var, ref = _fill(kind, T, D)
        yield f"fill D={D}", D, R.restate(kind, g["X"], g["Z"], g["inv_ls"], var, T), ref
    for D in PAIR_D:
        g, var, ref = _pair(kind, T, D)
        yield f"pairwise D={D}", D, R.restate(kind, g["X"], g["X"], g["inv_ls"], var, T), ref
    g, var, (xx, zz, G), ref = _gram(kind, T)
    yield "gram D=33", None, R.restate_gram(kind, xx, zz, G, var, T), ref


@pytest.mark.parametrize("T", TYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_restatement_is_inside_the_bound_and_the_constants_are_the_measured_ones(kind, T):
    """``restate`` against ``reference`` on every grid: inside ``rel_bound`` with factor 1 and no device-exponential term, the tiny
    entries inside the absolute rule; the flat excess over all grids is what ``C_KIND`` holds (within a factor 1.5)."""
    worst_c = -np.inf
    for name, D, got, ref in _cases(kind, T):
        bound = R.rel_bound(kind, T, ref, D, factor=1.0, exp_ulp=0.0)
        worst, frac = R.check_values(got, ref, bound, T, 1.3, f"{kind} {T.__name__} {name}")
        assert worst <= 1.0 and frac >= 0.9
        worst_c = max(worst_c, R.flat_excess(kind, T, got, ref, D))
    c = R.C_KIND[T][kind]
    print(f"{kind} {T.__name__}: measured flat constant {worst_c:.3f}, C_KIND {c}")
    assert worst_c <= c
    assert worst_c >= c / 1.5


@pytest.mark.parametrize("T", TYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_at_least_ninety_percent_of_every_grid_is_checked_relatively(kind, T):
    """The condition of the grid, from the reference alone, at every shape the GPU tests use (the row blocks of the 65536-row cases
    are sampled there from the same generator and checked when they run)."""
    fracs = {}
    for D in FILL_D:
        fracs[f"fill 130 x 130 D={D}"] = R.relative_mask(_fill(kind, T, D)[2], T).mean()
    for N, M, D in [(4097, 130, 8), (4166, 130, 8), (129, 1025, 8)]:
        fracs[f"fill {N} x {M}"] = R.relative_mask(_fill(kind, T, D, N, M)[2], T).mean()
    for D in PAIR_D:
        fracs[f"pairwise D={D}"] = R.relative_mask(_pair(kind, T, D)[2], T).mean()
    fracs["gram"] = R.relative_mask(_gram(kind, T)[3], T).mean()
    print({k: round(float(v), 3) for k, v in fracs.items()})
    assert min(fracs.values()) >= 0.9, fracs


@pytest.mark.parametrize("T", TYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_grid_covers_the_range_and_holds_the_planted_entries(kind, T):
    g, var, ref = _fill(kind, T, 3)
    a, s, K = ref["a"].astype(np.float64), ref["s"].astype(np.float64), ref["K"]
    k = R.K_SAME
    assert np.all(s[np.arange(k), np.arange(k)] == 0.0) and np.all(K[np.arange(k), np.arange(k)] == L(var))  # exact r = 0
    planted = s[k + 1:k + 1 + R.N_PLANT, k]
    assert np.allclose(planted, [1e-40, 0.81e-36, 1.21e-36, 1e-30], rtol=1e-5), planted  # both sides of the clamp at 1e-36
    far = K[k + 1 + R.N_PLANT:k + 1 + R.N_PLANT + R.N_FAR]
    assert np.all(far < R.far_below(T)) and np.all(far >= 0)  # far beyond underflow
    rel = R.relative_mask(ref, T)
    hist = np.histogram(a[rel], bins=10, range=(0.0, R.A_MAX[T]))[0]
    assert np.all(hist > 0), hist  # the relatively checked entries reach every tenth of [0, A_MAX]
    assert a[rel].max() > 0.93 * R.A_MAX[T]
    assert np.all(g["inv_ls"] <= 1 / 0.7) and np.all(g["inv_ls"] >= 1 / 1.7 - 1e-6)
    for key in ("X", "Z", "inv_ls"):
        assert np.array_equal(g[key].astype(T).astype(np.float64), g[key])  # values of the type: the device copy is exact
    gp, _, refp = _pair(kind, T, 5)
    assert np.array_equal(gp["X"][-1], gp["X"][1]) and refp["s"][129, 1] == 0  # r = 0 off the diagonal of k(X, X)


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_the_oracle_agrees_with_the_reference_entrywise(kind):
    """``oracle.K()`` forms r2 = |x / l|^2 + |z / l|^2 - 2 (x / l).(z / l) in fp64: three dot products of D terms and two additions,
    |dr2| <= (D + 4) u (|x~|^2 + |z~|^2 + 2 sum_d |x~_d z~_d|), plus 2 u amp for x / l against x * fl(1 / l) (two roundings per
    scaled coordinate).  Bound: |k'/k| |dr2| + (3 |a| + 16) u relative, the 1e3 * tiny rule below that."""
    T, u = np.float64, R.U[np.float64]
    for D in FILL_D:
        g, var, ref = _fill(kind, T, D)
        got = getattr(O, kind)(variance=var, lengthscales=1.0 / g["inv_ls"]).K(g["X"], g["Z"])
        Xs, Zs = np.abs(g["X"] * g["inv_ls"]), np.abs(g["Z"] * g["inv_ls"])
        mag = (Xs * Xs).sum(1)[:, None] + (Zs * Zs).sum(1)[None, :] + 2.0 * Xs @ Zs.T
        a = np.abs(ref["a"]).astype(np.float64)
        bound = R.log_slope(kind, a) * u * ((D + 4) * mag + 2.0 * ref["amp"]) + u * (3.0 * a + 16.0)
        worst, _ = R.check_values(got, ref, bound, T, var, f"oracle {kind} D={D}")
        assert worst <= 1.0
        rel = R.relative_mask(ref, T)
        print(f"oracle {kind} D={D}: largest bound {bound[rel].max():.2e}")
        assert bound[rel].max() < 1e-11  # the cross-check is a sharp one
