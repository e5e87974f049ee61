"""Entrywise reference, restatement, error bound and input grid for the kernel-matrix values ``variance * k_kind(s)`` that
``kernel_profile<KIND>`` of ``csrc/tsvgp_device.h`` forms at five sites (the fill, ``gram_to_kernel``, the epilogue of ``cov``,
``vgp_system``, ``greedy_step``).  Shared by tests/test_kernel_value_ref_cpu.py and tests/test_gpu_kernel_values.py.

``reference``   K = variance * k_kind(s), s = sum_d ((x_d - z_d) inv_ls_d)^2 in ``np.longdouble`` from the inputs AS THE KERNEL
                RECEIVES THEM (already rounded to the compute type; the variance as the C ABI passes it).  Profiles as
                include/tsvgp_hip.h defines them: SE exp(-s / 2); Matern r = sqrt(max(s, 1e-36)), (1 + sqrt(3) r) exp(-sqrt(3) r)
                and (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r).  Also returned per entry: the exponent's argument a (s / 2,
                sqrt(3) r, sqrt(5) r), s, and amp = sum_d 2 |x~_d - z~_d| (|x~_d| + |z~_d|) with x~ = x inv_ls.
``reference_gram``  the same profile at s = xx[n] + zz[m] - 2 G[n, m] from the given xx, zz, G (``tsvgp_gram_to_kernel_*``); a
                slightly negative s is taken as it is (SE: variance * exp(+small); Matern: the clamp).
``restate``     the kernel's arithmetic in ``np.float64`` / ``np.float32``: inputs scaled first (one rounded product each), the
                difference form, accumulation over d in index order (no FMA), the profile in the operation order of
                ``kernel_profile``.  exp is the correctly rounded one in fp64; in fp32 it is ``__expf``: t = fl(a * fl(log2 e)),
                then the correctly rounded 2^t.  ``restate_gram``: s = fl(fl(xx + zz) - 2 G).

The bound (u = 2^-53 or 2^-24, first order in u; ``rel_bound``)

    |ds|     <= u * (sum_d 2 |x~_d - z~_d| (|x~_d| + |z~_d|) + (D + 2) s)                      difference form
                  x~ = fl(x inv_ls) and z~ = fl(z inv_ls) are off by u |x~|, u |z~|, so their difference is off by u (|x~_d| + |z~_d|)
                  and its square by 2 |x~_d - z~_d| times that: the input-magnitude term, which alone matters at D = 1 (s small, x
                  large).  The subtraction, the square and the D - 1 additions of the sum are (D + 2) roundings relative to s.
    |ds|     <= u * (|xx + zz| + |s|)                                                           Gram form: two rounded additions
    |dK| / K <= |k'(s) / k(s)| |ds| + A |a| u + (E + factor * c_kind) u
                  |k'/k| = 1/2 (SE),  3/2 / (1 + a) (Matern-3/2),  5/6 (1 + a) / (1 + a + a^2 / 3) (Matern-5/2)
                  A |a| u: roundings of the exponent's ARGUMENT, each worth |a| u of exp(-a).  Matern: sqrt, the product with
                  sqrt(3) / sqrt(5), that constant's own rounding: 3.  fp32 adds ``__expf``: a * log2 e is rounded once and fl(log2 e) is
                  off by 0.16 u (EXPF_ARG = 1.16, computed below), as the kernel's comment says ("relative error ~|a| 2^-24").
                  E = 2: one ulp of the device's exponential (the library's fp64 exp, v_exp_f32), which the restatement's
                  correctly rounded exp does not have.
                  c_kind: the flat rest (the polynomial, the products with it and with the variance), MEASURED by
                  tests/test_kernel_value_ref_cpu.py as max (|dK| / K - |k'/k| |ds| - A |a| u) / u of ``restate`` against
                  ``reference`` over the grids below -- never from a kernel -- and kept in ``C_KIND``.  The GPU tests pass
                  factor = 2: the device may contract a * b + c and order the Matern polynomial differently.

An entry whose reference is below 1e3 * tiny of the type (fp32 flushes there, fp64 goes denormal) is held to
0 <= K <= 2e3 * tiny * variance instead (``check_values``); the grids keep that to under 10 % of the entries.

``grid``        rows placed radially so that a runs from 0 to the edge of the type's normal range (``A_MAX``: 708 in fp64, 84 in
                fp32), Z a small cloud around the origin, Z[:k] = X[:k] (exact r = 0), Z[k] = 0 with four planted rows at
                s = 1e-40, 0.81e-36, 1.21e-36, 1e-30 from it (both sides of the Matern clamp), two rows at three times the
                largest radius (far beyond underflow: +0.0, never NaN, never negative), lengthscales 0.7 + rand.
                ``pairwise=True`` puts the rows on one ray, for the sites that evaluate k(X, X).  ``P``: inv_ls [P, D] for the
                batched fill -- the geometry is laid out in latent 0's scaling, the other latents' lengthscales are up to 10 %
                longer per dimension, so every latent keeps the 90 %.
"""
import ctypes

import numpy as np

L = np.longdouble
U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
TINY = {np.float64: float(np.finfo(np.float64).tiny), np.float32: float(np.finfo(np.float32).tiny)}
A_MAX = {np.float64: 708.0, np.float32: 84.0}  # -log(tiny) = 708.4 / 87.3, -log(1e3 tiny) = 701.5 / 80.4
KINDS = {"SquaredExponential": 0, "Matern32": 2, "Matern52": 3}
SQRT3, SQRT5 = L(3) ** L(0.5), L(5) ** L(0.5)
LOG2E_F32 = np.float32(1.4426950408889634)
EXPF_ARG = 1.0 + abs(float(LOG2E_F32) / 1.4426950408889634 - 1.0) / U[np.float32]  # 1.16
ARG_ROUNDINGS = {"SquaredExponential": 0.0, "Matern32": 3.0, "Matern52": 3.0}
EXP_ULP = 2.0
# measured by tests/test_kernel_value_ref_cpu.py (it prints the figures and fails when they leave [C / 1.5, C])
# measured: fp64 1.22 / 2.26 / 2.91, fp32 1.18 / 2.03 / 2.69 (the worst case is the D = 1 fill or the Gram form each time)
C_KIND = {np.float64: {"SquaredExponential": 1.25, "Matern32": 2.3, "Matern52": 3.0},
          np.float32: {"SquaredExponential": 1.25, "Matern32": 2.1, "Matern52": 2.8}}
GPU_FACTOR = 2.0


def np_type(dtype):
    """np.float64 / np.float32 for a NumPy or torch dtype."""
    return np.float32 if "32" in str(dtype) else np.float64


def c_variance(variance, T):
    """The scalar as the C ABI passes it."""
    return float((ctypes.c_double if T is np.float64 else ctypes.c_float)(variance).value)


def _profile_l(kind, s):
    """(k, a) in longdouble."""
    if kind == "SquaredExponential":
        a = s / 2
        return np.exp(-a), a
    r = np.sqrt(np.maximum(s, L(1e-36)))
    if kind == "Matern32":
        a = SQRT3 * r
        return (1 + a) * np.exp(-a), a
    a = SQRT5 * r
    return (1 + a + L(5) / L(3) * r * r) * np.exp(-a), a


def reference(kind, X, Z, inv_ls, variance):
    """dict(K, a, s, amp) [N, M]: K, a, s longdouble; amp float64."""
    X, Z, il = np.asarray(X), np.asarray(Z), np.asarray(inv_ls)
    Xs, Zs = X.astype(L) * il.astype(L), Z.astype(L) * il.astype(L)
    s = np.zeros((X.shape[0], Z.shape[0]), L)
    amp = np.zeros(s.shape)
    for d in range(X.shape[1]):
        dd = Xs[:, d, None] - Zs[None, :, d]
        s += dd * dd
        amp += (2.0 * np.abs(dd) * (np.abs(Xs[:, d, None]) + np.abs(Zs[None, :, d]))).astype(np.float64)
    k, a = _profile_l(kind, s)
    return dict(K=L(variance) * k, a=a, s=s, amp=amp)


def reference_gram(kind, xx, zz, G, variance):
    """The profile at s = xx[n] + zz[m] - 2 G[n, m]; amp is |xx + zz| (the Gram form's bound takes it)."""
    xx, zz, G = np.asarray(xx).astype(L), np.asarray(zz).astype(L), np.asarray(G).astype(L)
    s = xx[:, None] + zz[None, :] - 2 * G
    k, a = _profile_l(kind, s)
    return dict(K=L(variance) * k, a=a, s=s, amp=np.abs(xx[:, None] + zz[None, :]).astype(np.float64))


def _exp_t(x, T):
    """exp of ``exp_nonpos<T>``: fp64 the (correctly rounded) library exp; fp32 ``__expf``."""
    if T is np.float64:
        return np.exp(x)
    t = (x * LOG2E_F32).astype(np.float32)
    with np.errstate(under="ignore"):
        return np.exp2(t.astype(np.float64)).astype(np.float32)


def _profile_t(kind, s, T):
    if kind == "SquaredExponential":
        return _exp_t(T(-0.5) * s, T)
    r = np.sqrt(np.where(s > T(1e-36), s, T(1e-36)))
    if kind == "Matern32":
        a = T(1.7320508075688772935) * r
        return (T(1) + a) * _exp_t(-a, T)
    a = T(2.2360679774997896964) * r
    return (T(1) + a + T(5.0 / 3.0) * r * r) * _exp_t(-a, T)


def restate(kind, X, Z, inv_ls, variance, T):
    """The fill's arithmetic in the type T: [N, M] of dtype T."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        il = np.asarray(inv_ls).astype(T)
        Xs, Zs = np.asarray(X).astype(T) * il, np.asarray(Z).astype(T) * il
        s = np.zeros((Xs.shape[0], Zs.shape[0]), T)
        for d in range(Xs.shape[1]):
            dd = Xs[:, d, None] - Zs[None, :, d]
            s = s + dd * dd
        return T(variance) * _profile_t(kind, s, T)


def restate_gram(kind, xx, zz, G, variance, T):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        xx, zz, G = (np.asarray(v).astype(T) for v in (xx, zz, G))
        s = (xx[:, None] + zz[None, :]) - T(2) * G
        return T(variance) * _profile_t(kind, s, T)


def log_slope(kind, a):
    """|k'(s) / k(s)| as a function of the exponent's argument a (float64)."""
    a = np.abs(np.asarray(a, np.float64))
    if kind == "SquaredExponential":
        return np.full(a.shape, 0.5)
    if kind == "Matern32":
        return 1.5 / (1.0 + a)
    return (5.0 / 6.0) * (1.0 + a) / (1.0 + a + a * a / 3.0)


def arg_roundings(kind, T):
    return ARG_ROUNDINGS[kind] + (EXPF_ARG if T is np.float32 else 0.0)


def ds_bound(ref, T, D=None):
    """u * (amp + (D + 2) s) for the difference form; D = None: the Gram form's u * (|xx + zz| + |s|)."""
    s = np.abs(ref["s"]).astype(np.float64)
    return U[T] * (ref["amp"] + ((D + 2.0) if D is not None else 1.0) * s)


def rel_bound(kind, T, ref, D=None, factor=1.0, exp_ulp=EXP_ULP, c_kind=None, extra=0.0):
    """The bound on |K - K_ref| / K_ref of the module docstring; ``extra``: further flat roundings of the site, in units of u."""
    a = np.abs(ref["a"]).astype(np.float64)
    c = C_KIND[T][kind] if c_kind is None else c_kind
    return log_slope(kind, a) * ds_bound(ref, T, D) + U[T] * (arg_roundings(kind, T) * a + exp_ulp + factor * c + extra)


def flat_excess(kind, T, got, ref, D=None):
    """max over the relatively checked entries of (|dK| / K - |k'/k| |ds| - A |a| u) / u: what ``C_KIND`` records."""
    rel = relative_mask(ref, T)
    err = (np.abs(np.asarray(got).astype(L) - ref["K"]) / np.where(rel, ref["K"], 1)).astype(np.float64)
    a = np.abs(ref["a"]).astype(np.float64)
    exc = (err - log_slope(kind, a) * ds_bound(ref, T, D) - U[T] * arg_roundings(kind, T) * a) / U[T]
    return float(np.max(exc[rel]))


def relative_mask(ref, T):
    """Entries held to the relative bound: the reference is at least 1e3 * tiny of the type."""
    return np.asarray(ref["K"] >= L(1e3 * TINY[T]))


def far_below(T):
    """1e-30 * tiny in longdouble (the product underflows in fp64): below it a value is far beyond the type's underflow."""
    return L(1e-30) * L(TINY[T])


def check_values(got, ref, bound, T, variance, what=""):
    """Assert the entrywise rule and return (worst |dK| / (K bound), fraction checked relatively).  ``got``: the kernel's values
    (any float dtype, exact in float64); ``bound``: relative bound per entry."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    assert not np.signbit(got).any(), f"{what}: negative values or -0.0"
    rel = relative_mask(ref, T)
    err = np.abs(got.astype(L) - ref["K"])
    ratio = (err / (np.where(rel, ref["K"], 1) * bound)).astype(np.float64)
    worst = float(np.max(ratio[rel])) if rel.any() else 0.0
    cap = 2e3 * TINY[T] * variance
    small_ok = got[~rel] <= cap
    far = np.asarray(ref["K"] < far_below(T))  # far beyond underflow: exactly +0.0
    frac = float(rel.mean())
    print(f"{what}: worst error / bound {worst:.3f} over {int(rel.sum())} entries ({100 * frac:.1f} % relative), "
          f"{int(far.sum())} entries far beyond underflow")
    if worst > 1.0:
        i = np.unravel_index(np.argmax(np.where(rel, ratio, 0)), ratio.shape)
        raise AssertionError(f"{what}: entry {i}: got {got[i]!r}, reference {float(ref['K'][i])!r}, a = {float(ref['a'][i]):.4g}, "
                             f"error / bound = {ratio[i]:.3f}")
    assert small_ok.all(), f"{what}: an entry below 1e3 * tiny exceeds 2e3 * tiny * variance"
    assert np.all(got[far] == 0.0), f"{what}: non-zero far beyond underflow"
    return worst, frac


K_SAME, N_PLANT, N_FAR = 4, 4, 2
PLANT_DELTA = (1e-20, 0.9e-18, 1.1e-18, 1e-15)  # s = 1e-40, 0.81e-36, 1.21e-36, 1e-30
MIN_ROWS = K_SAME + 1 + N_PLANT + N_FAR + 1


def radius_of(kind, a):
    """Scaled distance r at which the exponent's argument is a."""
    if kind == "SquaredExponential":
        return np.sqrt(2.0 * a)
    return a / (np.sqrt(3.0) if kind == "Matern32" else np.sqrt(5.0))


def grid(kind, T, N, M, D, seed=0, pairwise=False, P=None):
    """dict(X [N, D], Z [M, D], inv_ls [D] or [P, D], variance): float64 arrays holding values of the type T (rounded), so that
    ``torch.as_tensor(.., dtype)`` is exact.  M = 0: no Z (the sites that evaluate k(X, X)); pairwise: the rows on one ray."""
    assert N >= MIN_ROWS and (M == 0 or M >= K_SAME + 1)
    rng = np.random.RandomState(1000 * seed + 10 * D + KINDS[kind])
    ls = 0.7 + rng.rand(D)
    if P is not None:  # latent 0 as above; the others up to 10 % longer per dimension, so that a stays inside latent 0's range
        ls = np.concatenate([ls[None], ls[None] * (1.0 + 0.1 * rng.rand(P - 1, D))])
    il = (1.0 / ls).astype(T).astype(np.float64)
    il0 = il if P is None else il[0]  # the geometry is laid out in latent 0's scaling
    frac = rng.permutation(N) / (N - 1.0)
    frac[:K_SAME] = 0.002 * np.arange(K_SAME)  # the rows Z copies stay near the cloud
    r = radius_of(kind, frac * A_MAX[T])
    if pairwise:
        dirs = np.tile(rng.randn(1, D), (N, 1))
    else:
        dirs = rng.randn(N, D)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    X = (r[:, None] * dirs + 0.05 * rng.randn(N, D) / np.sqrt(D)) / il0
    k = K_SAME
    X[k] = 0.0
    for i, delta in enumerate(PLANT_DELTA):
        X[k + 1 + i] = 0.0
        X[k + 1 + i, 0] = delta / il0[0]
    far = radius_of(kind, A_MAX[T]) * 3.0
    for i in range(N_FAR):
        X[k + 1 + N_PLANT + i] = far * (1.0 + 0.1 * i) * dirs[k + 1 + N_PLANT + i] / il0
    X[N - 1] = X[1]  # a duplicate row: r = 0 off the diagonal of k(X, X)
    X = X.astype(T).astype(np.float64)
    out = dict(X=X, inv_ls=il, variance=1.3, kind=kind)
    if M:
        Z = (0.3 * rng.randn(M, D) / np.sqrt(D)) / il0
        Z = Z.astype(T).astype(np.float64)
        Z[:k] = X[:k]
        Z[k] = 0.0
        out["Z"] = Z
    return out
