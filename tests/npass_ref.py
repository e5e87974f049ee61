"""Operands and NumPy fp64 references for the three N-pass MFMA products (``tsvgp_trmm_*``, ``tsvgp_moments_*``,
``tsvgp_site_accum_*``) on EXACT arithmetic: small integers and dyadic weights, so that every partial sum of every output entry,
in any order, is representable in fp32 and in fp64.  A kernel then has to equal the reference bit for bit whatever its chunk order,
slice count or accumulation order.  No torch, no GPU: tests/test_npass_ref_cpu.py proves the exactness condition and that the probes
see the faults they are made for; tests/test_gpu_npass_values.py runs the kernels on the same cases.

Every generator returns a dict with the operands (float64 arrays holding the integers; the caller casts to the compute dtype, which
is exact), the references, and ``absum``: the largest sum of ABSOLUTE values of the terms of any output entry, times 2^e where 2^-e is
the smallest dyadic step in use.  Exact when ``absum < EXACT_LIMIT[dtype]``.
"""
import functools

import numpy as np

TILE = 128
EXACT_LIMIT = {"f32": 2.0 ** 24, "f64": 2.0 ** 53}
LOWER, UPPER, DENSE = 0, 1, 2  # TSVGP_TRI_*


def round_up(n, m=TILE):
    return (n + m - 1) // m * m


def tri_mask(Mp, mode):
    """1 where Tm[i, j] is inside the range of ``mode`` (j <= i, j >= i, all j)."""
    one = np.ones((Mp, Mp))
    return {LOWER: np.tril(one), UPPER: np.triu(one), DENSE: one}[mode]


def pz(x):
    """-0.0 -> +0.0: the kernels add products to accumulators that start at +0.0, which never yields -0.0."""
    return np.asarray(x, dtype=np.float64) + 0.0


# ----------------------------------------------------------------------------------------------------------- case lists
# (imported by the GPU file and by the CPU file: the two cannot drift)
KS = tuple(range(1, 10))  # Mp = 128 k
TRMM_CASES = [(128 * k, mode) for k in KS for mode in (LOWER, UPPER, DENSE)]
TRMM_SUM_NP = (256, 384)
MOMENTS_GRID = [(128 * k, mode, P) for k in KS for mode in (LOWER, UPPER, DENSE) for P in (1, 3)]
MOMENTS_TAILS = (1, 127, 128, 129, 255, 256, 257)
MOMENTS_TAIL_CASES = [(Mp, mode, P, N) for Mp, P in ((128, 1), (384, 3)) for mode in (LOWER, UPPER) for N in MOMENTS_TAILS]
MEANONLY_CASES = [(128 * k, P) for k in (1, 3, 9) for P in (1, 8)]
WIDE_M, WIDE_N = 8320, 100  # the triangular panel_kernel arms (fp64 only): gamma no longer fits panel1_kernel's dynamic LDS
# site sums: (Mp, P, Np, nsplits).  The slice lengths these reach are computed by slice_lengths() and asserted, not trusted.
SITE_NSPLITS = (1, 2, 3, 4, 5, 8, 16)
SITE_CASES = ([(Mp, P, Np, SITE_NSPLITS) for Mp in (128, 256, 384) for P in (1, 3, 8, 9) for Np in (128, 384, 640)]
              + [(1024, P, 384, (1, 5, 8) if P < 8 else (1, 3)) for P in (1, 3, 8, 9)]
              + [(256, 3, 4096, (1, 7, 64))])
ROUNDING_CASES = [(Mp, mode, P) for Mp in (128, 384, 1024) for mode in (LOWER, UPPER, DENSE) for P in (1, 3)]
ROUNDING_N = 257


def grid_rows(Mp):
    """Row count of the moments grid: every unit row, then 37 4-sparse rows (a partial last panel)."""
    return Mp + 37


# ----------------------------------------------------------------------------------------------------------- trmm
@functools.lru_cache(maxsize=2)
def trmm_placement(Mp, mode):
    """Tm[i, j] = 1 + i Mp + j inside the triangle (exactly zero outside), A = I: C[n, i] = Tm[i, n] reads every entry back by
    value."""
    i, j = np.indices((Mp, Mp))
    Tm = (1.0 + i * Mp + j) * tri_mask(Mp, mode)
    A = np.eye(Mp)
    return dict(A=A, Tm=Tm, C=pz(Tm.T.copy()), absum=float(np.abs(Tm).max()))


@functools.lru_cache(maxsize=2)
def trmm_sum(Mp, mode, Np):
    rng = np.random.RandomState(1000 + Mp + 7 * mode + Np)
    A = rng.randint(-1, 2, (Np, Mp)).astype(np.float64)
    Tm = rng.randint(-2, 3, (Mp, Mp)) * tri_mask(Mp, mode)
    return dict(A=A, Tm=Tm, C=pz(A @ Tm.T), absum=float((np.abs(A) @ np.abs(Tm).T).max()))


# ----------------------------------------------------------------------------------------------------------- moments
def moments_rows(rng, N, Mp):
    """[N, Mp]: rows 0 .. Mp - 1 are the unit vectors when N >= Mp, every further row (all rows when N < Mp) has four entries +-1 at
    random columns."""
    A = np.zeros((N, Mp))
    first = Mp if N >= Mp else 0
    A[np.arange(first), np.arange(first)] = 1.0
    for n in range(first, N):
        A[n, rng.choice(Mp, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
    return A


def pick_kdiag(q, k, of, used=()):
    """An integer among the values of q (so some row has var == 0 exactly), at rank k of `of` among the distinct ones, not in
    ``used``."""
    u = np.unique(q)
    idx = len(u) * k // of
    for step in range(len(u)):
        v = float(u[(idx + step) % len(u)])
        if v not in used:
            return v
    return float(u[idx % len(u)]) + 1.0 + len(used)  # (fewer distinct q than latents: N = 1)


def moments_values(A, Tm, gamma, kdiag, Y, N):
    """The documented outputs of tsvgp_moments_* for A [Np, Mp] (or [P, Np, Mp]), Tm [P, Mp, Mp], gamma [Mp, P], kdiag scalar or
    [P], lik_param = 0.5: mean, var [N, P]; g0, g1 [Np, P] of the Gaussian map (rows >= N zero); nonpos [Np / 128]."""
    P = Tm.shape[0]
    Np = A.shape[-2]
    Ap = lambda p: A[p] if A.ndim == 3 else A
    C = [Ap(p)[:N] @ Tm[p].T for p in range(P)]
    q = np.stack([np.sum(c * c, axis=1) for c in C], axis=1)
    mean = pz(np.stack([Ap(p)[:N] @ gamma[:, p] for p in range(P)], axis=1))
    var = pz(np.asarray(kdiag, dtype=np.float64).reshape(1, -1) - q)
    g0, g1 = np.zeros((Np, P)), np.zeros((Np, P))
    if Y is not None:
        g0[:N] = pz((Y - mean) / 0.5)
        g1[:N] = -0.5 / 0.5
    bad = np.zeros(Np, dtype=np.int64)
    bad[:N] = np.sum(~(var > 0), axis=1)
    nonpos = bad.reshape(-1, TILE).sum(axis=1).astype(np.int32)
    return dict(mean=mean, var=var, g0=g0, g1=g1, nonpos=nonpos, q=q)


@functools.lru_cache(maxsize=2)
def moments_case(Mp, mode, P, N):
    """Shared-operand and per-latent operands of one case.  ``shared``: A [Np, Mp], one integer kdiag; ``batched``: A [P, Np, Mp]
    (latent 0 is the shared one), distinct integer kdiag[p].  Both with the references of moments_values()."""
    rng = np.random.RandomState(2000 + Mp + 7 * mode + 13 * P + 31 * N)
    Np = round_up(N)
    A = np.zeros((P, Np, Mp))
    for p in range(P):
        A[p, :N] = moments_rows(rng, N, Mp)
    Tm = rng.randint(-1, 2, (P, Mp, Mp)) * tri_mask(Mp, mode)
    gamma = rng.randint(-3, 4, (Mp, P)).astype(np.float64)
    Y = rng.randint(-5, 6, (N, P)).astype(np.float64)
    absA = np.abs(A)
    s = np.stack([absA[p] @ np.abs(Tm[p]).T for p in range(P)])  # [P, Np, Mp]: sum_j |a_j| |Tm_ij|
    absum_q = float(np.max(np.sum(s * s, axis=-1)))
    out = {}
    for name, Ause in (("shared", A[0]), ("batched", A)):
        q = moments_values(Ause, Tm, gamma, 0.0, None, N)["q"]
        if name == "shared":
            kdiag = pick_kdiag(q, 1, 2)
        else:
            kdiag = []
            for p in range(P):
                kdiag.append(pick_kdiag(q[:, p], p + 1, P + 1, used=tuple(kdiag)))
        ref = moments_values(Ause, Tm, gamma, kdiag, Y, N)
        absum = max(absum_q + float(np.max(np.abs(kdiag))), float(np.max(absA[0] @ np.abs(gamma))) * 2 + 2 * 5)
        out[name] = dict(A=Ause, kdiag=kdiag, ref=ref, absum=absum)
    return dict(Tm=Tm, gamma=gamma, Y=Y, N=N, Np=Np, Mp=Mp, P=P, mode=mode, **out)


@functools.lru_cache(maxsize=2)
def meanonly_case(Mp, P):
    """TSVGP_LIK_MEANONLY: mean = A gamma and the Gaussian map at lik_param = 0.5 (g0 = 2 (y - mean), g1 = -1)."""
    rng = np.random.RandomState(3000 + Mp + P)
    N = grid_rows(Mp)
    Np = round_up(N)
    A = np.zeros((Np, Mp))
    A[:N] = moments_rows(rng, N, Mp)
    gamma = rng.randint(-3, 4, (Mp, P)).astype(np.float64)
    Y = rng.randint(-5, 6, (N, P)).astype(np.float64)
    mean = pz(A[:N] @ gamma)
    g0, g1 = np.zeros((Np, P)), np.zeros((Np, P))
    g0[:N], g1[:N] = pz((Y - mean) / 0.5), -1.0
    return dict(A=A, gamma=gamma, Y=Y, N=N, Np=Np, mean=mean, g0=g0, g1=g1, absum=float(np.max(np.abs(A) @ np.abs(gamma))) * 2 + 10)


WIDE_ABSUM = WIDE_M * 16.0 + WIDE_M  # |C[n, i]| <= 4 (4-sparse +-1 rows, Tm in {-1, 0, 1}): q <= 16 Mp, kdiag <= Mp


def wide_rows(seed=17):
    """[WIDE_N, WIDE_M]: 64 unit rows at the columns on either side of 32 tile edges spread over the width, then 4-sparse rows."""
    rng = np.random.RandomState(seed)
    A = np.zeros((WIDE_N, WIDE_M))
    edges = (np.arange(1, 33) * 2 * TILE)  # 256, 512, .., 8192
    cols = np.concatenate([edges - 1, edges])
    assert cols.max() < WIDE_M and len(cols) == 64
    A[np.arange(64), cols] = 1.0
    for n in range(64, WIDE_N):
        A[n, rng.choice(WIDE_M, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
    return A


# ----------------------------------------------------------------------------------------------------------- site sums
def site_chunk(esize, P):
    """Rows per chunk: 16 in syrk1_kernel (fp64, P <= 8) and syrk_kernel<T> (P > 8), 32 in syrk1f_kernel (fp32, P <= 8)."""
    return 32 if (esize == 4 and P <= 8) else 16


def site_ns_diag(nsplit, esize):
    return max(1, ((20 if esize == 8 else 22) * nsplit + 31) // 32)


def slice_bounds(Np, nsplit, esize, P):
    """The launcher's two partitions of the row range as stated in include/tsvgp_hip.h and its source: ({'off': [(row_lo, row_hi)
    per slice], 'diag': [...]}, chunk rows).  A slice is `per` = ceil(total / count) chunks, clamped to the total."""
    chunk = site_chunk(esize, P)
    total = Np // chunk
    out = {}
    for name, ns in (("off", nsplit), ("diag", site_ns_diag(nsplit, esize))):
        per = (total + ns - 1) // ns
        out[name] = [(min(s * per, total) * chunk, min((s + 1) * per, total) * chunk) for s in range(ns)]
    return out, chunk


def slice_lengths(Np, nsplit, esize, P):
    b, chunk = slice_bounds(Np, nsplit, esize, P)
    return {k: [(hi - lo) // chunk for lo, hi in v] for k, v in b.items()}


def site_sums(B, g0, g1):
    """acc2 [P, Mp, Mp], acc1 [P, Mp] for B [Np, Mp] or [P, Np, Mp]."""
    P = g0.shape[1]
    Bp = lambda p: B[p] if B.ndim == 3 else B
    acc2 = np.stack([Bp(p).T @ (g1[:, p, None] * Bp(p)) for p in range(P)])
    acc1 = np.stack([Bp(p).T @ g0[:, p] for p in range(P)])
    return pz(acc2), pz(acc1)


@functools.lru_cache(maxsize=2)
def site_case(Mp, P, Np, dt):
    """B [P, Np, Mp] in {-2..2} (latent 0 is the shared operand), g0 in {-3..3}; weight set 'int': g1 in {-1..-4}; weight set 'dyadic':
    g1 = -2^-(n mod E), E from dyadic_period for the dtype ``dt`` ('f32' / 'f64').  The last 5 rows carry zero weights."""
    rng = np.random.RandomState(4000 + Mp + 3 * P + Np)
    B = rng.randint(-2, 3, (P, Np, Mp)).astype(np.float64)
    g0 = rng.randint(-3, 4, (Np, P)).astype(np.float64)
    g1i = -rng.randint(1, 5, (Np, P)).astype(np.float64)
    g0[-5:], g1i[-5:] = 0.0, 0.0
    # sum_n |g1| |b_i| |b_j| <= max_i sum_n |g1| b_i^2 (Cauchy-Schwarz): the diagonal carries the largest entry
    diag_abs = lambda w: float(max(np.max(np.sum(w[:, p, None] * B[p] * B[p], axis=0)) for p in range(P)))
    live = np.ones((Np, P))
    live[-5:] = 0.0
    dyadic = lambda E: -(2.0 ** -(np.arange(Np) % E))[:, None] * live
    E = 27  # the largest period whose own sums pass the exactness condition (fp64: always 27, the crop value's scale 2^-26)
    while E > 1 and diag_abs(np.abs(dyadic(E))) * 2.0 ** (E - 1) >= EXACT_LIMIT[dt]:
        E -= 1
    g1d = dyadic(E)
    abs1 = float(max(np.max(np.abs(B[p]).T @ np.abs(g0[:, p])) for p in range(P)))
    sets = {}
    for name, g1, scale in (("int", g1i, 1.0), ("dyadic", g1d, 2.0 ** (E - 1))):
        sets[name] = dict(g1=g1, absum=max(diag_abs(np.abs(g1)) * scale, abs1), shared=site_sums(B[0], g0, g1), batched=site_sums(B, g0, g1))
    return dict(B=B, g0=g0, E=E, sets=sets, Mp=Mp, P=P, Np=Np)


# ----------------------------------------------------------------------------------------------------------- rounding family
def rounding_operands(Mp, mode, P, np_dtype, N=ROUNDING_N):
    """Graded random operands, rounded to the compute dtype first: row n of A / B scaled by 2^-(n mod 24), row i of Tm by
    2^-(i mod 16), g1 = -2^-(n mod 27), M = Mp - 37 live columns (the valid block), the rest zero."""
    rng = np.random.RandomState(5000 + Mp + 7 * mode + 13 * P)
    Np, M = round_up(N), Mp - 37
    r = lambda x: x.astype(np_dtype).astype(np.float64)
    A = np.zeros((Np, Mp))
    A[:N, :M] = rng.randn(N, M) * (2.0 ** -(np.arange(N) % 24))[:, None]
    Tm = np.zeros((P, Mp, Mp))
    Tm[:, :M, :M] = rng.randn(P, M, M) * (2.0 ** -(np.arange(M) % 16))[None, :, None]
    Tm *= tri_mask(Mp, mode)
    gamma = np.zeros((Mp, P))
    gamma[:M] = rng.randn(M, P)
    g0 = np.zeros((Np, P))
    g0[:N] = rng.randn(N, P)
    g1 = np.zeros((Np, P))
    g1[:N] = -(2.0 ** -(np.arange(N) % 27))[:, None]
    return dict(A=r(A), Tm=r(Tm), gamma=r(gamma), g0=r(g0), g1=r(g1), N=N, Np=Np, kdiag=2.5)


def rounding_bounds(op, u):
    """References (float64) and the entrywise bounds of the issue: K = Mp, s_i = sum_j |a_j| |Tm_ij|."""
    A, Tm, gamma, g0, g1, N, Np = op["A"], op["Tm"], op["gamma"], op["g0"], op["g1"], op["N"], op["Np"]
    P, Mp = Tm.shape[0], Tm.shape[1]
    K = Mp
    C = np.stack([A @ Tm[p].T for p in range(P)])
    S = np.stack([np.abs(A) @ np.abs(Tm[p]).T for p in range(P)])
    mean = A[:N] @ gamma
    var = op["kdiag"] - np.sum(C * C, axis=-1).T[:N]
    sq = np.sum(S * S, axis=-1).T[:N]
    acc2, acc1 = site_sums(A, g0, g1)
    abs2 = np.stack([np.abs(A).T @ (np.abs(g1[:, p, None]) * np.abs(A)) for p in range(P)])
    abs1 = np.stack([np.abs(A).T @ np.abs(g0[:, p]) for p in range(P)])
    return dict(C=(C, 2 * (K + 1) * u * S, S), mean=(mean, 2 * (K + 1) * u * (np.abs(A[:N]) @ np.abs(gamma)), np.abs(A[:N]) @ np.abs(gamma)),
                var=(var, 2 * u * ((3 * K + 1) * sq + abs(op["kdiag"]) + np.abs(var)), sq + abs(op["kdiag"]) + np.abs(var)),
                acc2=(acc2, 2 * (Np + 2) * u * abs2, abs2), acc1=(acc1, 2 * (Np + 1) * u * abs1, abs1))


# ----------------------------------------------------------------------------------------------------------- comparison
def first_difference(got, ref):
    """None when ``got`` equals ``ref`` bit for bit (as integer views: -0.0 != +0.0, NaN compared by payload); otherwise a message
    naming the first differing index with got / expected."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return f"shape / dtype {got.shape} {got.dtype} against {ref.shape} {ref.dtype}"
    bits = {8: np.int64, 4: np.int32, 1: np.uint8}[got.dtype.itemsize]
    diff = got.view(bits) != ref.view(bits)
    if not diff.any():
        return None
    idx = tuple(int(v) for v in np.argwhere(diff)[0])
    return f"{int(diff.sum())} of {diff.size} entries differ; first at {idx}: got {got[idx]!r}, expected {ref[idx]!r}"
