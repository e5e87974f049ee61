"""NumPy fp64 restatement of the greedy conditional-variance selection (``tsvgp_greedy_select_f64``, include/tsvgp_hip.h (9)) and
the dense Nystrom residual it is checked against.  Test infrastructure only: the package never imports it.

    k = variance * f_kind(r),  r^2 = sum_d ((x_d - z_d) * inv_ls_d)^2      (as tsvgp_kernel_fill_*)
    floor = max(threshold, 1e-12 * variance),  d[n] = variance,  C empty
    for j in 0 .. M-1:
        p = the lowest n with d[n] == max(d);   stop unless d[p] > floor        (count = j)
        c = (k(X, x_p) - sum_{i<j} C[i, :] * C[i, p]) / sqrt(d[p])
        C[j, :] = c;  d = max(d - c * c, 0);  d[p] = 0;  indices[j] = p;  pivots[j] = d[p] as found
"""
import numpy as np

SE, MATERN32, MATERN52 = 0, 2, 3

# (N, D, M, kind, ls, seed): X = RandomState(seed).randn(N, D), inv_ls = linspace(1, 1.5, D) / ls.  The smallest shapes that cross
# every edge of the kernels: one row (and M > N); one short of and one past the 128-row workgroup; M past 128, so every unroll
# remainder of the dot product's i-loop occurs; D at its limit.
PROBLEMS = [
    (1, 2, 4, SE, 1.0, 0),
    (127, 2, 16, MATERN52, 0.5, 1),
    (129, 3, 40, MATERN32, 0.5, 2),
    (389, 2, 130, SE, 0.3, 3),
    (389, 2, 130, MATERN52, 0.15, 4),
    (260, 32, 33, SE, 3.0, 5),
]
VARIANCE = 1.7


def problem(N, D, M, kind, ls, seed):
    X = np.random.RandomState(seed).randn(N, D)
    return X, np.linspace(1.0, 1.5, D) / ls


def profile(kind, s):
    """f_kind of the scaled squared distance s (GPflow: the Matern kernels take r = sqrt(max(s, 1e-36)))."""
    if kind == SE:
        return np.exp(-0.5 * s)
    r = np.sqrt(np.maximum(s, 1e-36))
    if kind == MATERN32:
        a = np.sqrt(3.0) * r
        return (1.0 + a) * np.exp(-a)
    if kind == MATERN52:
        a = np.sqrt(5.0) * r
        return (1.0 + a + 5.0 / 3.0 * r * r) * np.exp(-a)
    raise ValueError(f"kind {kind}")


def kmat(kind, X, Z, inv_ls, variance):
    """K(X, Z) [N, M] in the fill's difference form."""
    diff = (X * inv_ls)[:, None, :] - (Z * inv_ls)[None, :, :]
    return variance * profile(kind, np.sum(diff * diff, axis=-1))


def greedy_select(X, inv_ls, variance, kind, M, threshold=0.0):
    """Returns (indices [count], pivots [count], d [N], count)."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    floor = max(threshold, 1e-12 * variance)
    d = np.full(N, float(variance))
    C = np.zeros((M, N))
    indices, pivots = [], []
    for j in range(M):
        p = int(np.argmax(d))  # the first occurrence of the maximum: the lowest index
        if not d[p] > floor:
            break
        dp = d[p]
        c = (kmat(kind, X, X[p:p + 1], inv_ls, variance)[:, 0] - C[:j].T @ C[:j, p]) / np.sqrt(dp)
        C[j] = c
        d = np.maximum(d - c * c, 0.0)
        d[p] = 0.0
        indices.append(p)
        pivots.append(dp)
    return np.asarray(indices, dtype=np.int64), np.asarray(pivots), d, len(indices)


def nystrom_residual(X, S, inv_ls, variance, kind):
    """variance - diag(K_fS K_SS^-1 K_Sf) [N] by a dense solve; S a sequence of row numbers of X (may be empty).  The solve is LU
    with partial pivoting, not Cholesky: it also goes through for a K_SS that is singular to rounding (the first rows of clustered
    data), where the result is a rough figure, good for a comparison by orders of magnitude only."""
    X = np.asarray(X, dtype=np.float64)
    S = np.asarray(list(S), dtype=np.int64)
    if S.size == 0:
        return np.full(X.shape[0], float(variance))
    Kss = kmat(kind, X[S], X[S], inv_ls, variance)
    Kfs = kmat(kind, X, X[S], inv_ls, variance)
    return variance - np.sum(Kfs.T * np.linalg.solve(Kss, Kfs.T), axis=0)
