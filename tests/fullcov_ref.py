"""NumPy fp64 restatement of the joint predictions the models offer: GPflow's ``base_conditional(full_cov=True)`` and
``GPModel.predict_f_samples`` / ``sample_mvn`` (GPflow 2.2.1 [ext]: recalled, as the oracle's other [ext] items), driven by a
model's q(u) = N(m, S) from ``get_mean_chol_cov_inducing_posterior()`` -- the oracle's ``t_SVGP`` / ``t_SVGP_white`` or
``tests/sites_ref.t_SVGP_sites``.  The reference reaches this through ``gpflow.conditionals.conditional(..., full_cov=full_cov)``
(reference src/models/tsvgp.py:103-112, src/models/tsvgp_white.py:122, src/models/tsvgp_sites.py:179-187).

    Lm = chol(Kuu + 1e-6 I);  A = Lm^-1 Kmn;  c = Knn - A^T A;  A <- Lm^-T A;  mean = A^T m
    cov_p = c + (tril(S_p)^T A)^T (tril(S_p)^T A)                       S_p = chol(S)[p]
"""
import numpy as np

from oracle import tsvgp_oracle as O


def base_conditional_full_cov(Kmn, Kmm, Knn, f, q_sqrt):
    """Kmn [M, N], Kmm [M, M] (jitter included), Knn [N, N], f [M, R], q_sqrt [R, M, M] -> mean [N, R], cov [R, N, N]."""
    Lm = np.linalg.cholesky(Kmm)
    A = O._trsm(Lm, Kmn, lower=True)
    c = Knn - A.T @ A
    A = O._trsm(Lm, A, lower=True, adjoint=True)
    mean = A.T @ f
    cov = []
    for r in range(f.shape[-1]):
        LTA = np.tril(q_sqrt[r]).T @ A
        cov.append(c + LTA.T @ LTA)
    return mean, np.stack(cov)


def predict_f_full_cov(model, Xnew):
    """(mean [N, P], cov [P, N, N]) of ``model`` (anything with kernel, inducing_variable and q(u)) at Xnew [N, D]."""
    Xnew = np.asarray(Xnew, np.float64)
    q_mu, q_sqrt = model.get_mean_chol_cov_inducing_posterior()
    iv, kernel = model.inducing_variable, model.kernel
    Kmm = O.Kuu(iv, kernel, jitter=O.DEFAULT_JITTER)
    Kmn = O.Kuf(iv, kernel, Xnew)
    if isinstance(kernel, O.SeparateIndependent):  # separate_independent_conditional [ext]: base_conditional per latent
        outs = [base_conditional_full_cov(Kmn[p], Kmm[p], k.K(Xnew), q_mu[:, p:p + 1], q_sqrt[p:p + 1])
                for p, k in enumerate(kernel.kernels)]
        return np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=0)
    return base_conditional_full_cov(Kmn, Kmm, kernel.K(Xnew), q_mu, q_sqrt)


def sample_mvn_full_cov(mean, cov, epsilon, jitter=O.DEFAULT_JITTER):
    """f[s, :, p] = mean[:, p] + chol(cov_p + jitter I) eps[s, :, p]; mean [N, P], cov [P, N, N], epsilon [S, N, P] -> [S, N, P]."""
    mean, cov, eps = np.asarray(mean, np.float64), np.asarray(cov, np.float64), np.asarray(epsilon, np.float64)
    N = mean.shape[0]
    out = np.empty_like(eps)
    for p in range(mean.shape[1]):
        L = np.linalg.cholesky(cov[p] + jitter * np.eye(N))
        out[:, :, p] = mean[None, :, p] + eps[:, :, p] @ L.T
    return out


def sample_mvn_diag(mean, var, epsilon):
    """f = mean + sqrt(var) eps; mean, var [N, P], epsilon [S, N, P]."""
    return np.asarray(mean, np.float64)[None] + np.sqrt(np.asarray(var, np.float64))[None] * np.asarray(epsilon, np.float64)


def cov_update(T, sign, base):
    """What ``tsvgp_cov_*`` computes on the valid block: base + sign T T^T."""
    T = np.asarray(T, np.float64)
    return np.asarray(base, np.float64) + sign * (T @ T.T)
