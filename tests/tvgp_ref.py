"""NumPy fp64 restatement of the reference's ``t_VGP`` (reference src/models/tvgp.py), op for op: what the HIP path of
``t-svgp_amd/models/tvgp.py`` is held to.  Likelihood terms come from the oracle module.

``form="solve"`` follows the reference's own operations (Cholesky, triangular solves); ``form="inv"`` computes the same
quantities from explicit inverses, (K~^-1 + diag lambda_2)^-1 for the posterior: the two agree to the conditioning of the
problem, which bounds how far any correct implementation may sit from either (tests/test_tvgp_cpu.py).

Jitter conventions (both in the reference): ``elbo`` / ``update`` use K~ = K + default_jitter I (tvgp.py:82, :131); ``predict_f``
uses the un-jittered K for its variance (tvgp.py:179-186) and an alpha made with the jittered one.
"""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import tsvgp_oracle as O

DEFAULT_JITTER = 1e-6


class TVGPRef:
    def __init__(self, X, Y, kernel, likelihood, form="solve"):
        self.X, self.Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
        self.kernel, self.likelihood, self.form = kernel, likelihood, form
        N = self.X.shape[0]
        self.lambda_1 = np.zeros((N, 1))  # tvgp.py:55-56
        self.lambda_2 = 1e-6 * np.ones((N, 1))
        self.q_alpha = None

    def _posterior(self):
        """tvgp.py:77-96 / :126-140: (post_m, post_v, alpha, L, pseudo_y)."""
        N = self.X.shape[0]
        pseudo_y = self.lambda_1 / self.lambda_2
        sW = np.sqrt(np.abs(self.lambda_2))
        K = self.kernel.K(self.X) + np.eye(N) * DEFAULT_JITTER
        Bm = np.eye(N) + (sW @ sW.T) * K
        L = np.linalg.cholesky(Bm)
        if self.form == "solve":
            T = solve_triangular(L, np.tile(sW, (1, N)) * K, lower=True)
            post_v = (np.diag(K) - np.sum(T * T, axis=0)).reshape(N, 1)
            alpha = sW * solve_triangular(L.T, solve_triangular(L, sW * pseudo_y, lower=True), lower=False)
            post_m = K @ alpha
        else:
            Sigma = np.linalg.inv(np.linalg.inv(K) + np.diag(self.lambda_2[:, 0]))  # (K^-1 + lambda_2)^-1
            post_v = np.diag(Sigma).reshape(N, 1).copy()
            post_m = Sigma @ self.lambda_1
            alpha = np.linalg.inv(K) @ post_m
        return post_m, post_v, alpha, L, pseudo_y

    def elbo(self):
        post_m, post_v, alpha, L, pseudo_y = self._posterior()
        self.q_alpha = alpha
        E_q_log_lik = np.sum(self.likelihood.variational_expectations(post_m, post_v, self.Y))
        E_q_log_t = -np.sum(0.5 * self.lambda_2 * ((pseudo_y - post_m) ** 2 + post_v))
        log_Z = -(pseudo_y.T @ alpha).item() / 2.0 - np.sum(np.log(np.diag(L)))
        return log_Z - E_q_log_t + E_q_log_lik

    def update(self, beta=0.05):
        post_m, post_v, alpha, _, _ = self._posterior()
        self.q_alpha = alpha
        g0, g1 = self.likelihood.variational_expectations_grads(post_m, post_v, self.Y)
        self.lambda_1 = (1.0 - beta) * self.lambda_1 + beta * (g0 - 2.0 * (g1 * post_m))  # tvgp.py:156
        self.lambda_2 = (1.0 - beta) * self.lambda_2 + beta * (-2.0 * g1)  # tvgp.py:157

    def current_alpha(self):
        """alpha of the sites as they are now (the product recomputes it; the reference keeps the last elbo's / update's)."""
        return self._posterior()[2]

    def predict_f(self, Xnew, full_cov=False, alpha=None):
        """tvgp.py:162-193 with the Zero mean function; ``alpha`` None: the current sites' (``current_alpha``)."""
        alpha = self.current_alpha() if alpha is None else alpha
        Kx = self.kernel.K(self.X, Xnew)
        K = self.kernel.K(self.X)
        f_mean = Kx.T @ alpha
        A = K + np.diag(1.0 / self.lambda_2[:, 0])
        if self.form == "solve":
            LiKx = solve_triangular(np.linalg.cholesky(A), Kx, lower=True)
            quad = LiKx.T @ LiKx
        else:
            quad = Kx.T @ np.linalg.inv(A) @ Kx
        if full_cov:
            return f_mean, (self.kernel.K(Xnew) - quad)[None]
        return f_mean, (self.kernel.K_diag(Xnew) - np.diag(quad))[:, None]


def problem(N, D, lik, kernel_name="SquaredExponential", seed=0):
    """The seeded problem of the t_VGP tests: inputs spread so that K(X, X) stays well conditioned (see test_tvgp_cpu)."""
    rng = np.random.RandomState(100 * seed + 7 * N + D)

    def inputs(n):  # D = 1: a shuffled, jittered grid (no near-duplicates), centred; D > 1: a Gaussian cloud a few lengthscales wide
        if D == 1:
            return (0.7 * (rng.permutation(n) + 0.5 * rng.rand(n) - 0.5 * n))[:, None]
        return rng.randn(n, D) * (2.6 / np.sqrt(D))

    X = inputs(N)
    w = rng.randn(D, 1) / np.sqrt(D)
    f = np.sin(X @ w)
    if lik == "gaussian":
        Y = f + 0.3 * rng.randn(N, 1)
        likelihood = O.Gaussian(variance=0.2)
    else:
        Y = (f + 0.3 * rng.randn(N, 1) > 0).astype(np.float64)
        likelihood = O.Bernoulli()
    kernel = getattr(O, kernel_name)(variance=1.3, lengthscales=0.8 + 0.4 * rng.rand(D))
    Xnew = inputs(37) if D > 1 else 0.7 * N * (rng.rand(37, 1) - 0.5)
    return X, Y, kernel, likelihood, Xnew
