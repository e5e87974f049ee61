"""NumPy fp64 restatement of the reference's ``t_SVGP_sites`` (reference src/models/tsvgp_sites.py), op for op, on the oracle's
GPflow restatements (``oracle.tsvgp_oracle``: project_diag_sites, posterior_from_dense_site_white, conditional, prior_kl, the
likelihoods).  The parity target of tests/test_sites_cpu.py and tests/test_gpu_sites.py."""
import numpy as np

from oracle import tsvgp_oracle as O


class t_SVGP_sites:
    """src/models/tsvgp_sites.py:20-191 (Zero mean function; lambda_2 stored as its value, no softplus round trip)."""

    def __init__(self, data, kernel, likelihood, inducing_variable, *, num_latent_gps=1, lambda_1=None, lambda_2=None):
        X, Y = data
        self.data = (np.asarray(X, np.float64), np.asarray(Y, np.float64))  # :53
        self.num_data = self.data[0].shape[0]  # :51-52
        self.kernel, self.likelihood = kernel, likelihood
        self.num_latent_gps = num_latent_gps
        self.inducing_variable = O.inducingpoint_wrapper(inducing_variable)  # :54
        N = self.num_data
        self.lambda_1 = np.zeros((N, num_latent_gps)) if lambda_1 is None else np.array(lambda_1, np.float64)  # :79
        if lambda_2 is None:
            self.lambda_2 = np.ones((N, num_latent_gps)) * 1e-6  # :80-85
        else:
            self.lambda_2 = np.array(lambda_2, np.float64)
            assert self.lambda_2.ndim == 2  # :87
            self.num_latent_gps = self.lambda_2.shape[-1]

    def projection(self, X=None):
        """project_diag_sites(K_uf, lambda_1, lambda_2, cholesky=False) (:109-111): (l [M, P], L [P, M, M])."""
        X = self.data[0] if X is None else X
        K_uf = O.Kuf(self.inducing_variable, self.kernel, X)
        return O.project_diag_sites(K_uf, self.lambda_1, self.lambda_2, cholesky=False)

    def posterior_from(self, l, L):
        K_uu = O.Kuu(self.inducing_variable, self.kernel, jitter=O.DEFAULT_JITTER)  # :106-108
        return O.posterior_from_dense_site_white(K_uu, l, L)  # :112

    def get_mean_chol_cov_inducing_posterior(self):
        return self.posterior_from(*self.projection())

    def prior_kl(self):
        """:150-155 (gpflow prior_kl, whiten=False)."""
        q_mu, q_sqrt = self.get_mean_chol_cov_inducing_posterior()
        return O.prior_kl(self.inducing_variable, self.kernel, q_mu, q_sqrt, whiten=False)

    def predict_f(self, Xnew):
        """:180-191 (gpflow conditional, white=False)."""
        q_mu, q_sqrt = self.get_mean_chol_cov_inducing_posterior()
        return O.conditional(np.asarray(Xnew, np.float64), self.inducing_variable, self.kernel, q_mu, q_sqrt=q_sqrt, white=False)

    def elbo(self):
        """:161-178 (scale = num_data / X.shape[0] = 1)."""
        X, Y = self.data
        kl = self.prior_kl()
        f_mean, f_var = self.predict_f(X)
        ve = self.likelihood.variational_expectations(f_mean, f_var, Y)
        return np.sum(ve) * (self.num_data / X.shape[0]) - kl

    @staticmethod
    def site_update(lambda_1, lambda_2, mean, g0, g1, lr):
        """:133-148 on given moments and gradients: (lambda_1, lambda_2) after one step."""
        g0 = g0 - 2.0 * g1 * mean  # :133
        n1 = (1 - lr) * lambda_1 + lr * g0  # :139
        n2 = (1 - lr) * (-0.5 * lambda_2) + lr * g1  # :136, :140
        n2 = np.minimum(n2, -1e-8 * np.ones_like(n2))  # :144
        return n1, -2.0 * n2  # :147-148

    def natgrad_step(self, lr=0.1):
        """:116-148 (no data argument: self.data)."""
        X, Y = self.data
        mean, var = self.predict_f(X)  # :128
        g0, g1 = self.likelihood.variational_expectations_grads(mean, var, Y)  # :130-131 (GradientTape, no crop)
        self.lambda_1, self.lambda_2 = self.site_update(self.lambda_1, self.lambda_2, mean, g0, g1, lr)
