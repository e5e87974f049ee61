"""t-SVGP with one diagonal site per datum: mirror of the reference's ``t_SVGP_sites`` (reference src/models/tsvgp_sites.py).

The state is lambda_1, lambda_2 [N, 1] (``DiagSites``), one pair per row of the model's own data.  q(u) comes from projecting
the sites onto the inducing points (src/util.py:188-236 with cholesky=False and no K_uu) and the whitened-site posterior
(src/util.py:394-426):

    l = sum_n lambda_1n k_n,   L = sum_n lambda_2n k_n k_n^T      (k_n = K(Z, x_n))
    q(u) = N(m, S),  S = K6 (K6 + L + 1e-9 I)^-1 K6,  m = K6 (K6 + L + 1e-9 I)^-1 l      (K6 = K_uu + 1e-6 I)

which is ``t_SVGP_white``'s q(u) with (lambda_1, Lambda_2) = (l, L).  The N-sized work of one ``natgrad_step``:

    fill K(X, Z) -> projection (tsvgp_site_accum_* with the sites as weights) -> [all-reduce of acc2 | acc1]
    -> M x M operands (t_SVGP_white's, on (l, L); direct / whitened / two-product route as there)
    -> moments with no likelihood on the same K(X, Z) (after the whitening product on the whitened route)
    -> tsvgp_diag_site_step_*: g0, g1 of ve (never cropped) and the in-place update of every row's sites

The moments run with TSVGP_LIK_MEANONLY when ``skip_unused_variance`` is set and the likelihood is Gaussian: neither site
update reads the variance there, so the variance product -- one of the step's two N M^2 products -- is not formed.

Sharding: each rank builds the model on its own row shard (``distributed.shard_rows``) and keeps the sites of those rows; the
projection is the only exchange of a step (one all-reduce), the ELBO's sum of ve is reduced in ``elbo()``, and the scale
factor is 1 (num_data / X.shape[0] of the shard, as in the reference's single process).  Every decision that changes
rounding (the route from rank 0's cond(K6), the factorisation flags of the replicated M x M algebra) is the same on every rank.

Deviations: natgrad_step checks the M x M factorisations before it changes the sites (a failure leaves them untouched and
raises, or repeats the step on the next route, as ``t_SVGP_white`` does), but does not check the sign of the predictive
variance, as the reference does not; ``elbo`` and ``predict_f`` do (FloatingPointError), as ``t_SVGP_white``'s.  Only the
Zero mean function, one latent GP and one shared kernel are defined (the reference's util functions take element [0] of the
latent batch, util.py:425).  Hyperparameter gradients (``elbo_and_grads``) are not implemented: they flow through the
projection's K_uf as well.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _backend as B
from .. import distributed as D_
from ..base import default_jitter, to_tensor
from ..estep import EStepStats
from ..kernels import LinearCoregionalization, SeparateIndependent, refuse_sum
from ..sites import DiagSites
from .tsvgp import _PredictF, base_SVGP
from .tsvgp_white import t_SVGP_white


class t_SVGP_sites(base_SVGP):
    """Class for the t-SVGP model with sites (reference src/models/tsvgp_sites.py:20-191).  Likelihoods: Gaussian and Bernoulli,
    the arms of the fused site step (``tsvgp_diag_site_step_*``); ``StudentT``, ``Poisson``, ``Gamma``, ``Exponential`` and ``Ordinal``, whose map is a kernel of its own
    behind the moments of ``t_SVGP`` / ``t_SVGP_white``, raise NotImplementedError here."""

    # the M x M algebra and the route logic are t_SVGP_white's, on the projected (l, L) in place of its state
    DIRECT_MAX_COND = t_SVGP_white.DIRECT_MAX_COND
    ROBUST_MIN_COND = t_SVGP_white.ROBUST_MIN_COND
    _Z = t_SVGP_white._Z
    _as_device = t_SVGP_white._as_device
    _operands = t_SVGP_white._operands
    _run = t_SVGP_white._run
    _check = t_SVGP_white._check
    _cond_k6 = t_SVGP_white._cond_k6
    _use_direct = t_SVGP_white._use_direct
    _routed = t_SVGP_white._routed
    _white_joint = t_SVGP_white._joint
    _beta_q = staticmethod(t_SVGP_white._beta_q)

    def __init__(self, data, kernel, likelihood, inducing_variable, *, mean_function=None, num_latent_gps: int = 1,
                 lambda_1=None, lambda_2=None, num_latent=1, compute_dtype=None, device=None, projection="auto",
                 skip_unused_variance=False):
        x_data, y_data = data
        if getattr(likelihood, "lik_id", None) in B.COLUMN_MAP_LIKS:
            raise NotImplementedError(f"t_SVGP_sites does not take the {type(likelihood).__name__} likelihood: its likelihood map is "
                                      "fused into tsvgp_diag_site_step_*, which has Gaussian and Bernoulli arms only; use t_SVGP or "
                                      "t_SVGP_white")
        super().__init__(kernel, likelihood, inducing_variable, mean_function=mean_function, num_latent_gps=num_latent_gps,
                         num_data=int(x_data.shape[0]), compute_dtype=compute_dtype, device=device)
        if projection not in ("auto", "whitened", "direct"):
            raise ValueError("projection must be 'auto', 'whitened' or 'direct'")
        self.projection = projection
        self.skip_unused_variance = bool(skip_unused_variance)
        self._cond_cache = None
        self._direct_failed = False
        self._two_product = False
        refuse_sum(kernel, "t_SVGP_sites")
        if isinstance(kernel, LinearCoregionalization):
            raise NotImplementedError("t_SVGP_sites does not take LinearCoregionalization: mixed outputs are on t_SVGP only")
        if isinstance(kernel, SeparateIndependent):
            raise NotImplementedError("t_SVGP_sites takes one shared kernel (util.py:425 takes element [0] of the latent batch)")
        self.num_latent = num_latent or y_data.shape[1]  # tsvgp_sites.py:55
        self.num_inducing = self.inducing_variable.num_inducing
        # X and Y move to the device once, in the compute dtype the kernels read
        self.data = (to_tensor(x_data, dtype=self.compute_dtype, device=self.device).contiguous(),
                     to_tensor(y_data, dtype=self.compute_dtype, device=self.device).contiguous())
        self._init_variational_parameters(self.num_data, lambda_1, lambda_2)
        if getattr(likelihood, "latent_dim", 1) != 1:
            raise NotImplementedError("t_SVGP_sites is defined for one latent GP: a likelihood over several latents "
                                      f"({type(likelihood).__name__}, latent_dim = {likelihood.latent_dim}) needs t_SVGP")
        if self.data[1].dim() != 2 or self.data[1].shape[0] != self.num_data or self.data[1].shape[1] != 1:
            raise ValueError(f"Y must be [N, 1] = [{self.num_data}, 1], got {tuple(self.data[1].shape)}")
        self.whiten = False  # tsvgp_sites.py:59
        self._w32 = None  # fp32 copies of the sites (the fp32 projection's weights) and the parameter stamps they were made at
        self.name = "t_svgp_sites"

    def _init_variational_parameters(self, num_inducing, lambda_1, lambda_2):
        """lambda_1 = 0, lambda_2 = 1e-6 [N, P] (tsvgp_sites.py:61-89); ``num_inducing`` is the number of data, as there."""
        lambda_1 = np.zeros((num_inducing, self.num_latent_gps)) if lambda_1 is None else lambda_1
        if lambda_2 is None:
            lambda_2 = np.ones((num_inducing, self.num_latent_gps)) * 1e-6
        else:
            lambda_2 = lambda_2.value if hasattr(lambda_2, "value") else lambda_2
            assert lambda_2.ndim == 2
            self.num_latent_gps = lambda_2.shape[-1]
        if self.num_latent_gps != 1:
            raise NotImplementedError("posterior_from_dense_site_white takes element [0] of the latent batch (util.py:425): "
                                      "only num_latent_gps = 1 is defined")
        self.sites = DiagSites(lambda_1.value if hasattr(lambda_1, "value") else lambda_1, lambda_2, device=self.device)

    @property
    def lambda_1(self):
        """first natural parameter [N, P]"""
        return self.sites.lambda_1

    @property
    def lambda_2(self):
        """second natural parameter [N, P]"""
        return self.sites.lambda_2

    # -- projection ----------------------------------------------------------------------------------------------
    def _weights(self):
        """The padded fp64 state (l1, l2) [Np, 1] and the weights the projection reads: the state itself (fp64) or its fp32
        copies, refreshed only when a parameter was assigned or edited since they were made (the step keeps them current)."""
        l1, l2 = self.sites.padded()
        if self.compute_dtype == torch.float64:
            return l1, l2, l1, l2
        key = (self.lambda_1.stamp(), self.lambda_2.stamp())
        if self._w32 is None or self._w32[0] != key:
            self._w32 = (key, l1.to(torch.float32), l2.to(torch.float32))
        return l1, l2, self._w32[1], self._w32[2]

    def _project(self):
        """(l [M, 1], L [1, M, M], ticket): the projection of every rank's sites (one all-reduce of the packed sums) and the
        ticket that hands this rank's K(X, Z) to the moments of the same step."""
        eng = self._get_engine()
        X = self.data[0]
        _, _, w1, w2 = self._weights()
        acc2, acc1, ticket = eng.project_diag(X, self._Z(), self.kernel, w1, w2)
        zero = torch.zeros((), dtype=torch.float64, device=self.device)
        st = EStepStats(n_rows=X.shape[0], ve_sum=zero, nonpos=zero, acc2=acc2, acc1=acc1)
        acc2, acc1, _, _, _, _ = D_.reduce_stats(st, 1, self.num_inducing, True, self._reduce(), eng)
        L = 0.5 * (acc2 + acc2.transpose(-1, -2))
        return acc1.transpose(-1, -2), L, ticket

    # -- reference API -------------------------------------------------------------------------------------------
    def _posterior(self, l, L):
        """posterior_from_dense_site_white(K6, l, L) (util.py:394-426): (m [M, 1], chol S [1, M, M], K6)."""
        eng = self._get_engine()
        Kzz = eng.kuu(self._Z(), self.kernel)
        Id = torch.eye(Kzz.shape[0], dtype=torch.float64, device=Kzz.device)
        K6 = Kzz + default_jitter() * Id
        LR = torch.linalg.cholesky(K6 + L[0] + 1e-9 * Id)
        iLRK = torch.linalg.solve_triangular(LR, K6, upper=False)
        S_q = iLRK.transpose(-1, -2) @ iLRK
        m_q = K6 @ torch.cholesky_solve(l, LR)
        return m_q, torch.linalg.cholesky(S_q)[None], K6

    def get_mean_chol_cov_inducing_posterior(self):
        """tsvgp_sites.py:101-114: K_uu with default_jitter, the projection of the sites, posterior_from_dense_site_white."""
        l, L, _ = self._project()
        m_q, chol_S, _ = self._posterior(l, L)
        return m_q, chol_S

    def _prior_kl(self, l, L):
        """gpflow gauss_kl(q_mu, q_sqrt, K6) [ext], non-white (tsvgp_sites.py:150-155)."""
        m_q, Lq, K6 = self._posterior(l, L)
        Lp = torch.linalg.cholesky(K6)
        alpha = torch.linalg.solve_triangular(Lp, m_q, upper=False)
        LpiLq = torch.linalg.solve_triangular(Lp, Lq[0], upper=False)
        M = K6.shape[0]
        two_kl = (torch.sum(alpha * alpha) - float(M) - torch.sum(torch.log(torch.square(torch.diagonal(Lq[0]))))
                  + torch.sum(LpiLq * LpiLq) + torch.sum(torch.log(torch.square(torch.diagonal(Lp)))))
        return 0.5 * two_kl

    def prior_kl(self):
        l, L, _ = self._project()
        return self._prior_kl(l, L)

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False):
        """tsvgp_sites.py:180-191: gpflow conditional(q_mu, q_sqrt = chol S, white=False), which is
        mean = k^T R^-1 l, var = kff - k^T (K6^-1 - R^-1) k with R = K6 + L + 1e-9 I: t_SVGP_white's moments on (l, L).
        ``full_cov``: cov [1, N, N] over the rows of Xnew; ``full_output_cov``: [N, 1, 1].  With the default flags and a Xnew that
        requires grad the result takes part in torch autograd (``t_SVGP.predict_f``)."""
        if full_cov and full_output_cov:
            raise NotImplementedError(self._BOTH_COV)
        if full_cov:
            return self._joint(Xnew)
        Xg = None if full_output_cov else self._grad_rows(Xnew)
        if Xg is not None:
            return _PredictF.apply(Xg, self)
        mean, var = self._predict_marginal(self._as_device(Xnew))
        return mean, (torch.diag_embed(var) if full_output_cov else var)

    def _predict_marginal(self, Xd, want_operands=False):
        l, L, _ = self._project()
        return t_SVGP_white._predict_marginal(self, Xd, want_operands, l, L)

    def _predict_operands(self):
        l, L, _ = self._project()
        return t_SVGP_white._predict_operands(self, l, L)

    def _joint(self, Xnew, padded=False, engine=None):
        """t_SVGP_white's joint covariance on the projected (l, L)."""
        l, L, _ = self._project()
        return self._white_joint(Xnew, padded, engine, lambda_1=l, lambda_2=L)

    def predict_y(self, Xnew):
        return self.likelihood.predict_mean_and_var(*self.predict_f(Xnew))

    def predict_log_density(self, data):
        Fmu, Fvar = self.predict_f(data[0])
        return self.likelihood.predict_log_density(Fmu, Fvar, self._as_device(data[1]).to(Fmu.dtype))

    def maximum_log_likelihood_objective(self):
        return self.elbo()

    def training_loss(self):
        return -self.elbo()

    def elbo(self):
        """tsvgp_sites.py:161-178: sum ve * num_data / X.shape[0] - prior_kl, the scale being 1; with more than one rank the sum
        runs over every rank's rows."""
        X, Y = self.data
        l, L, ticket = self._project()
        kl = self._prior_kl(l, L)

        def go(direct, two_product):
            ops = self._operands(lambda_1=l, lambda_2=L, direct=direct, two_product=two_product)
            st = self._run_on(X, Y, ops, self.likelihood.lik_id | B.LIK_NOCROP, ticket)
            _, _, ve_sum, nonpos, _, _ = D_.reduce_stats(st, 1, self.num_inducing, False, self._reduce(), self._get_engine())
            self._check(ops, nonpos)
            return ve_sum - kl

        return self._routed(go)

    def _run_on(self, X, Y, ops, lik_id, ticket):
        """``_run`` on the K(X, Z) the projection left (no second fill)."""
        eng = self._get_engine()
        if ops.get("two_product"):
            return eng.run_two_product(X, Y, ops["Z"], self.kernel, whiten_T=ops["whiten_T"], moment_Tm=ops["moment_Tm"],
                                       gamma=ops["gamma"], lik_id=lik_id, lik_param=self.likelihood.lik_param, prefill=ticket)
        return eng.run(X, Y, ops["Z"], self.kernel, moment_Tm=ops["moment_Tm"], moment_mode=ops["moment_mode"],
                       gamma=ops["gamma"], lik_id=lik_id, lik_param=self.likelihood.lik_param, whiten_T=ops["whiten_T"],
                       whiten_mode=B.TRI_UPPER, prefill=ticket)

    def natgrad_step(self, lr=0.1):
        """One natural-gradient step on every datum's sites (tsvgp_sites.py:116-148); uses ``self.data``, returns None."""
        if not (0.0 <= float(lr) <= 1.0):
            raise ValueError("lr must lie in [0, 1]")
        eng = self._get_engine()
        X, Y = self.data
        l1, l2, w1, w2 = self._weights()
        l, L, ticket = self._project()
        lik_id = self.likelihood.lik_id
        mean_only = self.skip_unused_variance and lik_id == B.LIK_GAUSSIAN
        zero = torch.zeros(1, dtype=torch.float64, device=self.device)

        def go(direct, two_product):
            ops = self._operands(lambda_1=l, lambda_2=L, direct=direct, two_product=two_product)
            if two_product:
                st = eng.run_two_product(X, None, ops["Z"], self.kernel, whiten_T=ops["whiten_T"], moment_Tm=ops["moment_Tm"],
                                         gamma=ops["gamma"], want_moments=True, prefill=ticket)
                mean = st.mean.to(self.compute_dtype).contiguous()
                var = None if mean_only else st.var.to(self.compute_dtype).contiguous()
            else:
                mean, var = eng.diag_sites_moments(X, ops["Z"], self.kernel, ticket, whiten_T=ops["whiten_T"],
                                                   moment_Tm=ops["moment_Tm"], moment_mode=ops["moment_mode"], gamma=ops["gamma"],
                                                   mean_only=mean_only)
            self._check(ops, zero)  # the M x M factorisations (replicated: every rank decides alike) before the sites change
            return mean, var

        if X.shape[0] == 0:  # a rank with no rows: the replicated M x M algebra and its checks only
            self._routed(lambda direct, two_product: self._check(
                self._operands(lambda_1=l, lambda_2=L, direct=direct, two_product=two_product), zero))
            return
        mean, var = self._routed(go)
        # (the fp32 copies w1, w2 are written by the same launch: they stay current)
        eng.diag_site_step(mean, var, Y, lik_id, self.likelihood.lik_param, lr, l1, l2,
                           *((w1, w2) if self.compute_dtype == torch.float32 else ()))

    def elbo_and_grads(self, *args, **kwargs):
        raise NotImplementedError("hyperparameter gradients of t_SVGP_sites also flow through the projection's K_uf; "
                                  "not implemented")
