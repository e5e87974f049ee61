"""t-VGP, the exact (N x N) conjugate-computation model: mirror of the reference's ``t_VGP`` (reference src/models/tvgp.py).

The state is one diagonal site per datum, lambda_1, lambda_2 [N, 1] (``DiagSites``), and q(f) is proportional to p(f) t(f).  With
s = sqrt|lambda_2|, y~ = lambda_1 / lambda_2, K~ = K(X, X) + default_jitter() I and B = I + s s^T * K~ = L L^T (tvgp.py:78-96):

    post_v = diag K~ - colsum (L^-1 (s * K~))^2,   alpha = s * L^-T L^-1 (s * y~),   post_m = K~ alpha
    ELBO   = log Z - E_q log t + E_q log p(y | f),  log Z = -1/2 y~^T alpha - sum log diag L

No inverse and no N x N solve is formed on the host.  One pass is three launches on one stacked buffer S [(2 Np + 128) x Np]:

    tsvgp_vgp_system_f64    B, the rows R = K~ * s (row n = K~[n, :] s) and the row s y~, one kernel evaluation per pair
    tsvgp_potrf_solve_f64   B = L L^T; the rows ride through the factorisation and come out as C = R L^-T and z = L^-1 (s y~)
    tsvgp_vgp_rows_f64      post_v[n] = (variance + jitter) - |C[n]|^2,  post_m[n] = C[n] z,  the likelihood map, the sums of ve and
                            E_q log t, and the site update in place (update_variational_parameters; elbo runs it with beta = 0)

and log Z = -1/2 z^T z - sum log diag L.  ``predict_f`` (tvgp.py:162-193) factors the UN-jittered I + s s^T * K -- K + diag(1 /
lambda_2) up to the scaling by s -- with K(Xnew, X) s riding as right-hand-side rows; ``full_cov`` goes through ``tsvgp_cov_f64``.

Deviations from the reference: alpha is recomputed from the CURRENT sites (cached on the stamps of the sites and of the kernel
parameters) where the reference predicts with whatever the last ``elbo`` / update left in ``q_alpha``, i.e. the alpha of the sites
BEFORE its last update; a failed factorisation or a non-positive posterior variance raises FloatingPointError and leaves the sites
as they were; ``full_cov=True`` returns [1, N*, N*] as the sibling models do.  One latent GP, the Zero mean function, one
stationary kernel with D <= 32 and a likelihood over one latent.

``elbo_and_grads`` differentiates that ELBO with respect to the kernel variance, the lengthscales and the Gaussian noise variance
with the sites held fixed (reference tests/models/test_tvgp.py: test_gradient_wrt_hyperparameters; TensorFlow autodiff there).
With V = diag(s) L^-T (diag(s) rides through the factorisation as Np further right-hand-side rows), P = V V^T =
(K~ + |Lambda|^-1)^-1, alpha = V z and A^T = I - K~ P = I - C V^T, the posterior moves by dm = A^T dK~ alpha and dv_n = a_n^T dK~ a_n
(a_n column n of A).  With g0, g1 = d ve / d (m, v), never cropped, h0 = g0 - lambda_2 (y~ - m), h1 = g1 + 1/2 lambda_2, u = A h0 and
c = 1/2 alpha + u:

    d ELBO / d K~ = G = W + 1/2 (alpha c^T + c alpha^T),   W = A diag(h1) A^T - 1/2 P,   d ELBO / d theta = sum_ij G_ij dK_ij / d theta

The two N^3 products go through the BLAS library; the contraction with dK / d theta is ``tsvgp_vgp_kernel_grad_f64``, which forms G
in registers from W, alpha and c.  At a fixed point of the sites h0 = h1 = 0 and G = 1/2 (alpha alpha^T - P).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _backend as B
from ..base import default_device, default_float, default_jitter, to_tensor
from ..estep import MAX_INPUT_DIM
from ..kernels import LinearCoregionalization, SeparateIndependent, refuse_sum
from ..sites import DiagSites


class t_VGP:
    """Class for the t-VGP model (reference src/models/tvgp.py:18-193).  Likelihoods: Gaussian and Bernoulli, the arms of the fused
    row sweep (``tsvgp_vgp_rows_f64``); ``StudentT``, ``Poisson``, ``Gamma``, ``Exponential`` and ``Ordinal``, whose map is a kernel of its own behind the moments of
    ``t_SVGP`` / ``t_SVGP_white``, raise NotImplementedError here.  Like ``sample_functions``, the input gradients of the prediction
    (``predict_f_vjp``, ``predict_f`` under torch autograd) belong to the sparse models only: ``predict_f`` here returns no graph."""

    def __init__(self, data, kernel, likelihood, mean_function=None, num_latent=1, *, device=None):
        x_data, y_data = data
        if mean_function is not None:
            raise ValueError("t_VGP: only the default Zero mean function is implemented")
        refuse_sum(kernel, "t_VGP")
        if isinstance(kernel, LinearCoregionalization):
            raise NotImplementedError("t_VGP does not take LinearCoregionalization: mixed outputs are on t_SVGP only")
        if isinstance(kernel, SeparateIndependent):
            raise ValueError("t_VGP takes one kernel: it is defined for one latent GP")
        if getattr(likelihood, "lik_id", None) in B.COUPLED_LIKS or getattr(likelihood, "latent_dim", 1) != 1:
            raise ValueError("t_VGP is defined for a likelihood over one latent GP (tvgp.py:85: sW sW^T * K), got "
                             f"{type(likelihood).__name__}")
        if getattr(likelihood, "lik_id", None) in B.COLUMN_MAP_LIKS:
            raise NotImplementedError(f"t_VGP does not take the {type(likelihood).__name__} likelihood: its likelihood map is fused "
                                      "into tsvgp_vgp_rows_f64, which has Gaussian and Bernoulli arms only; use t_SVGP or t_SVGP_white")
        self.device = torch.device(device) if device is not None else default_device()
        X = to_tensor(x_data, dtype=default_float(), device=self.device).contiguous()
        Y = to_tensor(y_data, dtype=default_float(), device=self.device).contiguous()
        if X.dim() != 2 or X.shape[0] == 0:
            raise ValueError(f"X must be [N, D] with N >= 1, got {tuple(X.shape)}")
        if X.shape[1] > MAX_INPUT_DIM:
            raise ValueError(f"t_VGP builds its N x N system in one fused kernel: D <= {MAX_INPUT_DIM}, got {X.shape[1]}")
        self.num_data = int(X.shape[0])
        self.num_latent = num_latent or int(Y.shape[1])  # tvgp.py:52
        if self.num_latent != 1:
            raise ValueError(f"t_VGP is defined for one latent GP (tvgp.py:85: sW sW^T * K), got num_latent = {self.num_latent}")
        if Y.dim() != 2 or tuple(Y.shape) != (self.num_data, 1):
            raise ValueError(f"Y must be [N, 1] = [{self.num_data}, 1], got {tuple(Y.shape)}")
        self.kernel = kernel
        self.likelihood = likelihood
        self.mean_function = None
        self.num_latent_gps = 1
        self.compute_dtype = default_float()
        self.data = (X, Y)
        self.sites = DiagSites(np.zeros((self.num_data, 1)), 1e-6 * np.ones((self.num_data, 1)), device=self.device)  # tvgp.py:55-57
        self._engine = None
        self._alpha = None  # (key, alpha [N, 1])
        self.name = "t_vgp"

    @property
    def lambda_1(self):
        """first natural parameter [N, 1]"""
        return self.sites.lambda_1

    @property
    def lambda_2(self):
        """second natural parameter [N, 1]"""
        return self.sites.lambda_2

    def _get_engine(self):
        """The HIP kernel launcher; creating it fails loudly when the extension or the GPU is missing."""
        if self._engine is None:
            from ..estep import EStepEngine

            self._engine = EStepEngine(default_float(), self.device)
        return self._engine

    def _as_device(self, a):
        return to_tensor(a, dtype=default_float(), device=self.device).contiguous()

    @staticmethod
    def _judge_info(info):
        if int(info.item()) != 0:
            raise FloatingPointError("Cholesky decomposition was not successful (matrix not positive definite)")

    # -- the pass behind elbo and the update -------------------------------------------------------------------------
    def _pass(self, beta: float):
        """tvgp.py:77-111 / :126-160 on the GPU: returns the ELBO at the sites found on entry; ``beta`` != 0 then moves them."""
        eng = self._get_engine()
        X, Y = self.data
        N = self.num_data
        l1, l2 = self.sites.padded()
        jitter = default_jitter()
        S, Np = eng.vgp_system(X, self.kernel, l1, l2, jitter)
        self._judge_info(eng.vgp_factor(S, Np))  # before the sites change
        z = S[2 * Np, :N]
        log_Z = -0.5 * torch.dot(z, z) - torch.sum(torch.log(torch.diagonal(S[:N, :N])))  # tvgp.py:108-110: y~^T alpha = z^T z
        keep = self.sites._store.clone() if beta != 0.0 else None
        _, _, ve, eqt, nonpos = eng.vgp_rows(S[Np:2 * Np], N, self.kernel.variance.item() + jitter, z=S[2 * Np], Y=Y, l1=l1, l2=l2,
                                             lik_id=self.likelihood.lik_id, lik_param=self.likelihood.lik_param, beta=beta)
        bad = float(nonpos)
        if beta != 0.0:
            if bad:
                self.sites._store.copy_(keep)
            else:  # the kernel wrote through the pointers: tell the caches that key on the parameters
                self.lambda_1.version += 1
                self.lambda_2.version += 1
        if bad:
            raise FloatingPointError(f"non-positive posterior variance or non-finite moments at {bad:.0f} point(s)")
        return log_Z - eqt + ve  # tvgp.py:111

    # -- reference API -------------------------------------------------------------------------------------------------
    def elbo(self) -> torch.Tensor:
        """The evidence lower bound at the current sites (tvgp.py:72-112); a 0-dim fp64 tensor on the device."""
        return self._pass(0.0)

    def maximum_log_likelihood_objective(self, *args, **kwargs) -> torch.Tensor:
        return self.elbo()

    def elbo_and_grads(self):
        """The ELBO at the current sites and its gradient with respect to the kernel variance, the lengthscales and (Gaussian
        likelihood) the noise variance, with the sites held fixed (module docstring).  Returns (elbo, {"variance",
        "lengthscales", "likelihood_variance" (Gaussian only)}): gradients of the ELBO with respect to the constrained parameter
        values, ``lengthscales`` in the parameter's own shape -- the names and conventions of ``t_SVGP.elbo_and_grads``.  The
        sites are not modified; a failed factorisation or a non-positive variance raises FloatingPointError."""
        eng = self._get_engine()
        X, Y = self.data
        N = self.num_data
        k, lik = self.kernel, self.likelihood
        l1, l2 = self.sites.padded()
        jitter = default_jitter()
        S, Np, info, V = eng.vgp_grad_operands(X, k, l1, l2, jitter)
        self._judge_info(info)
        z = S[2 * Np, :N]
        log_Z = -0.5 * torch.dot(z, z) - torch.sum(torch.log(torch.diagonal(S[:N, :N])))
        mean, var, ve, eqt, nonpos = eng.vgp_rows(S[Np:2 * Np], N, k.variance.item() + jitter, z=S[2 * Np], Y=Y, l1=l1, l2=l2,
                                                  lik_id=lik.lik_id, lik_param=lik.lik_param, beta=0.0, want_mean=True,
                                                  want_var=True)
        bad = float(nonpos)
        if bad:
            raise FloatingPointError(f"non-positive posterior variance or non-finite moments at {bad:.0f} point(s)")
        elbo = log_Z - eqt + ve
        g0, g1 = eng.lik_grads(mean, var, Y, lik.lik_id, lik.lik_param)
        lam1, lam2, m, v = l1[:N, 0], l2[:N, 0], mean[:, 0], var[:, 0]
        h0 = g0 - lam2 * (lam1 / lam2 - m)
        h1 = g1 + 0.5 * lam2
        Vn, C = V[:N, :N], S[Np:Np + N, :N]
        alpha = Vn @ z
        At = C @ Vn.transpose(0, 1)  # A^T = I - C V^T
        At.neg_()
        torch.diagonal(At).add_(1.0)
        c = 0.5 * alpha + At.transpose(0, 1) @ h0
        W = eng._get("vgp_W", (Np, Np), default_float())  # rows and columns >= N are never read as values
        Wn = W[:N, :N]
        Wn.addmm_(At.transpose(0, 1), h1[:, None] * At, beta=0.0)  # A diag(h1) A^T
        Wn.addmm_(Vn, Vn.transpose(0, 1), alpha=-0.5)  # - 1/2 P
        dvar, dls = eng.vgp_kernel_grad(X, k, W, alpha, c)
        ls_shape = tuple(k.lengthscales.value.shape)
        grads = {"variance": dvar, "lengthscales": dls.sum().reshape(ls_shape) if k.lengthscales.value.numel() == 1
                 else dls.reshape(ls_shape)}
        if lik.lik_id == B.LIK_GAUSSIAN:
            s2 = lik.lik_param
            res = Y[:, 0] - m
            grads["likelihood_variance"] = torch.sum(-0.5 / s2 + 0.5 * (res * res + v) / (s2 * s2))
        return elbo, grads

    def training_loss(self) -> torch.Tensor:
        return -self.elbo()

    def training_loss_closure(self, *, compile=False):
        """``gpflow.models.InternalDataTrainingLossMixin.training_loss_closure`` [ext]: a zero-argument callable returning the
        negative ELBO (the model owns its data).  ``compile`` is accepted and ignored: there is no tracing compiler here."""
        return self.training_loss

    @property
    def trainable_parameters(self):
        """The parameters an M-step trains: kernel variance and lengthscales and the likelihood's parameters; the sites are not
        trainable and there is no inducing variable."""
        out = [par for par in (self.kernel.variance, self.kernel.lengthscales) if par.trainable]
        out += [par for par in vars(self.likelihood).values() if hasattr(par, "trainable") and par.trainable]
        return tuple(out)

    trainable_variables = trainable_parameters  # GPflow's name for the unconstrained counterparts

    def update_variational_parameters(self, beta=0.05) -> None:
        """One natural-gradient step on every datum's sites (tvgp.py:114-160), in place; the kernel and likelihood parameters are
        read as they are now."""
        beta = float(beta)
        if not (0.0 <= beta <= 1.0):
            raise ValueError("beta must lie in [0, 1]")
        self._pass(beta)

    @property
    def q_alpha(self) -> torch.Tensor:
        """alpha = s * L^-T L^-1 (s * y~) [N, 1] of the current sites (tvgp.py:95): K~ alpha is the posterior mean."""
        k = self.kernel
        key = (self.lambda_1.stamp(), self.lambda_2.stamp(), k.variance.stamp(), k.lengthscales.stamp(), int(k.kind))
        if self._alpha is not None and self._alpha[0] == key:
            return self._alpha[1]
        eng = self._get_engine()
        N = self.num_data
        l1, l2 = self.sites.padded()
        S, Np = eng.vgp_system(self.data[0], k, l1, l2, default_jitter(), rhs_rows=B.TILE)
        s = torch.sqrt(torch.abs(l2[:N, 0]))
        S[Np:].zero_()
        S[Np, :N] = s * (l1[:N, 0] / l2[:N, 0])
        self._judge_info(eng.vgp_factor(S, Np))
        # one triangular vector solve, off the hot path (predict_f only)
        Lt = torch.tril(S[:N, :N]).transpose(0, 1)
        alpha = (s * torch.linalg.solve_triangular(Lt, S[Np, :N, None], upper=True)[:, 0])[:, None].contiguous()
        self._alpha = (key, alpha)
        return alpha

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False):
        """tvgp.py:162-193: mean = K(Xnew, X) alpha [N*, 1]; var = k** - |L0^-1 (s * K(X, Xnew))|^2 [N*, 1] with L0 the factor of
        the un-jittered I + s s^T * K; ``full_cov``: [1, N*, N*]."""
        if full_output_cov:
            raise NotImplementedError("full_output_cov is not implemented (the reference asserts it is False)")
        eng = self._get_engine()
        Xn = self._as_device(Xnew)
        X = self.data[0]
        if Xn.dim() != 2 or Xn.shape[1] != X.shape[1] or Xn.shape[0] == 0:
            raise ValueError(f"Xnew must be [N*, {X.shape[1]}] with N* >= 1, got {tuple(Xn.shape)}")
        alpha = self.q_alpha
        N, Nn = self.num_data, int(Xn.shape[0])
        Nnp = B.round_up(Nn)
        l1, l2 = self.sites.padded()
        k = self.kernel
        variance = k.variance.item()
        S, Np = eng.vgp_system(X, k, l1, l2, 0.0, rhs_rows=Nnp)
        rows = S[Np:]  # [Nnp, Np]: K(Xnew, X), zero in the padding
        eng.se_fill(Xn, X, k.inv_lengthscales(X.shape[1], default_float(), self.device), variance, rows, k.kind)
        mean = rows[:Nn, :N] @ alpha
        rows[:Nn, :N].mul_(torch.sqrt(torch.abs(l2[:N, 0]))[None, :])
        self._judge_info(eng.vgp_factor(S, Np))
        if full_cov:
            cov = torch.empty((Nnp, Nnp), dtype=default_float(), device=self.device)
            eng.cov(rows, cov, Nn, sign=-1.0, X=Xn, inv_ls=k.inv_lengthscales(X.shape[1], default_float(), self.device),
                    variance=variance, kind=k.kind)
            out = cov[:Nn, :Nn][None]
            bad = float((~(torch.diagonal(out[0]) > 0)).sum())
        else:
            _, out, _, _, nonpos = eng.vgp_rows(rows, Nn, variance, want_var=True)
            bad = float(nonpos)
        if bad:
            raise FloatingPointError(f"non-positive predictive variance at {bad:.0f} point(s)")
        return mean, out

    def predict_y(self, Xnew):
        return self.likelihood.predict_mean_and_var(*self.predict_f(Xnew))

    def predict_log_density(self, data):
        Fmu, Fvar = self.predict_f(data[0])
        return self.likelihood.predict_log_density(Fmu, Fvar, self._as_device(data[1]).to(Fmu.dtype))
