"""Function-space samples of the sparse models by pathwise conditioning (Matheron's rule; Wilson, Borovitskiy, Terenin,
Mostowsky, Deisenroth 2020, "Efficiently sampling functions from Gaussian process posteriors" [ext]; nothing in the reference
draws functions).

A draw of latent GP p is a FUNCTION, fixed by a random-feature draw of the prior and by a draw of the inducing values,

    g_s(x) = sqrt(variance / L) sum_l ( w_s[l] cos(Omega_l . x~) + w_s[L + l] sin(Omega_l . x~) ),      x~ = x / lengthscales
    f_s(x) = g_s(x) + sum_m k(x, z_m) V[s, m],      V_s = K6^-1 (u_s - g_s(Z)),      u_s = m + chol(S) eps_s,

with K6 = K(Z, Z) + default_jitter() I and q(u) = N(m, S) of the model.  Evaluating it costs O(N (L + M) S) in one HIP kernel
(``tsvgp_pathwise_f64``) and no N-sized matrix, so the same draw can be read on any grid, in row chunks, on any rank.

Law: E f_s(x) = k(x, Z) K6^-1 m, the mean of ``predict_f``, exactly; the covariance is that of ``predict_f(full_cov=True)`` with
the prior term k(x, x') replaced by its L-feature estimate -- an error of O(variance / sqrt(L)) per prior covariance entry, which
the update carries along as (1 + |k(x, Z) K6^-1|_inf)^2 times that.  At the inducing points the draw interpolates whatever L is:
f_s(Z) = u_s - jitter V_s.  V is a difference of draws divided by K6: its entries grow like cond(K6) and sum_m k(x, z_m) V[s, m]
then cancels that many digits of fp64.

Random numbers: ``tsvgp_mc_normals_f64`` with the caller's seed and generator draw 4 * draw + j:

    j = 0   E [L, D]: sample 0, rows p L + l (p = 0 for a shared kernel: all latents then share Omega), columns d < D
    j = 1   the chi-square normals of the Matern kernels: the same rows, columns 0 .. 2 nu - 1
    j = 2   w [S, 2 L, P]
    j = 3   eps [S, M, P]

Omega = E for the squared exponential and E_l sqrt(2 nu / chi2_l), chi2_l the sum of the 2 nu squared normals of row l, for
Matern-nu (a multivariate Student-t with 2 nu degrees of freedom: the spectral density of the Matern kernel).
"""
from __future__ import annotations

import math

import torch

from . import _backend as B
from .base import default_jitter
from .estep import MAX_INPUT_DIM
from .kernels import SeparateIndependent, Sum, latent_kernels

_CHI2_NORMALS = {B.KERNEL_MATERN32: 3, B.KERNEL_MATERN52: 5}  # 2 nu


def spectral_frequencies(eng, kind: int, seed: int, draw: int, L: int, D: int, p: int = 0) -> torch.Tensor:
    """Omega [L, D] fp64 of latent kernel p (rows p L .. p L + L - 1 of the generator; see the module docstring)."""
    E = eng.mc_normals(1, L, D, seed, 4 * draw, row_offset=p * L)[0]
    nu2 = _CHI2_NORMALS.get(int(kind))
    if nu2 is None:
        return E
    c = eng.mc_normals(1, L, nu2, seed, 4 * draw + 1, row_offset=p * L)[0]
    return E * torch.sqrt(float(nu2) / (c * c).sum(dim=1))[:, None]


class FunctionSamples:
    """``num_samples`` posterior function draws of a sparse model (``base_SVGP.sample_functions``).  Calling it evaluates them:
    ``fs(Xnew) -> [S, N, P]`` fp64 on the model's device, for any N and any number of calls -- the same functions every time, and
    the same bits for the same row of Xnew whatever else is in the call.  Everything the draws depend on was copied when the
    object was made: later changes of the model do not reach it.

    ``u`` [S, M, P]: the inducing values of each draw.  The operands of the evaluation, read-only: ``Omega`` (one [L, D] per
    latent), ``W`` [P, S, 2 L] (scaled by sqrt(variance_p / L)), ``V`` [S, M, P] (the weights of the update), ``Z`` [M, D]."""

    def __init__(self, engine, kernels, Z, Omega, W, V, u, *, seed, draw):
        self._engine = engine
        self._kernels = kernels  # P private copies (or P references to ONE private copy: a shared kernel)
        self.Z = Z
        self.Omega = Omega  # (the same tensor P times for a shared kernel)
        self.W = W
        self._Vt = V.permute(2, 0, 1).contiguous()  # [P, S, M]
        self.V = V
        self.u = u
        self.num_samples = int(u.shape[0])
        self.num_features = int(Omega[0].shape[0])
        self.seed, self.draw = int(seed), int(draw)

    def _rows(self, Xnew) -> torch.Tensor:
        """Xnew on the engine's device in fp64, checked (torch's own ``.to``: gradients pass through it to the caller's leaf)."""
        X = Xnew if isinstance(Xnew, torch.Tensor) else torch.as_tensor(Xnew)
        X = X.to(device=self._engine.device, dtype=torch.float64)
        if X.dim() != 2 or X.shape[1] != self.Z.shape[1]:
            raise ValueError(f"Xnew must be [N, D] = [N, {self.Z.shape[1]}], got {tuple(X.shape)}")
        return X

    def _evaluate(self, X) -> torch.Tensor:
        eng = self._engine
        f = [eng.pathwise(X, self.Z, k, self.Omega[p], self.W[p], self._Vt[p]) for p, k in enumerate(self._kernels)]
        return torch.stack(f, dim=2)  # [S, N, P]

    def __call__(self, Xnew) -> torch.Tensor:
        """The draws at the rows of Xnew, [S, N, P].  With grad mode on and ``Xnew`` a tensor that requires grad, the result takes
        part in autograd: the same values bit for bit, and a backward that is one ``vjp`` (first derivatives only: a second
        derivative raises torch's error for once-differentiable functions).  No graph is kept between calls."""
        X = self._rows(Xnew)
        if torch.is_grad_enabled() and X.requires_grad:
            return _Evaluate.apply(X, self)
        return self._evaluate(X)

    def vjp(self, Xnew, cotangent) -> torch.Tensor:
        """sum_{s, p} cotangent[s, n, p] d f_{s, p}(x_n) / d x_n, [N, D] fp64 on the model's device: the vector-Jacobian product of
        ``fs(Xnew)`` with a cotangent [S, N, P], one ``tsvgp_pathwise_vjp_f64`` per latent (no [S, N, D] Jacobian, no N-sized
        matrix), summed over the latents in their order.  Exact, not a finite difference, and the same bits for the same row
        and cotangent column whatever else is in the call.  A draw is differentiable everywhere for every kernel offered: the
        random-feature part is smooth, and the update term sum_m k(x, z_m) V[s, m] is at least C^1 (the first odd power of
        |x~ - z~| in the profile is the third for Matern-3/2 and the fifth for Matern-5/2; the squared exponential is smooth): at
        an inducing point the gradient of its own term is zero.  Matern-1/2, whose profile has a kink at every inducing point,
        is not offered."""
        eng = self._engine
        X = self._rows(Xnew).detach()
        C = cotangent if isinstance(cotangent, torch.Tensor) else torch.as_tensor(cotangent)
        C = C.detach().to(device=eng.device, dtype=torch.float64)
        want = (self.num_samples, X.shape[0], len(self._kernels))
        if tuple(C.shape) != want:
            raise ValueError(f"cotangent must be [S, N, P] = {list(want)}, got {tuple(C.shape)}")
        dX = None
        for p, k in enumerate(self._kernels):
            part = eng.pathwise_vjp(X, self.Z, k, self.Omega[p], self.W[p], self._Vt[p], C[:, :, p])
            dX = part if dX is None else dX.add_(part)
        return dX


class _Evaluate(torch.autograd.Function):
    """``FunctionSamples.__call__`` for an input that requires grad: forward is the plain evaluation, backward one ``vjp`` at the
    saved (already converted) input."""

    @staticmethod
    def forward(ctx, X, fs):
        ctx.fs = fs
        ctx.save_for_backward(X)
        return fs._evaluate(X.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        (X,) = ctx.saved_tensors
        return ctx.fs.vjp(X, grad), None


def _private_copy(kernel):
    """A kernel of the same class with its own parameters: what the draw keeps of the model's kernel."""
    if isinstance(kernel, Sum):
        return Sum([_private_copy(k) for k in kernel.kernels])
    return type(kernel)(variance=kernel.variance.item(), lengthscales=kernel.lengthscales.value.clone(), active_dims=kernel.active_dims)


def sample_functions(model, eng, num_samples, num_features, seed, draw) -> FunctionSamples:
    """Builds the draws of ``base_SVGP.sample_functions`` on the fp64 launcher ``eng`` (argument checks are the caller's)."""
    S, L, P = int(num_samples), int(num_features), int(model.num_latent_gps)
    Z = model._Z().to(device=eng.device, dtype=torch.float64).contiguous().clone()
    M, D = Z.shape
    if D > MAX_INPUT_DIM:
        raise ValueError(f"sample_functions: the input dimension is limited to {MAX_INPUT_DIM} (TSVGP_MAX_BATCH, the normal "
                         f"generator's column limit), got D = {D}")
    m, chol_S = model.get_mean_chol_cov_inducing_posterior()  # [M, P], [P, M, M]
    separate = isinstance(model.kernel, SeparateIndependent)
    own = [_private_copy(k) for k in latent_kernels(model.kernel, P)] if separate else [_private_copy(model.kernel)] * P
    distinct = own if separate else own[:1]
    Omega = [spectral_frequencies(eng, k.kind, seed, draw, L, D, p) for p, k in enumerate(distinct)]
    K6 = torch.stack([eng.kuu(Z, k) for k in distinct])
    K6.diagonal(dim1=-2, dim2=-1).add_(default_jitter())
    L6, info = eng.cholesky(K6, overwrite=True)
    if float(model._read_flags(info.abs().sum().reshape(1).to(torch.float64))[0]) != 0:
        raise FloatingPointError("Cholesky decomposition was not successful (matrix not positive definite)")
    w = eng.mc_normals(S, 2 * L, P, seed, 4 * draw + 2)
    eps = eng.mc_normals(S, M, P, seed, 4 * draw + 3)
    u = m.to(torch.float64)[None] + torch.einsum("pmk,skp->smp", chol_S.to(torch.float64), eps)  # [S, M, P]
    W = torch.stack([w[:, :, p] * math.sqrt(own[p].variance.item() / L) for p in range(P)]).contiguous()  # [P, S, 2 L]
    V = torch.empty((S, M, P), dtype=torch.float64, device=eng.device)
    for p in range(P):
        q = p if separate else 0
        gZ = eng.pathwise(Z, None, own[p], Omega[q], W[p])  # [S, M]: the prior draws at the inducing points
        t = torch.linalg.solve_triangular(L6[q], (u[:, :, p] - gZ).t(), upper=False)
        V[:, :, p] = torch.linalg.solve_triangular(L6[q].t(), t, upper=True).t()
    return FunctionSamples(eng, own, Z, [Omega[p if separate else 0] for p in range(P)], W, V, u, seed=seed, draw=draw)
