"""Covariance functions on the hot path.

``SquaredExponential`` mirrors ``gpflow.kernels.SquaredExponential`` (the kernel every reference test, notebook and
experiment on this path uses: reference tests/models/test_tsvgp.py:100, experiments/uci_regression.py:186-187).
The N-sized evaluations K(X, Z) run in the HIP fill kernel (``tsvgp_se_fill_*``); nothing here loops over data.

``Sum`` (``k1 + k2``) adds up to four stationary components, each with its own variance, lengthscales and ``active_dims``;
its K(X, Z) is one launch of ``tsvgp_kernel_fill_sum_*`` ("Sum kernels").  ``Product`` (``k1 * k2``) multiplies them:
one launch of ``tsvgp_kernel_fill_prod_*`` for K(X, Z), one of ``tsvgp_kernel_grad_prod_*`` for the M-step contraction of all
components ("Product kernels").
"""
from __future__ import annotations

import torch

from .base import Parameter, to_tensor


class SquaredExponential:
    """k(x, z) = variance * exp(-0.5 * sum_d ((x_d - z_d) / lengthscales_d)^2)."""

    kind = 0  # TSVGP_KERNEL_SE: selects the profile inside the HIP fill kernel (include/tsvgp_hip.h)

    def __init__(self, variance=1.0, lengthscales=1.0, name=None, active_dims=None):
        self.variance = Parameter(variance)
        self.lengthscales = Parameter(lengthscales)
        self.name = name or type(self).__name__.lower()
        # the input columns this kernel acts on (gpflow's ``active_dims`` as a list); None: all of them.  On the device an
        # inactive column is a zero in inv_lengthscales(): no HIP kernel knows about it
        self.active_dims = None if active_dims is None else tuple(int(d) for d in active_dims)
        if self.active_dims is not None:
            if not self.active_dims or min(self.active_dims) < 0 or len(set(self.active_dims)) != len(self.active_dims):
                raise ValueError(f"active_dims must be a non-empty list of distinct column indices >= 0, got {active_dims}")
            ls = self.lengthscales.value
            if ls.dim() > 0 and ls.shape[0] != len(self.active_dims):
                raise ValueError(f"lengthscales has {ls.shape[0]} entries but active_dims names {len(self.active_dims)} columns")

    @property
    def ard(self) -> bool:
        return self.lengthscales.value.dim() > 0

    def __add__(self, other):
        return Sum([self, other])

    def __mul__(self, other):
        return Product([self, other])

    def stamp(self):
        """Cache key of the kernel's hyperparameters (identity + ``Parameter.stamp`` of each): what a carried-over K(X, Z), a
        cached factor or a captured graph that baked them in is keyed on."""
        return (id(self), self.variance.stamp(), self.lengthscales.stamp())

    def prior_variance(self) -> float:
        """k(x, x) as a Python float (no device read): the E-step's scalar ``kdiag``."""
        return self.variance.item()

    def gather_lengthscale_grad(self, dls: torch.Tensor) -> torch.Tensor:
        """The [D] lengthscale gradient of the HIP contraction in the shape of the parameter: the active columns (an ARD
        parameter) or their sum (an isotropic one)."""
        if self.active_dims is not None:
            dls = dls[list(self.active_dims)]
        return dls if self.ard else dls.sum()

    def inv_lengthscales(self, D: int, dtype=None, device=None) -> torch.Tensor:
        """[D] vector of 1/lengthscale (isotropic values are broadcast)."""
        # cached per parameter version: the E-step asks for it twice per step (K_uu, K(X, Z)) right behind the status
        # read of the previous step, where the GPU waits for the host
        # keyed on the Parameter object and on the tensor behind it as well: a replaced Parameter restarts its version at 0,
        # an in-place edit of .value bumps only the tensor's own counter.  The returned tensor is shared: read-only.
        par = self.lengthscales
        key = (id(par), par.version, par.value.data_ptr(), par.value._version, D, dtype, str(device))
        if self.active_dims is not None:
            return self._inv_lengthscales_active(key + (self.active_dims,), D, dtype, device)
        hit = self.__dict__.get("_inv_ls_cache")
        if hit is not None and hit[0] == key:
            return hit[1]
        ls = self.lengthscales.value
        if ls.dim() == 0:
            ls = ls.expand(D)
        if ls.shape[0] != D:
            raise ValueError(f"lengthscales has {ls.shape[0]} entries but the inputs have {D} columns")
        out = to_tensor(1.0 / ls, dtype, device).contiguous()
        self.__dict__["_inv_ls_cache"] = (key, out)
        return out

    def _inv_lengthscales_active(self, key, D, dtype, device) -> torch.Tensor:
        """``inv_lengthscales`` with ``active_dims``: zeros on the inactive columns -- (x_d - z_d) * 0 drops them from every
        scaled distance.  One cached vector per (D, dtype, device): an fp32 engine asks for the fp64 vector (K_uu) and the fp32
        one (K(X, Z)) in turn, and a step replayed from a captured graph must find both (the scatter below reads an index
        tensor made on the host, which a stream capture does not permit)."""
        slots = self.__dict__.setdefault("_inv_ls_slots", {})
        slot = (D, dtype, str(device))
        hit = slots.get(slot)
        if hit is not None and hit[0] == key:
            return hit[1]
        if max(self.active_dims) >= D:
            raise ValueError(f"active_dims {list(self.active_dims)} names a column beyond the inputs' {D}")
        ls = self.lengthscales.value
        inv = torch.zeros(D, dtype=ls.dtype, device=ls.device)
        inv[list(self.active_dims)] = 1.0 / (ls.expand(len(self.active_dims)) if ls.dim() == 0 else ls)
        out = to_tensor(inv, dtype, device).contiguous()
        slots[slot] = self.__dict__["_inv_ls_cache"] = (key, out)
        return out

    def K_diag(self, X) -> torch.Tensor:
        X = to_tensor(X)
        return self.variance.value.expand(X.shape[0]).clone()

    @staticmethod
    def _profile(s: torch.Tensor) -> torch.Tensor:
        return torch.exp(-0.5 * s)

    def K_torch(self, Z: torch.Tensor, variance: torch.Tensor, lengthscales: torch.Tensor) -> torch.Tensor:
        """K(Z, Z) as a differentiable torch expression of (variance, lengthscales, Z), difference form like the HIP
        fill.  Only for the M x M part of the M-step gradient (``t_SVGP.elbo_and_grads``); N-sized work never comes here."""
        if self.active_dims is not None:
            Z = Z[:, list(self.active_dims)]
        Zs = Z / lengthscales
        diff = Zs[:, None, :] - Zs[None, :, :]
        return variance * self._profile(torch.sum(diff * diff, dim=-1))


class Matern32(SquaredExponential):
    """``gpflow.kernels.Matern32`` [ext]: variance * (1 + sqrt(3) r) exp(-sqrt(3) r)."""

    kind = 2

    @staticmethod
    def _profile(s):
        a = torch.sqrt(3.0 * torch.clamp(s, min=1e-36))
        return (1.0 + a) * torch.exp(-a)


class Matern52(SquaredExponential):
    """``gpflow.kernels.Matern52`` [ext] (reference experiments/uci_regression.py:42-44):
    variance * (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)."""

    kind = 3

    @staticmethod
    def _profile(s):
        sc = torch.clamp(s, min=1e-36)
        a = torch.sqrt(5.0 * sc)
        return (1.0 + a + 5.0 / 3.0 * sc) * torch.exp(-a)


class Sum:
    """``gpflow.kernels.Sum`` [ext] of 1 to ``MAX_COMPONENTS`` stationary kernels (``SquaredExponential`` / ``Matern32`` /
    ``Matern52``, each with its own variance, lengthscales and ``active_dims``): k(x, z) = sum_c k_c(x, z), one latent GP.
    k(x, x) = sum_c variance_c stays a constant, so everything behind the fill takes it unchanged; K(X, Z) is ONE launch of
    ``tsvgp_kernel_fill_sum_*``."""

    MAX_COMPONENTS = 4  # TSVGP_MAX_COMPONENTS

    def __init__(self, kernels, name=None):
        flat = []
        for k in kernels:
            flat.extend(k.kernels if isinstance(k, Sum) else [k])
        if not flat:
            raise ValueError("Sum needs at least one component kernel")
        for k in flat:
            if isinstance(k, Product):
                raise NotImplementedError("a Sum of Product kernels is not implemented (the fused fill adds or multiplies "
                                          "stationary components, not both)")
            if isinstance(k, SeparateIndependent):
                raise ValueError(f"a Sum component must be a single-output stationary kernel, got the multi-output {type(k).__name__}")
            if not isinstance(k, SquaredExponential):
                raise ValueError(f"a Sum component must be SquaredExponential, Matern32 or Matern52, got {type(k).__name__}")
        if len(flat) > self.MAX_COMPONENTS:
            raise ValueError(f"Sum takes at most {self.MAX_COMPONENTS} components (TSVGP_MAX_COMPONENTS), got {len(flat)}")
        self.kernels = flat
        self.name = name or "sum"

    def __add__(self, other):
        return Sum([self, other])

    def __mul__(self, other):
        raise NotImplementedError("Sum * kernel: a Product of a Sum kernel is not implemented (the fused fill adds or multiplies "
                                  "stationary components, not both)")

    @property
    def kinds(self):
        return tuple(int(k.kind) for k in self.kernels)

    def stamp(self):
        """Covers every component's parameters (see ``SquaredExponential.stamp``)."""
        return (id(self),) + tuple(k.stamp() for k in self.kernels)

    def prior_variance(self) -> float:
        """k(x, x) = sum_c variance_c as a Python float (no device read), the components added in index order."""
        total = 0.0
        for k in self.kernels:
            total += k.variance.item()
        return total

    def variances(self):
        return [k.variance.item() for k in self.kernels]

    def inv_lengthscales(self, D: int, dtype=None, device=None) -> torch.Tensor:
        """[C, D] (contiguous): one row of 1/lengthscale per component, zeros on its inactive columns.  Cached per stamp of the
        components' lengthscales, one array per (D, dtype, device) as ``_inv_lengthscales_active``."""
        key = tuple(k.lengthscales.stamp() + (k.lengthscales.value.data_ptr(), k.active_dims) for k in self.kernels)
        slots = self.__dict__.setdefault("_inv_ls_slots", {})
        slot = (D, dtype, str(device))
        hit = slots.get(slot)
        if hit is not None and hit[0] == key:
            return hit[1]
        out = torch.stack([k.inv_lengthscales(D, dtype, device) for k in self.kernels]).contiguous()
        slots[slot] = (key, out)
        return out

    def K_diag(self, X) -> torch.Tensor:
        out = self.kernels[0].K_diag(X)
        for k in self.kernels[1:]:
            out = out + k.K_diag(X)
        return out

    def K_torch(self, Z: torch.Tensor, variances, lengthscales) -> torch.Tensor:
        """K(Z, Z) as a differentiable torch expression of (Z, the components' variances and lengthscales: one entry per
        component each), the components added in index order."""
        out = None
        for k, v, ls in zip(self.kernels, variances, lengthscales):
            Kc = k.K_torch(Z, v, ls)
            out = Kc if out is None else out + Kc
        return out


class Product:
    """``gpflow.kernels.Product`` [ext] of 1 to ``MAX_COMPONENTS`` stationary kernels (as the components of a ``Sum``):
    k(x, z) = prod_c k_c(x, z), one latent GP.  k(x, x) = prod_c variance_c is a constant, so everything behind the fill takes it
    unchanged; K(X, Z) is ONE launch of ``tsvgp_kernel_fill_prod_*`` and the M-step contraction of all components ONE launch of
    ``tsvgp_kernel_grad_prod_*``.  The component bookkeeping (``kinds``, ``stamp``, ``variances``, ``inv_lengthscales`` and its
    cache slots) is ``Sum``'s own; the two are siblings, so ``isinstance(k, Sum)`` never takes a product down a linear path."""

    MAX_COMPONENTS = Sum.MAX_COMPONENTS
    kinds = Sum.kinds
    stamp = Sum.stamp
    variances = Sum.variances
    inv_lengthscales = Sum.inv_lengthscales

    def __init__(self, kernels, name=None):
        flat = []
        for k in kernels:
            flat.extend(k.kernels if isinstance(k, Product) else [k])
        if not flat:
            raise ValueError("Product needs at least one component kernel")
        for k in flat:
            if isinstance(k, SeparateIndependent):
                raise ValueError(f"a Product component must be a single-output stationary kernel, got the multi-output {type(k).__name__}")
            if isinstance(k, Sum):
                raise NotImplementedError("a Product of a Sum kernel is not implemented (the fused fill adds or multiplies "
                                          "stationary components, not both)")
            if not isinstance(k, SquaredExponential):
                raise ValueError(f"a Product component must be SquaredExponential, Matern32 or Matern52, got {type(k).__name__}")
        if len(flat) > self.MAX_COMPONENTS:
            raise ValueError(f"Product takes at most {self.MAX_COMPONENTS} components (TSVGP_MAX_COMPONENTS), got {len(flat)}")
        self.kernels = flat
        self.name = name or "product"

    def __add__(self, other):
        raise NotImplementedError("Product + kernel: a Sum of Product kernels is not implemented (the fused fill adds or multiplies "
                                  "stationary components, not both)")

    def __mul__(self, other):
        return Product([self, other])

    def prior_variance(self) -> float:
        """k(x, x) = prod_c variance_c as a Python float (no device read), the components multiplied in index order."""
        total = 1.0
        for k in self.kernels:
            total *= k.variance.item()
        return total

    def K_diag(self, X) -> torch.Tensor:
        out = self.kernels[0].K_diag(X)
        for k in self.kernels[1:]:
            out = out * k.K_diag(X)
        return out

    def K_torch(self, Z: torch.Tensor, variances, lengthscales) -> torch.Tensor:
        """K(Z, Z) as a differentiable torch expression of (Z, the components' variances and lengthscales: one entry per
        component each), the components multiplied in index order."""
        out = None
        for k, v, ls in zip(self.kernels, variances, lengthscales):
            Kc = k.K_torch(Z, v, ls)
            out = Kc if out is None else out * Kc
        return out


COMBINED = (Sum, Product)  # one latent GP behind C stationary components: a constant k(x, x), one fused fill


def refuse_sum(kernel, where: str):
    """``NotImplementedError`` for a ``Sum`` or ``Product`` kernel where only a single stationary kernel is implemented."""
    if isinstance(kernel, Product):
        raise NotImplementedError(f"{where} does not take a Product kernel (a single SquaredExponential / Matern32 / Matern52 only)")
    if isinstance(kernel, Sum):
        raise NotImplementedError(f"{where} does not take a Sum kernel (a single SquaredExponential / Matern32 / Matern52 only)")


def refuse_product(kernel, where: str):
    """``NotImplementedError`` for a ``Product`` kernel where a ``Sum`` is taken but the product's own kernel is a later step."""
    if isinstance(kernel, Product):
        raise NotImplementedError(f"{where} does not take a Product kernel (it needs a kernel of its own, a later step)")


class SeparateIndependent:
    """``gpflow.kernels.SeparateIndependent`` [ext]: P independent latent GPs, one kernel each, no mixing matrix
    (reference docs/notebooks/heteroskedastic.py:62-67).  Used with ``SharedIndependentInducingVariables``; the
    E-step then carries K_uu as [P, M, M] (batched factorisations) and fills K(X, Z) once per latent."""

    def __init__(self, kernels, name=None):
        self.kernels = list(kernels)
        if not self.kernels:
            raise ValueError("SeparateIndependent needs at least one kernel")
        for k in self.kernels:
            refuse_sum(k, type(self).__name__)
        self.name = name or "separate_independent"

    @property
    def num_latent_gps(self) -> int:
        return len(self.kernels)

    def K_diag(self, X) -> torch.Tensor:
        return torch.stack([k.K_diag(X) for k in self.kernels], dim=1)  # [N, P]


class LinearCoregionalization(SeparateIndependent):
    """``gpflow.kernels.LinearCoregionalization(kernels, W)`` [ext]: P outputs f = W g mixed from L independent latent GPs g_l,
    one kernel each, W [P, L].  The sites, K_uu [L, M, M] and every N M^2-sized launch belong to the L latents exactly as under
    ``SeparateIndependent``; the mixing runs per row between the moments and the likelihood map (``tsvgp_lmc_mix_*``) and the
    chain rule back between the map and the site sums (``tsvgp_lmc_unmix_*``).  The likelihood sees Y [N, P]."""

    MAX_DIM = 32  # TSVGP_MAX_BATCH: the two kernels stage W [P, L] into LDS

    def __init__(self, kernels, W, name=None):
        super().__init__(kernels, name=name or "linear_coregionalization")
        self.W = W if isinstance(W, Parameter) else Parameter(W)
        self._check_w(self.W.value)

    def _check_w(self, W: torch.Tensor):
        L = len(self.kernels)
        if W.dim() != 2 or W.shape[1] != L:
            raise ValueError(f"W must be [P, L] = [P, {L}] (one column per latent kernel), got {tuple(W.shape)}")
        if not (1 <= W.shape[0] <= self.MAX_DIM and L <= self.MAX_DIM):
            raise ValueError(f"LinearCoregionalization takes at most {self.MAX_DIM} outputs and {self.MAX_DIM} latent GPs, got "
                             f"P = {W.shape[0]}, L = {L}")
        if not bool(torch.isfinite(W).all()):
            raise ValueError("W must be finite")

    @property
    def num_outputs(self) -> int:
        return int(self.W.value.shape[0])

    def device_W(self, device) -> torch.Tensor:
        """W [P, L] fp64, contiguous, on ``device``: what the two kernels read.  Cached per parameter stamp (checked again when
        the value changed)."""
        key = (self.W.stamp(), str(device))
        hit = self.__dict__.get("_w_cache")
        if hit is not None and hit[0] == key:
            return hit[1]
        self._check_w(self.W.value)
        out = self.W.value.detach().to(device=device, dtype=torch.float64).clone(memory_format=torch.contiguous_format)
        self.__dict__["_w_cache"] = (key, out)
        return out

    def K_diag(self, X) -> torch.Tensor:
        """The mixed prior variances [N, P]: sum_l W[p, l]^2 k_l(x, x)."""
        W = self.W.value.to(torch.float64)
        return super().K_diag(X).to(torch.float64) @ (W * W).t()


def latent_kernels(kernel, P: int):
    """The list of per-latent kernels behind ``kernel``: P references to one shared kernel, or the separate ones."""
    if isinstance(kernel, SeparateIndependent):
        if len(kernel.kernels) != P:
            raise ValueError(f"SeparateIndependent has {len(kernel.kernels)} kernels but the model has {P} latent GPs")
        return kernel.kernels
    return [kernel] * P
