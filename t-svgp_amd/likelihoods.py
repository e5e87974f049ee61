"""Likelihood objects of the hot path: ``Gaussian``, ``Bernoulli`` (probit, 20-point Gauss-Hermite),
``HeteroskedasticTFPConditional`` (Normal with an Exp scale over two latents, 20 x 20 Gauss-Hermite), ``Softmax`` (C latents,
Monte Carlo with an in-kernel counter-based generator: ``tsvgp_lik_map_softmax_*``), ``StudentT`` (20-point Gauss-Hermite) and
``Poisson`` (exp link, closed form): the last two one latent per target column, ``tsvgp_lik_map_scalar_*`` behind the moments;
``MultiClass`` (C latents, ``RobustMax`` link, 20-point Gauss-Hermite over the labelled latent: ``tsvgp_lik_map_robustmax_*``);
``Gamma`` and ``Exponential`` (exp link, closed form: a third arm of ``tsvgp_lik_map_scalar_*``) and ``Ordinal`` (ordered bins over
one latent, 20-point Gauss-Hermite: ``tsvgp_lik_map_ordinal_*``), one latent per target column like StudentT and Poisson.

Their N-sized maps -- variational expectations and the (mean, var) gradients the E-step needs
(reference src/models/tsvgp.py:256-263) -- run inside the fused HIP moments kernel
(``tsvgp_moments_*`` with ``lik`` = GAUSSIAN / BERNOULLI) or, for the likelihood that couples two latents, in
``tsvgp_lik_map_hetero_*`` behind the moments; the classes here only carry parameters and
the small predictive helpers drivers call on test points (experiments/uci_regression.py:157).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _backend as B
from .base import Parameter


class Gaussian:
    """gpflow.likelihoods.Gaussian [ext]."""

    lik_id = B.LIK_GAUSSIAN

    def __init__(self, variance=1.0):
        self.variance = Parameter(variance)

    @property
    def lik_param(self) -> float:
        return self.variance.item()

    def predict_mean_and_var(self, Fmu, Fvar):
        return Fmu, Fvar + self.variance.value

    def predict_log_density(self, Fmu, Fvar, Y):
        v = Fvar + self.variance.value
        return torch.sum(-0.5 * (math.log(2 * math.pi) + torch.log(v) + (Y - Fmu) ** 2 / v), dim=-1)


class Bernoulli:
    """gpflow.likelihoods.Bernoulli with the default probit link (1e-3 jitter) [ext]."""

    lik_id = B.LIK_BERNOULLI
    lik_param = 0.0
    num_gauss_hermite_points = 20

    @staticmethod
    def invlink(F):
        return 0.5 * (1.0 + torch.erf(F / math.sqrt(2.0))) * (1 - 2e-3) + 1e-3

    def predict_mean_and_var(self, Fmu, Fvar):
        p = self.invlink(Fmu / torch.sqrt(1 + Fvar))
        return p, p - torch.square(p)

    def predict_log_density(self, Fmu, Fvar, Y):
        p = self.invlink(Fmu / torch.sqrt(1 + Fvar))
        return torch.sum(torch.log(torch.where(Y == 1, p, 1 - p)), dim=-1)


def _gh_nodes(ref: torch.Tensor, n: int = 20):
    """(z [n] = hermgauss nodes * sqrt(2), log(w / sqrt(pi)) [n]) in the dtype and on the device of ``ref``."""
    z, w = np.polynomial.hermite.hermgauss(n)
    return (torch.as_tensor(z * math.sqrt(2.0), dtype=ref.dtype, device=ref.device),
            torch.as_tensor(np.log(w / math.sqrt(math.pi)), dtype=ref.dtype, device=ref.device))


class StudentT:
    """gpflow.likelihoods.StudentT(scale, df) [ext] (GPflow 2.2.1): ``scale`` a trainable positive parameter, ``df`` a plain
    float; Y [N, P], one independent column per latent.  The variational expectations and their gradients run on the GPU
    (``tsvgp_lik_map_scalar_*``, 20-point Gauss-Hermite); the predictive helpers here take the same 20 nodes.  ``t_SVGP`` and
    ``t_SVGP_white`` take it; ``t_SVGP_sites`` and ``t_VGP``, whose likelihood is fused into another kernel, do not."""

    lik_id = B.LIK_STUDENT_T
    latent_dim = 1
    num_gauss_hermite_points = 20

    def __init__(self, scale=1.0, df=3.0):
        if not float(df) > 0.0 or not math.isfinite(float(df)):
            raise ValueError(f"StudentT: df must be positive and finite, got {df!r}")
        if not float(scale) > 0.0:
            raise ValueError(f"StudentT: scale must be positive, got {scale!r}")
        self.df = float(df)
        self.scale = Parameter(scale)

    @property
    def lik_param(self):
        """(scale, df): the two scalars ``tsvgp_lik_map_scalar_*`` takes."""
        return (self.scale.item(), self.df)

    def graph_key(self):
        """What a captured step bakes in beside the stamped ``scale``: ``df`` is a plain attribute."""
        return (self.df,)

    def log_prob(self, F, Y):
        s, nu = self.scale.value.to(F.device, F.dtype), self.df
        const = math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi)
        return const - torch.log(s) - 0.5 * (nu + 1.0) * torch.log1p(torch.square((Y - F) / s) / nu)

    def predict_mean_and_var(self, Fmu, Fvar):
        if self.df <= 2.0:
            raise ValueError(f"StudentT: the predictive variance is not finite for df <= 2, got df = {self.df}")
        s = self.scale.value.to(Fmu.device, Fmu.dtype)
        return Fmu, Fvar + s * s * (self.df / (self.df - 2.0))

    def predict_log_density(self, Fmu, Fvar, Y):
        """log sum_i w_i p(y | f_i) over the 20 nodes, in log space, summed over the columns; [N]."""
        z, logw = _gh_nodes(Fmu, self.num_gauss_hermite_points)
        F = Fmu[..., None] + torch.sqrt(Fvar)[..., None] * z
        return torch.sum(torch.logsumexp(self.log_prob(F, Y[..., None]) + logw, dim=-1), dim=-1)


class Poisson:
    """gpflow.likelihoods.Poisson(binsize) [ext] (GPflow 2.2.1) with its default exp inverse link -- the one under which GPflow
    takes the variational expectations in closed form; any other ``invlink`` raises NotImplementedError.  Y [N, P] counts, one
    independent column per latent.  The E-step's map runs on the GPU (``tsvgp_lik_map_scalar_*``); the predictive helpers take
    20-point Gauss-Hermite as GPflow's ``ScalarLikelihood`` does.  ``t_SVGP`` and ``t_SVGP_white`` take it; ``t_SVGP_sites`` and
    ``t_VGP``, whose likelihood is fused into another kernel, do not."""

    lik_id = B.LIK_POISSON
    latent_dim = 1
    num_gauss_hermite_points = 20

    def __init__(self, binsize=1.0, invlink=None, **kwargs):
        if invlink is not None and invlink is not torch.exp and invlink is not np.exp and not _named(invlink, "exp"):
            raise NotImplementedError(f"Poisson: only the exp inverse link is implemented, got {invlink!r}")
        if kwargs:
            raise NotImplementedError(f"Poisson: unsupported arguments {sorted(kwargs)}")
        if not float(binsize) > 0.0 or not math.isfinite(float(binsize)):
            raise ValueError(f"Poisson: binsize must be positive and finite, got {binsize!r}")
        self.binsize = float(binsize)

    @property
    def lik_param(self):
        """(binsize, 0): the two scalars ``tsvgp_lik_map_scalar_*`` takes."""
        return (self.binsize, 0.0)

    def graph_key(self):
        return (self.binsize,)

    def log_prob(self, F, Y):
        return Y * (F + math.log(self.binsize)) - self.binsize * torch.exp(F) - torch.lgamma(Y + 1.0)

    def _nodes(self, Fmu, Fvar):
        z, logw = _gh_nodes(Fmu, self.num_gauss_hermite_points)
        return Fmu[..., None] + torch.sqrt(Fvar)[..., None] * z, logw

    def predict_mean_and_var(self, Fmu, Fvar):
        """E[y] = E_q[b e^f], Var[y] = E_q[b e^f + (b e^f)^2] - E[y]^2 over the 20 nodes."""
        F, logw = self._nodes(Fmu, Fvar)
        w = torch.exp(logw)
        rate = self.binsize * torch.exp(F)
        ey = torch.sum(w * rate, dim=-1)
        return ey, torch.sum(w * (rate + rate * rate), dim=-1) - ey * ey

    def predict_log_density(self, Fmu, Fvar, Y):
        F, logw = self._nodes(Fmu, Fvar)
        return torch.sum(torch.logsumexp(self.log_prob(F, Y[..., None]) + logw, dim=-1), dim=-1)


def _named(obj, name: str) -> bool:
    """``obj`` is a class called ``name`` or an instance of one (tfp.distributions.Normal, tfp.bijectors.Exp())."""
    return getattr(obj, "__name__", type(obj).__name__) == name


def mapped_parameter(likelihood):
    """("likelihood_<name>", Parameter) of the one trainable parameter whose derivative the likelihood's own map returns
    (``LikMapResult.dparam``): StudentT's scale, Gamma's shape, Ordinal's sigma; None for every other likelihood."""
    name = {B.LIK_STUDENT_T: "scale", B.LIK_GAMMA: "shape", B.LIK_ORDINAL: "sigma"}.get(getattr(likelihood, "lik_id", None))
    par = getattr(likelihood, name, None) if name else None  # (Exponential is the Gamma arm without a shape)
    return (f"likelihood_{name}", par) if isinstance(par, Parameter) else None


def _require_exp_link(cls: str, invlink, kwargs):
    if invlink is not None and invlink is not torch.exp and invlink is not np.exp and not _named(invlink, "exp"):
        raise NotImplementedError(f"{cls}: only the exp inverse link is implemented, got {invlink!r}")
    if kwargs:
        raise NotImplementedError(f"{cls}: unsupported arguments {sorted(kwargs)}")


class _ScalarQuadrature:
    """The predictive helpers of GPflow's ``ScalarLikelihood`` [ext] over the 20 Gauss-Hermite nodes, for a likelihood that gives
    ``log_prob(F, Y)``, ``conditional_mean(F)`` and ``conditional_variance(F)`` elementwise; Y [N, P], one column per latent."""

    latent_dim = 1
    num_gauss_hermite_points = 20

    def _nodes(self, Fmu, Fvar):
        z, logw = _gh_nodes(Fmu, self.num_gauss_hermite_points)
        return Fmu[..., None] + torch.sqrt(Fvar)[..., None] * z, logw

    def predict_mean_and_var(self, Fmu, Fvar):
        """E[y] = E_q[E[y | f]], Var[y] = E_q[Var[y | f] + E[y | f]^2] - E[y]^2 over the 20 nodes."""
        F, logw = self._nodes(Fmu, Fvar)
        w = torch.exp(logw)
        cm = self.conditional_mean(F)
        ey = torch.sum(w * cm, dim=-1)
        return ey, torch.sum(w * (self.conditional_variance(F) + cm * cm), dim=-1) - ey * ey

    def predict_log_density(self, Fmu, Fvar, Y):
        """log sum_i w_i p(y | f_i) over the 20 nodes, in log space, summed over the columns; [N]."""
        F, logw = self._nodes(Fmu, Fvar)
        return torch.sum(torch.logsumexp(self.log_prob(F, Y[..., None]) + logw, dim=-1), dim=-1)


class Gamma(_ScalarQuadrature):
    """gpflow.likelihoods.Gamma(invlink, shape) [ext] (GPflow 2.2.1) with its default exp inverse link: y ~ Gamma(shape a,
    scale exp(f)), ``shape`` a trainable positive parameter; any other ``invlink`` raises NotImplementedError.  Y [N, P] strictly
    positive, one independent column per latent.  Under the exp link the variational expectations are closed
    (``tsvgp_lik_map_scalar_*`` with TSVGP_LIK_GAMMA, on the GPU); the predictive helpers take 20-point Gauss-Hermite as GPflow's
    ``ScalarLikelihood`` does.  ``t_SVGP`` and ``t_SVGP_white`` take it; ``t_SVGP_sites`` and ``t_VGP``, whose likelihood is fused
    into another kernel, do not."""

    lik_id = B.LIK_GAMMA

    def __init__(self, invlink=None, shape=1.0, **kwargs):
        _require_exp_link("Gamma", invlink, kwargs)
        if not float(shape) > 0.0 or not math.isfinite(float(shape)):
            raise ValueError(f"Gamma: shape must be positive and finite, got {shape!r}")
        self.shape = Parameter(shape)

    @property
    def lik_param(self):
        """(shape, 0): the two scalars ``tsvgp_lik_map_scalar_*`` takes."""
        return (self.shape.item(), 0.0)

    def graph_key(self):
        """Nothing beside the stamped ``shape`` is baked into a captured step."""
        return ()

    def _shape(self) -> float:
        return self.shape.item()

    def log_prob(self, F, Y):
        """-a f - lgamma(a) + (a - 1) log y - y exp(-f); at a == 1 the power of y is skipped (y = 0 is then a target)."""
        a = self._shape()
        out = -a * F - math.lgamma(a) - Y * torch.exp(-F)
        return out if a == 1.0 else out + (a - 1.0) * torch.log(Y)

    def conditional_mean(self, F):
        return self._shape() * torch.exp(F)

    def conditional_variance(self, F):
        return self._shape() * torch.exp(2.0 * F)


class Exponential(Gamma):
    """gpflow.likelihoods.Exponential(invlink) [ext] (GPflow 2.2.1) with its default exp inverse link: y ~ Exp(rate exp(-f)),
    log p = -f - y exp(-f), E[y | f] = exp(f), Var[y | f] = exp(2 f).  It is the Gamma arm of the map at shape 1 exactly, where the
    power of y drops out of the density -- y = 0 is a legal waiting time -- and it has no trainable parameter.  Y [N, P] >= 0."""

    def __init__(self, invlink=None, **kwargs):
        _require_exp_link("Exponential", invlink, kwargs)

    @property
    def lik_param(self):
        """(1, 0, False): the Gamma arm's two scalars and "no parameter derivative"."""
        return (1.0, 0.0, False)

    def _shape(self) -> float:
        return 1.0


class Ordinal(_ScalarQuadrature):
    """gpflow.likelihoods.Ordinal(bin_edges) [ext] (GPflow 2.2.1): K = len(bin_edges) + 1 ordered classes over ONE latent,
    Y [N, P] labels 0 .. K-1 (one independent column per latent),
        p(y = k | f) = Phi~((e_k - f) / sigma) - Phi~((e_{k-1} - f) / sigma),   e_{-1} = -inf, e_{K-1} = +inf,
    Phi~ the probit with GPflow's 1e-3 jitter and ``sigma`` a trainable positive parameter (1.0); log p carries GPflow's + 1e-6.
    ``bin_edges`` are fixed at construction: 1-D, finite, strictly increasing, at most ``B.ORDINAL_MAX_EDGES`` of them.  The
    variational expectations and their gradients run on the GPU (``tsvgp_lik_map_ordinal_*``, 20-point Gauss-Hermite, the edges
    in an fp64 device tensor kept on this object); the predictive helpers take the same nodes.  ``t_SVGP`` and ``t_SVGP_white``
    take it; ``t_SVGP_sites`` and ``t_VGP`` do not."""

    lik_id = B.LIK_ORDINAL
    _CHUNK = 1 << 22  # elements per [rows, P, 20, K] evaluation of predict_mean_and_var

    def __init__(self, bin_edges, **kwargs):
        if kwargs:
            raise NotImplementedError(f"Ordinal: unsupported arguments {sorted(kwargs)}")
        edges = np.array(bin_edges.detach().cpu().numpy() if torch.is_tensor(bin_edges) else bin_edges, dtype=np.float64)
        if edges.ndim != 1 or not 1 <= edges.size <= B.ORDINAL_MAX_EDGES:
            raise ValueError(f"Ordinal: bin_edges must be 1-D with 1 to {B.ORDINAL_MAX_EDGES} entries, got shape {edges.shape}")
        if not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0.0):
            raise ValueError("Ordinal: bin_edges must be finite and strictly increasing")
        edges.setflags(write=False)  # the map's kernel trusts the order: nothing edits them after this check
        self.bin_edges = edges
        self.num_bins = edges.size + 1
        self.sigma = Parameter(1.0)
        self._edges_dev = {}  # device -> fp64 [K - 1]: made once per device (a captured graph holds its address)

    # the engine takes the likelihood's scalars through ``lik_param``; this one hands over itself (edges and sigma)
    @property
    def lik_param(self):
        return self

    def graph_key(self):
        """What a captured step bakes in beside the stamped ``sigma``: the edges."""
        return tuple(self.bin_edges.tolist())

    def device_edges(self, device) -> torch.Tensor:
        """The edges the map reads: one fp64 tensor per device for the life of this object."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        edges = self._edges_dev.get(device)
        if edges is None:
            edges = self._edges_dev[device] = torch.tensor(self.bin_edges.tolist(), dtype=torch.float64).to(device)
        return edges

    def _scaled_edges(self, ref):
        """(a, b) numerators: upper edges [K] with +inf last, lower edges [K] with -inf first, in the dtype and on the device of ``ref``."""
        e = torch.tensor(self.bin_edges.tolist(), dtype=ref.dtype, device=ref.device)
        inf = torch.full((1,), float("inf"), dtype=ref.dtype, device=ref.device)
        return torch.cat([e, inf]), torch.cat([-inf, e])

    @staticmethod
    def _probit(x):
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) * (1.0 - 2e-3) + 1e-3

    def log_prob(self, F, Y):
        """log(Phi~(a) - Phi~(b) + 1e-6); the difference, (1 - 2e-3)(Phi(a) - Phi(b)), from erfc on the side where both tail masses
        are small (as the kernel takes it).  A label that is no integer in [0, K) gives NaN."""
        up, lo = self._scaled_edges(F)
        Yf = torch.broadcast_to(Y.to(F.dtype), F.shape)
        ok = (Yf >= 0) & (Yf <= self.num_bins - 1) & (Yf == torch.floor(Yf))
        k = torch.where(ok, Yf, torch.zeros_like(Yf)).long()
        s = self.sigma.value.to(F.device, F.dtype)
        a, b = (up[k] - F) / s, (lo[k] - F) / s
        flip = b > 0
        hi, lw = torch.where(flip, -b, a), torch.where(flip, -a, b)
        r = math.sqrt(0.5)
        phi = 0.5 * (1.0 - 2e-3) * (torch.special.erfc(-r * hi) - torch.special.erfc(-r * lw))
        return torch.where(ok, torch.log(phi + 1e-6), torch.full_like(phi, float("nan")))

    def _phi(self, F):
        """[..., K]: the probability of every bin at F, without the 1e-6 (GPflow's ``_make_phi``)."""
        up, lo = self._scaled_edges(F)
        s = self.sigma.value.to(F.device, F.dtype)
        return self._probit((up - F[..., None]) / s) - self._probit((lo - F[..., None]) / s)

    def conditional_mean(self, F):
        ks = torch.arange(self.num_bins, dtype=F.dtype, device=F.device)
        return self._phi(F) @ ks

    def conditional_variance(self, F):
        ks = torch.arange(self.num_bins, dtype=F.dtype, device=F.device)
        phi = self._phi(F)
        return phi @ (ks * ks) - torch.square(phi @ ks)

    def predict_mean_and_var(self, Fmu, Fvar):
        """E[y | f] = sum_k k phi_k, Var[y | f] = sum_k k^2 phi_k - E[y | f]^2 under the 20 nodes, row chunk by row chunk."""
        per_row = max(1, int(np.prod(Fmu.shape[1:]))) * self.num_gauss_hermite_points * self.num_bins
        rows = max(1, self._CHUNK // per_row)
        parts = [_ScalarQuadrature.predict_mean_and_var(self, Fmu[lo:lo + rows], Fvar[lo:lo + rows])
                 for lo in range(0, max(Fmu.shape[0], 1), rows)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


class HeteroskedasticTFPConditional:
    """gpflow.likelihoods.HeteroskedasticTFPConditional [ext] with its defaults: Normal(loc=f0, scale=exp(f1)), two latent GPs
    per output (``latent_dim = 2``), Y [N, 1] (reference docs/notebooks/heteroskedastic.py:58-60).  The variational expectations
    and their gradients run on the GPU (``tsvgp_lik_map_hetero_*``); the predictive helpers here take the same 20 x 20
    Gauss-Hermite grid as GPflow's ``NDiagGHQuadrature(2, 20)``.  Only the Normal distribution and the Exp scale transform are
    implemented; ``distribution_class`` / ``scale_transform`` may be the tfp objects of those names or None (the defaults)."""

    lik_id = B.LIK_HETERO
    lik_param = 0.0
    latent_dim = 2
    num_gauss_hermite_points = 20
    _CHUNK = 1 << 15  # rows per [rows, 20, 20] grid evaluation of the predictive helpers

    def __init__(self, distribution_class=None, scale_transform=None, **kwargs):
        if distribution_class is not None and not _named(distribution_class, "Normal"):
            raise NotImplementedError(f"HeteroskedasticTFPConditional: only the Normal distribution is implemented, got "
                                      f"{distribution_class!r}")
        if scale_transform is not None and not _named(scale_transform, "Exp"):
            raise NotImplementedError(f"HeteroskedasticTFPConditional: only the Exp scale transform is implemented, got "
                                      f"{scale_transform!r}")
        if kwargs:
            raise NotImplementedError(f"HeteroskedasticTFPConditional: unsupported arguments {sorted(kwargs)}")

    def _grid(self, Fmu, Fvar):
        """(f0 [N, 20, 1], f1 [N, 1, 20], log w_i + log w_j [20, 20]) of the product grid."""
        z, w = np.polynomial.hermite.hermgauss(self.num_gauss_hermite_points)
        z = torch.as_tensor(z * math.sqrt(2.0), dtype=Fmu.dtype, device=Fmu.device)
        logw = torch.as_tensor(np.log(w / math.sqrt(math.pi)), dtype=Fmu.dtype, device=Fmu.device)
        sd = torch.sqrt(Fvar)
        f0 = (Fmu[:, 0:1] + sd[:, 0:1] * z)[:, :, None]
        f1 = (Fmu[:, 1:2] + sd[:, 1:2] * z)[:, None, :]
        return f0, f1, logw[:, None] + logw[None, :]

    def _chunks(self, *arrays):
        n = arrays[0].shape[0]
        for lo in range(0, max(n, 1), self._CHUNK):
            yield tuple(a[lo:lo + self._CHUNK] for a in arrays)

    def predict_mean_and_var(self, Fmu, Fvar):
        """E[y] = E_q[f0], Var[y] = E_q[exp(2 f1) + f0^2] - E[y]^2 over the 400-point grid; [N, 1] each."""
        means, variances = [], []
        for mu, var in self._chunks(Fmu, Fvar):
            f0, f1, logw = self._grid(mu, var)
            w = torch.exp(logw)
            ey = torch.sum(w * f0, dim=(1, 2))
            ey2 = torch.sum(w * (torch.exp(2.0 * f1) + f0 * f0), dim=(1, 2))
            means.append(ey[:, None])
            variances.append((ey2 - ey * ey)[:, None])
        return torch.cat(means), torch.cat(variances)

    def predict_log_density(self, Fmu, Fvar, Y):
        """log sum_ij w_i w_j p(y | f0_i, f1_j), summed in log space over the 400-point grid; [N]."""
        out = []
        for mu, var, y in self._chunks(Fmu, Fvar, Y):
            f0, f1, logw = self._grid(mu, var)
            logp = -0.5 * math.log(2 * math.pi) - f1 - 0.5 * (y[:, :, None] - f0) ** 2 * torch.exp(-2.0 * f1)
            out.append(torch.logsumexp((logp + logw).reshape(mu.shape[0], -1), dim=1))
        return torch.cat(out)


class Softmax:
    """gpflow.likelihoods.Softmax(num_classes) [ext] (GPflow 2.2.1, a ``MonteCarloLikelihood``): C = num_classes latent GPs,
    Y [N, 1] class labels 0 .. C-1, log p(y | f) = f_y - logsumexp_c f_c, every expectation a Monte Carlo average over
    ``num_monte_carlo_points`` (100; a plain attribute, as in GPflow) draws eps [S, N, C] at f = Fmu + sqrt(Fvar) eps (reference
    docs/notebooks/mnist.py).  The variational expectations and their gradients run on the GPU (``tsvgp_lik_map_softmax_*``)
    with the draws made inside the kernel by the counter-based generator of include/tsvgp_hip.h: the draw for
    (seed, draw, global row, sample, class) is a pure function of those integers.  ``draw`` counts the evaluations: each one
    (an E-step, an ELBO, a predictive helper without ``epsilon=``) takes the draws of the current ``draw`` and advances it by one,
    on the device too (``rng_state`` = int64 [seed, draw], advanced in-stream, so a replayed graph draws afresh).  ``row_offset`` is
    the global number of the first TRAINING row this process passes (a row shard sets it to its shard's first row; 0 otherwise);
    the predictive helpers number the test points they are given from 0 on every rank, whatever ``row_offset`` is.  ``seed`` and
    ``draw`` may be assigned at any time: the device words are edited in place, so a captured graph sees the new values."""

    lik_id = B.LIK_SOFTMAX
    _CHUNK = 1 << 13  # rows per [S, rows, C] evaluation of the predictive helpers

    def __init__(self, num_classes: int, seed: int = 0):
        if int(num_classes) != num_classes or not 2 <= num_classes <= B.MAX_BATCH:
            raise ValueError(f"Softmax: num_classes must be an integer in [2, {B.MAX_BATCH}], got {num_classes!r}")
        self.num_classes = self.latent_dim = int(num_classes)
        self.num_monte_carlo_points = 100
        self.row_offset = 0
        self._seed = int(seed)
        self._draw = 0
        # device -> int64 [seed, draw]: made ONCE per device and only ever edited in place -- a captured graph holds its address
        self._states = {}

    # the engine takes the likelihood's scalar through ``lik_param``; this likelihood's "parameter" is its generator state
    @property
    def lik_param(self):
        return self

    def _sync(self):
        """Host (seed, draw) -> every device copy, in place (a stream-ordered copy: replays enqueued later see it)."""
        for state in self._states.values():
            state.copy_(torch.tensor([self._seed, self._draw], dtype=torch.int64))

    @property
    def seed(self) -> int:
        return self._seed

    @seed.setter
    def seed(self, value: int):
        self._seed = int(value)
        self._sync()

    @property
    def draw(self) -> int:
        return self._draw

    @draw.setter
    def draw(self, value: int):
        self._draw = int(value)
        self._sync()

    def graph_key(self):
        """What a captured step bakes in of this likelihood (seed and draw are read from device memory: not part of it)."""
        return (self.num_classes, int(self.num_monte_carlo_points), int(self.row_offset))

    def rng_state(self, device) -> torch.Tensor:
        """The device words [seed, draw] the map reads: one tensor per device for the life of this object, never replaced."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        state = self._states.get(device)
        if state is None:
            state = self._states[device] = torch.tensor([self._seed, self._draw], dtype=torch.int64).to(device)
        return state

    def advance(self):
        """One evaluation consumed the current draws: draw + 1 on the host and, in-stream, on the device."""
        self._draw += 1
        for state in self._states.values():
            state[1:].add_(1)

    def _replayed(self, draw_before: int):
        """A graph replay ran the captured in-stream add: bring the host count level with it."""
        self._draw = int(draw_before) + 1

    def normals(self, N: int, dtype, device, row_offset=None) -> torch.Tensor:
        """eps [S, N, C] of the current (seed, draw) for the global rows row_offset .. row_offset + N (``tsvgp_mc_normals_*``);
        does not advance ``draw``."""
        if dtype not in (torch.float64, torch.float32):
            raise TypeError(f"Softmax.normals: float64 or float32, got {dtype}")
        S, C = int(self.num_monte_carlo_points), self.num_classes
        out = torch.empty((S, N, C), dtype=dtype, device=device)
        if N == 0:
            return out
        if out.device.type != "cuda":
            raise B.HipExtensionError("Softmax: the Monte Carlo draws are made by a HIP kernel; pass epsilon= on a CPU tensor")
        fn = getattr(B.lib(), "tsvgp_mc_normals_f64" if dtype == torch.float64 else "tsvgp_mc_normals_f32")
        with torch.cuda.device(out.device):
            B.check(fn(out.data_ptr(), self.seed, self._draw, int(self.row_offset if row_offset is None else row_offset), S, N, C,
                       torch.cuda.current_stream(out.device).cuda_stream), "tsvgp_mc_normals")
        return out

    def _samples(self, Fmu, Fvar, epsilon, lo, hi):
        """softmax inputs f [S, rows, C] of the rows lo .. hi."""
        mu, var = Fmu[lo:hi], Fvar[lo:hi]
        if epsilon is None:
            eps = self.normals(hi - lo, mu.dtype, mu.device, row_offset=lo)  # test points count from 0
        else:
            eps = torch.as_tensor(epsilon, dtype=mu.dtype, device=mu.device)[:, lo:hi]
        return mu[None] + torch.sqrt(var[None]) * eps

    def _check(self, Fmu, Fvar):
        if Fmu.dim() != 2 or Fmu.shape[1] != self.num_classes or Fvar.shape != Fmu.shape:
            raise ValueError(f"Softmax: Fmu, Fvar must be [N, {self.num_classes}], got {tuple(Fmu.shape)} and {tuple(Fvar.shape)}")

    def predict_mean_and_var(self, Fmu, Fvar, epsilon=None):
        """E[p], E[(p - p^2) + p^2] - E[p]^2 with p = softmax(f), averaged over the draws; [N, C] each."""
        self._check(Fmu, Fvar)
        means, variances = [], []
        for lo in range(0, max(Fmu.shape[0], 1), self._CHUNK):
            p = torch.softmax(self._samples(Fmu, Fvar, epsilon, lo, min(lo + self._CHUNK, Fmu.shape[0])), dim=-1)
            ey = p.mean(dim=0)
            means.append(ey)
            variances.append(((p - p * p) + p * p).mean(dim=0) - ey * ey)
        if epsilon is None:
            self.advance()
        return torch.cat(means), torch.cat(variances)

    def predict_log_density(self, Fmu, Fvar, Y, epsilon=None):
        """log (1/S sum_s p(y | f^s)), summed in log space; [N]."""
        self._check(Fmu, Fvar)
        if Y.dim() != 2 or Y.shape[1] != 1 or Y.shape[0] != Fmu.shape[0]:
            raise ValueError(f"Softmax: Y must be [N, 1] = [{Fmu.shape[0]}, 1], got {tuple(Y.shape)}")
        classes = torch.arange(self.num_classes, dtype=Fmu.dtype, device=Fmu.device)
        out = []
        for lo in range(0, max(Fmu.shape[0], 1), self._CHUNK):
            hi = min(lo + self._CHUNK, Fmu.shape[0])
            f = self._samples(Fmu, Fvar, epsilon, lo, hi)
            onehot = (Y[lo:hi].to(Fmu.dtype) == classes[None, :]).to(Fmu.dtype)  # [rows, C]; no label is used as an index
            logp = torch.sum(onehot[None] * f, dim=-1) - torch.logsumexp(f, dim=-1)
            out.append(torch.logsumexp(logp, dim=0) - math.log(logp.shape[0]))
        if epsilon is None:
            self.advance()
        return torch.cat(out)


class RobustMax:
    """gpflow.likelihoods.RobustMax(num_classes, epsilon) [ext]: the inverse link of ``MultiClass`` -- probability 1 - epsilon on the
    class whose latent is the largest, epsilon / (num_classes - 1) on each of the others.  A holder of the two numbers: the
    quadrature lives in ``MultiClass`` and in ``tsvgp_lik_map_robustmax_*``."""

    def __init__(self, num_classes: int, epsilon: float = 1e-3):
        if int(num_classes) != num_classes or not 2 <= num_classes <= B.MAX_BATCH:
            raise ValueError(f"RobustMax: num_classes must be an integer in [2, {B.MAX_BATCH}], got {num_classes!r}")
        if not 0.0 < float(epsilon) < 1.0:
            raise ValueError(f"RobustMax: epsilon must lie in (0, 1), got {epsilon!r}")
        self.num_classes = int(num_classes)
        self.epsilon = float(epsilon)

    @property
    def _eps_k1(self) -> float:
        return self.epsilon / (self.num_classes - 1.0)


class MultiClass:
    """gpflow.likelihoods.MultiClass(num_classes) [ext] (GPflow 2.2.1) with its default ``RobustMax`` inverse link: C = num_classes
    latent GPs, Y [N, 1] class labels 0 .. C-1, p(y | f) = 1 - epsilon where the labelled latent is the largest, epsilon / (C - 1)
    otherwise.  Every expectation is the 20-point Gauss-Hermite rule over the labelled latent of the probability that it is the
    largest (``RobustMax.prob_is_largest``), so -- unlike ``Softmax`` -- nothing is drawn: the E-step has a fixed point, a replayed
    graph repeats an eager step bit for bit and ``elbo_and_grads`` is exact.  The variational expectations and their gradients
    run on the GPU (``tsvgp_lik_map_robustmax_*``); the helpers here evaluate the same sum in torch on the test points."""

    lik_id = B.LIK_MULTICLASS
    num_gauss_hermite_points = 20
    _CHUNK = 1 << 22  # elements per [rows, C, C, 20] evaluation of the predictive helpers: the rows of a chunk follow from it

    def __init__(self, num_classes: int, invlink=None, epsilon: float = 1e-3, **kwargs):
        if int(num_classes) != num_classes or not 2 <= num_classes <= B.MAX_BATCH:
            raise ValueError(f"MultiClass: num_classes must be an integer in [2, {B.MAX_BATCH}], got {num_classes!r}")
        if kwargs:
            raise NotImplementedError(f"MultiClass: unsupported arguments {sorted(kwargs)}")
        if invlink is not None:
            if not isinstance(invlink, RobustMax):
                raise NotImplementedError(f"MultiClass: only the RobustMax inverse link is implemented, got {invlink!r}")
            if invlink.num_classes != int(num_classes):
                raise ValueError(f"MultiClass: the RobustMax link is over {invlink.num_classes} classes, the likelihood over "
                                 f"{num_classes}")
            epsilon = invlink.epsilon
        if not 0.0 < float(epsilon) < 1.0:
            raise ValueError(f"MultiClass: epsilon must lie in (0, 1), got {epsilon!r}")
        self.num_classes = self.latent_dim = int(num_classes)
        self.epsilon = float(epsilon)
        self.invlink = invlink if invlink is not None else RobustMax(self.num_classes, self.epsilon)

    # the engine takes the likelihood's scalar through ``lik_param``; this likelihood has two (C, epsilon): it hands over itself
    @property
    def lik_param(self):
        return self

    def graph_key(self):
        """What a captured step bakes in of this likelihood: both travel as kernel arguments."""
        return (self.num_classes, self.epsilon)

    def _check(self, Fmu, Fvar):
        if Fmu.dim() != 2 or Fmu.shape[1] != self.num_classes or Fvar.shape != Fmu.shape:
            raise ValueError(f"MultiClass: Fmu, Fvar must be [N, {self.num_classes}], got {tuple(Fmu.shape)} and {tuple(Fvar.shape)}")

    def log_prob(self, F, Y):
        """log(1 - epsilon) where argmax_c F == y, log(epsilon / (C - 1)) elsewhere; F [N, C], Y [N, 1] -> [N]."""
        hit = torch.argmax(F, dim=-1).to(F.dtype) == Y.to(F.dtype).reshape(-1)
        both = torch.tensor([math.log(self.invlink._eps_k1), math.log(1.0 - self.epsilon)], dtype=F.dtype, device=F.device)
        return torch.where(hit, both[1], both[0])

    def _prob_every_class(self, Fmu, Fvar):
        """[rows, C]: entry k the probability that latent k is the largest (``prob_is_largest`` with the label k)."""
        C = self.num_classes
        x, w = np.polynomial.hermite.hermgauss(self.num_gauss_hermite_points)
        x = torch.as_tensor(x, dtype=Fmu.dtype, device=Fmu.device)
        w = torch.as_tensor(w / math.sqrt(math.pi), dtype=Fmu.dtype, device=Fmu.device)
        X = Fmu[:, :, None] + x * torch.sqrt(torch.clamp(2.0 * Fvar, min=1e-10))[:, :, None]  # [rows, k, i]
        d = (X[:, :, None, :] - Fmu[:, None, :, None]) / torch.sqrt(torch.clamp(Fvar, min=1e-10))[:, None, :, None]  # [rows, k, c, i]
        cdf = 0.5 * (1.0 + torch.erf(d / math.sqrt(2.0))) * (1.0 - 2e-4) + 1e-4
        own = torch.eye(C, dtype=torch.bool, device=Fmu.device)[None, :, :, None]
        return torch.sum(torch.prod(torch.where(own, torch.ones_like(cdf), cdf), dim=2) * w, dim=-1)

    def _density(self, Fmu, Fvar):
        """p (1 - epsilon) + (1 - p) epsilon / (C - 1) for every class; [N, C], row chunk by row chunk."""
        self._check(Fmu, Fvar)
        out = []
        rows = max(1, self._CHUNK // (self.num_gauss_hermite_points * self.num_classes ** 2))
        for lo in range(0, max(Fmu.shape[0], 1), rows):
            p = self._prob_every_class(Fmu[lo:lo + rows], Fvar[lo:lo + rows])
            out.append(p * (1.0 - self.epsilon) + (1.0 - p) * self.invlink._eps_k1)
        return torch.cat(out)

    def predict_mean_and_var(self, Fmu, Fvar):
        """(ps, ps - ps^2) with ps [N, C] the predictive density of every class."""
        ps = self._density(Fmu, Fvar)
        return ps, ps - torch.square(ps)

    def predict_log_density(self, Fmu, Fvar, Y):
        """log of the predictive density of the labelled class; [N].  No label is used as an index."""
        if Y.dim() != 2 or Y.shape[1] != 1 or Y.shape[0] != Fmu.shape[0]:
            raise ValueError(f"MultiClass: Y must be [N, 1] = [{Fmu.shape[0]}, 1], got {tuple(Y.shape)}")
        ps = self._density(Fmu, Fvar)
        classes = torch.arange(self.num_classes, dtype=Fmu.dtype, device=Fmu.device)
        onehot = (Y.to(Fmu.dtype) == classes[None, :]).to(Fmu.dtype)
        return torch.log(torch.sum(onehot * ps, dim=-1))
