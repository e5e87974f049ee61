"""t-svgp_amd: MI355X-native natural-gradient E-step of t-SVGP behind the reference's GPflow-style API.

The directory name carries a hyphen (as the project layout prescribes), so import it with
``importlib.import_module("t-svgp_amd")`` or through the alias module ``tsvgp_amd`` at the repository root.
"""
from . import _backend, distributed, training, util
from ._backend import HipExtensionError, build_library
from .base import Parameter, default_float, default_jitter
from .inducing_variables import (InducingPoints, InducingSelection, KMeansInducing, KMeansSeeding,
                                 SharedIndependentInducingVariables, inducingpoint_wrapper, kmeans_inducing_points, kmeanspp_seeds,
                                 select_inducing_points)
from .kernels import LinearCoregionalization, Matern32, Matern52, Product, SeparateIndependent, SquaredExponential, Sum
from .likelihoods import Bernoulli, Gaussian, HeteroskedasticTFPConditional, MultiClass, Poisson, RobustMax, Softmax, StudentT
from .likelihoods import Exponential, Gamma, Ordinal
from .models import base_SVGP, t_SVGP, t_SVGP_sites, t_SVGP_white, t_VGP
from .pathwise import FunctionSamples
from .sites import DenseSites, DiagSites, Sites

__all__ = [
    "t_SVGP", "t_SVGP_white", "t_SVGP_sites", "t_VGP", "base_SVGP", "DenseSites", "DiagSites", "Sites", "SquaredExponential", "Gaussian", "Bernoulli", "HeteroskedasticTFPConditional", "Softmax", "StudentT", "Poisson",
    "MultiClass", "RobustMax", "Gamma", "Exponential", "Ordinal",
    "InducingPoints", "select_inducing_points", "InducingSelection", "kmeans_inducing_points", "KMeansInducing", "kmeanspp_seeds", "KMeansSeeding",
    "FunctionSamples",
    "SeparateIndependent", "LinearCoregionalization", "SharedIndependentInducingVariables", "Matern32", "Matern52", "Sum", "Product",
    "inducingpoint_wrapper", "Parameter", "default_float", "default_jitter", "HipExtensionError", "build_library",
    "distributed", "util", "training",
]
