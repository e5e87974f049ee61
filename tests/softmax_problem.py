"""The small multi-class problems the Softmax tests share (seeded), and the (model, oracle) pair builder."""
import numpy as np

from oracle import tsvgp_oracle as O
from tests.helpers import pkg
from tests.softmax_ref import Softmax as RefSoftmax


def problem(N=300, M=12, D=2, C=3, seed=0):
    """X in [-2, 2]^D, labels = argmax of C noisy linear scores (Y [N, 1] float), Z on a jittered spread of the data range."""
    rng = np.random.RandomState(seed)
    X = rng.rand(N, D) * 4 - 2
    W = rng.randn(D, C)
    Y = np.argmax(X @ W + 0.3 * rng.randn(N, C), axis=1)[:, None].astype(np.float64)
    Z = rng.rand(M, D) * 4 - 2
    return X, Y, Z


def pair(Z, C, kind="shared", seed=3, num_data=None, **kw):
    """(t_SVGP with Softmax, oracle t_SVGP with the restated Softmax sharing (seed, draw)): one shared Matern-5/2 kernel, or one
    SE kernel per latent ("separate" / "perlatent")."""
    p = pkg()
    if kind == "shared":
        kh, ko, ivh, ivo = p.Matern52(1.0, 1.5), O.Matern52(1.0, 1.5), Z, Z
    else:
        par = [(1.0 + 0.1 * c, 1.2 + 0.1 * c) for c in range(C)]
        kh = p.SeparateIndependent([p.SquaredExponential(v, l) for v, l in par])
        ko = O.SeparateIndependent([O.SquaredExponential(v, l) for v, l in par])
        ivh, ivo = p.SharedIndependentInducingVariables(Z), O.SharedIndependentInducingVariables(Z)
    hip = p.t_SVGP(kh, p.Softmax(C, seed=seed), ivh, num_latent_gps=C, num_data=num_data, **kw)
    ora = O.t_SVGP(ko, RefSoftmax(C, seed=seed), ivo, num_latent_gps=C, num_data=num_data)
    return hip, ora
