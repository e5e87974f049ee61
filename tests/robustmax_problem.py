"""What the MultiClass / RobustMax tests share (seeded): the small multi-class problems of tests/softmax_problem.py, the inputs of
the map checks and the (model, oracle) pair builder."""
import numpy as np

from oracle import tsvgp_oracle as O
from tests.helpers import pkg
from tests.robustmax_ref import MultiClass as RefMultiClass
from tests.softmax_problem import problem  # noqa: F401  (re-exported: X in [-2, 2]^D, labels = argmax of C noisy linear scores)


def map_inputs(N, C, seed=0):
    """mu ~ 1.5 randn, v log-uniform in [1e-4, 4], labels that take every class once N >= C (Y [N, 1] float)."""
    rng = np.random.RandomState(seed)
    mu = 1.5 * rng.randn(N, C)
    var = np.exp(rng.uniform(np.log(1e-4), np.log(4.0), (N, C)))
    y = rng.randint(0, C, N)
    y[:min(N, C)] = np.arange(C)[:min(N, C)]
    return mu, var, y[:, None].astype(np.float64)


def clip_rows(C=3):
    """Two rows on the clip path: v = 1e-12 in the labelled class (2 v < 1e-10), and v = 1e-12 in another class."""
    mu = np.array([[0.3, -0.2, 0.1], [0.5, 0.4, -0.6]])[:, :C]
    var = np.array([[1e-12, 0.5, 0.7], [0.4, 1e-12, 0.9]])[:, :C]
    y = np.array([[0.0], [0.0]])
    return mu, var, y


def blobs(N=200, seed=0, sep=1.5, sd=0.5):
    """Three Gaussian clusters of spread ``sd`` around the corners of a triangle of circumradius ``sep`` in the plane, the classes
    in turn (Y [N, 1] float); Z: the corners, the corners pushed out by half and two points halfway in (M = 8)."""
    rng = np.random.RandomState(seed)
    cent = sep * np.array([[1.0, 0.0], [-0.5, 0.866], [-0.5, -0.866]])
    y = np.arange(N) % 3
    X = cent[y] + sd * rng.randn(N, 2)
    Z = np.concatenate([cent, 1.5 * cent, 0.5 * cent[:2]])
    return X, y[:, None].astype(np.float64), Z


def pair(Z, C, kind="shared", epsilon=1e-3, num_data=None, **kw):
    """(t_SVGP with MultiClass, oracle t_SVGP with the restated MultiClass): one shared Matern-5/2 kernel, or one SE kernel per
    latent ("separate" / "perlatent")."""
    p = pkg()
    if kind == "shared":
        kh, ko, ivh, ivo = p.Matern52(1.0, 1.5), O.Matern52(1.0, 1.5), Z, Z
    else:
        par = [(1.0 + 0.1 * c, 1.2 + 0.1 * c) for c in range(C)]
        kh = p.SeparateIndependent([p.SquaredExponential(v, l) for v, l in par])
        ko = O.SeparateIndependent([O.SquaredExponential(v, l) for v, l in par])
        ivh, ivo = p.SharedIndependentInducingVariables(Z), O.SharedIndependentInducingVariables(Z)
    hip = p.t_SVGP(kh, p.MultiClass(C, epsilon=epsilon), ivh, num_latent_gps=C, num_data=num_data, **kw)
    ora = O.t_SVGP(ko, RefMultiClass(C, epsilon), ivo, num_latent_gps=C, num_data=num_data)
    return hip, ora
