"""NumPy ``Sum`` / ``active_dims`` wrappers around the CPU oracle's kernels (``oracle.tsvgp_oracle``), duck-typed the way the
oracle takes a kernel: ``K(X, X2=None)`` and ``K_diag(X)``.  Passed to ``O.t_SVGP``, ``O.t_SVGP_white``,
``O.gpr_log_marginal_likelihood`` / ``O.gpr_predict_f`` by tests/test_sum_kernel_cpu.py and tests/test_gpu_sum_kernel.py.

``Active(kernel, dims)``  the oracle kernel on the columns ``dims`` of its inputs (gpflow's ``active_dims``).
``Sum(kernels)``          K = sum_c K_c, K_diag = sum_c K_diag_c, the components added in index order.
``build(spec)``           both from one description, so that a test states its kernel once for the oracle and the package:
                          spec = [(class name, variance, lengthscales, active_dims or None), ...]; ``build_pkg(p, spec)`` is the
                          package's kernel of the same description (one entry: the base kernel itself, no ``Sum``)."""
import numpy as np

from oracle import tsvgp_oracle as O


class Active:
    def __init__(self, kernel, dims):
        self.kernel, self.dims = kernel, None if dims is None else list(dims)

    @property
    def variance(self):
        return self.kernel.variance

    @variance.setter
    def variance(self, v):
        self.kernel.variance = float(v)

    @property
    def lengthscales(self):
        return self.kernel.lengthscales

    @lengthscales.setter
    def lengthscales(self, v):
        self.kernel.lengthscales = np.asarray(v, dtype=np.float64)

    def _cols(self, X):
        X = np.asarray(X, dtype=np.float64)
        return X if self.dims is None else X[:, self.dims]

    def K(self, X, X2=None):
        return self.kernel.K(self._cols(X), None if X2 is None else self._cols(X2))

    def K_diag(self, X):
        return self.kernel.K_diag(X)


class Sum:
    def __init__(self, kernels):
        self.kernels = list(kernels)

    def K(self, X, X2=None):
        out = self.kernels[0].K(X, X2)
        for k in self.kernels[1:]:
            out = out + k.K(X, X2)
        return out

    def K_diag(self, X):
        out = self.kernels[0].K_diag(X)
        for k in self.kernels[1:]:
            out = out + k.K_diag(X)
        return out


def build(spec):
    """The oracle-side kernel of ``spec``."""
    comps = [Active(getattr(O, name)(variance=v, lengthscales=ls), dims) for name, v, ls, dims in spec]
    return comps[0] if len(comps) == 1 else Sum(comps)


def build_pkg(p, spec):
    """The package-side kernel of ``spec`` (``p``: the imported package)."""
    comps = [getattr(p, name)(variance=v, lengthscales=ls, active_dims=dims) for name, v, ls, dims in spec]
    return comps[0] if len(comps) == 1 else p.Sum(comps)
