"""NumPy ``Product`` wrapper around the CPU oracle's kernels (``oracle.tsvgp_oracle``), duck-typed the way the oracle takes a
kernel: ``K(X, X2=None)`` and ``K_diag(X)``.  Passed to ``O.t_SVGP`` and ``O.t_SVGP_white`` by tests/test_product_kernel_cpu.py
and tests/test_gpu_product_kernel.py.  The components are ``sum_kernel_ref.Active`` (the oracle kernel on its ``active_dims``).

``Product(kernels)``   K = prod_c K_c, K_diag = prod_c K_diag_c, the components multiplied in index order.
``build(spec)``        spec = [(class name, variance, lengthscales, active_dims or None), ...], the format of
                       tests/sum_kernel_ref.py; ``build_pkg(p, spec)`` is the package's ``Product`` of the same description.  Both
                       return a product even for one entry (a one-component product is a legitimate kernel here).
``value_problem(..)``  inputs, longdouble reference and entrywise bound of one fused product fill (below)."""
import numpy as np

from oracle import tsvgp_oracle as O
from tests import kernel_value_ref as R
from tests.sum_kernel_ref import Active


class Product:
    def __init__(self, kernels):
        self.kernels = list(kernels)

    def K(self, X, X2=None):
        out = self.kernels[0].K(X, X2)
        for k in self.kernels[1:]:
            out = out * k.K(X, X2)
        return out

    def K_diag(self, X):
        out = self.kernels[0].K_diag(X)
        for k in self.kernels[1:]:
            out = out * k.K_diag(X)
        return out


def build(spec):
    """The oracle-side kernel of ``spec``."""
    return Product([Active(getattr(O, name)(variance=v, lengthscales=ls), dims) for name, v, ls, dims in spec])


def build_pkg(p, spec):
    """The package-side kernel of ``spec`` (``p``: the imported package)."""
    return p.Product([getattr(p, name)(variance=v, lengthscales=ls, active_dims=dims) for name, v, ls, dims in spec])


# ---------------------------------------------------------------------------------------------------------------------
# the value problem of tests/test_gpu_prodfill_values.py, built on the CPU so that tests/test_product_kernel_cpu.py can assert its
# inclusion condition without a GPU
# ---------------------------------------------------------------------------------------------------------------------
OTHERS_SCALE = 1.0 / 16.0  # components 1.. take their inv_ls row times this (a power of two: exact in both types)


def value_problem(spec, T, N, M, D, x_is_z=False):
    """Inputs, longdouble reference and entrywise relative bound of one ``tsvgp_kernel_fill_prod_*`` call.

    ``spec``: [(class name, variance, zeroed input columns), ...] as ``SPECS`` of tests/test_gpu_sumfill_values.py.
    ``kernel_value_ref.grid(.., P=C)`` lays the rows out so that component 0's exponent argument a_0 runs to the edge of the
    type's normal range; left alone, C components of similar lengthscales would push the PRODUCT below the type's range on most
    entries, so components 1.. take their ``inv_ls`` row times 1/16 (a_c drops 16-fold for a Matern, 256-fold for the squared
    exponential) and the product stays above 1e3 * tiny on more than 90 % of the entries -- the inclusion condition
    ``check_values`` caps, asserted by the CPU test for every (C, D, type) the GPU test uses.

    Reference: variance * prod_c ``reference(kind_c, .., variance=1)["K"]``, variance = prod_c variance_c in index order as the C
    ABI passes it.  Bound: sum_c ``rel_bound(kind_c, T, ref_c, D, factor=GPU_FACTOR)`` + C u."""
    C = len(spec)
    g = R.grid(spec[0][0], T, max(N, R.MIN_ROWS), max(M, R.K_SAME + 1), D, P=C if C > 1 else None)
    Z = g["Z"][:M]
    X = Z if x_is_z else g["X"][:N]
    il = np.array(g["inv_ls"], dtype=np.float64).reshape(C, D)
    il[1:] *= OTHERS_SCALE
    for c, (_, _, off) in enumerate(spec):
        cols = [d for d in off if d < D]
        if len(cols) < D:
            il[c, cols] = 0.0
    kinds = [s[0] for s in spec]
    var = [R.c_variance(s[1], T) for s in spec]
    variance = 1.0
    for v in var:
        variance *= v
    variance = R.c_variance(variance, T)
    refs = [R.reference(kinds[c], X, Z, il[c], 1.0) for c in range(C)]
    K = R.L(variance) * refs[0]["K"]
    for r in refs[1:]:
        K = K * r["K"]
    bound = np.full(K.shape, C * R.U[T])
    for c in range(C):
        bound = bound + R.rel_bound(kinds[c], T, refs[c], D, factor=R.GPU_FACTOR)
    ref = dict(K=K, a=refs[0]["a"])
    for a in (X, Z, il):
        a.setflags(write=False)
    return dict(X=X, Z=Z, inv_ls=il, kinds=kinds, var=var, variance=variance, ref=ref, bound=bound, T=T,
                frac=float(R.relative_mask(ref, T).mean()))
