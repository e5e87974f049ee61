"""``Product`` kernels without a GPU: the class semantics, ``K_torch`` and its autograd gradient against the NumPy reference, the
four new C entry points (prototypes, ABI 5, argument checks that return before any launch), the self-check of
tests/kgrad_prod_ref.py against central differences, and the inclusion condition of tests/test_gpu_prodfill_values.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import kernel_value_ref as V
from tests import kgrad_prod_ref as G
from tests import product_kernel_ref as R
from tests.helpers import pkg
from tests.test_gpu_sumfill_values import SPECS

CPU = torch.device("cpu")
SPEC = [("Matern52", 1.3, 0.9, [0]), ("SquaredExponential", 0.7, [1.2, 1.5], [1, 2]), ("Matern32", 0.4, [1.0, 1.3, 0.9], None)]


# ------------------------------------------------------------------------------------------------ class semantics
def test_construction_flattening_and_the_limit_of_four():
    p = pkg()
    a, b, c, d, e = (p.SquaredExponential(), p.Matern32(active_dims=[1]), p.Matern52(), p.SquaredExponential(), p.Matern32())
    k = p.Product([p.Product([a, b]), c])
    assert k.kernels == [a, b, c] and k.kinds == (0, 2, 3) and k.name == "product"
    assert p.Product([a]).kernels == [a]
    assert p.Product([a, b, c, d]).kinds == (0, 2, 3, 0)
    with pytest.raises(ValueError, match="at most 4"):
        p.Product([a, b, c, d, e])
    with pytest.raises(ValueError, match="at least one"):
        p.Product([])
    with pytest.raises(ValueError, match="multi-output"):
        p.Product([a, p.SeparateIndependent([b, c])])
    with pytest.raises(ValueError, match="SquaredExponential, Matern32 or Matern52"):
        p.Product([a, object()])
    assert p.Product.MAX_COMPONENTS == p._backend.MAX_COMPONENTS == 4
    assert not isinstance(k, p.Sum) and not isinstance(a + b, p.Product)


def test_star_operator():
    p = pkg()
    a, b, c = p.SquaredExponential(), p.Matern32(), p.Matern52(active_dims=[0])
    k = a * b
    assert type(k) is p.Product and k.kernels == [a, b]
    k3 = k * c
    assert type(k3) is p.Product and k3.kernels == [a, b, c]
    assert (c * k).kernels == [c, a, b]  # a base kernel times a product flattens as well
    assert type(b * c) is p.Product  # __mul__ on the subclasses of SquaredExponential


def test_mixed_combinators_are_refused_by_name():
    p = pkg()
    a, b, c = p.SquaredExponential(), p.Matern32(), p.Matern52()
    with pytest.raises(NotImplementedError, match="Sum of Product"):
        p.Sum([a, b * c])
    with pytest.raises(NotImplementedError, match="Product of a Sum"):
        p.Product([a, b + c])
    with pytest.raises(NotImplementedError, match="Sum \\* kernel.*Product of a Sum"):
        (a + b) * c
    with pytest.raises(NotImplementedError, match="Product \\+ kernel.*Sum of Product"):
        (a * b) + c
    with pytest.raises(NotImplementedError, match="Sum of Product"):
        a + (b * c)
    with pytest.raises(NotImplementedError, match="Product of a Sum"):
        a * (b + c)


def test_stamp_changes_on_any_components_assign():
    p = pkg()
    k = R.build_pkg(p, SPEC)
    Z = np.random.RandomState(0).randn(6, 3)
    m = p.t_SVGP(k, p.Gaussian(), Z, device="cpu")
    seen = {(k.stamp(), m._kernel_versions())}
    for c in k.kernels:
        c.variance.assign(c.variance.item() * 1.5)
        seen.add((k.stamp(), m._kernel_versions()))
        c.lengthscales.assign(c.lengthscales.value * 1.5)
        seen.add((k.stamp(), m._kernel_versions()))
        c.lengthscales.value.mul_(2.0)  # in place: the tensor's own edit counter
        seen.add((k.stamp(), m._kernel_versions()))
    assert len(seen) == 1 + 3 * len(k.kernels)
    assert len({a for a, _ in seen}) == len(seen) and len({b for _, b in seen}) == len(seen)
    assert k.stamp()[0] == id(k) and k.stamp()[1:] == tuple(c.stamp() for c in k.kernels)


def test_prior_variance_variances_and_k_diag():
    p = pkg()
    k = R.build_pkg(p, SPEC)
    assert k.variances() == [1.3, 0.7, 0.4]
    assert k.prior_variance() == 1.3 * 0.7 * 0.4  # multiplied in index order
    assert p.estep.EStepEngine.kdiag(k) == k.prior_variance()
    X = np.random.RandomState(1).randn(7, 3)
    np.testing.assert_array_equal(k.K_diag(X).numpy(), np.full(7, 1.3 * 0.7 * 0.4))
    np.testing.assert_allclose(R.build(SPEC).K_diag(X), k.K_diag(X).numpy(), rtol=1e-15)


def test_inv_lengthscales_zero_pattern_and_cache():
    p = pkg()
    k = R.build_pkg(p, SPEC)
    il = k.inv_lengthscales(3, torch.float64, CPU)
    want = np.array([[1 / 0.9, 0, 0], [0, 1 / 1.2, 1 / 1.5], [1 / 1.0, 1 / 1.3, 1 / 0.9]])
    np.testing.assert_allclose(il.numpy(), want, rtol=1e-15)
    assert il.is_contiguous() and tuple(il.shape) == (3, 3)
    assert bool((il[0, 1:] == 0).all()) and il[1, 0].item() == 0.0
    assert k.inv_lengthscales(3, torch.float64, CPU) is il  # the cached array
    il32 = k.inv_lengthscales(3, torch.float32, CPU)
    assert il32.dtype == torch.float32 and k.inv_lengthscales(3, torch.float64, CPU) is il  # one slot per (D, dtype, device)
    k.kernels[1].lengthscales.assign([2.0, 4.0])
    il2 = k.inv_lengthscales(3, torch.float64, CPU)
    assert il2 is not il and il2[1, 1].item() == 0.5 and il2[1, 2].item() == 0.25
    with pytest.raises(ValueError, match="beyond the inputs"):
        k.inv_lengthscales(2, torch.float64, CPU)


def test_trainable_parameter_names():
    p = pkg()
    k = R.build_pkg(p, SPEC)
    m = p.t_SVGP(k, p.Gaussian(), np.zeros((4, 3)), device="cpu")
    names = p.training.trainable_parameters(m)
    want = [f"components.{c}.{n}" for c in range(3) for n in ("variance", "lengthscales")] + ["Z", "likelihood_variance"]
    assert list(names) == want
    for c, comp in enumerate(k.kernels):
        assert names[f"components.{c}.variance"][0] is comp.variance and names[f"components.{c}.lengthscales"][0] is comp.lengthscales
    assert len(m.trainable_parameters) == 2 * 3 + 2


def test_refusals_name_the_product():
    p = pkg()
    k = p.SquaredExponential() * p.Matern32(active_dims=[1])
    X, Y, Z = np.zeros((5, 2)), np.zeros((5, 1)), np.zeros((3, 2))
    with pytest.raises(NotImplementedError, match="t_SVGP_sites does not take a Product"):
        p.t_SVGP_sites((X, Y), k, p.Gaussian(), Z, device="cpu")
    with pytest.raises(NotImplementedError, match="t_VGP does not take a Product"):
        p.t_VGP((X, Y), k, p.Gaussian(), device="cpu")
    with pytest.raises(NotImplementedError, match="SeparateIndependent does not take a Product"):
        p.SeparateIndependent([p.SquaredExponential(), k])
    with pytest.raises(NotImplementedError, match="LinearCoregionalization does not take a Product"):
        p.LinearCoregionalization([k], np.ones((2, 1)))
    m = p.t_SVGP(k, p.Gaussian(), Z, device="cpu")
    with pytest.raises(NotImplementedError, match="sample_functions does not take a Product"):
        m.sample_functions(2)
    with pytest.raises(NotImplementedError, match="select_inducing_points does not take a Product"):
        p.select_inducing_points(X, k, 2)
    with pytest.raises(NotImplementedError, match="predict_f_vjp does not take a Product"):
        m.predict_f_vjp(X, np.ones((5, 1)))
    for model in (m, p.t_SVGP_white(k, p.Gaussian(), Z, device="cpu")):
        with pytest.raises(NotImplementedError, match="predict_f on an Xnew that requires grad does not take a Product"):
            model.predict_f(torch.zeros((5, 2), dtype=torch.float64, requires_grad=True))


def test_more_than_32_columns_and_more_than_16_in_the_gradient_are_refused_by_name():
    """The engine's entries raise before they touch the library or the device."""
    p = pkg()
    eng = object.__new__(p.estep.EStepEngine)
    eng.dtype, eng.device = torch.float64, CPU
    k = p.SquaredExponential() * p.Matern32()
    X = torch.zeros((4, 33), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="Product kernel takes at most 32"):
        eng.fill(X, X, k, torch.zeros((128, 128), dtype=torch.float64))
    X17 = torch.zeros((4, 17), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="M-step gradient of a Product kernel takes at most 16"):
        eng.kernel_grad_prod(X17, X17, k, None, None, None, None)


# ------------------------------------------------------------------------------------------------ K_torch
def _k_torch(k, Z, var=None, ls=None):
    var = [c.variance.value for c in k.kernels] if var is None else var
    ls = [c.lengthscales.value for c in k.kernels] if ls is None else ls
    return k.K_torch(Z, var, ls)


def test_k_torch_agrees_with_the_numpy_reference():
    p = pkg()
    Z = np.random.RandomState(3).randn(9, 3) * 1.3
    Z[1] = Z[0]  # r = 0 off the diagonal: the Matern clamp
    for spec in (SPEC, SPEC[:2], SPEC[:1], SPEC + [("SquaredExponential", 0.9, 2.0, [2])]):
        got = _k_torch(R.build_pkg(p, spec), torch.as_tensor(Z)).numpy()
        ref = R.build(spec).K(Z)
        assert np.max(np.abs(got - ref) / np.abs(ref)) <= 1e-14


def test_k_torch_autograd_against_central_differences():
    p = pkg()
    spec = SPEC[:2]
    Z0 = np.random.RandomState(4).randn(6, 3)
    W = np.random.RandomState(5).randn(6, 6)
    W = W + W.T

    def value(spec_, Z_):
        return float(np.sum(W * R.build(spec_).K(Z_)))

    k = R.build_pkg(p, spec)
    Zt = torch.tensor(Z0, requires_grad=True)
    var = [c.variance.value.clone().requires_grad_(True) for c in k.kernels]
    ls = [c.lengthscales.value.clone().requires_grad_(True) for c in k.kernels]
    grads = torch.autograd.grad(torch.sum(torch.as_tensor(W) * _k_torch(k, Zt, var, ls)), var + ls + [Zt])
    h = 1e-6

    def fd(change):
        up, dn = change(+h), change(-h)
        return (value(*up) - value(*dn)) / (2 * h)

    def with_field(c, field, idx, delta):
        s = [list(e) for e in spec]
        if idx is None:
            s[c][field] = s[c][field] + delta
        else:
            arr = np.array(s[c][field], dtype=np.float64)
            arr[idx] += delta
            s[c][field] = arr
        return [tuple(e) for e in s], Z0

    scale = max(abs(float(g.abs().max())) for g in grads)
    tol = 1e-7 * scale  # central differences at h = 1e-6: h^2 f''' ~ 1e-12 and rounding 1e-16 / h ~ 1e-10, relative to the scale
    for c in range(2):
        assert abs(float(grads[c]) - fd(lambda d: with_field(c, 1, None, d))) <= tol
    assert abs(float(grads[2]) - fd(lambda d: with_field(0, 2, None, d))) <= tol
    for i in range(2):
        assert abs(float(grads[3][i]) - fd(lambda d: with_field(1, 2, i, d))) <= tol
    for (m, d_) in [(0, 0), (3, 1), (5, 2)]:
        def moved(delta, m=m, d_=d_):
            Zc = Z0.copy()
            Zc[m, d_] += delta
            return spec, Zc
        assert abs(float(grads[4][m, d_]) - fd(moved)) <= tol


# ------------------------------------------------------------------------------------------------ the C ABI
FILL_ARGS = lambda ct: [ctypes.c_void_p] * 4 + [ct, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                              ctypes.c_int, ctypes.c_void_p]
GRAD_ARGS = lambda ct: [ctypes.c_void_p] * 4 + [ct, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int] \
    + [ctypes.c_void_p] * 4


def test_new_symbols_prototypes_and_abi_version():
    B = pkg()._backend
    lib = B.lib()
    header = open(B.HEADER_PATH).read()
    assert "#define TSVGP_ABI_VERSION 5" in header and B.ABI_VERSION == 5 and lib.tsvgp_abi_version() == 5
    for sfx, ct in (("f64", ctypes.c_double), ("f32", ctypes.c_float)):
        for name, args in ((f"tsvgp_kernel_fill_prod_{sfx}", FILL_ARGS(ct)), (f"tsvgp_kernel_grad_prod_{sfx}", GRAD_ARGS(ct))):
            assert hasattr(lib, name) and f"int {name}(" in header
            restype, argtypes = B._PROTOTYPES[name]
            assert restype is ctypes.c_int and list(argtypes) == args
            assert name in B.exported_symbols()
    T = "double"
    assert (f"int tsvgp_kernel_fill_prod_f64(const int *kinds_host, const {T} *X, const {T} *Z, const {T} *inv_ls, {T} variance,"
            in header)
    assert (f"int tsvgp_kernel_grad_prod_f64(const int *kinds_host, const {T} *X, const {T} *Z, const {T} *inv_ls, {T} variance,"
            in header)


@pytest.mark.parametrize("sfx,ctype", [("f64", "c_double"), ("f32", "c_float")])
def test_prod_fill_rejects_bad_arguments_before_any_launch(sfx, ctype):
    """Real host buffers, every pointer non-NULL: each call differs from a valid one in the one argument named."""
    lib = pkg()._backend.lib()
    ct = getattr(ctypes, ctype)
    esz = ctypes.sizeof(ct)
    N, M, D, ldk, C = 130, 130, 3, 256, 4
    buf = lambda n: (ct * n)()
    adr = ctypes.addressof
    aligned = lambda a: (adr(a) + 15) // 16 * 16
    X, Z, il, K = buf(N * D), buf(M * D), buf(C * D), buf(256 * ldk + 8)
    kinds = lambda *k: (ctypes.c_int * len(k))(*k)
    fill = getattr(lib, f"tsvgp_kernel_fill_prod_{sfx}")
    call = lambda k=kinds(0, 2, 3, 0), out=None, c=C, d=D, ld=ldk, n=N, m=M: fill(k, adr(X), adr(Z), adr(il), 1.3,
                                                                                 aligned(K) if out is None else out, n, m, d, ld, c, None)
    assert call(c=0) == 1 and call(c=5) == 1 and call(c=-1) == 1
    assert call(k=kinds(0, 1, 3, 0)) == 1  # the reserved kind
    assert call(k=kinds(0, 2, 3, 7)) == 1 and call(k=kinds(-1, 2, 3, 0)) == 1
    assert call(k=kinds(0, 2), c=2, out=aligned(K) + esz) == 1  # K one element behind the two-element boundary
    assert call(ld=ldk + 1) == 1 and call(ld=128) == 1  # odd, and narrower than round_up(M, 128)
    assert call(d=33) == 1 and call(d=0) == 1 and call(n=0) == 1 and call(m=0) == 1
    assert fill(None, adr(X), adr(Z), adr(il), 1.3, aligned(K), N, M, D, ldk, C, None) == 1
    assert fill(kinds(0, 2, 3, 0), adr(X), adr(Z), None, 1.3, aligned(K), N, M, D, ldk, C, None) == 1


@pytest.mark.parametrize("sfx,ctype", [("f64", "c_double"), ("f32", "c_float")])
def test_prod_grad_rejects_bad_arguments_before_any_launch(sfx, ctype):
    lib = pkg()._backend.lib()
    ct = getattr(ctypes, ctype)
    esz = ctypes.sizeof(ct)
    N, M, D, ldu, C = 130, 130, 3, 256, 4
    buf = lambda n: (ct * n)()
    adr = ctypes.addressof
    aligned = lambda a: (adr(a) + 15) // 16 * 16
    X, Z, il, U, g, beta = buf(N * D), buf(M * D), buf(C * D), buf(N * ldu + 8), buf(N), buf(M)
    parts = (ctypes.c_double * (256 * 16 * 4))()
    kinds = lambda *k: (ctypes.c_int * len(k))(*k)
    grad = getattr(lib, f"tsvgp_kernel_grad_prod_{sfx}")
    call = lambda k=kinds(0, 2, 3, 0), u=None, c=C, d=D, ld=ldu, n=N, m=M, gs=1, bs=1: grad(
        k, adr(X), adr(Z), adr(il), 1.3, aligned(U) if u is None else u, ld, adr(g), adr(g), gs, adr(beta), bs, n, m, d, c, adr(parts),
        adr(parts), adr(parts), None)
    assert call(c=0) == 1 and call(c=5) == 1
    assert call(k=kinds(0, 1, 3, 0)) == 1  # the reserved kind
    assert call(k=kinds(0, 2, 3, 7)) == 1
    assert call(d=17) == 1 and call(d=0) == 1 and call(n=0) == 1 and call(m=0) == 1
    assert call(ld=ldu + 1) == 1 and call(ld=128) == 1  # odd, and narrower than round_up(M, 128)
    assert call(u=aligned(U) + esz) == 1  # U one element behind the two-element boundary
    assert call(gs=0) == 1 and call(bs=0) == 1
    assert grad(None, adr(X), adr(Z), adr(il), 1.3, aligned(U), ldu, adr(g), adr(g), 1, adr(beta), 1, N, M, D, C, adr(parts), adr(parts),
                adr(parts), None) == 1


# ------------------------------------------------------------------------------------------------ the gradient reference's self-check
def test_kgrad_prod_ref_against_central_differences():
    """sum V o K with V held fixed, differentiated over (variance_c, lengthscale_cd, Z) at N = 40, M = 7, D = 3, C = 3."""
    rng = np.random.RandomState(12)
    N, M, D = 40, 7, 3
    kinds = ("matern52", "se", "matern32")
    X, Z = rng.randn(N, D), rng.randn(M, D)
    ls = 0.8 + rng.rand(3, D)
    var = [1.3, 0.7, 0.4]
    U, g0, g1, beta = rng.randn(N, M), rng.randn(N), rng.randn(N), rng.randn(M)
    Vfix = g0[:, None] * beta[None, :] - 2.0 * g1[:, None] * U
    out = G.fused(kinds, X, Z, 1.0 / ls, var, U, g0, g1, beta, rows=16)
    f = lambda Z_=Z, ls_=ls, var_=var: G.objective(kinds, X, Z_, ls_, var_, Vfix)
    h = 1e-6
    scale = max(np.max(np.abs(out["dZ"])), np.max(np.abs(out["dls"])), np.max(np.abs(out["dvar"])))
    tol = 1e-7 * scale  # as in the K_torch test above
    for c in range(3):
        up, dn = list(var), list(var)
        up[c] += h
        dn[c] -= h
        assert abs(out["dvar"][c] - (f(var_=up) - f(var_=dn)) / (2 * h)) <= tol
        for d in range(D):
            up, dn = ls.copy(), ls.copy()
            up[c, d] += h
            dn[c, d] -= h
            assert abs(out["dls"][c, d] - (f(ls_=up) - f(ls_=dn)) / (2 * h)) <= tol
    for m in range(M):
        for d in range(D):
            up, dn = Z.copy(), Z.copy()
            up[m, d] += h
            dn[m, d] -= h
            assert abs(out["dZ"][m, d] - (f(Z_=up) - f(Z_=dn)) / (2 * h)) <= tol
    assert out["A_vsum"] >= abs(out["vsum"]) and np.all(out["A_ls"] >= np.abs(out["dls"])) and np.all(out["A_Z"] >= np.abs(out["dZ"]))
    # one component: the single-kernel reference
    from tests import kgrad_ref
    one = G.fused(kinds[:1], X, Z, 1.0 / ls[:1], var[:1], U, g0, g1, beta)
    ref = kgrad_ref.fused(kinds[0], X, Z, 1.0 / ls[0], var[0], U, g0, g1, beta)
    np.testing.assert_allclose(one["dvar"][0], ref["dvar"], rtol=1e-13)
    np.testing.assert_allclose(one["dls"][0], ref["dls"], rtol=1e-12)
    np.testing.assert_allclose(one["dZ"], ref["dZ"], rtol=1e-12, atol=1e-14 * scale)
    np.testing.assert_allclose(one["A_Z"], ref["A_Z"], rtol=1e-12)


# ------------------------------------------------------------------------------------------------ the inclusion condition
@pytest.mark.parametrize("T", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_value_problem_keeps_ninety_percent_of_the_entries_relative(T, C):
    """``check_values`` holds at least 90 % of the entries to the relative rule: a cap on the input choice, asserted here for every
    (C, D, type) of tests/test_gpu_prodfill_values.py at N = 200, M = 64 (that file asserts it again at its own shapes).  With
    components 1.. at 1/16 of their ``inv_ls`` row the fraction of entries at or above 1e3 * tiny measures 96.3 - 97.7 % in fp64
    and 90.5 - 94.9 % in fp32 for C = 2, 4; with the rows as ``grid`` makes them most entries of a four-component product lie
    below the type's range.  From C = 2 on (component 0 a squared exponential, whose argument the grid bounds) every relatively
    checked entry has each a_c inside the type's normal range, so each component's ``rel_bound`` applies; C = 1 is the
    single-kernel grid itself."""
    for D in (1, 3, 8, 16, 32):
        pr = R.value_problem(SPECS[C], T, 200, 64, D)
        print(f"{T.__name__} C={C} D={D}: {100 * pr['frac']:.1f} % of the entries at or above 1e3 tiny")
        assert pr["frac"] >= 0.9
        rel = V.relative_mask(pr["ref"], T)
        for c in range(C if C > 1 else 0):
            a_c = V.reference(pr["kinds"][c], pr["X"], pr["Z"], pr["inv_ls"][c], 1.0)["a"]
            assert float(np.max(a_c[rel])) <= -np.log(V.TINY[T])  # 708.4 / 87.3
