"""CPU checks of the ``Sum`` kernel and ``active_dims``: construction, validation, the host-side algebra against the NumPy
reference of tests/sum_kernel_ref.py, the staleness stamps, the parameter names, the refusals by name and the argument checks
of ``tsvgp_kernel_fill_sum_*`` (host buffers: nothing launches)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import tsvgp_oracle as O
from tests import sum_kernel_ref as R
from tests.helpers import pkg

CPU = torch.device("cpu")

SPEC = [("SquaredExponential", 1.3, [0.9, 1.4], [0, 1]), ("Matern52", 0.6, [0.5, 0.8, 1.1], [2, 3, 4]),
        ("Matern32", 0.25, 0.7, None)]


def _relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


def test_construction_and_validation():
    p = pkg()
    with pytest.raises(ValueError):
        p.Sum([])
    five = [p.SquaredExponential() for _ in range(5)]
    with pytest.raises(ValueError, match="at most 4"):
        p.Sum(five)
    with pytest.raises(ValueError, match="multi-output"):
        p.Sum([p.SquaredExponential(), p.SeparateIndependent([p.SquaredExponential()])])
    with pytest.raises(ValueError, match="multi-output"):
        p.Sum([p.LinearCoregionalization([p.SquaredExponential()], np.ones((2, 1)))])
    assert len(p.Sum([p.Matern32()]).kernels) == 1 and len(p.Sum(five[:4]).kernels) == 4
    with pytest.raises(ValueError):
        p.SquaredExponential(active_dims=[0, 0])
    with pytest.raises(ValueError):
        p.SquaredExponential(active_dims=[])
    with pytest.raises(ValueError):
        p.Matern32(lengthscales=[1.0, 2.0], active_dims=[0, 1, 2])
    assert p.Matern52().active_dims is None


def test_plus_flattens():
    p = pkg()
    a, b, c, d = p.SquaredExponential(), p.Matern32(), p.Matern52(), p.SquaredExponential(active_dims=[1])
    s = a + b
    assert isinstance(s, p.Sum) and s.kernels == [a, b] and s.kinds == (0, 2)
    assert (s + c).kernels == [a, b, c] and (c + s).kernels == [c, a, b]
    assert ((a + b) + (c + d)).kernels == [a, b, c, d]
    assert p.Sum([s, p.Sum([c])]).kernels == [a, b, c]
    with pytest.raises(ValueError):
        (a + b) + (c + d) + p.Matern32()


def test_k_diag_and_k_torch_agree_with_the_numpy_reference():
    p = pkg()
    k, ref = R.build_pkg(p, SPEC), R.build(SPEC)
    rng = np.random.RandomState(0)
    Z = rng.randn(17, 5)
    np.testing.assert_allclose(k.K_diag(torch.as_tensor(Z)).cpu().numpy(), ref.K_diag(Z), rtol=1e-14)
    assert abs(k.prior_variance() - (1.3 + 0.6 + 0.25)) < 1e-15
    var = [c.variance.value.to(CPU) for c in k.kernels]
    ls = [c.lengthscales.value.to(CPU) for c in k.kernels]
    got = k.K_torch(torch.as_tensor(Z), var, ls).numpy()
    want = ref.K(Z)
    # the oracle's distance is GPflow's expanded form: its own rounding is ~1e-15 of |x|^2 on r^2, far inside 1e-14 of K here
    assert _relerr(got, want) < 1e-14
    # a base kernel with active_dims alone
    one = p.Matern32(variance=0.7, lengthscales=[0.8, 1.2], active_dims=[3, 1])
    ref1 = R.Active(O.Matern32(variance=0.7, lengthscales=[0.8, 1.2]), [3, 1])
    got1 = one.K_torch(torch.as_tensor(Z), one.variance.value.to(CPU), one.lengthscales.value.to(CPU)).numpy()
    assert _relerr(got1, ref1.K(Z)) < 1e-14


def test_inv_lengthscales_zero_pattern_and_cache_key():
    p = pkg()
    k = p.Matern52(lengthscales=[0.5, 2.0], active_dims=[3, 1])
    il = k.inv_lengthscales(5, torch.float64, CPU)
    np.testing.assert_array_equal(il.numpy(), [0.0, 0.5, 0.0, 2.0, 0.0])
    assert k.inv_lengthscales(5, torch.float64, CPU) is il  # cached
    assert len(k.__dict__["_inv_ls_cache"][0]) == 8 and k.__dict__["_inv_ls_cache"][0][-1] == (3, 1)
    k.active_dims = (1, 3)  # same parameter, other columns: the key must tell them apart
    np.testing.assert_array_equal(k.inv_lengthscales(5, torch.float64, CPU).numpy(), [0.0, 2.0, 0.0, 0.5, 0.0])
    iso = p.SquaredExponential(lengthscales=4.0, active_dims=[2])
    np.testing.assert_array_equal(iso.inv_lengthscales(3, torch.float32, CPU).numpy(), np.float32([0.0, 0.0, 0.25]))
    with pytest.raises(ValueError):
        iso.inv_lengthscales(2, torch.float64, CPU)
    # default None: the dense vector, and the key of before (seven entries)
    d = p.SquaredExponential(lengthscales=[1.0, 2.0])
    np.testing.assert_array_equal(d.inv_lengthscales(2, torch.float64, CPU).numpy(), [1.0, 0.5])
    assert len(d.__dict__["_inv_ls_cache"][0]) == 7
    s = R.build_pkg(p, SPEC)
    ils = s.inv_lengthscales(5, torch.float64, CPU)
    assert tuple(ils.shape) == (3, 5) and ils.is_contiguous()
    np.testing.assert_array_equal(ils.numpy() == 0.0, [[0, 0, 1, 1, 1], [1, 1, 0, 0, 0], [0, 0, 0, 0, 0]])
    assert s.inv_lengthscales(5, torch.float64, CPU) is ils
    s.kernels[1].lengthscales.assign([1.0, 1.0, 4.0])
    assert s.inv_lengthscales(5, torch.float64, CPU)[1, 4].item() == 0.25


def test_stamp_sees_every_component():
    p = pkg()
    s = R.build_pkg(p, SPEC)
    Z = np.random.RandomState(0).randn(6, 5)
    m = p.t_SVGP(s, p.Gaussian(), Z, device="cpu")
    w = p.t_SVGP_white(s, p.Gaussian(), Z, device="cpu")
    seen = {(s.stamp(), m._kernel_versions())}
    for c in s.kernels:
        c.variance.assign(c.variance.item() * 1.5)
        seen.add((s.stamp(), m._kernel_versions()))
        c.lengthscales.assign(c.lengthscales.value * 1.5)
        seen.add((s.stamp(), m._kernel_versions()))
        c.lengthscales.value.mul_(2.0)  # in place: the tensor's own edit counter
        seen.add((s.stamp(), m._kernel_versions()))
    assert len(seen) == 1 + 3 * len(s.kernels)
    assert len({a for a, _ in seen}) == len(seen) and len({b for _, b in seen}) == len(seen)
    assert w.kernel is s
    # a base kernel's stamp is the triple the models keyed on before
    b = p.Matern32()
    assert b.stamp() == (id(b), b.variance.stamp(), b.lengthscales.stamp())


def test_trainable_parameter_names():
    p = pkg()
    s = R.build_pkg(p, SPEC)
    m = p.t_SVGP(s, p.Gaussian(), np.zeros((4, 5)), device="cpu")
    names = p.training.trainable_parameters(m)
    want = [f"components.{c}.{n}" for c in range(3) for n in ("variance", "lengthscales")] + ["Z", "likelihood_variance"]
    assert list(names) == want
    for c, k in enumerate(s.kernels):
        assert names[f"components.{c}.variance"][0] is k.variance and names[f"components.{c}.lengthscales"][0] is k.lengthscales
    pars = m.trainable_parameters
    for k in s.kernels:
        assert any(q is k.variance for q in pars) and any(q is k.lengthscales for q in pars)
    assert len(pars) == 2 * 3 + 2


def test_refusals_name_the_sum():
    p = pkg()
    s = p.SquaredExponential() + p.Matern32(active_dims=[1])
    X, Y, Z = np.zeros((5, 2)), np.zeros((5, 1)), np.zeros((3, 2))
    with pytest.raises(NotImplementedError, match="Sum"):
        p.t_SVGP_sites((X, Y), s, p.Gaussian(), Z, device="cpu")
    with pytest.raises(NotImplementedError, match="Sum"):
        p.t_VGP((X, Y), s, p.Gaussian(), device="cpu")
    with pytest.raises(NotImplementedError, match="Sum"):
        p.SeparateIndependent([p.SquaredExponential(), s])
    with pytest.raises(NotImplementedError, match="Sum"):
        p.LinearCoregionalization([s], np.ones((2, 1)))
    with pytest.raises(NotImplementedError, match="Sum"):
        p.t_SVGP(s, p.Gaussian(), Z, device="cpu").sample_functions(2)
    with pytest.raises(NotImplementedError, match="Sum"):
        p.select_inducing_points(X, s, 2)
    # a base kernel with active_dims is an inv_ls with zeros: constructed everywhere
    a = p.Matern52(active_dims=[1])
    p.SeparateIndependent([a, a])
    p.t_SVGP_sites((X, Y), a, p.Gaussian(), Z, device="cpu")


def test_sum_refuses_more_than_32_columns_by_name():
    """The engine's entry raises before it touches the library or the device."""
    p = pkg()
    eng = object.__new__(p.estep.EStepEngine)
    s = p.SquaredExponential() + p.Matern32()
    X = torch.zeros((4, 33), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="Sum"):
        eng.fill(X, X, s, torch.zeros((128, 128), dtype=torch.float64))
    assert p.estep.EStepEngine.kdiag(s) == 2.0 and p.estep.EStepEngine.kdiag(p.Matern32(variance=0.3)) == 0.3


def test_new_symbols_and_abi_version():
    B = pkg()._backend
    lib = B.lib()
    assert B.ABI_VERSION == 5 and lib.tsvgp_abi_version() == 5
    assert hasattr(lib, "tsvgp_kernel_fill_sum_f64") and hasattr(lib, "tsvgp_kernel_fill_sum_f32")
    assert B.MAX_COMPONENTS == 4 == pkg().Sum.MAX_COMPONENTS
    assert B.SOURCES[0].endswith("tsvgp_kernels.hip")


@pytest.mark.parametrize("sfx,ctype", [("f64", "c_double"), ("f32", "c_float")])
def test_sum_fill_rejects_bad_arguments_before_any_launch(sfx, ctype):
    """Real host buffers, every pointer non-NULL: each call differs from a valid one in the one argument named."""
    lib = pkg()._backend.lib()
    ct = getattr(ctypes, ctype)
    esz = ctypes.sizeof(ct)
    N, M, D, ldk, C = 130, 130, 3, 256, 4
    buf = lambda n: (ct * n)()
    adr = ctypes.addressof
    aligned = lambda a: (adr(a) + 15) // 16 * 16
    X, Z, il, K = buf(N * D), buf(M * D), buf(C * D), buf(256 * ldk + 8)
    var = (ct * C)(1.3, 0.8, 0.5, 0.2)
    kinds = lambda *k: (ctypes.c_int * len(k))(*k)
    fill = getattr(lib, f"tsvgp_kernel_fill_sum_{sfx}")
    call = lambda k=kinds(0, 2, 3, 0), out=None, c=C, d=D, ld=ldk, n=N, m=M: fill(k, adr(X), adr(Z), adr(il), adr(var),
                                                                                 aligned(K) if out is None else out, n, m, d, ld, c, None)
    assert call(c=0) == 1 and call(c=5) == 1 and call(c=-1) == 1
    assert call(k=kinds(0, 1, 3, 0)) == 1  # the reserved kind
    assert call(k=kinds(0, 2, 3, 7)) == 1 and call(k=kinds(-1, 2, 3, 0)) == 1
    assert call(k=kinds(0, 2), c=2, out=aligned(K) + esz) == 1  # K one element behind the two-element boundary
    assert call(ld=ldk + 1) == 1 and call(ld=128) == 1  # odd, and narrower than round_up(M, 128)
    assert call(d=33) == 1 and call(d=0) == 1 and call(n=0) == 1 and call(m=0) == 1
    assert fill(None, adr(X), adr(Z), adr(il), adr(var), aligned(K), N, M, D, ldk, C, None) == 1
    assert fill(kinds(0, 2, 3, 0), adr(X), adr(Z), adr(il), None, aligned(K), N, M, D, ldk, C, None) == 1
