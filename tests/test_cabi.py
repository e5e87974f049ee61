"""CPU checks of the C-ABI boundary: the in-tree library loads and exports every symbol include/tsvgp_hip.h declares,
the ctypes prototypes cover exactly those symbols, and argument validation works without a GPU (no compute calls)."""
import os
import re

import pytest

from tests.helpers import pkg


def _declared_symbols(header):
    src = open(header).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(tsvgp_\w+)\s*\(", src)))


def test_library_builds_and_exports_every_declared_symbol(repo_root):
    B = pkg()._backend
    path = pkg().build_library()
    assert os.path.exists(path)
    lib = B.lib()
    declared = _declared_symbols(os.path.join(repo_root, "include", "tsvgp_hip.h"))
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/tsvgp_hip.h but not exported by {path}"
    assert sorted(B.exported_symbols()) == declared  # the ctypes table and the header agree
    assert lib.tsvgp_version().decode().startswith("tsvgp_hip gfx950")


def test_every_source_and_header_of_csrc_is_listed_for_the_build():
    """A ``*.hip`` missing from ``SOURCES`` is not linked; a ``*.h`` missing from ``HEADERS`` is not in ``build_library()``'s (and
    ``tools/isa_diff.py --keep``'s) staleness check, so an edit to it would reuse the previous build."""
    B = pkg()._backend
    on_disk = sorted(os.listdir(B.CSRC))
    assert sorted(os.path.basename(p) for p in B.SOURCES) == [f for f in on_disk if f.endswith(".hip")]
    assert sorted(os.path.basename(p) for p in B.HEADERS if os.path.dirname(p) == B.CSRC) == [f for f in on_disk if f.endswith(".h")]
    assert B.HEADER_PATH in B.HEADERS


def test_argument_validation_needs_no_gpu():
    lib = pkg()._backend.lib()
    # null pointers / unpadded sizes are rejected before any launch
    assert lib.tsvgp_trmm_f64(None, None, None, 128, 128, 0, None) == 1
    assert lib.tsvgp_trmm_f32(None, None, None, 100, 128, 0, None) == 1
    assert lib.tsvgp_moments_f64(None, None, None, None, 1.0, 0, 0.0, None, None, None, None, None, None, 1, 128, 128, 1, 0, None) == 1
    assert lib.tsvgp_site_accum_f64(None, None, None, None, None, None, 128, 128, 1, 1, None) == 1
    assert lib.tsvgp_potrf_f64(None, 128, 128, 1, 0, None, None, 0, None) == 1
    # diagonal tiles get ceil(20 ns / 32) slices in fp64 (syrk1_kernel) and ceil(23 ns / 32) in fp32 (syrk_kernel)
    assert lib.tsvgp_site_accum_work_bytes_f64(1024, 1, 15) == (28 * 15 + 8 * 10) * 128 * 128 * 8 + 10 * 1024 * 8
    assert lib.tsvgp_site_accum_work_bytes_f32(1024, 1, 15) == (28 * 15 + 8 * 11) * 128 * 128 * 4 + 11 * 1024 * 4
    assert lib.tsvgp_site_accum_work_bytes_f32(1000, 1, 15) == -1


def test_potrf_rejects_the_removed_block_step_flag_and_no_keeper_symbol_is_exported():
    """Bit 8 of ``flags`` selected the tile-dataflow diagonal kernel, which is gone: the three factorisation entry points return
    TSVGP_EINVAL for it from the mask check, in front of any launch (M = 128, one matrix, real host buffers: nothing reads them).
    Bit 16 (TSVGP_POTRF_FUSE) is still a valid selection and is exercised on the GPU (test_potrf_block_step_variants).  The clock
    keeper's two entry points are gone too: the library exports no ``tsvgp_keeper_*`` symbol."""
    import ctypes

    B = pkg()._backend
    lib = B.lib()
    M = 128
    A = (ctypes.c_double * (2 * M * M))()  # the matrix and, for potrf_solve, M right-hand-side rows below it
    work, X, Xt, T = ((ctypes.c_double * (M * M))() for _ in range(4))
    info = (ctypes.c_int32 * 1)()
    ptr = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert B.POTRF_SUBST | B.POTRF_RHS_UPPER | B.POTRF_DIAG_V1 | B.POTRF_FUSE == 23  # bit 8 is the one no name is left for
    for flags in (8, 8 | B.POTRF_DIAG_V1):
        assert lib.tsvgp_potrf_f64(ptr(A), M, M, 1, M * M, ptr(info), ptr(work), flags, None) == 1
        assert lib.tsvgp_potrf_inv_f64(ptr(A), M, M, 1, M * M, ptr(info), ptr(work), ptr(X), ptr(Xt), ptr(T), flags, None) == 1
        assert lib.tsvgp_potrf_solve_f64(ptr(A), M, M, 1, 2 * M * M, ptr(info), ptr(work), M, flags, None) == 1
    assert not hasattr(lib, "tsvgp_keeper_run") and not hasattr(lib, "tsvgp_keeper_signal")
    assert not [n for n in B.exported_symbols() if "keeper" in n]
    assert b"tsvgp_keeper_" not in open(os.environ.get("TSVGP_HIP_LIB", B.LIB_PATH), "rb").read()  # the dynamic symbol table's strings included


@pytest.mark.parametrize("entry", ["potrf", "potrf_solve", "potrf_inv"])
def test_potrf_rejects_layouts_its_16_byte_row_accesses_cannot_take(entry):
    """The kernels behind the three factorisation entries move rows with 16-byte loads and stores at A + b*stride + r*lda + c and
    factor the matrices of a batch side by side: an odd lda, an A off the 16-byte boundary, an odd stride in a batch and a stride
    that lets two matrices of a batch overlap, and a work, X, Xt or T off the boundary, are TSVGP_EINVAL in front of any launch
    (real host buffers, every pointer non-NULL: nothing reads them).  Each rejected call differs in ONE argument from a call the entry accepts (tests.helpers.
    potrf_layout_cases); that the accepted ones run and give the right factor is tests/test_gpu_chol_family.py's part.  One matrix
    keeps taking any stride when no rows ride along (the call in test_argument_validation_needs_no_gpu passes 0)."""
    import ctypes

    from tests.helpers import POTRF_AUX_OFF, potrf_layout_cases

    lib = pkg()._backend.lib()
    M = 128
    rhs_rows = M if entry == "potrf_solve" else 0
    aligned = lambda a: (ctypes.addressof(a) + 15) // 16 * 16
    work, X, Xt, T = ((ctypes.c_double * (2 * M * M + 2))() for _ in range(4))
    info = (ctypes.c_int32 * 2)()

    def call(lda, off, batch, stride):
        A = (ctypes.c_double * (batch * stride + 8))()
        a = aligned(A) + 8 * off
        if entry == "potrf":
            return lib.tsvgp_potrf_f64(a, M, lda, batch, stride, ctypes.addressof(info), aligned(work), 0, None)
        if entry == "potrf_solve":
            return lib.tsvgp_potrf_solve_f64(a, M, lda, batch, stride, ctypes.addressof(info), aligned(work), rhs_rows, 0, None)
        return lib.tsvgp_potrf_inv_f64(a, M, lda, batch, stride, ctypes.addressof(info), aligned(work), aligned(X), aligned(Xt),
                                       aligned(T), 0, None)

    cases = potrf_layout_cases(M, rhs_rows)
    assert len(cases) == 4
    for name, ok, bad in cases:
        assert sum(ok[key] != bad[key] for key in ok) == 1, name  # the neighbour differs in that one argument
        assert ok["lda"] % 2 == 0 and ok["off"] % 2 == 0 and ok["stride"] % 2 == 0 and ok["stride"] >= (M + rhs_rows) * ok["lda"], name
        assert call(**bad) == 1, f"{entry}: {name} was not rejected"
    # work (and X, Xt, T of the inverse path) are moved the same way: each one 8 bytes off the boundary, on the first accepted layout
    lay = cases[0][1]
    A = (ctypes.c_double * (lay["batch"] * lay["stride"] + 8))()
    a, inf = aligned(A), ctypes.addressof(info)
    assert POTRF_AUX_OFF[0] % 2 == 0 and POTRF_AUX_OFF[1] % 2 == 1
    bump = 8 * POTRF_AUX_OFF[1]
    if entry == "potrf":
        assert lib.tsvgp_potrf_f64(a, M, lay["lda"], lay["batch"], lay["stride"], inf, aligned(work) + bump, 0, None) == 1
    elif entry == "potrf_solve":
        assert lib.tsvgp_potrf_solve_f64(a, M, lay["lda"], lay["batch"], lay["stride"], inf, aligned(work) + bump, rhs_rows, 0, None) == 1
    else:
        for which in range(4):
            w, x, xt, t = (aligned(buf) + (bump if i == which else 0) for i, buf in enumerate((work, X, Xt, T)))
            assert lib.tsvgp_potrf_inv_f64(a, M, lay["lda"], lay["batch"], lay["stride"], inf, w, x, xt, t, 0, None) == 1, which


@pytest.mark.parametrize("sfx,ctype", [("f64", "c_double"), ("f32", "c_float")])
def test_kernel_matrix_entries_reject_an_output_off_its_vector_boundary(sfx, ctype):
    """The fill, ``tsvgp_gram_to_kernel_*`` and ``tsvgp_gram_to_gradw_*`` move a thread's two adjacent columns as one vector at
    K + n*ldk + m with m and ldk even: K (G and U of the gradient form) one element behind a two-element boundary -- 8 bytes off a
    16-byte boundary in fp64, 4 bytes off an 8-byte boundary in fp32 -- is TSVGP_EINVAL in front of any launch (real host buffers,
    every pointer non-NULL, every other argument valid: nothing reads them).  The fp32 layouts that only rule out the 16-byte
    stores -- K 8 bytes off, ldk or strideK 2 modulo 4 -- stay legal and RUN in tests/test_gpu_kernel_values.py."""
    import ctypes

    lib = pkg()._backend.lib()
    ct = getattr(ctypes, ctype)
    esz = ctypes.sizeof(ct)
    N, M, D, ldk, P = 130, 130, 3, 256, 2
    Np = 256
    buf = lambda n: (ct * n)()
    aligned = lambda a: (ctypes.addressof(a) + 15) // 16 * 16
    X, Z, il, xx, zz, g0, g1, beta = buf(N * D), buf(M * D), buf(P * D), buf(N), buf(M), buf(N), buf(N), buf(M)
    K, Ubuf = buf(P * (Np * ldk + 2) + 8), buf(Np * ldk + 8)
    vpart = (ctypes.c_double * int(lib.tsvgp_gram_to_gradw_parts(N, M)))()
    var = (ct * P)(1.3, 0.8)
    adr = ctypes.addressof
    off = aligned(K) + esz  # one element behind the boundary
    assert off % (2 * esz) == esz
    fill = getattr(lib, f"tsvgp_kernel_fill_{sfx}")
    assert fill(0, adr(X), adr(Z), adr(il), 1.3, off, N, M, D, ldk, None) == 1
    assert getattr(lib, f"tsvgp_se_fill_{sfx}")(adr(X), adr(Z), adr(il), 1.3, off, N, M, D, ldk, None) == 1
    batched = getattr(lib, f"tsvgp_kernel_fill_batched_{sfx}")
    assert batched(0, adr(X), adr(Z), adr(il), adr(var), off, Np * ldk + 2, N, M, D, ldk, P, None) == 1
    assert batched(0, adr(X), adr(Z), adr(il), adr(var), aligned(K), Np * ldk + 1, N, M, D, ldk, P, None) == 1  # K + strideK off it
    assert getattr(lib, f"tsvgp_gram_to_kernel_{sfx}")(3, off, adr(xx), adr(zz), 1.3, N, M, ldk, None) == 1
    gradw = getattr(lib, f"tsvgp_gram_to_gradw_{sfx}")
    tail = (adr(g0), adr(g1), 1, adr(beta), 1, N, M, ldk, adr(vpart), None)
    assert gradw(2, off, adr(xx), adr(zz), 1.3, aligned(Ubuf), ldk, *tail) == 1
    assert gradw(2, aligned(K), adr(xx), adr(zz), 1.3, aligned(Ubuf) + esz, ldk, *tail) == 1
    # an odd ldk was rejected before and still is
    assert fill(0, adr(X), adr(Z), adr(il), 1.3, aligned(K), N, M, D, ldk + 1, None) == 1


def test_product_path_fails_loudly_without_gpu():
    """No CPU fallback: with no ROCm device the model refuses to run the E-step (it never routes through the oracle)."""
    import numpy as np
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = pkg()
    m = p.t_SVGP(p.SquaredExponential(), p.Gaussian(0.1), np.zeros((4, 2)) + np.arange(4)[:, None])
    for call in (lambda: m.natgrad_step((np.zeros((5, 2)), np.zeros((5, 1)))), lambda: m.elbo((np.zeros((5, 2)), np.zeros((5, 1)))),
                 lambda: m.predict_f(np.zeros((5, 2)))):
        with pytest.raises(p.HipExtensionError):
            call()
    w = p.t_SVGP_white(p.SquaredExponential(), p.Gaussian(0.1), np.zeros((4, 2)) + np.arange(4)[:, None])
    data = (np.zeros((5, 2)), np.zeros((5, 1)))
    for call in (lambda: w.natgrad_step(data), lambda: w.elbo(data), lambda: w.predict_f(data[0]), lambda: m.elbo_and_grads(data)):
        with pytest.raises(p.HipExtensionError):
            call()
    assert lib_validation_extra()


def lib_validation_extra():
    lib = pkg()._backend.lib()
    ok = lib.tsvgp_potrf_inv_f64(None, 128, 128, 1, 0, None, None, None, None, None, 0, None) == 1
    ok &= lib.tsvgp_kernel_fill_f64(7, None, None, None, 1.0, None, 10, 4, 2, 128, None) == 1
    ok &= lib.tsvgp_kernel_grad_f64(0, None, None, None, 1.0, None, 128, None, None, 1, None, 1, 10, 4, 2, None, None, None, None) == 1
    ok &= lib.tsvgp_kernel_grad_rows() == 1024 and lib.tsvgp_kernel_grad_dpad(5) == 8
    return bool(ok)


def test_package_never_imports_the_oracle(repo_root):
    """oracle/ is test infrastructure: nothing under t-svgp_amd/ may import or reference it."""
    for dirpath, _, files in os.walk(os.path.join(repo_root, "t-svgp_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in text, f"{f} mentions the oracle"
