"""Host-side driver of one N-pass of the E-step on one GPU: owns the HBM work buffers and launches the HIP kernels.

Data layout in HBM (T = compute dtype, fp64 or fp32; Np/Mp = N/M rounded up to 128, padding zero-filled):

    X    [N  x D ]  inputs (row-major, read once per pass by the fill kernel)
    Y    [N  x P ]  targets
    Kfu  [Np x Mp]  cross-covariance K(X, Z), written once by ``tsvgp_se_fill``
    B    [Np x Mp]  whitened cross-covariance  B = Kfu U9^-T  (Kuu + jitter I = U9 U9^T), written by ``tsvgp_trmm``
                    (whitened / projected routes only; on the projected route a = U9^-T b then overwrites Kfu)
    g0,g1[Np x P ]  likelihood gradients (rows >= N are zero)
    work            partial 128x128 tiles of the weighted Gram, [P][nsplit][ntri][128*128] (+ first-order partials)

Kernel sequence of ``run(..., sites=True)`` by projection route (models/tsvgp.py):
    direct:     fill -> moments(UPPER, on Kfu) -> site_accum(Kfu)
    whitened:   fill -> trmm(UPPER) -> moments(UPPER, on B) -> site_accum(B)
    projected:  fill -> trmm(UPPER) -> moments(UPPER, on B) -> trmm(LOWER) -> site_accum(a)
``mean_only`` replaces the moments product by one HBM-bound sweep (Gaussian likelihood, TSVGP_LIK_MEANONLY).
A likelihood that couples the latents of a row (``LIK_HETERO``: two latents, ``LIK_SOFTMAX`` / ``LIK_MULTICLASS``: C latents; Y [N x 1]) cannot run in
the moments kernels' per-latent epilogue: its pass runs the moments of every latent with no likelihood (mean, var), then its map
on them, then the site sums of the route -- ``run`` with P = latent_dim on one kernel, ``_run_batched`` on separate kernels, and a
two-sweep form on the one-pass-per-latent path (``_run_separate_coupled``).  The scalar likelihoods that have no arm in the moments
kernels (``LIK_STUDENT_T``, ``LIK_POISSON``, ``LIK_GAMMA``, ``LIK_ORDINAL``; Y [N x P], one column per latent) take the same passes.  Every map from
(mean, var, Y) to (g0, g1, ve, nonpos) that runs as a launch of its own, the Gaussian / Bernoulli one of the stored-tile and
two-product passes included, goes through ``EStepEngine.lik_map``.
Under ``LinearCoregionalization`` (P outputs mixed from the L latents of separate kernels by W [P, L], Y [N, P]) any such likelihood
takes the mapped passes with ``_mixed_map`` for the map: ``lmc_mix`` (latent moments -> mixed), ``lik_map`` on the outputs,
``lmc_unmix`` (the gradients back onto the latents), and the site sums over the L latents.
The two other N-sized launches of a pass have one entry each
as well, for the shared operand [Np, Mp] and the per-latent one [P, Np, Mp] alike: ``EStepEngine.moments`` (``_moments_then_map`` is
the mapped pass's pair of it and ``lik_map``) and ``EStepEngine._site_sums``.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import _backend as B
from .distributed import world_size
from .kernels import COMBINED, LinearCoregionalization, Product, SeparateIndependent, Sum, refuse_product
from .side_branch import SideBranch, SideStream

MAX_INPUT_DIM = 32  # the fill kernel pads D to a compile-time size (1, 2, 4, 8, 16, 32)
MAX_INPUT_DIM_GRAD = 16  # tsvgp_kernel_grad_* (M-step): 1, 2, 4, 8, 16; beyond: GEMM form (tsvgp_gram_to_gradw_*)


@dataclass
class EStepStats:
    """Per-shard outputs of one N-pass (all fp64 on the model device)."""

    n_rows: int
    ve_sum: torch.Tensor  # scalar: sum of variational expectations over the shard's rows
    nonpos: torch.Tensor  # scalar: number of rows with non-positive predictive variance
    acc2: Optional[torch.Tensor] = None  # [P, M, M] sum_n g1 b_n b_n^T (whitened coordinates)
    acc1: Optional[torch.Tensor] = None  # [P, M]    sum_n g0 b_n
    mean: Optional[torch.Tensor] = None  # [N, P]
    var: Optional[torch.Tensor] = None  # [N, P]
    g0: Optional[torch.Tensor] = None  # [N, P]
    g1: Optional[torch.Tensor] = None  # [N, P]
    tile: Optional[torch.Tensor] = None  # [Np, Mp] the stored triangular product t_n = Tm k_n (run(keep_tile=True))
    dparam: Optional[torch.Tensor] = None  # scalar: sum of d ve / d (likelihood parameter) over the rows (LIK_STUDENT_T: scale,
    # LIK_GAMMA: shape, LIK_ORDINAL: sigma)
    # LinearCoregionalization (mean, var, g0, g1, acc2, acc1 above are the L latents'): the P mixed outputs' counterparts
    fmu: Optional[torch.Tensor] = None  # [N, P] mixed mean
    fvar: Optional[torch.Tensor] = None  # [N, P] mixed variance
    g0_f: Optional[torch.Tensor] = None  # [N, P] d ve / d fmu
    g1_f: Optional[torch.Tensor] = None  # [N, P] d ve / d fvar, never cropped
    dW: Optional[torch.Tensor] = None  # [P, L] sum of d ve / d W over the rows (a pass with LIK_NOCROP)


@dataclass
class LikMapResult:
    """What ``EStepEngine.lik_map`` wrote: cached buffers of the engine, or the caller's own where it handed them in."""

    g0: torch.Tensor  # [Np, P] d ve / d mean (rows >= N zero)
    g1: torch.Tensor  # [Np, P] d ve / d var (rows >= N zero)
    ve_partial: torch.Tensor  # fp64 sums of ve per 128 rows: [Np / 128], or [P, Np / 128] from the per-column scalar map
    nonpos_partial: torch.Tensor  # int32 counts of rows with var <= 0, the same shape
    dparam: Optional[torch.Tensor] = None  # scalar: sum of d ve / d parameter over the rows (StudentT, Gamma, Ordinal)
    # ``_mixed_map`` (g0, g1 above are then the L latents'): the mixed moments and the map's own gradients [Np, P], the sum of d ve / d W
    fmu: Optional[torch.Tensor] = None
    fvar: Optional[torch.Tensor] = None
    g0_f: Optional[torch.Tensor] = None
    g1_f: Optional[torch.Tensor] = None
    dW: Optional[torch.Tensor] = None


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def per_latent(t, p):
    """Entry p of a per-latent operand given as None, a list, a [P, M, M] tensor or one shared [M, M] tensor."""
    if t is None:
        return None
    if isinstance(t, (list, tuple)):
        return t[p]
    return t[p] if t.dim() == 3 else t


def site_sum_chunk_rows(f64: bool, P: int) -> int:
    """Rows per k-chunk of the site-sum kernel that runs for this type and latent count: syrk1_kernel (fp64) 16,
    syrk1f_kernel (fp32, P <= 8) 32, the round-2 syrk_kernel (P > 8, either type) 16.  A slice shorter than one chunk is an
    empty workgroup (harmless, wasted): the slice count is capped at Np / this."""
    return 32 if (not f64 and P <= 8) else 16


def site_sum_slices(Mp: int, P: int, Np, slots: int, f64: bool, oversubscribe=None) -> int:
    """The slice count of ``EStepEngine.choose_nsplit`` as a pure function of the shape and of the resident workgroup slots
    (256 for fp64, 512 for fp32 on MI355X): see there for the cost model and the measurements behind it."""
    nt = Mp // B.TILE
    n_off = nt * (nt - 1) // 2
    num = 20 if f64 else 22  # TSVGP_SYRK1_DIAG_NUM / TSVGP_SYRK1F_DIAG_NUM
    ns_diag = lambda ns: max(1, (num * ns + 31) // 32)
    if Np is None or oversubscribe is not None:
        # (no row count, or a forced oversubscription: the largest count that fits one round, times the factor)
        ns = 1
        while P * (n_off * (ns + 1) + nt * ns_diag(ns + 1)) <= slots:
            ns += 1
        return ns * (oversubscribe if oversubscribe is not None else 8)
    chunks = max(1, Np // site_sum_chunk_rows(f64, P))  # the kernels' chunks: 16 rows (fp64) / 32 rows (fp32, P <= 8)
    overhead = 14.0
    best, best_t = 1, None
    for ns in range(1, max(1, min(chunks // 32, 1024)) + 1):
        nd = ns_diag(ns)
        rounds = -(-(P * (n_off * ns + nt * nd)) // slots)
        per = max(-(-chunks // ns) if n_off else 0, -(-chunks // nd) * num / 32.0)
        t = rounds * (per + overhead) * (1.02 if rounds == 1 else 1.0)
        if best_t is None or t < best_t * (1.0 - 1e-9):
            best, best_t = ns, t
    return best


def gaussian_g1_const(lik_id, lik_param, dtype=torch.float64):
    """The value every live row of g1 takes under a homoskedastic Gaussian likelihood, as the moments kernel writes it --
    -1 / (2 s2), cropped at -1e-8 unless LIK_NOCROP, rounded to the compute ``dtype`` -- or None when ``lik_id`` is another
    likelihood or ``lik_param`` is no finite positive scalar: what a model hands ``EStepEngine.run(g1_const=...)``."""
    if (lik_id & 0xFF) != B.LIK_GAUSSIAN or not isinstance(lik_param, (int, float)) or not (0.0 < lik_param < math.inf):
        return None
    c = -0.5 / float(lik_param)
    if not (lik_id & B.LIK_NOCROP):
        c = min(c, -1e-8)
    return float(torch.tensor(c, dtype=torch.float64).to(dtype))


class EStepEngine:
    """Launches the C-ABI kernels (include/tsvgp_hip.h) on torch-allocated device memory."""

    def __init__(self, compute_dtype=torch.float64, device=None):
        self.lib = B.lib()  # raises HipExtensionError when the extension is not built
        if not torch.cuda.is_available():
            raise B.HipExtensionError("no ROCm device visible: the t-SVGP E-step has no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise B.HipExtensionError(f"EStepEngine needs a ROCm device, got {self.device}")
        self.dtype = compute_dtype
        self.sfx = B.suffix(compute_dtype)
        self._buf = {}
        self._slots = None
        self.nsplit_override = None
        self.syrk_oversubscribe = None  # None: by kernel (see choose_nsplit)
        self._b_tag = None  # identifies the contents of the cached whitened buffer B
        self._side = SideStream(self.device)  # owner of the side stream (start_fill, the models' epilogue operands)
        self.last_batched = False  # the last pass over separate kernels ran as batched launches
        self.last_trmm_batch = 1  # latents per whitening launch of that pass
        self.profile = None  # set to a dict to record (start, stop) HIP events per kernel launch on the launch stream
        self.profile_only = None  # a set of kernel names: bracket only these launches
        self.constant_weight_sites = True  # ``run`` takes ``g1_const`` (the models ask before they pass it)
        self.site_sum_calls = {"general": 0, "constant_weight": 0}  # launches of ``_site_sums`` by form
        self._g1c = None  # (value, P, device tensor) of the last constant-weight launch
        # A/B switch: round 4's diagonal-block kernel instead of round 5's (TSVGP_POTRF_DIAG_V1)
        self.potrf_flags = B.POTRF_DIAG_V1 if os.environ.get("TSVGP_POTRF_DIAG_V1") == "1" else 0

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _fn(self, name, dtype=None):
        return getattr(self.lib, f"{name}_{B.suffix(dtype) if dtype is not None else self.sfx}")

    def _get(self, key, shape, dtype):
        t = self._buf.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._buf[key] = t
        return t

    def _launch(self, name, status_fn):
        """Runs one C-ABI launch; with profiling on, brackets it with events on the stream it is launched on (events
        come from a pool: creating two per launch costs the host ~0.1 ms per step, which shows at small shards)."""
        if self.profile is None or (self.profile_only is not None and name not in self.profile_only):
            B.check(status_fn(), name)
            return
        e0, e1 = self._event(), self._event()
        e0.record(torch.cuda.current_stream(self.device))
        B.check(status_fn(), name)
        e1.record(torch.cuda.current_stream(self.device))
        self.profile.setdefault(name, []).append((e0, e1))

    def _event(self):
        pool = self.__dict__.setdefault("_event_pool", [])
        return pool.pop() if pool else torch.cuda.Event(enable_timing=True)

    def reserve_events(self, n: int):
        """Pre-creates n timing events (bench.py: before the timed region)."""
        pool = self.__dict__.setdefault("_event_pool", [])
        while len(pool) < n:
            pool.append(torch.cuda.Event(enable_timing=True))

    def profile_summary(self):
        """{kernel: (launches, mean ms, min ms, median ms, max ms, [ms in launch order])} from the recorded events (synchronises); the events go
        back to the pool."""
        torch.cuda.synchronize(self.device)
        out = {}
        pool = self.__dict__.setdefault("_event_pool", [])
        for name, evs in (self.profile or {}).items():
            series = [a.elapsed_time(b) for a, b in evs]  # in launch order
            ms = sorted(series)
            n = len(ms)
            med = 0.0 if n == 0 else (ms[n // 2] if n % 2 else 0.5 * (ms[n // 2 - 1] + ms[n // 2]))
            out[name] = (n, sum(ms) / max(n, 1), ms[0] if n else 0.0, med, ms[-1] if n else 0.0, series)
            for a, b in evs:
                pool += [a, b]
        if self.profile is not None:
            self.profile.clear()
        return out

    def release(self):
        """Drop the cached work buffers."""
        self._buf.clear()
        self._b_tag = None

    @contextlib.contextmanager
    def private_buffers(self):
        """A fresh set of work buffers (and no warm tag) for the body -- a capture, whose graph owns what it allocates: yields
        the dict for the caller to keep alive and puts the engine's own pair back on exit, also on error."""
        saved = self._buf, self._b_tag
        self._buf, self._b_tag = {}, None
        try:
            yield self._buf
        finally:
            self._buf, self._b_tag = saved

    def fork(self, reads=(), writes=(), **payload):
        """``SideStream.fork`` on this engine's side stream: the body runs there, the yielded ``SideBranch`` keeps ``reads`` and
        ``writes`` alive until its ``join()``."""
        return self._side.fork(reads, writes, **payload)

    @property
    def side_open(self) -> bool:
        """Whether a fork has created the side stream yet."""
        return self._side.stream is not None

    def slots(self) -> int:
        if self._slots is None:
            with torch.cuda.device(self.device):
                s = int(self._fn("tsvgp_site_accum_slots")())
            if s <= 0:
                raise B.HipExtensionError("tsvgp_site_accum_slots failed")
            self._slots = s
        return self._slots

    def choose_nsplit(self, Mp: int, P: int, Np: int = None) -> int:
        """Number of N-slices per off-diagonal tile of the weighted Gram (diagonal tiles cost less per row and get
        correspondingly fewer, longer slices: the rule of syrk_ns_diag in the kernel source, mirrored in ``ns_diag`` below).
        All workgroups of the launch take the same time by construction, so the launch runs in ROUNDS of `slots` workgroups
        (one per CU for fp64, two for fp32) and costs  rounds * (chunks per slice + o):  o ~ 14 chunk-times per workgroup for
        its first fetch, the 128 x 128 partial tile it writes and the reduction's read of it (fitted at M = 512: 58 / 116 /
        232 / 464 / 651 slices take 4.20 / 4.27 / 4.43 / 4.64 / 4.85 ms, gpurun_out/r3m/kbench_m512.txt).  The slice count is
        the one that minimises this: whole rounds, and few of them.  At N = 1e6 (gpurun_out/r3m/nsplit_rounds.txt):
        M = 1024 fp64: 62 slices (2048 workgroups = 8 rounds exactly) 15.19 ms, 124: 15.32, 224 (28.9 rounds): 15.62,
        56 (7.2 rounds): 17.0; M = 1024 fp32: 61 slices 7.65 ms, 120: 7.99; M = 512 fp64: 120 slices 4.15 ms, 651: 4.72.
        A launch of exactly one round is charged 2 % more (nothing evens out the diagonal against the off-diagonal tiles:
        M = 512, 29 slices = one round 4.33 ms against 4.20 for two)."""
        return site_sum_slices(Mp, P, Np, self.slots(), self.dtype == torch.float64, self.syrk_oversubscribe)

    def _padded_gamma(self, gamma: torch.Tensor, Mp: int, P: int) -> torch.Tensor:
        """gamma [M, P] fp64 -> [Mp, P] in the compute dtype, rows >= M zero: a cached buffer whose padding is zeroed once (it was a
        fill and a copy per pass in front of the moments kernel)."""
        M = gamma.shape[0]
        if M == Mp and gamma.dtype == self.dtype and gamma.is_contiguous():
            return gamma
        out = self._buf.get("pad_gamma")
        if out is None or tuple(out.shape) != (Mp, P) or out.dtype != self.dtype:
            out = self._buf["pad_gamma"] = torch.zeros((Mp, P), dtype=self.dtype, device=self.device)
        out[:M].copy_(gamma)
        return out

    def _pad_square(self, A: torch.Tensor, Mp: int, key: str = None) -> torch.Tensor:
        """[.., M, M] fp64 -> zero-padded contiguous [.., Mp, Mp] in the compute dtype (a cached buffer per key)."""
        M = A.shape[-1]
        if M == Mp and A.dtype == self.dtype and A.is_contiguous():
            return A
        shape = tuple(A.shape[:-2]) + (Mp, Mp)
        out = self._buf.get(key) if key else None
        if out is None or tuple(out.shape) != shape:
            out = torch.zeros(shape, dtype=self.dtype, device=self.device)
            if key:
                self._buf[key] = out
        out[..., :M, :M] = A
        return out

    # ------------------------------------------------------------------ kernels
    def se_fill(self, X: torch.Tensor, Z: torch.Tensor, inv_ls: torch.Tensor, variance: float, out: torch.Tensor,
                kind: int = B.KERNEL_SE):
        """out[Np x Mp] <- K(X, Z) (padding zero) for the stationary kernel ``kind``.  X, Z, inv_ls, out share one dtype."""
        N, D = X.shape
        M = Z.shape[0]
        if D > MAX_INPUT_DIM:
            # beyond the fused kernel's compile-time sizes the scaled distance is a GEMM (GPflow's own square_distance
            # form): x~ z~^T from the BLAS library into the padded buffer, then tsvgp_gram_to_kernel_* in place
            Xs, Zs = X * inv_ls, torch.zeros((out.shape[1], D), dtype=X.dtype, device=X.device)
            Zs[:M] = Z * inv_ls
            torch.mm(Xs, Zs.t(), out=out[:N])
            xx, zz = (Xs * Xs).sum(dim=1).contiguous(), (Zs[:M] * Zs[:M]).sum(dim=1).contiguous()
            fn = self._fn("tsvgp_gram_to_kernel", X.dtype)
            with torch.cuda.device(self.device):
                self._launch("tsvgp_se_fill", lambda: fn(kind, out.data_ptr(), xx.data_ptr(), zz.data_ptr(), float(variance),
                                                         N, M, out.shape[1], self._stream()))
            return out
        fn = self._fn("tsvgp_kernel_fill", X.dtype)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_se_fill" if N != M or X.data_ptr() != Z.data_ptr() else "tsvgp_se_fill(Kuu)",
                         lambda: fn(kind, X.data_ptr(), Z.data_ptr(), inv_ls.data_ptr(), float(variance), out.data_ptr(),
                                    N, M, D, out.shape[1], self._stream()))
        return out

    def sum_fill(self, X: torch.Tensor, Z: torch.Tensor, kernel: Sum, out: torch.Tensor):
        """out[Np x Mp] <- sum_c K_c(X, Z) (padding zero) for a ``Sum`` kernel: one launch of ``tsvgp_kernel_fill_sum_*``."""
        N, D = X.shape
        M = Z.shape[0]
        if D > MAX_INPUT_DIM:
            raise NotImplementedError(f"a Sum kernel takes at most {MAX_INPUT_DIM} input columns (the fused fill's compile-time "
                                      f"sizes; the GEMM form is per component), got D = {D}")
        C = len(kernel.kernels)
        inv_ls = kernel.inv_lengthscales(D, X.dtype, self.device)  # [C, D]
        kinds = (ctypes.c_int * C)(*kernel.kinds)
        var = ((ctypes.c_double if X.dtype == torch.float64 else ctypes.c_float) * C)(*kernel.variances())
        fn = self._fn("tsvgp_kernel_fill_sum", X.dtype)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_se_fill" if N != M or X.data_ptr() != Z.data_ptr() else "tsvgp_se_fill(Kuu)",
                         lambda: fn(kinds, X.data_ptr(), Z.data_ptr(), inv_ls.data_ptr(), var, out.data_ptr(), N, M, D,
                                    out.stride(0), C, self._stream()))
        return out

    def prod_fill(self, X: torch.Tensor, Z: torch.Tensor, kernel: Product, out: torch.Tensor):
        """out[Np x Mp] <- prod_c K_c(X, Z) (padding zero) for a ``Product`` kernel: one launch of ``tsvgp_kernel_fill_prod_*``."""
        N, D = X.shape
        M = Z.shape[0]
        if D > MAX_INPUT_DIM:
            raise NotImplementedError(f"a Product kernel takes at most {MAX_INPUT_DIM} input columns (the fused fill's compile-time "
                                      f"sizes; the GEMM form is per component), got D = {D}")
        C = len(kernel.kernels)
        inv_ls = kernel.inv_lengthscales(D, X.dtype, self.device)  # [C, D]
        kinds = (ctypes.c_int * C)(*kernel.kinds)
        var = kernel.prior_variance()
        fn = self._fn("tsvgp_kernel_fill_prod", X.dtype)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_se_fill" if N != M or X.data_ptr() != Z.data_ptr() else "tsvgp_se_fill(Kuu)",
                         lambda: fn(kinds, X.data_ptr(), Z.data_ptr(), inv_ls.data_ptr(), var, out.data_ptr(), N, M, D,
                                    out.stride(0), C, self._stream()))
        return out

    def fill(self, X: torch.Tensor, Z: torch.Tensor, kernel, out: torch.Tensor):
        """out[Np x Mp] <- K(X, Z) (padding zero) of ONE latent GP's kernel: a stationary kernel through ``se_fill``, a ``Sum``
        through ``sum_fill``, a ``Product`` through ``prod_fill``.  X, Z and out share one dtype."""
        if isinstance(kernel, Product):
            return self.prod_fill(X, Z, kernel, out)
        if isinstance(kernel, Sum):
            return self.sum_fill(X, Z, kernel, out)
        return self.se_fill(X, Z, kernel.inv_lengthscales(X.shape[1], X.dtype, self.device), kernel.variance.item(), out, kernel.kind)

    @staticmethod
    def kdiag(kernel) -> float:
        """The prior variance k(x, x) of ONE latent GP's kernel as a Python float: ``variance``, its sum over a ``Sum``, its
        product over a ``Product``."""
        return kernel.prior_variance() if isinstance(kernel, COMBINED) else kernel.variance.item()

    def kuu(self, Z: torch.Tensor, kernel) -> torch.Tensor:
        """K(Z, Z) in fp64, [M, M] (no jitter); [P, M, M] for separate per-latent kernels."""
        if isinstance(kernel, SeparateIndependent):
            return torch.stack([self.kuu(Z, k) for k in kernel.kernels])
        Z = Z.to(device=self.device, dtype=torch.float64).contiguous()
        M, D = Z.shape
        Mp = B.round_up(M)
        out = torch.empty((Mp, Mp), dtype=torch.float64, device=self.device)
        self.fill(Z, Z, kernel, out)
        return out[:M, :M].contiguous()

    def tri_copy(self, src: torch.Tensor, M: int, scale: float = 1.0, flip: int = 0, out: torch.Tensor = None,
                 diag_add: float = 0.0) -> torch.Tensor:
        """[nb, M, M] contiguous <- triangle / index reversal of the leading M x M block of src [nb, R, C]
        (``tsvgp_tri_copy_shift_f64``: flip 0 = lower triangle, 1 = reversed indices, upper triangle, 2 = reversed, everything,
        3 = as it is, everything); ``diag_add`` is added on the diagonal behind the scale.
        ``out``: a [nb, >= M, >= M] view (unit element stride) whose leading M x M blocks are written instead."""
        nb, R, C = src.shape
        if out is None:
            out = torch.empty((nb, M, M), dtype=torch.float64, device=self.device)
        assert src.stride(2) == 1 and out.stride(2) == 1 and out.shape[0] == nb
        with torch.cuda.device(self.device):
            B.check(self.lib.tsvgp_tri_copy_shift_f64(src.data_ptr(), src.stride(1), src.stride(0), out.data_ptr(), out.stride(1),
                                                      out.stride(0), M, nb, float(scale), float(diag_add), int(flip), self._stream()),
                    "tsvgp_tri_copy")
        return out

    def cholesky_solve_upper(self, A: torch.Tensor, Lrhs, robust: bool = False, beside_fill: bool = False):
        """Upper-form factorisation AND the triangular solve behind it in one pass (``tsvgp_potrf_solve_f64``):
            A = U U^T (U upper triangular, as ``cholesky(upper_form=True)``),   D = U^-1 Lrhs^T   (upper triangular)
        for A [.., M, M] and a lower triangular Lrhs [.., M, M] -- reference src/util.py:168-175 with W = I + L^T K L for A and the
        site factor L for Lrhs; with the identity for Lrhs, D = U^-1 is the inverse factor (what K_uu + jitter I needs, reference
        src/models/tsvgp.py:270-271: the same batch, the same launches).  The index-reversed right-hand side J L J rides through
        the factorisation of J A J as extra panel rows and comes out as (J L J) C^-T = (C^-1 J L^T J)^T; one transposing pass turns
        that into D.  Replaces the inverse recursion (three levels of launch pairs), two triangle copies, a 1024^3 GEMM and a triu
        pass on the critical path of the replicated M x M chain.  ``Lrhs`` may be a LIST of [n_i, M, M] tensors, one run of the
        batch each.  Returns (U, info, D); no host synchronisation.
        ``beside_fill``: the N-sized K(X, Z) fill is in flight on the side stream and will outlast this call.  Round 5's panel
        kernel holds a strip and two column blocks of operands in 250 registers per lane and cannot share a CU with the fill's
        workgroups (224 registers per lane left), round 4's block step (78-87 registers per kernel) can: under the fill of
        N = 1e6 rows the call takes 1.69 ms with round 4's step and 2.13 ms with round 5's (profiles/r05_potrf_under_fill_ab.txt),
        alone 0.49 against 0.45."""
        # ``A`` may also be a LIST of (matrices [n_i, M, M], shift) runs of the batch: run i is factored as matrices_i + shift_i I.
        # The shift rides on the pass that writes J A J where the factorisation reads it, so W = I + L^T K L and K_uu + jitter I
        # need no assembled batch, no copy and no additions on the diagonal in front of this call (round 5).
        if isinstance(A, (list, tuple)):
            runs = [(a.reshape(-1, a.shape[-1], a.shape[-1]), float(sh)) for a, sh in A]
            M = runs[0][0].shape[-1]
            nb = sum(r.shape[0] for r, _ in runs)
            batch_shape = (nb,)
        else:
            M = A.shape[-1]
            batch_shape = A.shape[:-2]
            nb = 1
            for d in batch_shape:
                nb *= int(d)
            runs = [(A.reshape(nb, M, M), 0.0)]
        job = self.solve_upper_begin(nb, M)
        a0 = 0
        for A3, shift in runs:
            self.solve_upper_put(job, a0, A3, shift)
            a0 += A3.shape[0]
        parts, b0 = (list(Lrhs) if isinstance(Lrhs, (list, tuple)) else [Lrhs]), 0
        for part in parts:
            b0 += self.solve_upper_put_rhs(job, b0, part)
        assert b0 == nb, "one right-hand side per matrix of the batch"
        U, info, Dm = self.solve_upper_run(job, robust=robust, beside_fill=beside_fill)
        out_shape = tuple(batch_shape) + (M, M)
        return U.reshape(out_shape), info, Dm.reshape(out_shape)

    # The same call in pieces, for a caller whose operands become available at different times (t_SVGP._site_operands: K_uu +
    # jitter I and both right-hand sides exist before the two GEMMs that make W, and a shard's K(X, Z) fill starts right behind W:
    # handed over early, their passes run on an idle chip -- 7 us each -- instead of beside the fill -- 20-30 us each).
    def solve_upper_begin(self, nb: int, M: int) -> dict:
        """The tall operand [nb, 2 Mp, Mp] of ``tsvgp_potrf_solve_f64``: J A J on top, the right-hand-side rows below."""
        Mp = B.round_up(M)
        tall = (torch.empty if Mp == M else torch.zeros)((nb, 2 * Mp, Mp), dtype=torch.float64, device=self.device)
        if Mp != M:
            tall[:, :Mp].diagonal(dim1=-2, dim2=-1)[:, M:] = 1.0  # chol([[A, 0], [0, I]]) = [[C, 0], [0, I]]
        return dict(tall=tall, nb=nb, M=M, Mp=Mp)

    def solve_upper_put(self, job: dict, b0: int, A3: torch.Tensor, shift: float = 0.0) -> int:
        """Matrices b0 .. of the batch <- A3 [n, M, M] + shift I (index-reversed where the factorisation reads them)."""
        M, Mp = job["M"], job["Mp"]
        A3 = A3.to(device=self.device, dtype=torch.float64).reshape(-1, M, M)
        if A3.stride(2) != 1:
            A3 = A3.contiguous()
        self.tri_copy(A3, M, 1.0, 2, out=job["tall"][b0:b0 + A3.shape[0], :Mp], diag_add=shift)  # J (A + shift I) J
        return A3.shape[0]

    def solve_upper_put_rhs(self, job: dict, b0: int, L3: torch.Tensor) -> int:
        """Right-hand sides b0 .. <- the lower triangular L3 [n, M, M] (J tril(L) J: upper triangular, the rows the solve carries along)."""
        M, Mp = job["M"], job["Mp"]
        L3 = L3.to(device=self.device, dtype=torch.float64).reshape(-1, M, M)
        if L3.stride(2) != 1:
            L3 = L3.contiguous()
        self.tri_copy(L3, M, 1.0, 1, out=job["tall"][b0:b0 + L3.shape[0], Mp:])
        return L3.shape[0]

    def solve_upper_run(self, job: dict, robust: bool = False, beside_fill: bool = False):
        """Factor and solve what ``solve_upper_put`` / ``solve_upper_put_rhs`` handed over: (U [nb, M, M], info, D [nb, M, M])."""
        tall, nb, M, Mp = job["tall"], job["nb"], job["M"], job["Mp"]
        info = torch.empty(nb, dtype=torch.int32, device=self.device)
        work = self._get("potrf_work", (nb, 128 * 128), torch.float64)
        flags = (B.POTRF_SUBST if robust else 0) | B.POTRF_RHS_UPPER | self.potrf_flags | (B.POTRF_DIAG_V1 if beside_fill else 0)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_potrf", lambda: self.lib.tsvgp_potrf_solve_f64(
                tall.data_ptr(), Mp, Mp, nb, 2 * Mp * Mp, info.data_ptr(), work.data_ptr(), Mp, flags, self._stream()))
        U = self.tri_copy(tall[:, :Mp], M, 1.0, 1)
        Dm = torch.empty((nb, M, M), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            B.check(self.lib.tsvgp_flip_transpose_f64(tall[:, Mp:].data_ptr(), Mp, 2 * Mp * Mp, Dm.data_ptr(), M, M * M, M, nb,
                                                      self._stream()), "tsvgp_flip_transpose")
        return U, info, Dm

    def cholesky(self, A: torch.Tensor, inverse: bool = False, overwrite: bool = False, robust: bool = False,
                 scale: float = 1.0, upper_form: bool = False):
        """Batched lower Cholesky on the GPU through ``tsvgp_potrf_f64`` (no host synchronisation).
        A [.., M, M] fp64 (lower triangle referenced) -> (L [.., M, M] with zeros above the diagonal, info [batch] int32);
        with ``inverse`` also inv(L) (``tsvgp_potrf_inv_f64``), lower triangular with exact zeros above.
        ``overwrite``: A is a temporary of the caller and may be factored in place (no copy when M is a multiple of 128).
        ``robust``: solve the panels below each diagonal block by substitution (TSVGP_POTRF_SUBST) instead of multiplying
        with the INVERTED diagonal block, which costs a factor cond(L_kk) of accuracy in the trailing matrix -- irrelevant
        for the matrices of a well-conditioned K_uu (and ~0.15 ms faster), but a numerically barely definite matrix
        (cond ~ 1e14, lambda_min ~ 30 eps lambda_max) then fails where LAPACK-style factorisations go through.  The
        callers ask for it on the "projected" route, whose matrices are of that kind.
        ``scale``: the factor is returned times this (the leading minus of tsvgp.py:300 rides on the triangle copy).
        ``upper_form``: A = U U^T with U upper triangular -- the input is read with reversed indices, factored, and the
        factor (and inverse) written back reversed (``util.rev_cholesky`` without its four flip passes)."""
        A = A.to(device=self.device, dtype=torch.float64)
        flags = (B.POTRF_SUBST if robust else 0) | self.potrf_flags
        M = A.shape[-1]
        batch_shape = A.shape[:-2]
        Mp = B.round_up(M)
        nb = 1
        for d in batch_shape:
            nb *= int(d)
        if upper_form:
            W = self.tri_copy(A.reshape(nb, M, M), M, 1.0, 2)  # J A J (a fresh buffer of ours)
            if Mp != M:
                Wp = torch.zeros((nb, Mp, Mp), dtype=torch.float64, device=self.device)
                Wp[:, :M, :M] = W
                Wp.diagonal(dim1=-2, dim2=-1)[:, M:] = 1.0
                W = Wp
        elif Mp == M:  # no padding: one copy (or none) instead of a zero fill plus a copy
            W = A.reshape(nb, M, M)
            # (a contiguous view at an odd element offset of its storage is not on the 16-byte boundary the kernels need: copy it)
            if not (overwrite and W.is_contiguous() and W.data_ptr() == A.data_ptr() and W.data_ptr() % 16 == 0):
                W = W.clone(memory_format=torch.contiguous_format)
        else:
            W = torch.zeros((nb, Mp, Mp), dtype=torch.float64, device=self.device)
            W[:, :M, :M] = A.reshape(nb, M, M)
            W.diagonal(dim1=-2, dim2=-1)[:, M:] = 1.0  # chol([[A, 0], [0, I]]) = [[L, 0], [0, I]]  (a fill: capturable)
        info = torch.empty(nb, dtype=torch.int32, device=self.device)
        work = self._get("potrf_work", (nb, 128 * 128), torch.float64)
        out_shape = tuple(batch_shape) + (M, M)
        with torch.cuda.device(self.device):
            if inverse:
                X = torch.empty((2, nb, Mp, Mp), dtype=torch.float64, device=self.device)  # inv(L) and its transpose
                T = self._get("potrf_T", (nb, Mp, Mp), torch.float64)
                self._launch("tsvgp_potrf", lambda: self.lib.tsvgp_potrf_inv_f64(
                    W.data_ptr(), Mp, Mp, nb, Mp * Mp, info.data_ptr(), work.data_ptr(), X[0].data_ptr(), X[1].data_ptr(),
                    T.data_ptr(), flags, self._stream()))
            else:
                self._launch("tsvgp_potrf", lambda: self.lib.tsvgp_potrf_f64(
                    W.data_ptr(), Mp, Mp, nb, Mp * Mp, info.data_ptr(), work.data_ptr(), flags, self._stream()))
        L = self.tri_copy(W, M, scale, 1 if upper_form else 0).reshape(out_shape)
        if inverse:
            if upper_form:
                Xi = self.tri_copy(X[0], M, 1.0, 1).reshape(out_shape)
            else:
                Xi = X[0, :, :M, :M].reshape(out_shape)
            return L, info, Xi
        return L, info

    # ------------------------------------------------------------------ fused M x M helpers of the epilogue
    def site_target(self, G1, LLt, c_ll, c_g, jitter, rows, num_data):
        """(target, G1s) of ``tsvgp_site_target_f64``: G1s = (G1 + G1^T) / 2, target = c_ll LLt + c_g s G1s + jitter I with
        s = num_data / rows (rows: device scalar) or 1 when num_data is None.  [P, M, M] fp64."""
        G1, LLt = G1.contiguous(), LLt.contiguous()
        P, M = G1.shape[0], G1.shape[-1]
        target, G1s = torch.empty_like(G1), torch.empty_like(G1)
        with torch.cuda.device(self.device):
            B.check(self.lib.tsvgp_site_target_f64(G1.data_ptr(), LLt.data_ptr(), target.data_ptr(), G1s.data_ptr(), M, P,
                                                   float(c_ll), float(c_g), float(jitter),
                                                   rows.data_ptr() if num_data is not None else None,
                                                   float(num_data) if num_data is not None else 0.0, self._stream()),
                    "tsvgp_site_target")
        return target, G1s

    def site_update(self, G1, G0, LLt, meanZ, l1_old, lr, jitter, rows, num_data):
        """(target [P, M, M], lambda_1_new [M, P]) of ``tsvgp_site_update_f64``: the symmetrised G1 goes straight into the matrix of
        the final factorisation (1 - lr) LLt - 2 lr s sym(G1) + jitter I and into the chain rule G0 - 2 sym(G1) meanZ, whose
        convex combination with the old lambda_1 comes out of the same call."""
        G1, LLt = G1.contiguous(), LLt.contiguous()
        G0, meanZ, l1_old = G0.contiguous(), meanZ.contiguous(), l1_old.contiguous()
        P, M = G1.shape[0], G1.shape[-1]
        target, l1_new = torch.empty_like(G1), torch.empty_like(l1_old)
        work = self._get("site_update_work", (P * ((M + 31) // 32) * M,), torch.float64)
        with torch.cuda.device(self.device):
            B.check(self.lib.tsvgp_site_update_f64(G1.data_ptr(), G0.data_ptr(), LLt.data_ptr(), meanZ.data_ptr(), l1_old.data_ptr(),
                                                   target.data_ptr(), l1_new.data_ptr(), work.data_ptr(), M, P, float(lr),
                                                   float(jitter), rows.data_ptr() if num_data is not None else None,
                                                   float(num_data) if num_data is not None else 0.0, self._stream()),
                    "tsvgp_site_update")
        return target, l1_new

    def site_beta(self, Dm, v, l1):
        """beta [M, P] = l1 - D^T (D v) per latent (``tsvgp_site_beta_f64``): D [P, M, M] upper triangular, v = K6 l1 and l1 [M, P]."""
        Dm, v, l1 = Dm.contiguous(), v.contiguous(), l1.contiguous()
        P, M = Dm.shape[0], Dm.shape[-1]
        beta = torch.empty_like(l1)
        work = self._get("site_beta_work", (P * M * (1 + (M + 63) // 64),), torch.float64)
        with torch.cuda.device(self.device):
            B.check(self.lib.tsvgp_site_beta_f64(Dm.data_ptr(), v.data_ptr(), l1.data_ptr(), work.data_ptr(), beta.data_ptr(), M, P,
                                                 self._stream()), "tsvgp_site_beta")
        return beta

    def gemv(self, A: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """A v per latent (``tsvgp_gemv_f64``): A [M, M] (one matrix for every latent) or [P, M, M] row-major, v [M, P] -> [M, P]."""
        A, v = A.contiguous(), v.contiguous()
        M, P = v.shape
        y = torch.empty_like(v)
        with torch.cuda.device(self.device):
            B.check(self.lib.tsvgp_gemv_f64(A.data_ptr(), 0 if A.dim() == 2 else M * M, v.data_ptr(), y.data_ptr(), M, P, self._stream()),
                    "tsvgp_gemv")
        return y

    def step_status(self, infos_a, infos_b, nonpos):
        """[3] fp64 device tensor (sum |info| of the prelude factorisations, nonpos, sum |info| of the final one)."""
        cat = lambda ts: None if len(ts) == 0 else (ts[0] if len(ts) == 1 else torch.cat(list(ts))).contiguous()
        a, b = cat(infos_a), cat(infos_b)
        nonpos = nonpos.reshape(1).to(torch.float64)
        flags = torch.empty(3, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            B.check(self.lib.tsvgp_step_status_f64(_ptr(a), 0 if a is None else a.numel(), _ptr(b), 0 if b is None else b.numel(),
                                                   nonpos.data_ptr(), flags.data_ptr(), self._stream()), "tsvgp_step_status")
        return flags

    def sym_pack(self, acc2: torch.Tensor, out: torch.Tensor):
        """Lower triangles of acc2 [P, M, M] (any row / matrix stride) -> out [P * M (M + 1) / 2] (``tsvgp_sym_pack_f64``)."""
        P, M = acc2.shape[0], acc2.shape[-1]
        assert acc2.stride(2) == 1
        with torch.cuda.device(self.device):
            B.check(self.lib.tsvgp_sym_pack_f64(acc2.data_ptr(), acc2.stride(1), acc2.stride(0), M, P, out.data_ptr(),
                                                self._stream()), "tsvgp_sym_pack")
        return out

    def sym_unpack(self, packed: torch.Tensor, P: int, M: int) -> torch.Tensor:
        out = torch.empty((P, M, M), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            B.check(self.lib.tsvgp_sym_unpack_f64(packed.data_ptr(), out.data_ptr(), M, M * M, M, P, self._stream()),
                    "tsvgp_sym_unpack")
        return out

    def trmm(self, A: torch.Tensor, Tm: torch.Tensor, C: torch.Tensor, mode: int):
        Np, Mp = A.shape
        with torch.cuda.device(self.device):
            self._launch("tsvgp_trmm", lambda: self._fn("tsvgp_trmm")(A.data_ptr(), Tm.data_ptr(), C.data_ptr(), Np, Mp,
                                                                      mode, self._stream()))
        return C

    def lik_map(self, mean, var, Y, lik_id, lik_param, N, Np, *, g0=None, g1=None, ve_partial=None,
                nonpos_partial=None) -> LikMapResult:
        """The likelihood map as a launch of its own, for every likelihood id: (mean, var) [N, P] and Y ([N, 1] under a coupled
        likelihood, [N, P] otherwise), contiguous and of one dtype (fp64 or fp32: it picks the kernel), -> g0, g1 [Np, P] (rows
        >= N zero) and the per-128-row partials of ve and of the rows with var <= 0.  ``lik_id`` may carry LIK_NOCROP.
          LIK_GAUSSIAN, LIK_BERNOULLI   ``tsvgp_lik_map_*``            ``lik_param``: the likelihood's scalar
          LIK_HETERO                    ``tsvgp_lik_map_hetero_*``     P = 2
          LIK_SOFTMAX                   ``tsvgp_lik_map_softmax_*``    P = C; ``lik_param`` is the Softmax object: its sample count, row
                                        offset and device generator state, whose draw this call advances in-stream
          LIK_MULTICLASS                ``tsvgp_lik_map_robustmax_*``  P = C; ``lik_param`` is the MultiClass object: its epsilon
          LIK_STUDENT_T, LIK_POISSON    ``tsvgp_lik_map_scalar_*``     ``lik_param`` = (param0, param1); one launch per column, each with
                                        its own run of the partials [P, Np / 128]; StudentT: ``dparam`` = sum d ve / d scale
          LIK_GAMMA                     ``tsvgp_lik_map_scalar_*``     ``lik_param`` = (shape, 0) (Exponential: (1, 0, False), no ``dparam``);
                                        ``dparam`` = sum d ve / d shape
          LIK_ORDINAL                   ``tsvgp_lik_map_ordinal_*``    ``lik_param`` is the Ordinal object: its fp64 edges on this device
                                        and sigma; launches and partials as the scalar maps'; ``dparam`` = sum d ve / d sigma
        Outputs the caller does not hand in are cached buffers of their own ("coupled_g0/g1", "ve_partial" / "nonpos_partial",
        "scalar_*"): the site sums read them where they are, and a one-latent pass of the same call (``site_grads``) does not
        overwrite them."""
        T = mean.dtype
        lik = lik_id & 0xFF
        P = mean.shape[1]
        nblk = Np // B.TILE
        scalar = lik in B.COLUMN_MAP_LIKS  # one launch per latent column
        g0 = self._get("coupled_g0", (Np, P), T) if g0 is None else g0
        g1 = self._get("coupled_g1", (Np, P), T) if g1 is None else g1
        key, shape = ("scalar_", (P, nblk)) if scalar else ("", (nblk,))
        ve_partial = self._get(key + "ve_partial", shape, torch.float64) if ve_partial is None else ve_partial
        nonpos_partial = self._get(key + "nonpos_partial", shape, torch.int32) if nonpos_partial is None else nonpos_partial
        res = LikMapResult(g0, g1, ve_partial, nonpos_partial)
        ins = (mean.data_ptr(), var.data_ptr(), Y.data_ptr())
        outs = (g0.data_ptr(), g1.data_ptr(), ve_partial.data_ptr(), nonpos_partial.data_ptr())
        with torch.cuda.device(self.device):
            if lik in (B.LIK_GAUSSIAN, B.LIK_BERNOULLI):
                self._launch("tsvgp_lik_map", lambda: self._fn("tsvgp_lik_map", T)(
                    *ins, int(lik_id), float(lik_param), *outs, N, Np, P, self._stream()))
            elif lik == B.LIK_HETERO:
                self._launch("tsvgp_lik_map_hetero", lambda: self._fn("tsvgp_lik_map_hetero", T)(
                    *ins, int(lik_id), *outs, N, Np, self._stream()))
            elif lik == B.LIK_SOFTMAX:
                state = lik_param.rng_state(self.device)
                self._launch("tsvgp_lik_map_softmax", lambda: self._fn("tsvgp_lik_map_softmax", T)(
                    *ins, int(lik_id), P, int(lik_param.num_monte_carlo_points), state.data_ptr(), int(lik_param.row_offset), None,
                    *outs, N, Np, self._stream()))
                lik_param.advance()
            elif lik == B.LIK_MULTICLASS:  # deterministic: one launch, nothing to advance
                self._launch("tsvgp_lik_map_robustmax", lambda: self._fn("tsvgp_lik_map_robustmax", T)(
                    *ins, int(lik_id), P, float(lik_param.epsilon), *outs, N, Np, self._stream()))
            elif scalar:
                if tuple(Y.shape) != tuple(mean.shape) or tuple(var.shape) != tuple(mean.shape):
                    raise ValueError(f"mean, var and Y must share one shape [N, P], got {tuple(mean.shape)}, {tuple(var.shape)}, "
                                     f"{tuple(Y.shape)}")
                if not (mean.is_contiguous() and var.is_contiguous() and Y.is_contiguous()):
                    raise ValueError("the scalar likelihood map reads contiguous [N, P] arrays")
                # a likelihood with a trainable parameter: StudentT's scale, Gamma's shape, Ordinal's sigma (Exponential, the Gamma
                # arm at shape 1, has none and says so with a third entry: (1, 0, False))
                trainable = lik in (B.LIK_STUDENT_T, B.LIK_GAMMA, B.LIK_ORDINAL) and not (
                    lik == B.LIK_GAMMA and len(lik_param) > 2 and not lik_param[2])
                dpar = self._get("scalar_dparam_partial", (P, nblk), torch.float64) if trainable else None
                if lik == B.LIK_ORDINAL:  # ``lik_param`` is the Ordinal object: its edges on this device, its sigma
                    edges, sigma = lik_param.device_edges(self.device), float(lik_param.sigma.item())
                    fn = self._fn("tsvgp_lik_map_ordinal", T)
                    name, args = "tsvgp_lik_map_ordinal", (int(lik_id), edges.data_ptr(), int(edges.numel()), sigma)
                else:
                    p0, p1 = float(lik_param[0]), float(lik_param[1])
                    fn = self._fn("tsvgp_lik_map_scalar", T)
                    name, args = "tsvgp_lik_map_scalar", (int(lik_id), p0, p1)
                for p in range(P):
                    off = p * mean.element_size()
                    self._launch(name, lambda: fn(
                        ins[0] + off, ins[1] + off, ins[2] + off, P, *args, outs[0] + off, outs[1] + off, P,
                        ve_partial[p].data_ptr(), _ptr(None if dpar is None else dpar[p]), nonpos_partial[p].data_ptr(), N, Np,
                        self._stream()))
                res.dparam = None if dpar is None else dpar.sum()
            else:
                raise ValueError(f"lik_map: no likelihood map for lik_id {lik_id}")
        return res

    def lmc_mix(self, mean_g, var_g, W, N, Np, *, Fmu=None, Fvar=None, count=True):
        """``tsvgp_lmc_mix_*``: latent moments (mean_g, var_g) [N, L], contiguous and of one dtype (it picks the kernel), and W
        [P, L] fp64 on the device -> (Fmu, Fvar [N, P], nonpos_partial [Np / 128] int32 or None without ``count``).  Outputs the
        caller does not hand in are cached buffers ("lmc_fmu", "lmc_fvar", "lmc_nonpos_partial")."""
        T, L, P = mean_g.dtype, mean_g.shape[1], W.shape[0]
        if tuple(mean_g.shape) != (N, L) or tuple(var_g.shape) != (N, L) or tuple(W.shape) != (P, L) or W.dtype != torch.float64:
            raise ValueError(f"lmc_mix: mean_g, var_g [N, L] and W [P, L] fp64, got {tuple(mean_g.shape)}, {tuple(var_g.shape)}, "
                             f"{tuple(W.shape)} {W.dtype}")
        if not (mean_g.is_contiguous() and var_g.is_contiguous() and W.is_contiguous()) or var_g.dtype != T:
            raise ValueError("lmc_mix reads contiguous arrays of one dtype")
        Fmu = self._get("lmc_fmu", (N, P), T) if Fmu is None else Fmu
        Fvar = self._get("lmc_fvar", (N, P), T) if Fvar is None else Fvar
        bad = self._get("lmc_nonpos_partial", (Np // B.TILE,), torch.int32) if count else None
        with torch.cuda.device(self.device):
            self._launch("tsvgp_lmc_mix", lambda: self._fn("tsvgp_lmc_mix", T)(
                mean_g.data_ptr(), var_g.data_ptr(), W.data_ptr(), Fmu.data_ptr(), Fvar.data_ptr(), _ptr(bad), N, Np, L, P,
                self._stream()))
        return Fmu, Fvar, bad

    def lmc_unmix(self, g0_f, g1_f, W, N, Np, *, nocrop=False, mean_g=None, var_g=None, g0_g=None, g1_g=None):
        """``tsvgp_lmc_unmix_*``: the map's gradients (g0_f, g1_f) [Np, P] and W [P, L] -> (g0_g, g1_g [Np, L] with zero padding
        rows, g1_g cropped at -1e-8 unless ``nocrop``; dW [P, L] fp64 or None).  With the latent moments (mean_g, var_g) [N, L]
        given, dW = sum_n d ve_n / d W: the per-block sums of the launch, added over the blocks here.  Outputs the caller does not
        hand in are the cached "coupled_g0" / "coupled_g1" the site sums of a mapped pass read."""
        T, P, L = g0_f.dtype, W.shape[0], W.shape[1]
        if tuple(g0_f.shape) != (Np, P) or tuple(g1_f.shape) != (Np, P) or W.dtype != torch.float64 or g1_f.dtype != T:
            raise ValueError(f"lmc_unmix: g0_f, g1_f [Np, P] = [{Np}, {P}] of one dtype and W fp64, got {tuple(g0_f.shape)}, "
                             f"{tuple(g1_f.shape)}")
        want_dW = mean_g is not None
        if want_dW and (var_g is None or tuple(mean_g.shape) != (N, L) or tuple(var_g.shape) != (N, L) or mean_g.dtype != T
                        or var_g.dtype != T or not (mean_g.is_contiguous() and var_g.is_contiguous())):
            raise ValueError(f"lmc_unmix: dW needs mean_g and var_g [N, L] = [{N}, {L}], contiguous, in the gradients' dtype")
        if not (g0_f.is_contiguous() and g1_f.is_contiguous() and W.is_contiguous()):
            raise ValueError("lmc_unmix reads contiguous arrays")
        g0_g = self._get("coupled_g0", (Np, L), T) if g0_g is None else g0_g
        g1_g = self._get("coupled_g1", (Np, L), T) if g1_g is None else g1_g
        part = self._get("lmc_dW_partial", (Np // B.TILE, P, L), torch.float64) if want_dW else None
        with torch.cuda.device(self.device):
            self._launch("tsvgp_lmc_unmix", lambda: self._fn("tsvgp_lmc_unmix", T)(
                g0_f.data_ptr(), g1_f.data_ptr(), W.data_ptr(), B.LIK_NOCROP if nocrop else 0, g0_g.data_ptr(), g1_g.data_ptr(),
                _ptr(mean_g if want_dW else None), _ptr(var_g if want_dW else None), _ptr(part), N, Np, L, P, self._stream()))
        return g0_g, g1_g, (part.sum(dim=0) if want_dW else None)

    def _mixed_map(self, mean_g, var_g, Y, W, lik_id, lik_param, N, Np) -> LikMapResult:
        """The map of a pass under ``LinearCoregionalization``: ``lmc_mix`` of the L latents' moments, ``lik_map`` of a
        one-latent-per-column likelihood on the P mixed outputs (never cropped: the crop of tsvgp.py:262-263 is the latents'),
        ``lmc_unmix`` back.  The result's g0, g1 [Np, L] are what the site sums read; its nonpos_partial counts the rows the map
        rejected and those with a bad latent moment (a row may be in both: the sum is only compared with zero).  A pass with
        LIK_NOCROP -- the M-step's -- also returns dW."""
        lik = lik_id & 0xFF
        if lik in B.COUPLED_LIKS:
            raise ValueError("LinearCoregionalization takes a likelihood with one latent per output column, not a coupled one")
        nocrop = bool(lik_id & B.LIK_NOCROP)
        P, T = W.shape[0], mean_g.dtype
        Fmu, Fvar, bad = self.lmc_mix(mean_g, var_g, W, N, Np)
        f = self.lik_map(Fmu, Fvar, Y, lik | B.LIK_NOCROP, lik_param, N, Np, g0=self._get("lmc_g0f", (Np, P), T),
                         g1=self._get("lmc_g1f", (Np, P), T))
        g0, g1, dW = self.lmc_unmix(f.g0, f.g1, W, N, Np, nocrop=nocrop, mean_g=mean_g if nocrop else None,
                                    var_g=var_g if nocrop else None)
        return LikMapResult(g0, g1, f.ve_partial, torch.cat([f.nonpos_partial.reshape(-1), bad]), dparam=f.dparam, fmu=Fmu,
                            fvar=Fvar, g0_f=f.g0, g1_f=f.g1, dW=dW)

    def _mixed_stats(self, stats, lm, N, want_moments, want_grads):
        """The mixed outputs' entries of ``EStepStats`` from what ``_mixed_map`` left in cached buffers: fp64 copies."""
        if lm is None or lm.fmu is None:
            return
        stats.dW = lm.dW
        if want_moments:
            stats.fmu, stats.fvar = lm.fmu.to(torch.float64, copy=True), lm.fvar.to(torch.float64, copy=True)
        if want_grads:
            stats.g0_f, stats.g1_f = lm.g0_f[:N].to(torch.float64, copy=True), lm.g1_f[:N].to(torch.float64, copy=True)

    @staticmethod
    def _fused_param(lik_id, lik_param) -> float:
        """The parameter of a likelihood fused into the moments kernel.  A pass with no likelihood (predictions) ignores
        ``lik_param``: models hand over their likelihood's whatever the pass, and a mapped likelihood's is no float."""
        return 0.0 if (lik_id & 0xFF) == B.LIK_NONE else float(lik_param)

    def moments(self, A, Tm, gam, kdiag, N, moment_mode, *, lik_id=B.LIK_NONE, lik_param=0.0, mean_only=False, Y=None, mean=None,
                var=None, g0=None, g1=None):
        """The fused moments launch, the only one: A [Np, Mp], one operand and one prior variance ``kdiag`` for all P latents
        (``tsvgp_moments_*``), or A [P, Np, Mp] with a sequence of P prior variances (``tsvgp_moments_batched_*``).  Tm [P, Mp, Mp]
        and gam [Mp, P] are the padded operands; Y [N, P], mean, var [N, P] and g0, g1 [Np, P] are read / written where given
        (None: that array is not touched).  ``lik_id`` (flag bits included) selects the epilogue's likelihood with its own
        ``lik_param``; ``mean_only`` adds TSVGP_LIK_MEANONLY.  Returns the cached (ve_partial [Np / 128] fp64, nonpos_partial
        int32) the launch wrote."""
        Np, Mp = A.shape[-2:]
        P = gam.shape[1]
        ve_partial = self._get("ve_partial", (Np // B.TILE,), torch.float64)
        nonpos_partial = self._get("nonpos_partial", (Np // B.TILE,), torch.int32)
        if A.dim() == 3:
            fn, operand, kdiag = self._fn("tsvgp_moments_batched"), (A.data_ptr(), Np * Mp), (ctypes.c_double * P)(*kdiag)
        else:
            fn, operand = self._fn("tsvgp_moments"), (A.data_ptr(),)
        flags = (lik_id | B.LIK_MEANONLY) if mean_only else lik_id
        with torch.cuda.device(self.device):
            self._launch("tsvgp_moments", lambda: fn(
                *operand, Tm.data_ptr(), gam.data_ptr(), _ptr(Y), kdiag, flags, self._fused_param(lik_id, lik_param), _ptr(mean),
                _ptr(var), _ptr(g0), _ptr(g1), ve_partial.data_ptr(), nonpos_partial.data_ptr(), N, Np, Mp, P, moment_mode,
                self._stream()))
        return ve_partial, nonpos_partial

    def _moments_then_map(self, A, Tm, gam, kdiag, Y, lik_id, lik_param, N, Np, moment_mode, mean_only=False, mix=None):
        """The pass of a likelihood whose map runs behind the moments (``B.MAPPED_LIKS``): the moments of every latent with no
        likelihood into the cached "coupled_mean" / "coupled_var" [N, P] (they stay on this stream), then ``lik_map`` on them --
        or, with ``mix`` (W [outputs, P] of a ``LinearCoregionalization``), ``_mixed_map``.
        Returns (mean, var, LikMapResult)."""
        if mean_only:
            raise ValueError("mean_only needs a likelihood whose gradients do not depend on the predictive variance")
        P = gam.shape[1]
        mean, var = self._get("coupled_mean", (N, P), self.dtype), self._get("coupled_var", (N, P), self.dtype)
        self.moments(A, Tm, gam, kdiag, N, moment_mode, mean=mean, var=var)
        if mix is not None:
            return mean, var, self._mixed_map(mean, var, Y, mix, lik_id, lik_param, N, Np)
        return mean, var, self.lik_map(mean, var, Y, lik_id, lik_param, N, Np)

    @staticmethod
    def _check_y(Y, N, P, lik_id, lik_param=None, outputs=None):
        """Y [N, P]; a coupled likelihood (LIK_HETERO: two latents, LIK_SOFTMAX, LIK_MULTICLASS: C) maps its latents onto ONE target column:
        Y [N, 1], P = latent_dim.  ``outputs`` (the rows of W under ``LinearCoregionalization``): Y [N, outputs], no coupled likelihood."""
        lik = lik_id & 0xFF
        if outputs is not None:
            if lik in B.COUPLED_LIKS:
                raise ValueError("LinearCoregionalization takes a likelihood with one latent per output column, not a coupled one")
            if Y is None or Y.dim() != 2 or Y.shape[0] != N or Y.shape[1] != outputs:
                raise ValueError(f"Y must be [N, P] = [{N}, {outputs}] (P: the rows of W), got {None if Y is None else tuple(Y.shape)}")
            return
        if lik in B.COUPLED_LIKS:
            name = {B.LIK_HETERO: "heteroskedastic", B.LIK_SOFTMAX: "Softmax", B.LIK_MULTICLASS: "MultiClass"}[lik]
            C = 2 if lik == B.LIK_HETERO else getattr(lik_param, "latent_dim", None)  # (hetero passes lik_param = 0.0)
            if P != C or Y is None or Y.dim() != 2 or Y.shape[0] != N or Y.shape[1] != 1:
                own = "" if lik == B.LIK_HETERO else " (its latent_dim)"
                raise ValueError(f"the {name} likelihood needs {C} latent GPs{own} and Y [N, 1] = [{N}, 1], got "
                                 f"P = {P} and Y {None if Y is None else tuple(Y.shape)}")
        elif Y.dim() != 2 or Y.shape[0] != N or Y.shape[1] != P:
            raise ValueError(f"Y must be [N, P] = [{N}, {P}], got {tuple(Y.shape)}")

    def kernel_grad(self, X, Z, kernel, U, g0, g1, beta):
        """N-sized part of d ELBO / d (variance, lengthscales, Z) for ONE latent GP (``tsvgp_kernel_grad_*``):
        sum_{n,m} V[n,m] dK[n,m]/d theta with V = g0 beta^T - 2 g1 * U.  X [N, D], Z [M, D], U [Np, Mp] (compute dtype);
        g0, g1: columns of the [Np, P] gradient buffers (any element stride), beta [M] fp64.
        Returns (d_variance scalar, d_lengthscales [D], d_Z [M, D]) in fp64."""
        T, dev = self.dtype, self.device
        X = X.to(device=dev, dtype=T).contiguous()
        Z = Z.to(device=dev, dtype=T).contiguous()
        N, D = X.shape
        M = Z.shape[0]
        if D > MAX_INPUT_DIM_GRAD:
            return self._kernel_grad_gemm(X, Z, kernel, U, g0, g1, beta)
        Mp = B.round_up(M)
        inv_ls = kernel.inv_lengthscales(D, T, dev)
        rows, Dp = int(self.lib.tsvgp_kernel_grad_rows()), int(self.lib.tsvgp_kernel_grad_dpad(D))
        nrb, ncb = (N + rows - 1) // rows, (Mp + 511) // 512
        zpart = torch.empty((nrb, Mp, Dp), dtype=torch.float64, device=dev)
        lpart = torch.empty((nrb, ncb, Dp), dtype=torch.float64, device=dev)
        vpart = torch.empty((nrb, ncb), dtype=torch.float64, device=dev)
        bt = beta.to(device=dev, dtype=T).contiguous()
        assert g0.dim() == 1 and g1.dim() == 1 and g0.stride(0) == g1.stride(0)
        with torch.cuda.device(dev):
            self._launch("tsvgp_kernel_grad", lambda: self._fn("tsvgp_kernel_grad")(
                kernel.kind, X.data_ptr(), Z.data_ptr(), inv_ls.data_ptr(), kernel.variance.item(), U.data_ptr(), U.shape[1],
                g0.data_ptr(), g1.data_ptr(), g0.stride(0), bt.data_ptr(), 1, N, M, D, zpart.data_ptr(), lpart.data_ptr(),
                vpart.data_ptr(), self._stream()))
        return vpart.sum(), lpart.sum(dim=(0, 1))[:D], zpart.sum(dim=0)[:M, :D]

    def kernel_grad_prod(self, X, Z, kernel, U, g0, g1, beta):
        """``kernel_grad`` for a ``Product`` kernel: all C parameter sets in ONE ``tsvgp_kernel_grad_prod_*`` launch on U.
        Returns (d_variance [C], d_lengthscales [C, D], d_Z [M, D]) in fp64; d / d variance_c = (prod variance / variance_c) * the
        launch's sum of V prod_c f_c."""
        T, dev = self.dtype, self.device
        X = X.to(device=dev, dtype=T).contiguous()
        Z = Z.to(device=dev, dtype=T).contiguous()
        N, D = X.shape
        M = Z.shape[0]
        if D > MAX_INPUT_DIM_GRAD:
            raise NotImplementedError(f"the M-step gradient of a Product kernel takes at most {MAX_INPUT_DIM_GRAD} input columns "
                                      f"(tsvgp_kernel_grad_prod_*'s compile-time sizes; the GEMM form is per kernel), got D = {D}")
        C = len(kernel.kernels)
        Mp = B.round_up(M)
        inv_ls = kernel.inv_lengthscales(D, T, dev)  # [C, D]
        kinds = (ctypes.c_int * C)(*kernel.kinds)
        variances = kernel.variances()
        var = kernel.prior_variance()
        rows, Dp = int(self.lib.tsvgp_kernel_grad_rows()), int(self.lib.tsvgp_kernel_grad_dpad(D))
        nrb, ncb = (N + rows - 1) // rows, (Mp + 511) // 512
        zpart = torch.empty((nrb, Mp, Dp), dtype=torch.float64, device=dev)
        lpart = torch.empty((nrb, ncb, C, Dp), dtype=torch.float64, device=dev)
        vpart = torch.empty((nrb, ncb), dtype=torch.float64, device=dev)
        bt = beta.to(device=dev, dtype=T).contiguous()
        assert g0.dim() == 1 and g1.dim() == 1 and g0.stride(0) == g1.stride(0)
        with torch.cuda.device(dev):
            self._launch("tsvgp_kernel_grad", lambda: self._fn("tsvgp_kernel_grad_prod")(
                kinds, X.data_ptr(), Z.data_ptr(), inv_ls.data_ptr(), var, U.data_ptr(), U.shape[1], g0.data_ptr(), g1.data_ptr(),
                g0.stride(0), bt.data_ptr(), 1, N, M, D, C, zpart.data_ptr(), lpart.data_ptr(), vpart.data_ptr(), self._stream()))
        # variance / variance_c without a division: the product of the others, in index order
        others = []
        for c in range(C):
            o = 1.0
            for c2, v in enumerate(variances):
                if c2 != c:
                    o *= v
            others.append(o)
        dvar = vpart.sum() * torch.tensor(others, dtype=torch.float64, device=dev)
        return dvar, lpart.sum(dim=(0, 1))[:, :D], zpart.sum(dim=0)[:M, :D]

    def _kernel_grad_gemm(self, X, Z, kernel, U, g0, g1, beta):
        """``kernel_grad`` for D beyond the fused kernel's sizes, in the GEMM form of the large-D fill (reference
        docs/notebooks/mnist.py:117-192, D = 784): G = x~ z~^T from the BLAS library, ``tsvgp_gram_to_gradw_*`` turns it into
        W = -2 variance V * k'(r2) in place and sums V k(r2); what is left is one [Mp, N] x [N, D] GEMM and the row / column
        sums of W.  X, Z already in the compute dtype on the device."""
        T, dev = self.dtype, self.device
        N, D = X.shape
        M = Z.shape[0]
        Np, Mp = B.round_up(N), B.round_up(M)
        inv_ls = kernel.inv_lengthscales(D, T, dev)
        Xs = X * inv_ls
        Zs = torch.zeros((Mp, D), dtype=T, device=dev)
        Zs[:M] = Z * inv_ls
        W = self._get("gradW", (Np, Mp), T)
        torch.mm(Xs, Zs.t(), out=W[:N])
        xx = (Xs * Xs).sum(dim=1).contiguous()
        zz = (Zs[:M] * Zs[:M]).sum(dim=1).contiguous()
        vpart = torch.empty(int(self.lib.tsvgp_gram_to_gradw_parts(N, M)), dtype=torch.float64, device=dev)
        bt = beta.to(device=dev, dtype=T).contiguous()
        assert g0.dim() == 1 and g1.dim() == 1 and g0.stride(0) == g1.stride(0)
        with torch.cuda.device(dev):
            self._launch("tsvgp_kernel_grad", lambda: self._fn("tsvgp_gram_to_gradw")(
                kernel.kind, W.data_ptr(), xx.data_ptr(), zz.data_ptr(), kernel.variance.item(), U.data_ptr(), U.shape[1],
                g0.data_ptr(), g1.data_ptr(), g0.stride(0), bt.data_ptr(), 1, N, M, Mp, vpart.data_ptr(), self._stream()))
        f64 = torch.float64
        colsum = W.sum(dim=0, dtype=f64)[:M]  # [M]
        rowsum = W[:N].sum(dim=1, dtype=f64)  # [N]
        WtX = torch.mm(W[:N, :M].t(), Xs).to(f64)  # [M, D]
        Zs64, Xs64, il = Zs[:M].to(f64), Xs.to(f64), inv_ls.to(f64)
        dZ = (WtX - Zs64 * colsum[:, None]) * il
        dl = (torch.einsum("nd,n->d", Xs64 * Xs64, rowsum) - 2.0 * (Zs64 * WtX).sum(dim=0)
              + torch.einsum("md,m->d", Zs64 * Zs64, colsum)) * il
        return vpart.sum(), dl, dZ

    def moments_vjp(self, X, Z, kernel, U, cm, cv, beta, dX, accumulate=False):
        """Input gradient of the marginal moments of ONE latent GP (``tsvgp_moments_vjp_*``), into dX [N, D] fp64 (contiguous):

            dX[n, d] (+)= sum_m (cm[n] beta[m] - 2 cv[n] U[n, m]) dK[n, m] / dX[n, d],     U = K(X, Z) Q

        X [N, D <= 32], Z [M, D]; U [>= N, ldu >= M] in the compute dtype with 16-byte aligned rows (the engine's [Np, Mp] buffers
        are); cm, cv: 1-D views of N elements in the compute dtype with one element stride (columns of an [N, P] array); beta [M].
        ``accumulate``: add to dX instead of writing it.  One launch on the current stream."""
        T, dev = self.dtype, self.device
        X = X.to(device=dev, dtype=T).contiguous()
        Z = Z.to(device=dev, dtype=T).contiguous()
        N, D = X.shape
        M = Z.shape[0]
        if D < 1 or D > MAX_INPUT_DIM:
            raise ValueError(f"moments_vjp: 1 <= D <= {MAX_INPUT_DIM} (the compile-time sizes of tsvgp_moments_vjp_*), got {D}")
        if Z.shape[1] != D or U.dim() != 2 or U.dtype != T or U.shape[0] < N or U.shape[1] < M or U.stride(1) != 1:
            raise ValueError(f"moments_vjp: Z must be [M, {D}] and U [>= {N}, >= {M}] in {T}, got {tuple(Z.shape)} and {tuple(U.shape)}")
        if not (cm.dim() == cv.dim() == 1 and cm.shape[0] == cv.shape[0] == N and cm.dtype == cv.dtype == T
                and (N == 1 or cm.stride(0) == cv.stride(0) >= 1)):
            raise ValueError(f"moments_vjp: cm and cv must be 1-D views of N = {N} elements in {T} with one stride")
        if tuple(dX.shape) != (N, D) or dX.dtype != torch.float64 or not dX.is_contiguous():
            raise ValueError(f"moments_vjp: dX must be a contiguous fp64 [{N}, {D}]")
        bt = beta.to(device=dev, dtype=T).contiguous()
        if tuple(bt.shape) != (M,):
            raise ValueError(f"moments_vjp: beta must be [M] = [{M}], got {tuple(bt.shape)}")
        inv_ls = kernel.inv_lengthscales(D, T, dev)
        cstride = max(int(cm.stride(0)), 1)
        with torch.cuda.device(dev):
            self._launch("tsvgp_moments_vjp", lambda: self._fn("tsvgp_moments_vjp")(
                int(kernel.kind), X.data_ptr(), Z.data_ptr(), inv_ls.data_ptr(), kernel.variance.item(), U.data_ptr(), U.stride(0),
                cm.data_ptr(), cv.data_ptr(), cstride, bt.data_ptr(), 1, N, M, D, dX.data_ptr(), 1 if accumulate else 0,
                self._stream()))
        return dX

    def predict_vjp(self, X, Z, kernel, beta, Q, cm, cv=None) -> torch.Tensor:
        """The vector-Jacobian product of the marginal prediction with respect to the rows of X, [N, D] fp64:

            mean[n, p] = k_n^T beta_p,   var[n, p] = k(x, x) - k_n^T Q_p k_n,   dX = sum_p (cm_p d mean_p + cv_p d var_p) / dX

        X [N, D <= 32], Z [M, D]; ``kernel``: one kernel shared by the latents, a ``SeparateIndependent`` or a list of one kernel
        per latent; beta [M, P] and Q [P, M, M] (symmetric) fp64; cm, cv [N, P] (``cv=None``: zeros, the mean alone).
        Per kernel one K(X, Z) fill, per latent U = K_fu Q_p by the BLAS library into the engine's "U" buffer (the dense branch of
        ``t_SVGP.elbo_and_grads``, in the compute dtype) and one ``moments_vjp``, latents in index order.  The N-sized memory is
        the engine's reusable "Kfu" and "U" buffers."""
        if isinstance(kernel, SeparateIndependent):
            kernels = list(kernel.kernels)
        elif isinstance(kernel, (list, tuple)):
            kernels = list(kernel)
        else:
            kernels = [kernel]
        for kern in kernels:  # before anything is moved or allocated
            refuse_product(kern, "predict_f_vjp")
        T, dev = self.dtype, self.device
        X = X.detach().to(device=dev, dtype=T).contiguous()
        Z = Z.detach().to(device=dev, dtype=T).contiguous()
        if X.dim() != 2 or Z.dim() != 2 or Z.shape[1] != X.shape[1] or X.shape[0] < 1:
            raise ValueError(f"predict_vjp: X must be [N >= 1, D] and Z [M, D] with equal D, got {tuple(X.shape)} and {tuple(Z.shape)}")
        N, D = X.shape
        M = Z.shape[0]
        if D > MAX_INPUT_DIM:
            raise ValueError(f"predict_vjp: the input dimension is limited to {MAX_INPUT_DIM} (the compile-time sizes of the K(X, Z) "
                             f"fill and of tsvgp_moments_vjp_*), got D = {D}")
        beta = beta.detach().to(device=dev, dtype=torch.float64)
        Q = Q.detach().to(device=dev, dtype=torch.float64)
        Q = Q[None] if Q.dim() == 2 else Q
        P = Q.shape[0]
        if tuple(beta.shape) != (M, P) or tuple(Q.shape) != (P, M, M):
            raise ValueError(f"predict_vjp: beta must be [M, P] and Q [P, M, M] with M = {M}, got {tuple(beta.shape)} and {tuple(Q.shape)}")
        # contiguous copies: autograd hands a backward expanded (stride 0) gradients after a plain .sum(), and the launch reads the
        # columns of both arrays with one element stride
        cm = cm.detach().to(device=dev, dtype=T).contiguous()
        if tuple(cm.shape) != (N, P) or (cv is not None and tuple(cv.shape) != (N, P)):
            raise ValueError(f"predict_vjp: the cotangents must be [N, P] = [{N}, {P}]")
        cv = torch.zeros_like(cm) if cv is None else cv.detach().to(device=dev, dtype=T).contiguous()
        if len(kernels) not in (1, P):
            raise ValueError(f"predict_vjp: one kernel or one per latent (P = {P}), got {len(kernels)}")
        if len(kernels) == P and all(k is kernels[0] for k in kernels):
            kernels = kernels[:1]  # the same object for every latent: one fill
        Np, Mp = B.round_up(N), B.round_up(M)
        self._b_tag = None  # "Kfu" is rewritten below
        self._side.wait_stale()
        Kfu = self._get("Kfu", (Np, Mp), T)
        Ubuf = self._get("U", (Np, Mp), T)
        dX = torch.empty((N, D), dtype=torch.float64, device=dev)
        for p in range(P):
            kern = kernels[p if len(kernels) > 1 else 0]
            if p == 0 or len(kernels) > 1:
                self.fill(X, Z, kern, Kfu)
            torch.mm(Kfu, self._pad_square(0.5 * (Q[p] + Q[p].T), Mp, "pad_Q"), out=Ubuf)
            # (a Sum: dK is the sum of its components' dK_c on the same U -- one launch each, accumulating behind the first)
            for c, comp in enumerate(kern.kernels if isinstance(kern, Sum) else [kern]):
                self.moments_vjp(X, Z, comp, Ubuf, cm[:, p], cv[:, p], beta[:, p], dX, accumulate=p > 0 or c > 0)
        return dX

    def selftest_mfma(self, dtype=None):
        """Runs one MFMA and returns (a, b, c) for a host-side check of the fragment maps."""
        dtype = dtype or self.dtype
        g = torch.Generator(device="cpu").manual_seed(7)
        a = torch.randn(16, 4, generator=g, dtype=torch.float64).to(dtype).to(self.device)
        b = torch.randn(4, 16, generator=g, dtype=torch.float64).to(dtype).to(self.device)
        c = torch.zeros(16, 16, dtype=dtype, device=self.device)
        with torch.cuda.device(self.device):
            B.check(self._fn("tsvgp_selftest_mfma", dtype)(a.data_ptr(), b.data_ptr(), c.data_ptr(), self._stream()),
                    "tsvgp_selftest_mfma")
        return a, b, c

    # ------------------------------------------------------------------ one kernel per latent, batched over the latents
    batch_separate = True  # False: always one pass per latent through a single K(X, Z) buffer (the round-1 path)
    batch_mem_fraction = 0.8  # of the device memory still free: what the [P, Np, Mp] operand of a batched pass may take

    _per_latent = staticmethod(per_latent)

    def _batch_plan(self, N, M, kernel, P, whiten_T, whiten_mode, project_T, moments_on_kfu, D=0):
        """Can the pass over P separately-parameterised latents run as batched launches (tsvgp_*_batched_*)?  Needs one
        kernel family, at most MAX_BATCH latents, no "projected" latent (its second product is not in place), the
        whitening in upper form (in place) and room for the [P, Np, Mp] operand.  Returns the list of whitened latents
        or None for the per-latent path."""
        if not self.batch_separate or P < 2 or P > B.MAX_BATCH or moments_on_kfu:
            return None
        if len({k.kind for k in kernel.kernels}) != 1:
            return None
        if D > MAX_INPUT_DIM:  # the GEMM-based fill of large input dimensions is per latent
            return None
        if any(self._per_latent(project_T, p) is not None for p in range(P)):
            return None
        whitened = [p for p in range(P) if self._per_latent(whiten_T, p) is not None]
        if whitened and whiten_mode != B.TRI_UPPER:
            return None
        Np, Mp = B.round_up(N), B.round_up(M)
        need = P * Np * Mp * torch.empty((), dtype=self.dtype).element_size()
        have = self._buf.get("KfuP")
        if have is None or tuple(have.shape) != (P, Np, Mp) or have.dtype != self.dtype:
            free, _ = torch.cuda.mem_get_info(self.device)
            free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
            if have is not None:
                free += have.numel() * have.element_size()
            if need > self.batch_mem_fraction * free:
                return None
        return whitened

    def _fill_batched(self, X, Z, kernel, KfuP):
        """K(X, Z) of every latent's kernel into KfuP [P, Np, Mp] with one launch per MAX_BATCH latents."""
        T, dev = self.dtype, self.device
        N, D = X.shape
        M = Z.shape[0]
        if D > MAX_INPUT_DIM:
            raise ValueError(f"input dimension D = {D} exceeds the HIP fill kernel's limit of {MAX_INPUT_DIM}")
        P = len(kernel.kernels)
        inv_ls = torch.stack([k.inv_lengthscales(D, T, dev) for k in kernel.kernels]).contiguous()  # [P, D]
        ctype = ctypes.c_double if T == torch.float64 else ctypes.c_float
        fn = self._fn("tsvgp_kernel_fill_batched", T)
        stride = KfuP.shape[1] * KfuP.shape[2]
        with torch.cuda.device(dev):
            for p0 in range(0, P, B.MAX_BATCH):
                n = min(B.MAX_BATCH, P - p0)
                var = (ctype * n)(*[k.variance.item() for k in kernel.kernels[p0:p0 + n]])
                self._launch("tsvgp_se_fill", lambda: fn(kernel.kernels[0].kind, X.data_ptr(), Z.data_ptr(),
                                                         inv_ls[p0].data_ptr(), var, KfuP[p0].data_ptr(), stride, N, M, D,
                                                         KfuP.shape[2], n, self._stream()))
        return KfuP

    def _run_batched(self, X, Y, Z, kernel, whitened, *, moment_Tm, moment_mode, gamma, lik_id, lik_param, whiten_T,
                     sites, want_moments, want_grads, mean_only, prefill=None, mix=None, g1_const=None) -> EStepStats:
        """One pass for P latents with one kernel each as batched launches: fill [P, Np, Mp] -> in-place whitening of the
        latents that ask for it -> moments -> site sums (4 launches; BASELINE configs[4])."""
        T, dev = self.dtype, self.device
        X = X.to(device=dev, dtype=T).contiguous()
        Z = Z.to(device=dev, dtype=T).contiguous()
        N, M, P = X.shape[0], Z.shape[0], moment_Tm.shape[0]
        Np, Mp = B.round_up(N), B.round_up(M)
        need_g = lik_id != B.LIK_NONE
        # the map runs behind the moments: coupled latents, a scalar map, or any likelihood on mixed outputs
        mapped = (lik_id & 0xFF) in B.MAPPED_LIKS or (need_g and mix is not None)
        if need_g:
            Y = Y.to(device=dev, dtype=T).contiguous()
        self._b_tag = None
        self._buf.pop("Kfu", None)  # the single-latent operand buffers are not needed beside the batched one
        self._buf.pop("B", None)
        KfuP = self._get("KfuP", (P, Np, Mp), T)
        stride = Np * Mp
        if prefill is not None:
            prefill.take("KfuP", KfuP)
        else:
            self._side.wait_stale()
            self._fill_batched(X, Z, kernel, KfuP)
        # whitening in place, one launch per run of consecutive whitened latents: B_p = K_p U9_p^-T (upper form)
        runs, start = [], None
        for p in range(P + 1):
            on = p < P and p in whitened
            if on and start is None:
                start = p
            if not on and start is not None:
                runs.append((start, p))
                start = None
        fn_trmm = self._fn("tsvgp_trmm_batched")
        self.last_trmm_batch = max([hi - lo for lo, hi in runs], default=1)
        for lo, hi in runs:
            Wt = torch.stack([self._per_latent(whiten_T, p) for p in range(lo, hi)])
            Wp = self._pad_square(Wt, Mp, f"pad_LinvP{hi - lo}")
            with torch.cuda.device(dev):
                self._launch("tsvgp_trmm", lambda: fn_trmm(KfuP[lo].data_ptr(), stride, Wp.data_ptr(), Mp * Mp,
                                                           KfuP[lo].data_ptr(), stride, Np, Mp, B.TRI_UPPER, hi - lo,
                                                           self._stream()))
        Tm = self._pad_square(moment_Tm, Mp, "pad_Tm")
        gam = self._padded_gamma(gamma, Mp, P)
        kdiag = [k.variance.item() for k in kernel.kernels]
        lm = None
        if mapped:
            mean, var, lm = self._moments_then_map(KfuP, Tm, gam, kdiag, Y, lik_id, lik_param, N, Np, moment_mode, mean_only, mix)
            g0, g1, ve_partial, nonpos_partial = lm.g0, lm.g1, lm.ve_partial, lm.nonpos_partial  # what the common tail reads
        else:
            g0 = self._get("g0", (Np, P), T) if need_g else None
            g1 = self._get("g1", (Np, P), T) if need_g else None
            mean = torch.empty((N, P), dtype=T, device=dev) if want_moments else None
            var = torch.empty((N, P), dtype=T, device=dev) if (want_moments and not mean_only) else None
            ve_partial, nonpos_partial = self.moments(KfuP, Tm, gam, kdiag, N, moment_mode, lik_id=lik_id, lik_param=lik_param,
                                                      mean_only=mean_only, Y=Y if need_g else None, mean=mean, var=var, g0=g0, g1=g1)
        stats = EStepStats(n_rows=N, ve_sum=ve_partial.sum(), nonpos=nonpos_partial.sum().to(torch.float64),
                           dparam=None if lm is None else lm.dparam)
        if want_moments:  # (the mapped path's mean / var are cached buffers: copies)
            stats.mean = mean.to(torch.float64, copy=mapped)
            stats.var = None if var is None else var.to(torch.float64, copy=mapped)
        if want_grads and need_g:
            stats.g0, stats.g1 = g0[:N].to(torch.float64), g1[:N].to(torch.float64)
        self._mixed_stats(stats, lm, N, want_moments, want_grads)
        if sites:
            stats.acc2, stats.acc1 = self._site_sums(KfuP, g0, g1, P, M, g1_const=None if mapped else g1_const)
        self.last_batched = True
        return stats

    def _run_separate(self, X, Y, Z, kernel, *, moment_Tm, gamma, whiten_T, project_T, want_grads, prefill=None,
                      **kw) -> EStepStats:
        """Separate per-latent kernels (K_uu [P, M, M]).  Batched launches over the latents when ``_batch_plan`` allows
        (one [P, Np, Mp] operand: 8.2 GB per latent at N = 1e6, M = 1024, fp64 -- 66 GB of the 288 GB at P = 8);
        otherwise one fill + moments + accumulation pass per latent through the single-latent kernels and ONE K(X, Z)
        buffer."""
        P = moment_Tm.shape[0]
        if len(kernel.kernels) != P:
            raise ValueError(f"{len(kernel.kernels)} kernels for {P} latent GPs")
        lik_id = kw.get("lik_id", B.LIK_NONE)
        # P outputs mixed from these latents (LinearCoregionalization): W [outputs, P] on the device when there is a likelihood
        # to apply to the mixed moments; a pass without one returns the latents' moments as under SeparateIndependent
        mix = kernel.device_W(self.device) if (isinstance(kernel, LinearCoregionalization) and lik_id != B.LIK_NONE) else None
        if mix is not None:
            kw["mean_only"] = False  # the mixed map takes (Fmu, Fvar) whatever the likelihood reads of them
        # the map runs behind the moments: coupled latents, a scalar map, or any likelihood on mixed outputs
        mapped = (lik_id & 0xFF) in B.MAPPED_LIKS or mix is not None
        g1_const = kw.pop("g1_const", None)
        if not mapped:  # (behind a map the gradients are per row: the general form)
            kw["g1_const"] = g1_const
        if mapped or Y is not None:
            self._check_y(Y, X.shape[0], P, lik_id, kw.get("lik_param"), outputs=None if mix is None else mix.shape[0])
        if X.shape[0] > 0:
            if prefill is not None and prefill.name == "KfuP":  # the batched fill is already under way (start_fill)
                whitened = [p for p in range(P) if self._per_latent(whiten_T, p) is not None]
            else:
                whitened = self._batch_plan(X.shape[0], Z.shape[0], kernel, P, whiten_T,
                                            kw.get("whiten_mode", B.TRI_UPPER), project_T, kw.get("moments_on_kfu", False),
                                            D=X.shape[1])
            if whitened is not None:
                return self._run_batched(X, Y, Z, kernel, whitened, moment_Tm=moment_Tm, moment_mode=kw["moment_mode"],
                                         gamma=gamma, lik_id=kw.get("lik_id", B.LIK_NONE), lik_param=kw.get("lik_param", 0.0),
                                         whiten_T=whiten_T, sites=kw.get("sites", False),
                                         want_moments=kw.get("want_moments", False), want_grads=want_grads,
                                         mean_only=kw.get("mean_only", False), prefill=prefill, mix=mix,
                                         g1_const=kw.get("g1_const"))
        self.last_batched = False
        if mapped and X.shape[0] > 0:  # (an empty shard contributes zeros through the loop below)
            return self._run_separate_coupled(X, Y, Z, kernel, moment_Tm=moment_Tm, gamma=gamma, whiten_T=whiten_T,
                                              project_T=project_T, want_grads=want_grads, mix=mix, **kw)
        parts = []
        for p, kp in enumerate(kernel.kernels):
            # (per-latent routes: None = this latent works on K_fu directly)
            st = self.run(X, None if (Y is None or mix is not None) else Y[:, p:p + 1], Z, kp, moment_Tm=moment_Tm[p:p + 1], gamma=gamma[:, p:p + 1],
                          whiten_T=per_latent(whiten_T, p), project_T=per_latent(project_T, p), want_grads=want_grads, **kw)
            if want_grads and st.g0 is not None:
                st.g0, st.g1 = st.g0.clone(), st.g1.clone()  # views of a buffer the next latent overwrites
            parts.append(st)

        def cat(name, dim):
            vals = [getattr(s, name) for s in parts]
            return None if vals[0] is None else torch.cat(vals, dim=dim)

        out = EStepStats(n_rows=parts[0].n_rows, ve_sum=sum(s.ve_sum for s in parts), nonpos=sum(s.nonpos for s in parts))
        out.mean, out.var, out.g0, out.g1 = cat("mean", 1), cat("var", 1), cat("g0", 1), cat("g1", 1)
        out.acc2, out.acc1 = cat("acc2", 0), cat("acc1", 0)
        return out

    def _run_separate_coupled(self, X, Y, Z, kernel, *, moment_Tm, gamma, whiten_T, project_T, want_grads, lik_id, sites=False,
                              want_moments=False, mean_only=False, mix=None, **kw) -> EStepStats:
        """The one-pass-per-latent path under a likelihood whose map runs behind the moments (``B.MAPPED_LIKS``): a coupled map
        needs the moments of ALL latents before any site sum, and this path has one K(X, Z) buffer.  Sweep 1: fill (and whitening)
        + moments with no likelihood, per latent; the map over [N, P] (``lik_map``); sweep 2 (``sites`` only): fill (and whitening / projection)
        again + the site sums of each latent with its column of the map (``run(site_grads=...)``).  The refill costs one
        K(X, Z) fill (plus the whitening product where the route has one) per latent -- the alternative, keeping both operands,
        is the batched path's [P, Np, Mp] buffer, and this path runs exactly when that does not fit or is not wanted."""
        if mean_only:
            raise ValueError("mean_only needs a likelihood whose gradients do not depend on the predictive variance")
        T, dev = self.dtype, self.device
        N, P = X.shape[0], moment_Tm.shape[0]
        Np = B.round_up(N)
        lik_param = kw.pop("lik_param", None)
        per = self._per_latent
        mean = self._get("coupled_mean", (N, P), T)
        var = self._get("coupled_var", (N, P), T)
        for p, kp in enumerate(kernel.kernels):
            st = self.run(X, None, Z, kp, moment_Tm=moment_Tm[p:p + 1], gamma=gamma[:, p:p + 1], whiten_T=per(whiten_T, p),
                          want_moments=True, **kw)
            mean[:, p] = st.mean[:, 0]
            var[:, p] = st.var[:, 0]
        Yc = Y.to(device=dev, dtype=T).contiguous()
        if mix is not None:  # P outputs mixed from the latents: mix, map, un-mix
            lm = self._mixed_map(mean, var, Yc, mix, lik_id, lik_param, N, Np)
        else:
            lm = self.lik_map(mean, var, Yc, lik_id, lik_param, N, Np)
        g0, g1 = lm.g0, lm.g1
        out = EStepStats(n_rows=N, ve_sum=lm.ve_partial.sum(), nonpos=lm.nonpos_partial.sum().to(torch.float64), dparam=lm.dparam)
        if want_moments:
            out.mean, out.var = mean.to(torch.float64, copy=True), var.to(torch.float64, copy=True)
        if want_grads:
            out.g0, out.g1 = g0[:N].to(torch.float64, copy=True), g1[:N].to(torch.float64, copy=True)
        self._mixed_stats(out, lm, N, want_moments, want_grads)
        if sites:
            acc2, acc1 = [], []
            for p, kp in enumerate(kernel.kernels):
                st = self.run(X, None, Z, kp, moment_Tm=moment_Tm[p:p + 1], gamma=gamma[:, p:p + 1], whiten_T=per(whiten_T, p),
                              project_T=per(project_T, p), sites=True, site_grads=(g0[:, p:p + 1], g1[:, p:p + 1]), **kw)
                acc2.append(st.acc2)
                acc1.append(st.acc1)
            out.acc2, out.acc1 = torch.cat(acc2, dim=0), torch.cat(acc1, dim=0)
        return out

    # ------------------------------------------------------------------ K(X, Z) fill beside the M x M prelude
    def start_fill(self, X, Z, kernel, b_tag=None, want="Kfu", routes=None):
        """Starts the K(X, Z) fill of the next ``run`` on a side stream and returns a ticket for ``run(prefill=...)``.
        The fill needs only X, Z and the kernel parameters, so it can run beside the latency-bound M x M prelude
        (factorisations of one workgroup each, small GEMMs) that the main stream executes between this call and
        ``run``: 3.26 -> 2.6 ms for the pair at N = 1e6, M = 1024 (script removed, code in git history; result in docs/history_r01-r03.md).  Returns None when there is
        nothing to overlap: separate kernels on the per-latent path (one fill per latent), an operand ``run`` would reuse
        (warm E-steps), a stream capture in progress.  ``routes``: the projection route of every latent (separate kernels:
        the batched pass, whose fill this starts, needs all of them direct or whitened)."""
        if self.device.type != "cuda" or X.shape[0] == 0:
            return None
        # (fork / join, also inside a capture, and what keeps the converted inputs alive: side_branch.py)
        T, dev = self.dtype, self.device
        N, D = X.shape
        M = Z.shape[0]
        Np, Mp = B.round_up(N), B.round_up(M)
        separate = isinstance(kernel, SeparateIndependent)
        if separate:
            P = len(kernel.kernels)
            if routes is None or any(r == "projected" for r in routes):
                return None
            if self._batch_plan(N, M, kernel, P, None, B.TRI_UPPER, None, False, D=D) is None:
                return None
        elif (b_tag is not None and self._b_tag == (want, b_tag) and self._buf.get(want) is not None
                and tuple(self._buf[want].shape) == (Np, Mp)):
            return None
        Xc = X.to(device=dev, dtype=T).contiguous()
        Zc = Z.to(device=dev, dtype=T).contiguous()
        self._b_tag = None
        if separate:
            self._buf.pop("Kfu", None)
            self._buf.pop("B", None)
            buf = self._get("KfuP", (P, Np, Mp), T)
            with self.fork(reads=(Xc, Zc), writes=(buf,), name="KfuP", buf=buf) as branch:
                self._fill_batched(Xc, Zc, kernel, buf)
        else:
            inv_ls = kernel.inv_lengthscales(D, T, dev)
            buf = self._get("Kfu", (Np, Mp), T)
            with self.fork(reads=(Xc, Zc, inv_ls), writes=(buf,), name="Kfu", buf=buf,
                           key=(X.data_ptr(), tuple(X.shape), Z.data_ptr(), tuple(Z.shape), id(kernel))) as branch:
                self.fill(Xc, Zc, kernel, buf)
        return branch

    # ------------------------------------------------------------------ one N-pass
    def run(self, X, Y, Z, kernel, *, moment_Tm, moment_mode, gamma, lik_id=B.LIK_NONE, lik_param=0.0,
            whiten_T=None, whiten_mode=B.TRI_UPPER, project_T=None, sites=False, want_moments=False, want_grads=False,
            b_tag=None, mean_only=False, prefill=None, moments_on_kfu=False, project_mode=B.TRI_LOWER,
            keep_tile=False, site_grads=None, g1_const=None) -> EStepStats:
        """One pass over the shard's rows.

        g1_const (``estep.gaussian_g1_const``; LIK_GAUSSIAN only): the number g1 holds on every row, which lets the site sums run in
        their constant-weight form (``_site_sums``).  Ignored where the gradients come out of a map behind the moments (mixed
        outputs un-mix g1 per row).

        keep_tile (one latent, no whitening): the triangular product of the moments, t_n = Tm k_n, is STORED (``tsvgp_trmm``
        into the buffer "Tt", returned as ``stats.tile``) and the moments are assembled from it -- mean by a matrix-vector
        product, var = kdiag - |t_n|^2 by a row norm, the gradients by ``lik_map`` -- instead of being squared and summed
        inside the fused kernel.  For the M-step (t_SVGP.elbo_and_grads), which needs Q k_n = Tm^T t_n for every row: a second
        triangular product of the stored tile instead of a dense N M^2 GEMM with Q = Tm^T Tm.

        X [N, D], Y [N, P] (or None when lik_id == NONE), Z [M, D];
        whiten_T [M, M] fp64: the inverted triangular factor of Kuu + jitter I (B[n, i] = sum_j Kfu[n, j] whiten_T[i, j]
        over the triangle ``whiten_mode`` names), or None (moments then act on Kfu directly);
        project_T [M, M] fp64 (needs whiten_T): the "projected" route -- after the moments the site sums are taken over
        a = project_T-product of B (a[n, i] = sum_{j <= i} B[n, j] project_T[i, j], i.e. a = U9^-T b = K9^-1 k with
        project_T = U9^-T), written over the K(X, Z) buffer;
        moment_Tm [P, M, M] fp64 and gamma [M, P] fp64: operands of the fused moments kernel;
        sites=True also accumulates (acc2, acc1) = (sum g1 a a^T, sum g0 a) over the rows a of the same operand the
        moments used: the whitened B when whiten_T is given, Kfu itself otherwise (the "direct" projection).
        b_tag: a hashable description of (X, Z, kernel parameters, jitter).  When it equals the tag of the B buffer left
        by the previous call, the fill and the whitening are skipped and B is reused ("warm" E-step: consecutive
        E-steps with unchanged hyperparameters, as in the reference's E/M loop, experiments/uci_regression.py:152-153).
        moments_on_kfu (with whiten_T): the moments act on K(X, Z) itself (moment_Tm / gamma in k coordinates) and only the
        site sums use the whitened / projected operand, whose products then run AFTER the moments: the variant in
        which nothing on the moments side depends on the factor of K_uu + jitter I.  project_mode: triangle of project_T.
        prefill: the ticket of ``start_fill`` for the same (X, Z, kernel): the fill is already under way on the side
        stream; this call waits for it instead of filling.
        mean_only (likelihood NONE or GAUSSIAN): skip the variance product of the moments (TSVGP_LIK_MEANONLY) -- the
        Gaussian g0, g1 do not depend on it; ``var`` is then None and ``ve_sum`` NaN.
        lik_id in ``B.MAPPED_LIKS`` (coupled: P = latent_dim, Y [N, 1]; LIK_STUDENT_T / LIK_POISSON: Y [N, P]; ``lik_param`` as
        ``lik_map`` takes it): moments of all latents with no likelihood, then ``lik_map``, then the site sums;
        ``stats.dparam`` = sum d ve / d scale (StudentT).
        site_grads (lik_id NONE, one kernel): (g0, g1) [Np, P] in the compute dtype, rows >= N zero -- the site sums (and with
        ``keep_tile`` the stored product) of this pass with gradients a coupled map made elsewhere; the moments product then
        runs only for ``want_moments`` / ``keep_tile``, and ``ve_sum`` / ``nonpos`` are zero (the map's call counts them).
        """
        if isinstance(kernel, SeparateIndependent):
            return self._run_separate(X, Y, Z, kernel, moment_Tm=moment_Tm, moment_mode=moment_mode, gamma=gamma,
                                      lik_id=lik_id, lik_param=lik_param, whiten_T=whiten_T, whiten_mode=whiten_mode,
                                      project_T=project_T, sites=sites, want_moments=want_moments, want_grads=want_grads,
                                      mean_only=mean_only, moments_on_kfu=moments_on_kfu, project_mode=project_mode,
                                      prefill=prefill, g1_const=g1_const)
        if site_grads is not None and lik_id != B.LIK_NONE:
            raise ValueError("site_grads replaces the likelihood: lik_id must be LIK_NONE")
        if g1_const is not None and (lik_id & 0xFF) != B.LIK_GAUSSIAN:
            raise ValueError("g1_const: only a homoskedastic Gaussian likelihood has one g1 for every row")
        if mean_only and (lik_id & 0xFF) not in (B.LIK_NONE, B.LIK_GAUSSIAN):
            raise ValueError("mean_only needs a likelihood whose gradients do not depend on the predictive variance")
        T, dev = self.dtype, self.device
        X = X.to(device=dev, dtype=T).contiguous()
        Z = Z.to(device=dev, dtype=T).contiguous()
        N, D = X.shape
        M = Z.shape[0]
        P = moment_Tm.shape[0]
        if N == 0:
            # One rank of several may hold no rows (N < world size): it contributes zeros to the all-reduce instead of
            # raising alone while the other ranks wait in the collective.  A single process with no data is an error.
            if world_size() == 1:
                raise ValueError("empty data: natgrad_step / elbo need at least one row")
            zero = torch.zeros((), dtype=torch.float64, device=dev)
            st = EStepStats(n_rows=0, ve_sum=zero, nonpos=zero.clone())
            if sites:
                st.acc2 = torch.zeros((P, M, M), dtype=torch.float64, device=dev)
                st.acc1 = torch.zeros((P, M), dtype=torch.float64, device=dev)
            if want_moments:
                st.mean = torch.zeros((0, P), dtype=torch.float64, device=dev)
                st.var = None if mean_only else torch.zeros((0, P), dtype=torch.float64, device=dev)
            return st
        if X.dim() != 2 or Z.dim() != 2 or Z.shape[1] != D:
            raise ValueError(f"X must be [N, D] and Z [M, D] with equal D, got {tuple(X.shape)} and {tuple(Z.shape)}")
        mapped = (lik_id & 0xFF) in B.MAPPED_LIKS  # the map runs behind the moments: coupled latents or a scalar map
        if lik_id != B.LIK_NONE:
            self._check_y(Y, N, P, lik_id, lik_param)
            Y = Y.to(device=dev, dtype=T).contiguous()
        Np, Mp = B.round_up(N), B.round_up(M)
        variance = self.kdiag(kernel)

        # The N x M operand of the moments / site kernels: the whitened B = Kfu U^-T, or Kfu itself ("direct" route).
        # A tagged operand left by the previous call is reused when the tag matches (warm E-steps).
        want = "B" if whiten_T is not None else "Kfu"
        late_whiten = moments_on_kfu and whiten_T is not None
        if late_whiten:
            b_tag = None  # K(X, Z) and B are both consumed in this pass: nothing to carry over
        reuse = (b_tag is not None and self._b_tag == (want, b_tag) and self._buf.get(want) is not None
                 and tuple(self._buf[want].shape) == (Np, Mp))
        if reuse:
            A = self._buf[want]
        else:
            self._b_tag = None
            Kfu = self._get("Kfu", (Np, Mp), T)
            if prefill is not None:
                prefill.take("Kfu", Kfu)
            else:
                self._side.wait_stale()
                self.fill(X, Z, kernel, Kfu)
            A = Kfu
            if whiten_T is not None and not late_whiten:
                Bw = self._get("B", (Np, Mp), T)
                self.trmm(Kfu, self._pad_square(whiten_T, Mp, "pad_Linv"), Bw, whiten_mode)
                A = Bw
            if b_tag is not None:
                self._b_tag = (want, b_tag)

        Tm = self._pad_square(moment_Tm, Mp, "pad_Tm")
        gam = self._padded_gamma(gamma, Mp, P)
        need_g = lik_id != B.LIK_NONE or site_grads is not None
        g0 = self._get("g0", (Np, P), T) if need_g else None
        g1 = self._get("g1", (Np, P), T) if need_g else None
        mean = torch.empty((N, P), dtype=T, device=dev) if want_moments else None
        var = torch.empty((N, P), dtype=T, device=dev) if (want_moments and not mean_only) else None
        tile, lm = None, None
        if site_grads is not None:
            g0.copy_(site_grads[0])
            g1.copy_(site_grads[1])
        if keep_tile:
            if P != 1 or mean_only or whiten_T is not None or not need_g:
                raise ValueError("keep_tile: one latent, a likelihood, no whitening")
            if mapped:
                raise ValueError("keep_tile: a likelihood whose map runs behind the moments comes in through site_grads")
            tile = self._get("Tt", (Np, Mp), T)
            self.trmm(A, Tm[0], tile, moment_mode)
            mean = torch.mv(A[:N], gam[:, 0]).reshape(N, 1)  # gam: [Mp, 1], rows >= M zero
            var = (variance - torch.linalg.vector_norm(tile[:N], dim=1).square()).reshape(N, 1)
            if site_grads is None:  # (the map writes the partials the moments launch would: the same cached buffers)
                res = self.lik_map(mean, var, Y, lik_id, lik_param, N, Np, g0=g0, g1=g1)
                ve_partial, nonpos_partial = res.ve_partial, res.nonpos_partial
        elif mapped:
            mean, var, lm = self._moments_then_map(A, Tm, gam, variance, Y, lik_id, lik_param, N, Np, moment_mode, mean_only)
            g0, g1, ve_partial, nonpos_partial = lm.g0, lm.g1, lm.ve_partial, lm.nonpos_partial  # what the common tail reads
            if want_moments:
                mean, var = mean.clone(), var.clone()
        elif site_grads is not None and not want_moments:
            pass  # the site sums alone
        else:
            own = site_grads is None  # (with site_grads the launch writes mean / var only: g0, g1 hold the caller's)
            ve_partial, nonpos_partial = self.moments(A, Tm, gam, variance, N, moment_mode, lik_id=lik_id, lik_param=lik_param,
                                                      mean_only=mean_only, Y=Y if lik_id != B.LIK_NONE else None, mean=mean,
                                                      var=var, g0=g0 if own else None, g1=g1 if own else None)
        if site_grads is not None:
            zero = torch.zeros((), dtype=torch.float64, device=dev)
            stats = EStepStats(n_rows=N, ve_sum=zero, nonpos=zero.clone())
        else:
            stats = EStepStats(n_rows=N, ve_sum=ve_partial.sum(), nonpos=nonpos_partial.sum().to(torch.float64),
                               dparam=None if lm is None else lm.dparam)
        stats.tile = tile
        if want_moments:
            stats.mean, stats.var = mean.to(torch.float64), (None if var is None else var.to(torch.float64))
        if want_grads and need_g:
            stats.g0, stats.g1 = g0[:N].to(torch.float64), g1[:N].to(torch.float64)

        if late_whiten and sites:  # the site sums' operand, now that the moments have read K(X, Z)
            Bw = self._get("B", (Np, Mp), T)
            self.trmm(A, self._pad_square(whiten_T, Mp, "pad_Linv"), Bw, whiten_mode)
            A = Bw
        if sites and project_T is not None:
            if whiten_T is None:
                raise ValueError("project_T needs whiten_T")
            Aproj = self._get("Kfu", (Np, Mp), T)  # K(X, Z) itself is no longer needed once B exists
            self.trmm(A, self._pad_square(project_T, Mp, "pad_proj"), Aproj, project_mode)
            A = Aproj
        if sites:
            stats.acc2, stats.acc1 = self._site_sums(A, g0, g1, P, M, g1_const=None if mapped else g1_const)
        return stats

    def _site_sums(self, A, g0, g1, P, M, g1_const=None):
        """(sum_n g1 a a^T [P, M, M], sum_n g0 a [P, M]) over the rows of one operand A [Np, Mp] shared by the P latents
        (``tsvgp_site_accum_*``) or of one operand per latent, A [P, Np, Mp] (``tsvgp_site_accum_batched_*``); g0, g1 [Np, P] with
        zero padding rows.  The only launch of either.

        g1_const (a float, P <= 8): the constant-weight form (``tsvgp_site_accum_cw_*``) -- g1 is that number on every live row,
        so the kernels sum a a^T unweighted and the reduction scales the sums once; ``g1`` is not read.  Above eight latents the
        general form runs on ``g1`` whatever ``g1_const`` says.  ``site_sum_calls`` counts the launches of either form."""
        dev = self.device
        cw = g1_const is not None and P <= 8
        Np, Mp = A.shape[-2:]
        nsplit = self.nsplit_override or self.choose_nsplit(Mp, P, Np)
        nsplit = max(1, min(nsplit, Np // site_sum_chunk_rows(self.dtype == torch.float64, P)))
        nbytes = int(self._fn("tsvgp_site_accum_work_bytes")(Mp, P, nsplit))
        work = self._get("work", (nbytes,), torch.uint8)
        acc2 = torch.empty((P, Mp, Mp), dtype=torch.float64, device=dev)
        acc1 = torch.empty((P, Mp), dtype=torch.float64, device=dev)
        name = "tsvgp_site_accum_cw" if cw else "tsvgp_site_accum"
        if A.dim() == 3:
            fn, operand = self._fn(name + "_batched"), (A.data_ptr(), Np * Mp)
        else:
            fn, operand = self._fn(name), (A.data_ptr(),)
        if cw:  # the P scalars on the device, kept while the value stays (it moves with the likelihood's variance: an M-step)
            if self._g1c is None or self._g1c[:2] != (float(g1_const), P):
                self._g1c = (float(g1_const), P, torch.full((P,), float(g1_const), dtype=torch.float64, device=dev))
            weights = self._g1c[2]
        else:
            weights = g1
        self.site_sum_calls["constant_weight" if cw else "general"] += 1
        with torch.cuda.device(dev):
            self._launch("tsvgp_site_accum", lambda: fn(*operand, g0.data_ptr(), weights.data_ptr(), acc2.data_ptr(), acc1.data_ptr(),
                                                        work.data_ptr(), Np, Mp, P, nsplit, self._stream()))
        return acc2[:, :M, :M], acc1[:, :M]

    def run_two_product(self, X, Y, Z, kernel, *, whiten_T, moment_Tm, gamma, lik_id=B.LIK_NONE, lik_param=0.0, sites=False,
                        want_moments=False, prefill=None) -> EStepStats:
        """The pass of ``t_SVGP_white`` with the reference's OWN two-product variance (src/util.py:76-86):
            var = kff - |LA^-1 k|^2 + |LR^-1 k|^2 = kff - |b|^2 + |T2 b|^2,   b = U6^-1 k (whiten_T = U6^-1, upper form),
        T2 = U_R^-1 U6 (``moment_Tm``, upper triangular), mean = b^T gamma.  Used when Lambda_2 + 1e-9 I is not positive definite
        (the single triangular product of ``run`` needs its factor; the reference only needs K + Lambda_2 + 1e-9 I).  Sequence:
        fill -> trmm (B) -> moments with NO likelihood (mean, kff - |T2 b|^2) -> |b|^2 by a row reduction of B -> the
        likelihood map on the assembled moments (``lik_map``) -> site sums over B.  One shared kernel, one latent.
        ``prefill``: as ``run``."""
        T, dev = self.dtype, self.device
        st = self.run(X, None, Z, kernel, moment_Tm=moment_Tm, moment_mode=B.TRI_UPPER, gamma=gamma, lik_id=B.LIK_NONE,
                      whiten_T=whiten_T, whiten_mode=B.TRI_UPPER, want_moments=True, prefill=prefill)
        N, M = X.shape[0], Z.shape[0]
        Np, Mp = B.round_up(N), B.round_up(M)
        Bw = self._buf["B"]  # the whitened operand of the pass just run
        kff = self.kdiag(kernel)
        bn = torch.linalg.vector_norm(Bw[:N], dim=1).to(torch.float64)
        var = (2.0 * kff - bn * bn)[:, None] - st.var  # st.var = kff - |T2 b|^2
        stats = EStepStats(n_rows=N, ve_sum=torch.zeros((), dtype=torch.float64, device=dev), nonpos=(~(var > 0)).sum().to(torch.float64))
        if want_moments:
            stats.mean, stats.var = st.mean, var
        if lik_id != B.LIK_NONE:
            Yc = Y.to(device=dev, dtype=T).contiguous()
            self._check_y(Yc, N, 1, lik_id, lik_param)
            lm = self.lik_map(st.mean.to(T).contiguous(), var.to(T).contiguous(), Yc, lik_id, lik_param, N, Np,
                              g0=self._get("g0", (Np, 1), T), g1=self._get("g1", (Np, 1), T))
            stats.ve_sum, stats.nonpos, stats.dparam = lm.ve_partial.sum(), lm.nonpos_partial.sum().to(torch.float64), lm.dparam
            if sites:
                stats.acc2, stats.acc1 = self._site_sums(Bw, lm.g0, lm.g1, 1, M)
        return stats

    # ------------------------------------------------------------------ joint predictions
    def cov(self, tile: torch.Tensor, C: torch.Tensor, N: int, *, sign: float = -1.0, X=None, inv_ls=None, variance: float = 0.0,
            kind: int = B.KERNEL_SE, accumulate: bool = False):
        """C [Np, ldc] <- base + sign * tile tile^T (``tsvgp_cov_*``): base = variance * k(x_i, x_j) from X [N, D <= 32] and
        inv_ls [D], or what the lower triangle of C holds (``accumulate``).  tile [Np, Mp] and C in one of the two compute
        dtypes; rows and columns >= N of C become the identity block."""
        Np, Mp = tile.shape
        if C.dtype != tile.dtype or C.shape[0] != Np or C.stride(1) != 1 or tile.stride(1) != 1 or tile.stride(0) != Mp:
            raise ValueError("cov: tile [Np, Mp] contiguous and C [Np, >= Np] with unit column stride, in one dtype")
        D = 0 if accumulate else X.shape[1]
        fn = self._fn("tsvgp_cov", tile.dtype)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_cov", lambda: fn(int(kind), tile.data_ptr(), _ptr(None if accumulate else X),
                                                 _ptr(None if accumulate else inv_ls), float(variance), float(sign), C.data_ptr(),
                                                 int(N), Np, Mp, D, C.stride(0), B.COV_ACCUMULATE if accumulate else 0,
                                                 self._stream()))
        return C

    def full_cov(self, X, Z, kernel, *, moment_Tm, moment_mode, gamma, whiten_T=None, whiten_mode=B.TRI_UPPER,
                 two_product=False, padded=False):
        """Joint posterior of the latents over the rows of X [N, D] (GPflow conditional(full_cov=True) [ext]; reference
        src/models/tsvgp.py:103-112): (mean [N, P], cov [P, N, N], nonpos) in fp64, from the operands ``run`` takes.  Per latent
        p, with a_n the row of K(X, Z_p) (or its whitening product b_n = whiten_T a_n):

            mean[:, p] = a gamma[:, p],    cov_p = K_p(X, X) - t t^T,    t_n = moment_Tm[p] a_n   (``tsvgp_trmm`` into a tile)
            two_product (``run_two_product``'s variance):  cov = K(X, X) - b b^T + (T2 b)(T2 b)^T,   T2 = moment_Tm[0]

        One shared kernel or ``SeparateIndependent`` (per-latent inv_ls, variance, moment_Tm); D > 32: K(X, X) by the GEMM-form
        fill into cov_p, then the accumulating form of ``tsvgp_cov_*``.  One [Np, Mp] tile and one [Np, Np] matrix are live per
        latent beside the [P, Np, Np] result.  ``nonpos``: how many diagonal entries are not positive (the assert_positive of
        src/models/tsvgp.py:113, what ``run`` counts for the marginal variances).  ``padded``: cov is returned as the
        [P, Np, Np] buffer itself (identity block in the padding: ``cholesky(overwrite=True)`` factors it in place; the memory
        check then counts the factor that call returns as well)."""
        T, dev = self.dtype, self.device
        X = X.to(device=dev, dtype=T).contiguous()
        Z = Z.to(device=dev, dtype=T).contiguous()
        if X.dim() != 2 or Z.dim() != 2 or Z.shape[1] != X.shape[1]:
            raise ValueError(f"X must be [N, D] and Z [M, D] with equal D, got {tuple(X.shape)} and {tuple(Z.shape)}")
        N, D = X.shape
        M = Z.shape[0]
        P = moment_Tm.shape[0]
        if N == 0:
            raise ValueError("full_cov needs at least one test point")
        separate = isinstance(kernel, SeparateIndependent)
        if separate and len(kernel.kernels) != P:
            raise ValueError(f"{len(kernel.kernels)} kernels for {P} latent GPs")
        if two_product and (P != 1 or whiten_T is None or separate):
            raise ValueError("two_product: one latent, one kernel, a whitening factor")
        Np, Mp = B.round_up(N), B.round_up(M)
        esz = 8 if T == torch.float64 else 4
        need = (2 if padded else 1) * P * Np * Np * 8 + (0 if T == torch.float64 else Np * Np * esz) + 3 * Np * Mp * esz
        free, _ = torch.cuda.mem_get_info(dev)
        free += torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        if need > free:
            raise ValueError(f"full_cov: {P} joint covariance(s) of {N} test points need {need / 2 ** 30:.1f} GiB of device memory "
                             f"({P} x {Np} x {Np} fp64), {free / 2 ** 30:.1f} GiB are free; predict fewer points at a time")
        self._b_tag = None  # the operand buffers below are overwritten
        cov = torch.empty((P, Np, Np), dtype=torch.float64, device=dev)
        Cw = None if T == torch.float64 else torch.empty((Np, Np), dtype=T, device=dev)
        mean = torch.empty((N, P), dtype=torch.float64, device=dev)
        gam = self._padded_gamma(gamma, Mp, P)
        Kfu = self._get("Kfu", (Np, Mp), T)
        tile = self._get("Tt", (Np, Mp), T)
        self._side.wait_stale()
        for p in range(P):
            kp = kernel.kernels[p] if separate else kernel
            if p == 0 or separate:
                self.fill(X, Z, kp, Kfu)
            A = Kfu
            wt = self._per_latent(whiten_T, p)
            if wt is not None:
                A = self._get("B", (Np, Mp), T)
                self.trmm(Kfu, self._pad_square(wt, Mp, "pad_Linv"), A, whiten_mode)
            Tm = self._pad_square(moment_Tm[p], Mp, "pad_Tm1")
            self.trmm(A, Tm, tile, moment_mode)
            mean[:, p] = torch.mv(A[:N], gam[:, p])  # gam: [Mp, P], rows >= M zero
            C = cov[p] if Cw is None else Cw
            if D > MAX_INPUT_DIM or isinstance(kp, COMBINED):
                # the GEMM form, or the fused fill of a Sum or a Product (the padding is zero: the call below sets it)
                self.fill(X, X, kp, C)
                base = dict(accumulate=True)
            else:
                base = dict(X=X, inv_ls=kp.inv_lengthscales(D, T, dev), variance=kp.variance.item(), kind=kp.kind)
            if two_product:
                self.cov(A, C, N, sign=-1.0, **base)
                self.cov(tile, C, N, sign=1.0, accumulate=True)
            else:
                self.cov(tile, C, N, sign=-1.0, **base)
            if Cw is not None:
                cov[p].copy_(Cw)
        diag = cov.diagonal(dim1=-2, dim2=-1)[:, :N]
        nonpos = (~(diag > 0)).sum().to(torch.float64)
        return mean, (cov if padded else cov[:, :N, :N]), nonpos

    def mc_normals(self, S: int, N: int, C: int, seed: int, draw: int, row_offset: int = 0) -> torch.Tensor:
        """eps [S, N, C] fp64 of ``tsvgp_mc_normals_f64``: the draw of (seed, draw, row_offset + n, s, c)."""
        if not (1 <= C <= B.MAX_BATCH):
            raise ValueError(f"the normal generator takes 1 <= C <= {B.MAX_BATCH} columns, got {C}")
        if not (1 <= S <= B.MC_MAX_SAMPLES):
            raise ValueError(f"the normal generator takes 1 <= S <= {B.MC_MAX_SAMPLES} samples, got {S}")
        if N < 1 or row_offset < 0 or S * N * ((C + 3) // 4) > (2 ** 31 - 1) * 256:
            raise ValueError(f"the normal generator takes N >= 1, row_offset >= 0 and S N ceil(C / 4) <= (2^31 - 1) 256, got "
                             f"S = {S}, N = {N}, C = {C}, row_offset = {row_offset}")
        out = torch.empty((S, N, C), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            B.check(self.lib.tsvgp_mc_normals_f64(out.data_ptr(), int(seed), int(draw), int(row_offset), S, N, C, self._stream()),
                    "tsvgp_mc_normals")
        return out

    def _pathwise_operands(self, X, Z, kernel, Omega, W, V):
        """The operands of ``pathwise`` / ``pathwise_vjp`` on the device in fp64, checked: (X, Z, Omega, W, V, inv_ls, variance, N, M,
        L, D, S), M = 0 and Z = V = None without an update."""
        if isinstance(kernel, SeparateIndependent):
            raise ValueError("pathwise: one kernel per call; pass the latent's own kernel")
        f64 = lambda t: t.to(device=self.device, dtype=torch.float64).contiguous()
        X, Omega, W = f64(X), f64(Omega), f64(W)
        if X.dim() != 2 or X.shape[0] < 1:
            raise ValueError(f"pathwise: X must be [N >= 1, D], got {tuple(X.shape)}")
        N, D = X.shape
        if D < 1 or D > MAX_INPUT_DIM:
            raise ValueError(f"pathwise: 1 <= D <= {MAX_INPUT_DIM} (TSVGP_MAX_BATCH, the normal generator's column limit), got {D}")
        if Omega.dim() != 2 or Omega.shape[0] < 1 or Omega.shape[1] != D:
            raise ValueError(f"pathwise: Omega must be [L >= 1, D] = [L, {D}], got {tuple(Omega.shape)}")
        L = Omega.shape[0]
        if W.dim() != 2 or W.shape[0] < 1 or W.shape[1] != 2 * L:
            raise ValueError(f"pathwise: W must be [S >= 1, 2 L] = [S, {2 * L}], got {tuple(W.shape)}")
        S = W.shape[0]
        M = 0
        if V is not None:
            V, Z = f64(V), f64(Z)
            M = Z.shape[0]
            if Z.dim() != 2 or Z.shape[1] != D or tuple(V.shape) != (S, M):
                raise ValueError(f"pathwise: Z must be [M, {D}] and V [S, M] = [{S}, {M}], got {tuple(Z.shape)} and {tuple(V.shape)}")
        if M == 0:
            Z = V = None
        inv_ls = kernel.inv_lengthscales(D, torch.float64, self.device)
        return X, Z, Omega, W, V, inv_ls, kernel.variance.item(), N, M, L, D, S

    def pathwise(self, X, Z, kernel, Omega, W, V=None) -> torch.Tensor:
        """S pathwise function draws of one latent GP at the rows of X (``tsvgp_pathwise_f64``), [S, N] fp64:

            out[s, n] = sum_l (W[s, l] cos(Omega_l . x~_n) + W[s, L + l] sin(Omega_l . x~_n)) + sum_m V[s, m] k(x_n, z_m)

        X [N, D <= 32], Z [M, D], ``kernel`` one stationary kernel (lengthscales, variance and profile of k and of x~ = x / l),
        Omega [L, D], W [S, 2 L] (already scaled by sqrt(variance / L)), V [S, M]; ``V=None``: the first sum alone (Z is not read).
        fp64 whatever the engine's compute dtype; launches on the current stream, ``PATHWISE_MAX_S`` samples per launch."""
        X, Z, Omega, W, V, inv_ls, variance, N, M, L, D, S = self._pathwise_operands(X, Z, kernel, Omega, W, V)
        out = torch.empty((S, N), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            for s0 in range(0, S, B.PATHWISE_MAX_S):
                sc = min(B.PATHWISE_MAX_S, S - s0)
                self._launch("tsvgp_pathwise", lambda: self.lib.tsvgp_pathwise_f64(
                    int(kernel.kind), X.data_ptr(), _ptr(Z), inv_ls.data_ptr(), variance, Omega.data_ptr(),
                    W[s0:s0 + sc].data_ptr(), _ptr(V[s0:s0 + sc] if M else None), out[s0:s0 + sc].data_ptr(), N, M, L, D, sc, N,
                    self._stream()))
        return out

    def pathwise_vjp(self, X, Z, kernel, Omega, W, V, C) -> torch.Tensor:
        """The vector-Jacobian product of ``pathwise`` with respect to X (``tsvgp_pathwise_vjp_f64``), [N, D] fp64:

            dX[n, d] = sum_s C[s, n] d out[s, n] / d X[n, d]

        The operands of ``pathwise`` (``V=None``: the prior part alone) and the cotangents C [S, N].  ``PATHWISE_MAX_S`` samples
        per launch on the current stream; the chunks' results are added in chunk order on the device (no host read, the same bits
        every time)."""
        X, Z, Omega, W, V, inv_ls, variance, N, M, L, D, S = self._pathwise_operands(X, Z, kernel, Omega, W, V)
        if not isinstance(C, torch.Tensor) or tuple(C.shape) != (S, N):
            raise ValueError(f"pathwise_vjp: C must be [S, N] = [{S}, {N}], got {tuple(getattr(C, 'shape', ()))}")
        C = C.to(device=self.device, dtype=torch.float64).contiguous()
        dX = torch.empty((N, D), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            for s0 in range(0, S, B.PATHWISE_MAX_S):
                sc = min(B.PATHWISE_MAX_S, S - s0)
                part = dX if s0 == 0 else torch.empty_like(dX)
                self._launch("tsvgp_pathwise_vjp", lambda: self.lib.tsvgp_pathwise_vjp_f64(
                    int(kernel.kind), X.data_ptr(), _ptr(Z), inv_ls.data_ptr(), variance, Omega.data_ptr(),
                    W[s0:s0 + sc].data_ptr(), _ptr(V[s0:s0 + sc] if M else None), C[s0:s0 + sc].data_ptr(), N, part.data_ptr(),
                    N, M, L, D, sc, self._stream()))
                if s0 > 0:
                    dX += part
        return dX

    # ------------------------------------------------------------------ per-datum diagonal sites (t_SVGP_sites)
    def project_diag(self, X, Z, kernel, w1, w2):
        """The projection of per-datum sites onto the inducing points (reference src/util.py:188-236 with cholesky=False and
        no K_uu):  acc2 = sum_n w2_n k_n k_n^T [1, M, M],  acc1 = sum_n w1_n k_n [1, M]  over k_n = K(Z, x_n), fp64 -- the fill
        and ``_site_sums`` with the caller's weights w1, w2 [Np, 1] (compute dtype, rows >= N zero) in place of the
        likelihood gradients.  The filled K(X, Z) stays in the buffer: the returned ticket hands it to ``run(prefill=...)`` /
        ``run_two_product`` / ``diag_sites_moments`` of the same step, which then do not fill again."""
        T, dev = self.dtype, self.device
        X = X.to(device=dev, dtype=T).contiguous()
        Z = Z.to(device=dev, dtype=T).contiguous()
        N, D = X.shape
        M = Z.shape[0]
        Np, Mp = B.round_up(N), B.round_up(M)
        if tuple(w1.shape) != (Np, 1) or tuple(w2.shape) != (Np, 1) or w1.dtype != T or w2.dtype != T:
            raise ValueError(f"site weights must be [Np, 1] = [{Np}, 1] in {T}")
        if N == 0:
            zero = torch.zeros((1, M, M), dtype=torch.float64, device=dev)
            return zero, torch.zeros((1, M), dtype=torch.float64, device=dev), None
        self._b_tag = None
        Kfu = self._get("Kfu", (Np, Mp), T)
        self._side.wait_stale()
        self.se_fill(X, Z, kernel.inv_lengthscales(D, T, dev), kernel.variance.item(), Kfu, kernel.kind)
        acc2, acc1 = self._site_sums(Kfu, w1, w2, 1, M)
        return acc2, acc1, SideBranch.inline(dev, reads=(X, Z), name="Kfu", buf=Kfu)

    def diag_sites_moments(self, X, Z, kernel, ticket, *, whiten_T, moment_Tm, moment_mode, gamma, mean_only=False):
        """mean, var [N, 1] in the compute dtype (cached buffers; var None with ``mean_only``) on the K(X, Z) that
        ``project_diag`` left (``ticket``): the whitening product when ``whiten_T`` is given, then the moments with no
        likelihood (TSVGP_LIK_MEANONLY with ``mean_only``)."""
        T, dev = self.dtype, self.device
        N, M = X.shape[0], Z.shape[0]
        Np, Mp = B.round_up(N), B.round_up(M)
        Kfu = self._buf.get("Kfu")
        if ticket is None or ticket.buf is not Kfu:
            raise RuntimeError("diag_sites_moments needs the ticket of this engine's last project_diag")
        ticket.join()
        A = Kfu
        if whiten_T is not None:
            A = self._get("B", (Np, Mp), T)
            self.trmm(Kfu, self._pad_square(whiten_T, Mp, "pad_Linv"), A, B.TRI_UPPER)
        Tm = self._pad_square(moment_Tm, Mp, "pad_Tm")
        gam = self._padded_gamma(gamma, Mp, 1)
        mean = self._get("ds_mean", (N, 1), T)
        var = None if mean_only else self._get("ds_var", (N, 1), T)
        self.moments(A, Tm, gam, kernel.variance.item(), N, moment_mode, mean_only=mean_only, mean=mean, var=var)
        return mean, var

    def diag_site_step(self, mean, var, Y, lik_id, lik_param, lr, l1, l2, l1c=None, l2c=None):
        """One launch of ``tsvgp_diag_site_step_*``: the likelihood map on (mean, var, Y) [N, P] in the compute dtype and the
        in-place site update of l1, l2 [Np, P] (fp64; fp32 copies into l1c, l2c for the fp32 engine).  ``var`` None: Gaussian
        only (no variance read; the ve partials are then NaN).  Returns (ve_sum, nonpos) as fp64 device scalars."""
        T, dev = self.dtype, self.device
        N, P = mean.shape
        Np = l1.shape[0]
        if T == torch.float32 and (l1c is None or l2c is None):
            raise ValueError("the fp32 site step writes fp32 copies of the sites: l1c, l2c are required")
        Yc = Y.to(device=dev, dtype=T).contiguous()
        nblk = Np // B.TILE
        ve_partial = self._get("ve_partial", (nblk,), torch.float64)
        nonpos_partial = self._get("nonpos_partial", (nblk,), torch.int32)
        args = [mean.data_ptr(), _ptr(var), Yc.data_ptr(), int(lik_id), float(lik_param), float(lr), l1.data_ptr(), l2.data_ptr()]
        if T == torch.float32:
            args += [l1c.data_ptr(), l2c.data_ptr()]
        args += [ve_partial.data_ptr(), nonpos_partial.data_ptr(), N, Np, P, self._stream()]
        with torch.cuda.device(dev):
            self._launch("tsvgp_diag_site_step", lambda: self._fn("tsvgp_diag_site_step")(*args))
        return ve_partial.sum(), nonpos_partial.sum().to(torch.float64)

    # ------------------------------------------------------------------ t_VGP: the exact N x N model (models/tvgp.py)
    def vgp_system(self, X, kernel, l1, l2, jitter: float, rhs_rows=None, extra_rows: int = 0):
        """The stacked operand of ``vgp_factor`` (``tsvgp_vgp_system_f64``): B = I + s s^T * (K(X, X) + jitter I) in rows
        [0, Np) of a cached fp64 buffer S [Np + rhs, Np] and, with ``rhs_rows`` None, the model's own right-hand sides behind it
        (K~ s in rows [Np, 2 Np), s y~ in row 2 Np; rhs = Np + 128).  ``rhs_rows`` = r: B only (TSVGP_VGP_NO_ROWS) and r rows --
        a multiple of 128 -- left for the caller to fill.  X [N, D <= 32] fp64 on the device; l1, l2: the padded site state
        [Np, 1].  ``extra_rows`` (a multiple of 128): that many further rows behind the model's own, left for the caller to fill
        (``vgp_grad_operands``: diag(s)).  Returns (S, Np)."""
        N, D = X.shape
        if D > MAX_INPUT_DIM:
            raise ValueError(f"t_VGP builds its N x N system in one fused kernel: D <= {MAX_INPUT_DIM}, got {D}")
        Np = B.round_up(N)
        own = rhs_rows is None
        rhs = Np + B.TILE if own else int(rhs_rows)
        if extra_rows % B.TILE or extra_rows < 0:
            raise ValueError("vgp_system: extra_rows a non-negative multiple of 128")
        rhs += int(extra_rows)
        if rhs % B.TILE or l1.shape[0] < Np or l2.shape[0] < Np or X.dtype != torch.float64 or not X.is_contiguous():
            raise ValueError("vgp_system: X fp64 contiguous, sites padded to Np rows, rhs_rows a multiple of 128")
        S = self._get("vgp_S", (Np + rhs, Np), torch.float64)
        inv_ls = kernel.inv_lengthscales(D, torch.float64, self.device)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_vgp_system", lambda: self.lib.tsvgp_vgp_system_f64(
                int(kernel.kind), X.data_ptr(), inv_ls.data_ptr(), kernel.variance.item(), float(jitter), l1.data_ptr(),
                l2.data_ptr(), S.data_ptr(), N, Np, D, Np, 0 if own else B.VGP_NO_ROWS, self._stream()))
        return S, Np

    def vgp_factor(self, S, Np: int):
        """B = L L^T in place and the rows below it -> rows L^-T (``tsvgp_potrf_solve_f64``; B has eigenvalues >= 1: the plain
        panels).  Returns info [1] int32 (no host synchronisation)."""
        rows, lds = S.shape
        info = torch.empty(1, dtype=torch.int32, device=self.device)
        work = self._get("potrf_work", (1, 128 * 128), torch.float64)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_potrf", lambda: self.lib.tsvgp_potrf_solve_f64(
                S.data_ptr(), Np, lds, 1, rows * lds, info.data_ptr(), work.data_ptr(), rows - Np, self.potrf_flags, self._stream()))
        return info

    def vgp_rows(self, C, N: int, kdiag: float, *, z=None, Y=None, l1=None, l2=None, lik_id=B.LIK_NONE, lik_param=0.0, beta=0.0,
                 want_mean=False, want_var=False):
        """One launch of ``tsvgp_vgp_rows_f64`` over the solved rows C [Np, ldc] (a view of S): mean = C z, var = kdiag - |C|^2
        per row, and with a likelihood the sums of ve and of E_q log t and the in-place update of the padded sites l1, l2 by the
        step ``beta`` (0: the sites are not written).  Returns (mean [N, 1] | None, var [N, 1] | None, ve_sum, eqt_sum, nonpos):
        fp64 device tensors, the sums as scalars."""
        Np, K = C.shape
        nblk = Np // B.TILE
        mean = torch.empty((N, 1), dtype=torch.float64, device=self.device) if want_mean else None
        var = torch.empty((N, 1), dtype=torch.float64, device=self.device) if want_var else None
        ve_partial = self._get("ve_partial", (nblk,), torch.float64)
        eqt_partial = self._get("eqt_partial", (nblk,), torch.float64)
        nonpos_partial = self._get("nonpos_partial", (nblk,), torch.int32)
        lik = lik_id != B.LIK_NONE
        with torch.cuda.device(self.device):
            self._launch("tsvgp_vgp_rows", lambda: self.lib.tsvgp_vgp_rows_f64(
                C.data_ptr(), C.stride(0), _ptr(z), _ptr(Y), _ptr(l1), _ptr(l2), float(kdiag), int(lik_id), float(lik_param),
                float(beta), _ptr(mean), _ptr(var), ve_partial.data_ptr() if lik else None, eqt_partial.data_ptr() if lik else None,
                nonpos_partial.data_ptr(), N, Np, K, self._stream()))
        nonpos = nonpos_partial.sum().to(torch.float64)
        if not lik:
            return mean, var, None, None, nonpos
        return mean, var, ve_partial.sum(), eqt_partial.sum(), nonpos

    def vgp_grad_operands(self, X, kernel, l1, l2, jitter: float):
        """The factorisation of ``vgp_system`` / ``vgp_factor`` with diag(s), s = sqrt|lambda_2|, riding as Np further plain
        right-hand-side rows behind the model's own: they come out as V = diag(s) L^-T (V V^T = (K~ + |Lambda|^-1)^-1).  One
        stacked buffer S [(3 Np + 128) x Np]; L, C and z are where ``vgp_system`` + ``vgp_factor`` leave them.  Returns
        (S, Np, info, V [Np, Np], a view of rows [2 Np + 128, 3 Np + 128))."""
        N = X.shape[0]
        S, Np = self.vgp_system(X, kernel, l1, l2, jitter, extra_rows=B.round_up(N))
        V = S[2 * Np + B.TILE:]
        V.zero_()
        torch.diagonal(V)[:N] = torch.sqrt(torch.abs(l2[:N, 0]))
        return S, Np, self.vgp_factor(S, Np), V

    def lik_grads(self, mean, var, Y, lik_id, lik_param):
        """g0 = d ve / d mean, g1 = d ve / d var [N] at (mean, var, Y) [N, 1] fp64, never cropped (``lik_map`` in fp64 with
        LIK_NOCROP): the gradients of the bound, not the site update's."""
        N = mean.shape[0]
        Np = B.round_up(N)
        nblk = Np // B.TILE
        lm = self.lik_map(mean, var, Y, int(lik_id) | B.LIK_NOCROP, lik_param, N, Np,
                          g0=self._get("vgp_g0", (Np, 1), torch.float64), g1=self._get("vgp_g1", (Np, 1), torch.float64),
                          ve_partial=self._get("vgp_lik_ve", (nblk,), torch.float64),
                          nonpos_partial=self._get("vgp_lik_nonpos", (nblk,), torch.int32))
        return lm.g0[:N, 0], lm.g1[:N, 0]

    def vgp_kernel_grad(self, X, kernel, W, a, c):
        """sum_ij G[i, j] dK(X, X)[i, j] / d theta, G = W + 1/2 (a c^T + c a^T), for theta = variance and the lengthscales
        (``tsvgp_vgp_kernel_grad_f64``).  X [N, D <= 32] fp64; W [Np, ldw] fp64 symmetric, of which the lower block triangle of
        128 x 128 tiles is read; a, c [>= N] fp64.  Returns (dvar 0-dim, dls [D]): dls[d] is the derivative with respect to
        lengthscale d of an ARD kernel; for one shared lengthscale the caller adds them up."""
        N, D = X.shape
        if D > MAX_INPUT_DIM:
            raise ValueError(f"vgp_kernel_grad: D <= {MAX_INPUT_DIM}, got {D}")
        Np = B.round_up(N)
        if (W.dtype != torch.float64 or W.dim() != 2 or W.shape[0] < Np or W.shape[1] < Np or W.stride(1) != 1 or W.stride(0) % 2
                or X.dtype != torch.float64 or not X.is_contiguous()):
            raise ValueError("vgp_kernel_grad: X fp64 contiguous, W fp64 [Np, >= Np] with unit column stride and an even row stride")
        a = a.reshape(-1).to(torch.float64).contiguous()
        c = c.reshape(-1).to(torch.float64).contiguous()
        if a.shape[0] < N or c.shape[0] < N:
            raise ValueError("vgp_kernel_grad: a, c need N entries")
        size = int(self.lib.tsvgp_vgp_kernel_grad_parts(Np, D))
        if size <= 0:
            raise ValueError(f"vgp_kernel_grad: no partials layout for Np = {Np}, D = {D}")
        part = self._get("vgp_kgrad_part", (size,), torch.float64)
        inv_ls = kernel.inv_lengthscales(D, torch.float64, self.device)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_vgp_kernel_grad", lambda: self.lib.tsvgp_vgp_kernel_grad_f64(
                int(kernel.kind), X.data_ptr(), inv_ls.data_ptr(), kernel.variance.item(), W.data_ptr(), W.stride(0), a.data_ptr(),
                c.data_ptr(), N, Np, D, part.data_ptr(), self._stream()))
        nt = Np // B.TILE
        cols = size // (nt * (nt + 1) // 2 + 1)
        total = part[size - cols:]
        return total[0].clone(), total[1:1 + D] * inv_ls

    def greedy_select(self, X, kernel, M: int, threshold: float = 0.0):
        """Greedy conditional-variance selection of at most M rows of X as inducing points (``tsvgp_greedy_select_f64``):
        pivoted Cholesky of K(X, X) that always takes the row with the largest residual prior variance and stops when that
        falls to ``floor = max(threshold, 1e-12 * variance)`` or below.  X [N, D <= 32] on this device (converted to fp64 when
        it is not: the arithmetic is fp64 whatever the engine's compute dtype), ``kernel`` one stationary kernel.

        Allocates the transposed factor C [M, Np] fp64 for the length of the call -- 8 M Np bytes, 8.4 GB at N = 1e6,
        M = 1024 -- plus d [Np] and the outputs; makes the one call (2 M launches, no host read between them) and reads
        ``count`` back once.  Returns ``(indices [count] int64, pivots [count], d [N], count)``, tensors on the device:
        d is the residual conditional variance diag(K_ff - K_fS K_SS^-1 K_Sf), exactly 0 at every picked row."""
        if isinstance(kernel, SeparateIndependent):
            raise ValueError("greedy_select: one kernel defines one conditional variance; pass the latent's kernel you mean")
        if X.dim() != 2 or X.shape[0] < 1:
            raise ValueError("greedy_select: X must be [N >= 1, D]")
        N, D = X.shape
        M = int(M)
        if M < 1:
            raise ValueError(f"greedy_select: M >= 1, got {M}")
        if D < 1 or D > MAX_INPUT_DIM:
            raise ValueError(f"greedy_select: 1 <= D <= {MAX_INPUT_DIM}, got {D}")
        variance = kernel.variance.item()
        floor = max(float(threshold), 1e-12 * variance)
        X = X.to(device=self.device, dtype=torch.float64).contiguous()
        Np = B.round_up(N)
        nbytes = int(self.lib.tsvgp_greedy_select_work_bytes(N, M))
        if nbytes <= 0:
            raise ValueError(f"greedy_select: no workspace layout for N = {N}, M = {M}")
        inv_ls = kernel.inv_lengthscales(D, torch.float64, self.device)
        C = torch.empty((M, Np), dtype=torch.float64, device=self.device)
        d = torch.empty((Np,), dtype=torch.float64, device=self.device)
        indices = torch.zeros((M,), dtype=torch.int64, device=self.device)
        pivots = torch.zeros((M,), dtype=torch.float64, device=self.device)
        count = torch.zeros((1,), dtype=torch.int32, device=self.device)
        work = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_greedy_select", lambda: self.lib.tsvgp_greedy_select_f64(
                int(kernel.kind), X.data_ptr(), inv_ls.data_ptr(), variance, floor, C.data_ptr(), Np, d.data_ptr(),
                indices.data_ptr(), pivots.data_ptr(), count.data_ptr(), work.data_ptr(), N, M, D, self._stream()))
        n = int(count.item())  # the one device -> host read (it also keeps C alive until the launches are through)
        return indices[:n], pivots[:n], d[:N], n

    def kmeans_assign(self, X, C, inv_ls):
        """The assignment step of Lloyd's k-means (``tsvgp_kmeans_assign_f64``): for every row of X [N, D <= 32] the lowest m
        whose centre C[m] is nearest in the scaled coordinates x * inv_ls, without any N x M array.  fp64 whatever the engine's
        compute dtype.  Returns ``(labels [N] int32, dist [N], inertia 0-dim)`` on the device: dist the minimal scaled squared
        distance, inertia the sum of the per-workgroup partial sums (one fixed-shape reduction: the same bits in every call of
        the same N and D)."""
        if X.dim() != 2 or X.shape[0] < 1 or C.dim() != 2 or C.shape[0] < 1 or C.shape[1] != X.shape[1]:
            raise ValueError(f"kmeans_assign: X [N >= 1, D] and C [M >= 1, D], got {tuple(X.shape)} and {tuple(C.shape)}")
        N, D = X.shape
        M = C.shape[0]
        if D < 1 or D > MAX_INPUT_DIM:
            raise ValueError(f"kmeans_assign: 1 <= D <= {MAX_INPUT_DIM}, got {D}")
        X = X.to(device=self.device, dtype=torch.float64).contiguous()
        C = C.to(device=self.device, dtype=torch.float64).contiguous()
        inv_ls = inv_ls.to(device=self.device, dtype=torch.float64).contiguous()
        if tuple(inv_ls.shape) != (D,):
            raise ValueError(f"kmeans_assign: inv_ls must be [{D}], got {tuple(inv_ls.shape)}")
        nparts = int(self.lib.tsvgp_kmeans_assign_parts(N, D))
        if nparts <= 0:
            raise ValueError(f"kmeans_assign: no launch geometry for N = {N}, D = {D}")
        labels = torch.empty((N,), dtype=torch.int32, device=self.device)
        dist = torch.empty((N,), dtype=torch.float64, device=self.device)
        part = torch.empty((nparts,), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_kmeans_assign", lambda: self.lib.tsvgp_kmeans_assign_f64(
                X.data_ptr(), C.data_ptr(), inv_ls.data_ptr(), labels.data_ptr(), dist.data_ptr(), part.data_ptr(), N, M, D,
                self._stream()))
        return labels, dist, part.sum()

    def kmeans_update(self, X, labels, C_old):
        """The centroid step of Lloyd's k-means (``tsvgp_kmeans_update_f64``): C_new[m] = the mean of the rows of X labelled m,
        summed in a fixed order (no atomics), or C_old[m] bit for bit when there is none.  The segments come from torch: a stable
        sort of the labels (rows of a cluster in increasing row number), ``bincount`` and ``cumsum``.  Returns
        ``(C_new [M, D], counts [M] int64)`` on the device."""
        if X.dim() != 2 or X.shape[0] < 1 or C_old.dim() != 2 or C_old.shape[0] < 1 or C_old.shape[1] != X.shape[1]:
            raise ValueError(f"kmeans_update: X [N >= 1, D] and C_old [M >= 1, D], got {tuple(X.shape)} and {tuple(C_old.shape)}")
        N, D = X.shape
        M = C_old.shape[0]
        if D < 1 or D > MAX_INPUT_DIM:
            raise ValueError(f"kmeans_update: 1 <= D <= {MAX_INPUT_DIM}, got {D}")
        if tuple(labels.shape) != (N,):
            raise ValueError(f"kmeans_update: labels must be [{N}], got {tuple(labels.shape)}")
        X = X.to(device=self.device, dtype=torch.float64).contiguous()
        C_old = C_old.to(device=self.device, dtype=torch.float64).contiguous()
        labels = labels.to(device=self.device)
        order = torch.sort(labels, stable=True).indices
        counts = torch.bincount(labels, minlength=M)[:M]  # (a label >= M has no segment: its rows are left out)
        offsets = torch.zeros((M + 1,), dtype=torch.int64, device=self.device)
        torch.cumsum(counts, 0, out=offsets[1:])
        C_new = torch.empty_like(C_old)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_kmeans_update", lambda: self.lib.tsvgp_kmeans_update_f64(
                X.data_ptr(), order.data_ptr(), offsets.data_ptr(), C_old.data_ptr(), C_new.data_ptr(), N, M, D, self._stream()))
        return C_new, counts

    def kmeanspp(self, X, inv_ls, M: int, L: int, seed: int):
        """k-means++ seeding with L greedy local trials per centre (``tsvgp_kmeanspp_f64``): M rows of X [N, D <= 32], each
        drawn with probability proportional to its scaled squared distance to the nearest row already taken.  fp64 whatever
        the engine's compute dtype; X must be finite (the caller checks).  One call, 2 M + 2 launches, no host read; the
        workspace is one double per workgroup and trial.  Returns ``(indices [M] int64, dist [N], pot_hist [M],
        cand [M, L] int64, cand_pot [M, L], unif [M, L])`` on the device."""
        if X.dim() != 2 or X.shape[0] < 1:
            raise ValueError(f"kmeanspp: X must be [N >= 1, D], got {tuple(X.shape)}")
        N, D = X.shape
        M, L, seed = int(M), int(L), int(seed)
        if D < 1 or D > MAX_INPUT_DIM:
            raise ValueError(f"kmeanspp: 1 <= D <= {MAX_INPUT_DIM}, got {D}")
        if not 1 <= M <= N:
            raise ValueError(f"kmeanspp: 1 <= M <= N = {N}, got {M}")
        if not 1 <= L <= B.KMEANSPP_MAX_TRIALS:
            raise ValueError(f"kmeanspp: 1 <= L <= {B.KMEANSPP_MAX_TRIALS}, got {L}")
        if not -2 ** 63 <= seed < 2 ** 63:
            raise ValueError(f"kmeanspp: seed must fit a signed 64-bit integer, got {seed}")
        X = X.to(device=self.device, dtype=torch.float64).contiguous()
        inv_ls = inv_ls.to(device=self.device, dtype=torch.float64).contiguous()
        if tuple(inv_ls.shape) != (D,):
            raise ValueError(f"kmeanspp: inv_ls must be [{D}], got {tuple(inv_ls.shape)}")
        nwork = int(self.lib.tsvgp_kmeanspp_work(N, D, L))
        if nwork <= 0:
            raise ValueError(f"kmeanspp: no launch geometry for N = {N}, D = {D}, L = {L}")
        f64 = dict(dtype=torch.float64, device=self.device)
        indices = torch.empty((M,), dtype=torch.int64, device=self.device)
        cand = torch.empty((M, L), dtype=torch.int64, device=self.device)
        dist, pot_hist, work = torch.empty((N,), **f64), torch.empty((M,), **f64), torch.empty((nwork,), **f64)
        cand_pot, unif = torch.empty((M, L), **f64), torch.empty((M, L), **f64)
        with torch.cuda.device(self.device):
            self._launch("tsvgp_kmeanspp", lambda: self.lib.tsvgp_kmeanspp_f64(
                X.data_ptr(), inv_ls.data_ptr(), seed, M, L, indices.data_ptr(), dist.data_ptr(), pot_hist.data_ptr(),
                cand.data_ptr(), cand_pot.data_ptr(), unif.data_ptr(), work.data_ptr(), N, D, self._stream()))
        return indices, dist, pot_hist, cand, cand_pot, unif
