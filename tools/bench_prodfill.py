"""The fused fill and the fused M-step gradient of a Product kernel beside what they stand in for (writes
profiles/prodfill_bench.txt).

N = 1e6, M = 1024, D = 8, fp64 and fp32, C = 1 .. 4 components (kinds SE, Matern-3/2, Matern-5/2, SE in this order, each with its
own lengthscales; X = randn, Z = X[:M]):

  fill   fused    one ``tsvgp_kernel_fill_prod_*`` launch
         sum      ``tsvgp_kernel_fill_sum_*`` at the same C: the yardstick -- the same kernel and arithmetic, a multiply for an fma
         split    C ``tsvgp_kernel_fill_*`` launches (component 0 into K, every other one into a second buffer) plus C - 1
                  ``torch.mul_`` of the two buffers: what the product costs without the fused kernel
  grad   fused    one ``tsvgp_kernel_grad_prod_*`` launch (all C parameter sets)
         single   C launches of ``tsvgp_kernel_grad_*`` on the same U: what a Sum pays for its C parameter sets

Every launch is timed ALONE between two events on an otherwise idle stream, with a device synchronisation in front; warm-up
launches first, then ``--repeats`` of each, the variants interleaved round by round; medians and ranges.  The split and single
forms' times are the sums of their launches' medians (nothing overlaps: each waits for the one before it through the same
buffers).  No threshold is asserted.

    python tools/bench_prodfill.py [--rows 1000000] [--m 1024] [--dim 8] [--warmup 3] [--repeats 50] [--out profiles/prodfill_bench.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tsvgp_amd as p  # noqa: E402

B = p._backend
KINDS = [B.KERNEL_SE, B.KERNEL_MATERN32, B.KERNEL_MATERN52, B.KERNEL_SE]
VARIANCES = [1.3, 0.8, 0.5, 0.2]


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def fmt(ts):
    return f"{statistics.median(ts):8.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prodfill_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = B.lib()
    N, M, D = a.rows, a.m, a.dim
    Np, Mp = B.round_up(N), B.round_up(M)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_prodfill.py: {torch.cuda.get_device_name(dev)}, N = {N}, M = {M}, D = {D}; each launch alone between two "
        f"events, {a.warmup} warm-up, median (min .. max) of {a.repeats}")
    g = torch.Generator(device="cpu").manual_seed(0)
    X64 = torch.randn(N, D, generator=g, dtype=torch.float64)
    ls64 = (0.7 + torch.rand(4, D, generator=g, dtype=torch.float64)) * 2.0
    rows, Dp = int(lib.tsvgp_kernel_grad_rows()), int(lib.tsvgp_kernel_grad_dpad(D))
    nrb, ncb = (N + rows - 1) // rows, (Mp + 511) // 512
    for dtype, sfx, ct in ((torch.float64, "f64", ctypes.c_double), (torch.float32, "f32", ctypes.c_float)):
        X = X64.to(dev, dtype).contiguous()
        Z = X[:M].clone()
        inv_ls = (1.0 / ls64).to(dev, dtype).contiguous()  # [4, D]
        K = torch.empty((Np, Mp), dtype=dtype, device=dev)
        K2 = torch.empty((Np, Mp), dtype=dtype, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        fill_prod, fill_sum = getattr(lib, f"tsvgp_kernel_fill_prod_{sfx}"), getattr(lib, f"tsvgp_kernel_fill_sum_{sfx}")
        fill = getattr(lib, f"tsvgp_kernel_fill_{sfx}")
        grad_prod, grad = getattr(lib, f"tsvgp_kernel_grad_prod_{sfx}"), getattr(lib, f"tsvgp_kernel_grad_{sfx}")
        gb = Np * Mp * K.element_size() / 1e9

        def prodvar(C):
            v = 1.0
            for c in range(C):
                v *= VARIANCES[c]
            return v

        def fused(C, out=K):
            kinds = (ctypes.c_int * C)(*KINDS[:C])
            B.check(fill_prod(kinds, X.data_ptr(), Z.data_ptr(), inv_ls.data_ptr(), prodvar(C), out.data_ptr(), N, M, D, Mp, C, stream),
                    "fused")

        def summed(C, out=K):
            kinds, var = (ctypes.c_int * C)(*KINDS[:C]), (ct * C)(*VARIANCES[:C])
            B.check(fill_sum(kinds, X.data_ptr(), Z.data_ptr(), inv_ls.data_ptr(), var, out.data_ptr(), N, M, D, Mp, C, stream), "sum")

        def single(c, out):
            B.check(fill(KINDS[c], X.data_ptr(), Z.data_ptr(), inv_ls[c].data_ptr(), VARIANCES[c], out.data_ptr(), N, M, D, Mp, stream),
                    "fill")

        # the two forms compute the same matrix (up to the rounding of the order of operations): checked once, on 4096 rows
        fused(4)
        ref = torch.ones((4096, M), dtype=torch.float64, device=dev)
        for c in range(4):
            single(c, K2)
            ref *= K2[:4096, :M].double()
        err = float((K[:4096, :M].double() - ref).abs().max() / ref.abs().max())
        say(f"{sfx}: fused (C = 4) against the product of four plain fills, first 4096 rows: max abs difference / max = {err:.2e}")

        variants = {("fused", C): (lambda C=C: fused(C)) for C in range(1, 5)}
        for C in range(1, 5):
            variants[("sum", C)] = (lambda C=C: summed(C))
        for c in range(4):
            variants[("plain", c)] = (lambda c=c: single(c, K if c == 0 else K2))
        variants[("mul", 0)] = lambda: K.mul_(K2)

        # the gradient: U = randn in the engine's layout, g0, g1, beta of order 1
        U = torch.randn((Np, Mp), generator=torch.Generator(device=dev).manual_seed(1), dtype=dtype, device=dev)
        g0 = torch.randn(Np, generator=torch.Generator(device=dev).manual_seed(2), dtype=dtype, device=dev)
        g1 = torch.randn(Np, generator=torch.Generator(device=dev).manual_seed(3), dtype=dtype, device=dev)
        beta = torch.randn(M, generator=torch.Generator(device=dev).manual_seed(4), dtype=dtype, device=dev)
        zpart = torch.empty((nrb, Mp, Dp), dtype=torch.float64, device=dev)
        lpart = torch.empty((nrb, ncb, 4, Dp), dtype=torch.float64, device=dev)
        vpart = torch.empty((nrb, ncb), dtype=torch.float64, device=dev)

        def gfused(C):
            kinds = (ctypes.c_int * C)(*KINDS[:C])
            B.check(grad_prod(kinds, X.data_ptr(), Z.data_ptr(), inv_ls.data_ptr(), prodvar(C), U.data_ptr(), Mp, g0.data_ptr(),
                              g1.data_ptr(), 1, beta.data_ptr(), 1, N, M, D, C, zpart.data_ptr(), lpart.data_ptr(), vpart.data_ptr(),
                              stream), "grad_prod")

        def gsingle(c):
            B.check(grad(KINDS[c], X.data_ptr(), Z.data_ptr(), inv_ls[c].data_ptr(), VARIANCES[c], U.data_ptr(), Mp, g0.data_ptr(),
                         g1.data_ptr(), 1, beta.data_ptr(), 1, N, M, D, zpart.data_ptr(), lpart.data_ptr(), vpart.data_ptr(), stream),
                    "grad")

        for C in range(1, 5):
            variants[("gfused", C)] = (lambda C=C: gfused(C))
        for c in range(4):
            variants[("gsingle", c)] = (lambda c=c: gsingle(c))

        times = {k: [] for k in variants}
        for rep in range(a.warmup + a.repeats):
            for k, fn in variants.items():
                t = timed(fn)
                if rep >= a.warmup:
                    times[k].append(t)
        med = {k: statistics.median(v) for k, v in times.items()}
        say(f"{sfx}: output {gb:.2f} GB")
        for c in range(4):
            say(f"  plain fill, component {c} (kind {KINDS[c]}):  {fmt(times[('plain', c)])}")
        say(f"  torch.mul_ of two [Np, Mp] buffers:  {fmt(times[('mul', 0)])}")
        for C in range(1, 5):
            split = sum(med[("plain", c)] for c in range(C)) + (C - 1) * med[("mul", 0)]
            f = med[("fused", C)]
            say(f"  fill C = {C}: fused {fmt(times[('fused', C)])}  {gb / f:.2f} TB/s written;  sum fill {fmt(times[('sum', C)])}  "
                f"fused / sum = {f / med[('sum', C)]:.3f};  split (medians summed) {split:8.3f} ms  split / fused = {split / f:.2f}")
        for c in range(4):
            say(f"  single-kernel gradient, component {c} (kind {KINDS[c]}):  {fmt(times[('gsingle', c)])}")
        for C in range(1, 5):
            singles = sum(med[("gsingle", c)] for c in range(C))
            f = med[("gfused", C)]
            say(f"  grad C = {C}: fused {fmt(times[('gfused', C)])}  {gb / f:.2f} TB/s of U read;  C single launches (medians summed) "
                f"{singles:8.3f} ms  singles / fused = {singles / f:.2f}")
        del K, K2, U
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
