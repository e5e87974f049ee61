"""The fused fill of a Sum kernel beside the split form it replaces (writes profiles/sumfill_bench.txt).

N = 1e6, M = 1024, D = 8, fp64 and fp32, C = 1 .. 4 components (kinds SE, Matern-3/2, Matern-5/2, SE in this order, each with its
own lengthscales; X = randn, Z = X[:M]):

  fused   one ``tsvgp_kernel_fill_sum_*`` launch
  split   C ``tsvgp_kernel_fill_*`` launches (component 0 into K, every other one into a second buffer) plus C - 1
          ``torch.add_`` of the two buffers: what the sum costs without the fused kernel
  plain   ``tsvgp_kernel_fill_*`` of component 0 alone, beside the fused fill at C = 1

Every launch is timed ALONE between two events on an otherwise idle stream, with a device synchronisation in front; warm-up
launches first, then ``--repeats`` of each, the variants interleaved round by round; medians and ranges.  The split form's time
is the sum of its launches' medians (nothing overlaps: each waits for the one before it through the same buffers).

    python tools/bench_sumfill.py [--rows 1000000] [--m 1024] [--dim 8] [--warmup 3] [--repeats 50] [--out profiles/sumfill_bench.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sumfill_bench.txt"))
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

    say(f"tools/bench_sumfill.py: {torch.cuda.get_device_name(dev)}, N = {N}, M = {M}, D = {D}; each launch alone between two "
        f"events, {a.warmup} warm-up, median (min .. max) of {a.repeats}")
    g = torch.Generator(device="cpu").manual_seed(0)
    X64 = torch.randn(N, D, generator=g, dtype=torch.float64)
    ls64 = 0.7 + torch.rand(4, D, generator=g, dtype=torch.float64)
    for dtype, sfx, ct in ((torch.float64, "f64", ctypes.c_double), (torch.float32, "f32", ctypes.c_float)):
        X = X64.to(dev, dtype).contiguous()
        Z = X[:M].clone()
        inv_ls = (1.0 / ls64).to(dev, dtype).contiguous()  # [4, D]
        K = torch.empty((Np, Mp), dtype=dtype, device=dev)
        K2 = torch.empty((Np, Mp), dtype=dtype, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        fill_sum, fill = getattr(lib, f"tsvgp_kernel_fill_sum_{sfx}"), getattr(lib, f"tsvgp_kernel_fill_{sfx}")
        gb = Np * Mp * K.element_size() / 1e9

        def fused(C, out=K):
            kinds, var = (ctypes.c_int * C)(*KINDS[:C]), (ct * C)(*VARIANCES[:C])
            B.check(fill_sum(kinds, X.data_ptr(), Z.data_ptr(), inv_ls.data_ptr(), var, out.data_ptr(), N, M, D, Mp, C, stream), "fused")

        def single(c, out):
            B.check(fill(KINDS[c], X.data_ptr(), Z.data_ptr(), inv_ls[c].data_ptr(), VARIANCES[c], out.data_ptr(), N, M, D, Mp, stream),
                    "fill")

        # the two forms compute the same matrix (up to the rounding of the order of operations): checked once, on 4096 rows
        fused(4)
        ref = torch.zeros((4096, M), dtype=torch.float64, device=dev)
        for c in range(4):
            single(c, K2)
            ref += K2[:4096, :M].double()
        err = float((K[:4096, :M].double() - ref).abs().max() / ref.abs().max())
        say(f"{sfx}: fused (C = 4) against the sum of four plain fills, first 4096 rows: max abs difference / max = {err:.2e}")

        variants = {("fused", C): (lambda C=C: fused(C)) for C in range(1, 5)}
        for c in range(4):
            variants[("plain", c)] = (lambda c=c: single(c, K if c == 0 else K2))
        variants[("add", 0)] = lambda: K.add_(K2)
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
        say(f"  torch.add_ of two [Np, Mp] buffers:  {fmt(times[('add', 0)])}")
        for C in range(1, 5):
            split = sum(med[("plain", c)] for c in range(C)) + (C - 1) * med[("add", 0)]
            f = med[("fused", C)]
            say(f"  C = {C}: fused {fmt(times[('fused', C)])}  {gb / f:.2f} TB/s written;  split (medians summed) "
                f"{split:8.3f} ms;  split / fused = {split / f:.2f}")
        say(f"  C = 1: fused / plain = {med[('fused', 1)] / med[('plain', 0)]:.3f}")
        del K, K2
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
