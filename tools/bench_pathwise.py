"""The pathwise evaluation kernel beside the same sum composed from existing pieces (HIP events; writes profiles/pathwise_bench.txt).

``EStepEngine.pathwise`` (``tsvgp_pathwise_f64``: one thread per row, no N-sized operand) at N* = 1e6, M = 1024, D = 8,
L in {1024, 4096}, S in {1, 16}, Matern-5/2 kernel, X = randn; and beside it the baseline, the same sum from code that was
there before the kernel: ``tsvgp_kernel_fill_f64`` for K(X, Z), ``torch.mm`` for the arguments Omega . x~, ``torch.cos`` /
``torch.sin`` and ``torch.mm`` for the weighted sums, in row chunks (``--chunk`` rows: the [chunk, L] feature arrays are the
N-sized operands the kernel does not have).  Warm-up calls, then ``--repeats`` calls of each, interleaved in one process, every
call between two events on the stream; median and range.  The work the sum needs, counted from the shapes: N L sine / cosine
pairs, N M kernel-profile evaluations and N (L + M) (D + 2 S) multiply-adds (D per argument or distance, 2 S per frequency -- S
per inducing point is counted as 2 S as well); each is printed over the kernel's time.

    python tools/bench_pathwise.py [--rows 1000000] [--m 1024] [--dim 8] [--features 1024 4096] [--samples 1 16] [--chunk 65536]
                                   [--warmup 1] [--repeats 5] [--out profiles/pathwise_bench.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tsvgp_amd as p  # noqa: E402


def composed(engine, X, Z, kernel, Omega, W, V, chunk):
    """out [S, N] from the fill, torch.cos / torch.sin and torch.mm, ``chunk`` rows at a time."""
    N, D = X.shape
    M, L = Z.shape[0], Omega.shape[0]
    inv_ls = kernel.inv_lengthscales(D, torch.float64, X.device)
    Kfu = torch.empty((p._backend.round_up(min(chunk, N)), p._backend.round_up(M)), dtype=torch.float64, device=X.device)
    out = torch.empty((W.shape[0], N), dtype=torch.float64, device=X.device)
    Ot, Wc, Ws = (Omega * inv_ls).t().contiguous(), W[:, :L].contiguous(), W[:, L:].contiguous()
    for r in range(0, N, chunk):
        Xc = X[r:r + chunk]
        R = Xc.shape[0]
        engine.se_fill(Xc, Z, inv_ls, kernel.variance.item(), Kfu, kernel.kind)
        arg = Xc @ Ot  # [R, L]
        o = out[:, r:r + R]
        torch.mm(Wc, torch.cos(arg).t(), out=o)
        o.addmm_(Ws, torch.sin(arg).t())
        o.addmm_(V, Kfu[:R, :M].t())
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--features", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathwise_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N, M, D = a.rows, a.m, a.dim
    rng = np.random.RandomState(0)
    kernel = p.Matern52(variance=1.3, lengthscales=np.linspace(1.0, 1.5, D))
    X = torch.as_tensor(rng.randn(N, D), device=dev)
    Z = X[:M].clone()
    engine = p.estep.EStepEngine(torch.float64, dev)
    say(f"# tools/bench_pathwise.py: N* = {N}, M = {M}, D = {D}, Matern-5/2 kernel, X = randn, fp64; baseline in chunks of {a.chunk} rows")
    say(f"# per line: median (min .. max) of {a.repeats} calls after {a.warmup} warm-up call(s), the two interleaved, HIP events around each call")
    for L in a.features:
        Omega = p.pathwise.spectral_frequencies(engine, kernel.kind, 0, 0, L, D)
        for S in a.samples:
            W = torch.as_tensor(rng.randn(S, 2 * L) * np.sqrt(1.3 / L), device=dev)
            V = torch.as_tensor(rng.randn(S, M), device=dev)
            fns = {"hip": lambda: engine.pathwise(X, Z, kernel, Omega, W, V),
                   "composed": lambda: composed(engine, X, Z, kernel, Omega, W, V, a.chunk)}
            for fn in fns.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in fns}
            outs = {}
            for _ in range(a.repeats):
                for k, fn in fns.items():
                    ms, outs[k] = timed(fn)
                    times[k].append(ms)
            gap = float((outs["hip"] - outs["composed"]).abs().max())
            sincos, prof, fma = float(N) * L, float(N) * M, float(N) * (L + M) * (D + 2 * S)
            for k, ts in times.items():
                med = statistics.median(ts)
                say(f"L = {L:5d} S = {S:3d} {k:9s} {med:9.2f} ms ({min(ts):.2f} .. {max(ts):.2f})  {sincos / med / 1e6:8.1f} G sincos/s, "
                    f"{prof / med / 1e6:8.1f} G profiles/s, {fma / med / 1e6:9.1f} G multiply-adds/s")
            say(f"L = {L:5d} S = {S:3d} hip / composed = {statistics.median(times['hip']) / statistics.median(times['composed']):.3f}, "
                f"max |hip - composed| = {gap:.2e} (max |value| {float(outs['composed'].abs().max()):.2f})")
            del outs
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
