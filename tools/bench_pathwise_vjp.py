"""The input gradient of the pathwise draws beside the value kernel and beside torch autograd (HIP events; writes
profiles/pathwise_vjp_bench.txt).

At N* = 1e6, M = 1024, D = 8, L in {1024, 4096}, S in {1, 16}, Matern-5/2 kernel, X = randn, per (L, S):

    value        ``EStepEngine.pathwise``      (``tsvgp_pathwise_f64`` alone: the yardstick, measured in the same run)
    vjp          ``EStepEngine.pathwise_vjp``  (``tsvgp_pathwise_vjp_f64`` alone)
    fs fwd       ``fs(X)`` with X requiring grad (the autograd Function's forward: the value launch and the stack)
    fs fwd+bwd   the same and ``f.backward(C)``
    torch fwd+bwd  the same sum written in torch (``torch.cos`` / ``torch.sin`` / ``torch.mm`` as tools/bench_pathwise.py has it, and
                 the Matern-5/2 profile of the expanded squared distance in torch ops, since the HIP fill carries no graph), forward
                 and ``backward(C)`` in chunks of ``--chunk`` rows: the [chunk, L] and [chunk, M] arrays autograd keeps are the
                 N-sized operands the kernels do not have.

Warm-up calls, then ``--repeats`` calls of each, interleaved in one process, every call between two events on the stream; median
and range.  Clocks: the numbers are wall-clock times of a device that sets its own clock under load; ratios taken within one run
are steadier than the times themselves, and a difference of a few per cent between two runs is not a finding.

    python tools/bench_pathwise_vjp.py [--rows 1000000] [--m 1024] [--dim 8] [--features 1024 4096] [--samples 1 16]
                                       [--chunk 65536] [--warmup 1] [--repeats 5] [--out profiles/pathwise_vjp_bench.txt]
"""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tsvgp_amd as p  # noqa: E402


def torch_forward_backward(X, Z, inv_ls, variance, Omega, W, V, C, chunk):
    """dX [N, D] by torch autograd through the torch formulation of the Matern-5/2 draw, ``chunk`` rows at a time."""
    L = Omega.shape[0]
    zt = Z * inv_ls
    z2 = (zt * zt).sum(dim=1)
    Wc, Ws = W[:, :L].contiguous(), W[:, L:].contiguous()
    dX = torch.empty_like(X)
    for r in range(0, X.shape[0], chunk):
        Xc = X[r:r + chunk].detach().requires_grad_()
        xt = Xc * inv_ls
        arg = xt @ Omega.t()  # [R, L]
        s2 = ((xt * xt).sum(dim=1)[:, None] + z2[None, :] - 2.0 * (xt @ zt.t())).clamp_min(1e-36)
        a = math.sqrt(5.0) * torch.sqrt(s2)
        K = variance * (1.0 + a + (5.0 / 3.0) * s2) * torch.exp(-a)  # [R, M]
        f = Wc @ torch.cos(arg).t() + Ws @ torch.sin(arg).t() + V @ K.t()  # [S, R]
        f.backward(C[:, r:r + chunk])
        dX[r:r + chunk] = Xc.grad
    return dX


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pathwise_vjp_bench.txt"))
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
    inv_ls = kernel.inv_lengthscales(D, torch.float64, dev)
    say(f"# tools/bench_pathwise_vjp.py: N* = {N}, M = {M}, D = {D}, Matern-5/2 kernel, X = randn, fp64; torch autograd in chunks of "
        f"{a.chunk} rows")
    say(f"# per line: median (min .. max) of {a.repeats} calls after {a.warmup} warm-up call(s), interleaved, HIP events around each call; "
        "wall-clock times at the device's own clock: compare within this run")
    for L in a.features:
        Omega = p.pathwise.spectral_frequencies(engine, kernel.kind, 0, 0, L, D)
        for S in a.samples:
            W = torch.as_tensor(rng.randn(S, 2 * L) * np.sqrt(1.3 / L), device=dev)
            V = torch.as_tensor(rng.randn(S, M), device=dev)
            C = torch.as_tensor(rng.randn(S, N), device=dev)
            C3 = C[:, :, None].contiguous()
            fs = p.FunctionSamples(engine, [kernel], Z, [Omega], W[None], V[:, :, None], torch.zeros((S, M, 1), device=dev), seed=0, draw=0)
            Xg = X.clone().requires_grad_()

            def fs_forward_backward():
                Xg.grad = None
                fs(Xg).backward(C3)
                return Xg.grad

            fns = {"value": lambda: engine.pathwise(X, Z, kernel, Omega, W, V),
                   "vjp": lambda: engine.pathwise_vjp(X, Z, kernel, Omega, W, V, C),
                   "fs fwd": lambda: fs(Xg),
                   "fs fwd+bwd": fs_forward_backward,
                   "torch fwd+bwd": lambda: torch_forward_backward(X, Z, inv_ls, 1.3, Omega, W, V, C, a.chunk)}
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
            med = {k: statistics.median(ts) for k, ts in times.items()}
            for k, ts in times.items():
                say(f"L = {L:5d} S = {S:3d} {k:14s} {med[k]:9.2f} ms ({min(ts):.2f} .. {max(ts):.2f})")
            same = torch.equal(outs["vjp"], outs["fs fwd+bwd"])
            gap = float((outs["vjp"] - outs["torch fwd+bwd"]).abs().max())
            say(f"L = {L:5d} S = {S:3d} vjp / value = {med['vjp'] / med['value']:.3f}, fs fwd+bwd / fs fwd = "
                f"{med['fs fwd+bwd'] / med['fs fwd']:.3f}, fs fwd+bwd / torch fwd+bwd = {med['fs fwd+bwd'] / med['torch fwd+bwd']:.3f}; "
                f"autograd gives the launch's bits: {same}; max |vjp - torch| = {gap:.2e} (max |dX| {float(outs['vjp'].abs().max()):.2f})")
            del outs, fs, Xg
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
