"""The greedy inducing-point selection beside the same loop in torch (HIP events; writes profiles/select_bench.txt).

``EStepEngine.greedy_select`` (``tsvgp_greedy_select_f64``: 2 M launches, the factor transposed, one host read of the count) at
N = 1e6, D = 8, M in {256, 512, 1024}, squared-exponential kernel, X = randn; and beside it the same M steps written in torch on
the device, no HIP of this project: ``mv`` on a row-major factor [N, M], ``argmax``, gathers, no host read inside the loop (so
no stop test: the shapes here never meet it).  Warm-up calls, then ``--repeats`` calls of each, interleaved in one process, every
call between two events on the stream; median and range.  The bytes the algorithm has to move are the factor rows read back,
8 Np count^2 / 2; they are printed over the call time as a fraction of bench.py's HBM_PEAK_GBS.

    python tools/bench_select.py [--rows 1000000] [--dim 8] [--m 256 512 1024] [--warmup 1] [--repeats 3] [--out profiles/select_bench.txt]
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
from bench import HBM_PEAK_GBS  # noqa: E402


def torch_select(Xs, variance, M):
    """The selection loop in torch: Xs = X * inv_ls [N, D] on the device.  Returns (indices, pivots, d)."""
    N = Xs.shape[0]
    L = torch.empty((N, M), dtype=torch.float64, device=Xs.device)
    d = torch.full((N,), variance, dtype=torch.float64, device=Xs.device)
    idx = torch.empty(M, dtype=torch.int64, device=Xs.device)
    piv = torch.empty(M, dtype=torch.float64, device=Xs.device)
    for j in range(M):
        pj = torch.argmax(d).reshape(1)
        dp = d.index_select(0, pj)
        diff = Xs - Xs.index_select(0, pj)
        c = variance * torch.exp(-0.5 * (diff * diff).sum(dim=1))
        if j:
            c -= torch.mv(L[:, :j], L.index_select(0, pj)[0, :j])
        c /= torch.sqrt(dp)
        L[:, j] = c
        d = torch.clamp(d - c * c, min=0.0)
        d.index_fill_(0, pj, 0.0)
        idx[j:j + 1] = pj
        piv[j:j + 1] = dp
    return idx, piv, d


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
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--m", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N, D = a.rows, a.dim
    Np = p._backend.round_up(N)
    variance = 1.0
    kernel = p.SquaredExponential(variance=variance, lengthscales=np.linspace(1.0, 1.5, D))
    X = torch.as_tensor(np.random.RandomState(0).randn(N, D), device=dev)
    Xs = X * kernel.inv_lengthscales(D, torch.float64, dev)
    engine = p.estep.EStepEngine(torch.float64, dev)
    say(f"# tools/bench_select.py: N = {N}, D = {D}, SE kernel, X = randn, fp64; HBM_PEAK_GBS = {HBM_PEAK_GBS:.0f}")
    say(f"# per line: median (min .. max) of {a.repeats} calls after {a.warmup} warm-up call(s), the two interleaved, HIP events around each call")
    for M in a.m:
        fns = {"hip": lambda: engine.greedy_select(X, kernel, M), "torch": lambda: torch_select(Xs, variance, M)}
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
        count = outs["hip"][3]
        same = int((outs["hip"][0] == outs["torch"][0][:count]).sum()) if count == M else -1
        nbytes = 8.0 * Np * count * count / 2.0
        for k, ts in times.items():
            med = statistics.median(ts)
            say(f"M = {M:5d} {k:6s} {med:10.2f} ms ({min(ts):.2f} .. {max(ts):.2f})  {nbytes / 1e9:8.1f} GB of factor reads -> "
                f"{nbytes / med / 1e6:7.1f} GB/s = {nbytes / med / 1e6 / HBM_PEAK_GBS:.3f} of peak")
        say(f"M = {M:5d} count = {count}, last pivot {float(outs['hip'][1][-1]):.4f}, hip / torch = "
            f"{statistics.median(times['hip']) / statistics.median(times['torch']):.3f}, same picks as the torch loop: {same} of {count}")
        del outs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
