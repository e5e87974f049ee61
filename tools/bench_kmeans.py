"""Lloyd's k-means for inducing points beside the same loop in torch and beside the K(X, Z) fill (writes profiles/kmeans_bench.txt).

``EStepEngine.kmeans_assign`` / ``kmeans_update`` (``tsvgp_kmeans_assign_f64``, ``tsvgp_kmeans_update_f64``) at N = 1e6, D = 8,
M in {256, 512, 1024}, X = randn, C = X[:M], fp64.  Kernel times are taken between the engine's own events (``engine.profile``):
the assignment launch, the update launch alone, and ``tsvgp_kernel_fill_f64`` at the same (N, M, D) -- the same distance
arithmetic plus an exp and an N x M store.  Around whole calls, between two events on the stream: ``kmeans_update`` with its
stable sort, bincount and cumsum; ``kmeans_inducing_points(max_iter=10)`` (on this data ten iterations and the closing
assignment, one host read per iteration); and the same loop in torch on the device, no HIP of this project -- ``cdist`` over
row chunks, ``argmin``, ``index_add_`` -- whose centres depend on the order its atomics land in.  Warm-up calls, then
``--repeats`` of each, interleaved in one process; median and range.  The assignment's arithmetic is 3 N M D fp64 operations
(a subtraction and a fused multiply-add per coordinate, the latter counted twice); the rate is printed beside the time.

    python tools/bench_kmeans.py [--rows 1000000] [--dim 8] [--m 256 512 1024] [--warmup 2] [--repeats 5] [--out profiles/kmeans_bench.txt]
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

TORCH_CHUNK = 65536  # rows per cdist block of the torch loop: 0.5 GB of distances at M = 1024


def torch_iteration(Xs, X, Cs):
    """One Lloyd iteration in torch: Xs = X * il, Cs = C * il.  Returns (labels, inertia, C_new in original coordinates)."""
    N, M = Xs.shape[0], Cs.shape[0]
    labels = torch.empty((N,), dtype=torch.int64, device=Xs.device)
    best = torch.empty((N,), dtype=torch.float64, device=Xs.device)
    for a in range(0, N, TORCH_CHUNK):
        d = torch.cdist(Xs[a:a + TORCH_CHUNK], Cs)
        best[a:a + TORCH_CHUNK], labels[a:a + TORCH_CHUNK] = torch.min(d, dim=1)
    sums = torch.zeros((M, X.shape[1]), dtype=torch.float64, device=Xs.device).index_add_(0, labels, X)
    counts = torch.bincount(labels, minlength=M)
    return labels, (best * best).sum(), sums / counts.clamp(min=1)[:, None]


def torch_lloyd(X, il, C, iters):
    Xs = X * il
    for _ in range(iters):
        labels, inertia, Cn = torch_iteration(Xs, X, C * il)
        C = Cn
    labels, inertia, _ = torch_iteration(Xs, X, C * il)
    return C, labels, inertia


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--m", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N, D = a.rows, a.dim
    Np = p._backend.round_up(N)
    ls = np.linspace(1.0, 1.5, D)
    X = torch.as_tensor(np.random.RandomState(0).randn(N, D), device=dev)
    il = torch.as_tensor(1.0 / ls, device=dev)
    engine = p.estep.EStepEngine(torch.float64, dev)
    say(f"# tools/bench_kmeans.py: N = {N}, D = {D}, X = randn, C = X[:M], lengthscales linspace(1, 1.5, D), fp64")
    say(f"# per line: median (min .. max) of {a.repeats} after {a.warmup} warm-up, everything of one M interleaved in one process;")
    say("# [kernel]: between the engine's events around the launch; [call]: two events around the whole host call")
    for M in a.m:
        C = X[:M].clone()
        Mp = p._backend.round_up(M)
        K = torch.empty((Np, Mp), dtype=torch.float64, device=dev)
        labels0 = engine.kmeans_assign(X, C, il)[0]
        ev = {k: [] for k in ("assign", "update", "fill")}
        calls = {k: [] for k in ("update+sort", "hip 10 it", "torch 1 it", "torch 10 it")}
        Xs = X * il
        for rep in range(a.warmup + a.repeats):
            engine.profile = {}
            engine.kmeans_assign(X, C, il)
            ms_upd, (C1, counts) = timed(lambda: engine.kmeans_update(X, labels0, C))
            engine.se_fill(X, C, il, 1.0, K)
            prof = engine.profile_summary()
            engine.profile = None
            ms_hip, res = timed(lambda: p.kmeans_inducing_points(X, M, lengthscales=ls, max_iter=10))
            ms_t1, tout = timed(lambda: torch_iteration(Xs, X, C * il))
            ms_t10, tres = timed(lambda: torch_lloyd(X, il, C, 10))
            if rep < a.warmup:
                continue
            ev["assign"].append(prof["tsvgp_kmeans_assign"][1])
            ev["update"].append(prof["tsvgp_kmeans_update"][1])
            ev["fill"].append(prof["tsvgp_se_fill"][1])
            for k, v in zip(calls, (ms_upd, ms_hip, ms_t1, ms_t10)):
                calls[k].append(v)
        ops = 3.0 * N * M * D
        med = {k: statistics.median(v) for k, v in {**ev, **calls}.items()}
        say(f"M = {M:5d} [kernel] assignment          {fmt(ev['assign'])}  {ops / med['assign'] / 1e9:7.2f} Tflop/s fp64 (3 N M D operations)")
        say(f"M = {M:5d} [kernel] K(X, Z) fill        {fmt(ev['fill'])}  assignment / fill = {med['assign'] / med['fill']:.3f}")
        say(f"M = {M:5d} [kernel] update              {fmt(ev['update'])}")
        say(f"M = {M:5d} [call]   update with sort    {fmt(calls['update+sort'])}")
        say(f"M = {M:5d} [call]   torch, 1 iteration  {fmt(calls['torch 1 it'])}  torch / (assignment + update with sort) = "
            f"{med['torch 1 it'] / (med['assign'] + med['update+sort']):.2f}")
        say(f"M = {M:5d} [call]   kmeans_inducing_points(max_iter=10): {fmt(calls['hip 10 it'])}  ({res.n_iter} iterations, converged "
            f"{res.converged}, inertia {float(res.inertia):.6e})")
        say(f"M = {M:5d} [call]   torch, 10 iterations + closing pass:  {fmt(calls['torch 10 it'])}  torch / hip = "
            f"{med['torch 10 it'] / med['hip 10 it']:.2f}  (inertia {float(tres[2]):.6e}, labels equal to hip: "
            f"{int((tres[1] == res.labels).sum())} of {N})")
        # what the first assignment gives, against the torch iteration's (the two agree unless a row sits on a rounding-level tie)
        same = int((tout[0] == labels0.to(torch.int64)).sum())
        say(f"M = {M:5d} first assignment equal to torch's argmin on {same} of {N} rows; smallest cluster {int(counts.min())} rows")
        del K, res, tres, tout
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
