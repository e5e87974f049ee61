"""k-means++ seeding on the device beside the same algorithm in torch, beside the greedy selection and beside its own floor
(writes profiles/kmeanspp_bench.txt).

``EStepEngine.kmeanspp`` (``tsvgp_kmeanspp_f64``) at N = 1e6, D = 8, M in {256, 512, 1024}, the default 2 + floor(ln M) trials per
centre, X = randn, fp64.  Around whole calls, between two events on the stream, everything of one M interleaved in one process:
the seeding call (2 M + 2 launches, no host read); the same algorithm in torch ops on the device, fed the same uniforms --
``cdist`` to the L candidates, ``minimum``, ``cumsum``, ``searchsorted``, no host read either; ``select_inducing_points`` at the
same shape (the other way to a good start: a kernel, O(N M^2) work and an N x M factor); and ``kmeans_inducing_points(max_iter=10)``
from X[:M], from the greedy selection and from the seeding, with the inertia each ends at.  The floor is what the algorithm cannot
avoid on this layout: (M - 1) rounds that each read X and read and write mind, 8 N (D + 2) bytes, at 8 TB/s, plus 2 M + 2 launches
at the cost of an empty launch measured in the same run (the call at N = 1, M = 1 -- four launches of one workgroup each --
enqueued back to back).  Warm-up calls, then ``--repeats`` of each; median and range.

    python tools/bench_kmeanspp.py [--rows 1000000] [--dim 8] [--m 256 512 1024] [--warmup 2] [--repeats 5] [--out profiles/kmeanspp_bench.txt]
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

HBM_BYTES_PER_S = 8.0e12


def torch_kmeanspp(Xs, u):
    """The seeding in torch on the scaled rows Xs = X * il with the uniforms u [M, L]: (indices [M], mind [N], pot).  No host read."""
    N = Xs.shape[0]
    M, L = u.shape
    idx = torch.empty((M,), dtype=torch.int64, device=Xs.device)
    i0 = (u[0, 0] * N).floor().to(torch.int64).clamp(max=N - 1)
    idx[0] = i0
    d = Xs - Xs[i0]
    mind = (d * d).sum(dim=1)
    pot = mind.sum()
    for r in range(1, M):
        cand = torch.searchsorted(torch.cumsum(mind, 0), u[r] * pot, right=True).clamp(max=N - 1)
        c = torch.cdist(Xs, Xs[cand])
        trial = torch.minimum(mind[:, None], c * c)
        pots = trial.sum(dim=0)
        js = torch.argmin(pots).view(1)
        mind, pot = trial.index_select(1, js)[:, 0], pots.index_select(0, js)[0]
        idx[r] = cand.index_select(0, js)[0]
    return idx, mind, pot


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeanspp_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N, D = a.rows, a.dim
    ls = np.linspace(1.0, 1.5, D)
    X = torch.as_tensor(np.random.RandomState(0).randn(N, D), device=dev)
    il = torch.as_tensor(1.0 / ls, device=dev)
    Xs = X * il
    kernel = p.SquaredExponential(variance=1.0, lengthscales=ls)
    engine = p.estep.EStepEngine(torch.float64, dev)
    tiny = X[:1].clone()

    def empty_launches(calls=256):
        for _ in range(calls):
            engine.kmeanspp(tiny, il, 1, 1, 0)

    say(f"# tools/bench_kmeanspp.py: N = {N}, D = {D}, X = randn, lengthscales linspace(1, 1.5, D), fp64, seed 0, L = 2 + floor(ln M)")
    say(f"# per line: median (min .. max) of {a.repeats} after {a.warmup} warm-up, everything of one M interleaved in one process;")
    say("# every time is taken between two events around the whole host call")
    for M in a.m:
        L = 2 + int(math.log(M))
        keys = ("hip", "torch", "greedy", "empty", "lloyd first", "lloyd greedy", "lloyd k-means++")
        ts = {k: [] for k in keys}
        for rep in range(a.warmup + a.repeats):
            ms_hip, out = timed(lambda: engine.kmeanspp(X, il, M, L, 0))
            ms_torch, tout = timed(lambda: torch_kmeanspp(Xs, out[5]))
            ms_sel, sel = timed(lambda: p.select_inducing_points(X, kernel, M))
            ms_empty, _ = timed(empty_launches)
            ms_l1, km_first = timed(lambda: p.kmeans_inducing_points(X, M, lengthscales=ls, max_iter=10))
            ms_l2, km_sel = timed(lambda: p.kmeans_inducing_points(X, M, init=sel, lengthscales=ls, max_iter=10))
            ms_l3, km_pp = timed(lambda: p.kmeans_inducing_points(X, M, init="k-means++", seed=0, lengthscales=ls, max_iter=10))
            if rep >= a.warmup:
                for k, v in zip(keys, (ms_hip, ms_torch, ms_sel, ms_empty / (256 * 4), ms_l1, ms_l2, ms_l3)):
                    ts[k].append(v)
        med = {k: statistics.median(v) for k, v in ts.items()}
        launches = 2 * M + 2
        traffic = (M - 1) * 8.0 * N * (D + 2) / HBM_BYTES_PER_S * 1e3
        floor = traffic + launches * med["empty"]
        same = int((tout[0] == out[0]).sum())
        say(f"M = {M:5d} L = {L} [call] tsvgp_kmeanspp_f64          {fmt(ts['hip'])}  {launches} launches, potential {float(out[2][-1]):.6e}")
        say(f"M = {M:5d} L = {L} [call] the same in torch           {fmt(ts['torch'])}  torch / hip = {med['torch'] / med['hip']:.2f}  "
            f"(potential {float(tout[2]):.6e}, {same} of {M} indices equal to hip's)")
        say(f"M = {M:5d} L = {L} [call] select_inducing_points      {fmt(ts['greedy'])}  greedy / hip = {med['greedy'] / med['hip']:.2f}")
        say(f"M = {M:5d} L = {L} floor: {traffic:.3f} ms of traffic ((M - 1) 8 N (D + 2) bytes at 8 TB/s) + {launches} launches at "
            f"{med['empty'] * 1e3:.2f} us (empty launch, {fmt(ts['empty'])}) = {floor:.3f} ms;  hip / floor = {med['hip'] / floor:.2f}")
        for name, key, km in (("X[:M]", "lloyd first", km_first), ("greedy", "lloyd greedy", km_sel), ("k-means++", "lloyd k-means++", km_pp)):
            say(f"M = {M:5d} L = {L} [call] kmeans_inducing_points(max_iter=10) from {name:9s} {fmt(ts[key])}  ({km.n_iter} iterations, "
                f"inertia {float(km.inertia):.6e})" + (" (the seeding included)" if name == "k-means++" else ""))
        del out, tout, sel, km_first, km_sel, km_pp
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
