"""E-step time of the Softmax likelihood (HIP events; writes profiles/softmax_bench.txt).

1. One E-step at N = 1e6, M = 1024, D = 8, C = 10, S = 100, one shared Matern-5/2 kernel, fp64 and fp32, eager, beside the same
   shape with the Gaussian likelihood and P = 10 (the yardstick): warm-up steps, then ``--steps`` timed steps between two events,
   repeated ``--repeats`` times (median and range reported); then one step with per-kernel events (EStepEngine.profile) for the
   map's own time and its share of the step.
2. The generator alone: ``tsvgp_mc_normals`` on the SAME number of draws (S * N * C = 1e9) as 100 launches of one sample
   (S = 1, N = 1e6, C = 10) each, all into ONE scratch slice of 1e7 values (80 MB in fp64, not the 8 GB array): the generator's
   arithmetic plus an 80 MB store per launch, which the map does not pay -- an upper bound on the generator's part of the map.
3. The MNIST-shaped step: N = 200, M = 100, D = 784, C = 10, eager and graph-replayed.

    python tools/bench_softmax.py [--rows 1000000] [--M 1024] [--steps 5] [--warmup 2] [--repeats 3] [--out profiles/softmax_bench.txt]
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


def timed(fn, steps, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--D", type=int, default=8)
    ap.add_argument("--C", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.RandomState(0)
    N, M, D, C = a.rows, a.M, a.D, a.C
    X = torch.as_tensor(rng.randn(N, D), device=dev)
    scores = X @ torch.as_tensor(rng.randn(D, C), device=dev) + 0.5 * torch.randn(N, C, device=dev, dtype=torch.float64)
    Ys = scores.argmax(dim=1, keepdim=True).to(torch.float64).contiguous()
    Yg = torch.sin(scores).contiguous()
    Z = X[:M].cpu().numpy().copy()
    say(f"# tools/bench_softmax.py: N = {N}, M = {M}, D = {D}, C = P = {C}, S = 100, one shared Matern-5/2 kernel, eager steps")
    say(f"# per line: median (min .. max) of {a.repeats} windows of {a.steps} steps after {a.warmup} warm-up steps, HIP events")
    for dtype in (torch.float64, torch.float32):
        res = {}
        for lik in ("gaussian", "softmax"):
            L = p.Softmax(C, seed=1) if lik == "softmax" else p.Gaussian(0.1)
            Y = Ys if lik == "softmax" else Yg
            m = p.t_SVGP(p.Matern52(1.0, 2.0), L, Z, num_latent_gps=C, num_data=N, compute_dtype=dtype, device=dev, use_graph=False)
            res[lik] = timed(lambda: m.natgrad_step((X, Y), lr=0.1), a.steps, a.warmup, a.repeats)
            eng = m._get_engine()
            eng.profile = {}
            m.natgrad_step((X, Y), lr=0.1)
            prof = {k: round(sum(v[5]), 4) for k, v in eng.profile_summary().items()}
            eng.profile = None
            med, lo, hi = res[lik]
            say(f"{str(dtype):14s} {lik:8s} step {med:9.3f} ms ({lo:.3f} .. {hi:.3f})  routes {m._routes(1e-9)[0]}")
            say(f"    per-kernel events of one more step [ms]: {prof}")
            if lik == "softmax":
                mp_ms = prof.get("tsvgp_lik_map_softmax", float("nan"))
                say(f"    map tsvgp_lik_map_softmax: {mp_ms:.3f} ms = {100 * mp_ms / med:.1f} % of the step; the rest {med - mp_ms:.3f} ms")
            del m, eng
            torch.cuda.empty_cache()
        say(f"{str(dtype):14s} softmax / gaussian = {res['softmax'][0] / res['gaussian'][0]:.4f}")
        # the generator alone: S launches of one sample into one scratch slice
        lik = p.Softmax(C, seed=1)
        lik.num_monte_carlo_points = 1

        def gen():
            for _ in range(100):
                lik.normals(N, dtype, dev)

        med, lo, hi = timed(gen, 1, 1, a.repeats)
        say(f"{str(dtype):14s} generator alone: 100 x tsvgp_mc_normals(S = 1, N = {N}, C = {C}) into one {N * C * (8 if dtype == torch.float64 else 4) / 1e6:.0f} MB "
            f"slice: {med:.3f} ms ({lo:.3f} .. {hi:.3f}) for {100 * N * C:.2e} draws (includes 100 stores of the slice, which the map does not pay: an upper bound on the draws' part of the map)")
    del X, Ys, Yg, scores
    torch.cuda.empty_cache()
    # the MNIST-shaped step
    N2, M2, D2 = 200, 100, 784
    X2 = torch.as_tensor(rng.rand(N2 + M2, D2), device=dev)
    Y2 = torch.as_tensor(rng.randint(0, C, (N2, 1)).astype(np.float64), device=dev)
    Z2 = X2[N2:].cpu().numpy().copy()
    X2 = X2[:N2].contiguous()
    say(f"# MNIST-shaped step: N = {N2}, M = {M2}, D = {D2}, C = {C}, Matern-5/2 ARD, fp64, num_data = 60000")
    for graph in (False, True):
        m = p.t_SVGP(p.Matern52(1.0, np.full(D2, 28.0)), p.Softmax(C, seed=1), Z2, num_latent_gps=C, num_data=60000, device=dev,
                     use_graph=graph)
        med, lo, hi = timed(lambda: m.natgrad_step((X2, Y2), lr=0.03), 200, 5, a.repeats)
        captured = any(isinstance(e, dict) for e in m._graphs.values())
        say(f"{'graph replay' if graph else 'eager':14s} step {med:9.4f} ms ({lo:.4f} .. {hi:.4f}){'' if captured == graph else '  (NOT captured)'}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
