"""E-step time of the heteroskedastic likelihood against the Gaussian one on the same two-latent model (HIP events).

N = 1e6, M = 1024, D = 8, P = 2 with one SE kernel per latent (SeparateIndependent), fp64 by default: the notebook's model
(reference docs/notebooks/heteroskedastic.py:58-76) at the headline size.  Per path (batched launches / one pass per latent)
and likelihood: warm-up steps, then ``--steps`` timed E-steps between two events, then one step with per-kernel events
(EStepEngine.profile) for the share of the coupled map (tsvgp_lik_map_hetero) and of the fills.

    python tools/bench_hetero.py [--rows 1000000] [--M 1024] [--D 8] [--steps 5] [--warmup 2] [--f32] [--paths batched,perlatent]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as p  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--D", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--f32", action="store_true")
    ap.add_argument("--paths", default="batched,perlatent")
    ap.add_argument("--liks", default="gaussian,hetero")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.RandomState(0)
    N, M, D = a.rows, a.M, a.D
    X = torch.as_tensor(rng.randn(N, D), device=dev)
    f = torch.sin(X @ torch.as_tensor(rng.randn(D, 2), device=dev))
    Yh = (f[:, :1] + torch.exp(0.3 * f[:, 1:]) * torch.randn(N, 1, device=dev, dtype=torch.float64)).contiguous()
    Yg = (f + 0.3 * torch.randn(N, 2, device=dev, dtype=torch.float64)).contiguous()
    Z = X[:M].cpu().numpy().copy()
    dtype = torch.float32 if a.f32 else torch.float64
    out = []
    for path in a.paths.split(","):
        for lik in a.liks.split(","):
            kern = p.SeparateIndependent([p.SquaredExponential(1.0, 1.0), p.SquaredExponential(0.5, 1.0)])
            L = p.HeteroskedasticTFPConditional() if lik == "hetero" else p.Gaussian(0.1)
            Y = Yh if lik == "hetero" else Yg
            m = p.t_SVGP(kern, L, p.SharedIndependentInducingVariables(Z), num_latent_gps=2, num_data=N, compute_dtype=dtype,
                         device=dev, use_graph=False)
            eng = m._get_engine()
            eng.batch_separate = path == "batched"
            for _ in range(a.warmup):
                m.natgrad_step((X, Y), lr=0.5)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                m.natgrad_step((X, Y), lr=0.5)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.steps
            eng.profile = {}
            m.natgrad_step((X, Y), lr=0.5)
            kern_ms = {k: (v[0], round(sum(v[5]), 4)) for k, v in eng.profile_summary().items()}
            eng.profile = None
            row = dict(path=path, lik=lik, batched=eng.last_batched, routes=m._routes(1e-9), N=N, M=M, D=D, dtype=str(dtype),
                       step_ms=round(ms, 3), kernels_ms=kern_ms)
            print(json.dumps(row), flush=True)
            out.append(row)
            del m, eng
            torch.cuda.empty_cache()
    for path in a.paths.split(","):
        rows = {r["lik"]: r for r in out if r["path"] == path}
        if "gaussian" in rows and "hetero" in rows:
            g, h = rows["gaussian"]["step_ms"], rows["hetero"]["step_ms"]
            print(f"{path}: hetero {h:.3f} ms / gaussian {g:.3f} ms = {h / g:.4f}", flush=True)


if __name__ == "__main__":
    main()
