"""Time of the joint-covariance kernel ``tsvgp_cov_*`` against the composition its pieces allow without it (HIP events).

At N* in {2048, 8192}, M = 1024, D = 8, both array types, on the same [Np x Mp] tile T:
    fused:        tsvgp_cov_*(T) -> C = K(X*, X*) - T T^T                              (one launch, lower block triangle + mirror)
    composition:  tsvgp_kernel_fill_*(X*, X*) -> K;  torch.addmm(K, T, T^T, alpha=-1)   (a fill, a full GEMM, three passes over N*^2)
Each variant: ``--warmup`` launches, then ``--reps`` timed launches between two events; median of ``--rounds`` such rounds, the
two variants alternating.  Useful flops = N*^2 Mp (half the products of the full GEMM, two flops each), against the matrix peaks
78.6 (fp64) / 157.3 (fp32) TFLOP/s.  Then end to end on a trained t_SVGP: predict_f(full_cov=True) and
predict_f_samples(S = 100), wall time around a synchronisation.

    python tools/bench_fullcov.py [--out profiles/fullcov_bench.txt] [--sizes 2048,8192] [--M 1024] [--D 8]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
p = importlib.import_module("t-svgp_amd")
B = p._backend
estep = importlib.import_module("t-svgp_amd.estep")
PEAK = {torch.float64: 78.6e12, torch.float32: 157.3e12}


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "fullcov_bench.txt"))
    ap.add_argument("--sizes", default="2048,8192")
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--D", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"tsvgp_cov_* against kernel_fill + addmm; M = {a.M}, D = {a.D}; median of {a.rounds} rounds of {a.reps} launches",
             f"device: {torch.cuda.get_device_name(dev)}; library: {B.lib().tsvgp_version().decode()}"]
    rng = np.random.RandomState(0)
    for dtype in (torch.float64, torch.float32):
        eng = estep.EStepEngine(dtype, dev)
        for N in [int(s) for s in a.sizes.split(",")]:
            Np, Mp = B.round_up(N), B.round_up(a.M)
            X = torch.as_tensor(rng.randn(N, a.D), dtype=dtype, device=dev)
            inv_ls = torch.ones(a.D, dtype=dtype, device=dev)
            T = torch.zeros((Np, Mp), dtype=dtype, device=dev)
            T[:N] = torch.as_tensor(rng.randn(N, Mp) / np.sqrt(2 * Mp), dtype=dtype, device=dev)
            C, K = torch.empty((Np, Np), dtype=dtype, device=dev), torch.empty((Np, Np), dtype=dtype, device=dev)
            out = torch.empty((Np, Np), dtype=dtype, device=dev)
            fused = lambda: eng.cov(T, C, N, sign=-1.0, X=X, inv_ls=inv_ls, variance=1.0, kind=B.KERNEL_SE)

            def composed():
                eng.se_fill(X, X, inv_ls, 1.0, K, B.KERNEL_SE)
                torch.addmm(K, T, T.t(), alpha=-1.0, out=out)

            tf, tc = [], []
            for _ in range(a.rounds):
                tf.append(timed(fused, a.warmup, a.reps))
                tc.append(timed(composed, a.warmup, a.reps))
            err = float((C[:N, :N] - out[:N, :N]).abs().max())
            mf, mc = statistics.median(tf), statistics.median(tc)
            frac = N * N * Mp / (mf * 1e-3) / PEAK[dtype]
            lines.append(f"{B.suffix(dtype)} N* = {N}: fused {mf:.4f} ms (min {min(tf):.4f}, max {max(tf):.4f}; {frac:.3f} of the matrix peak "
                         f"on N*^2 Mp flops), fill + addmm {mc:.4f} ms (min {min(tc):.4f}, max {max(tc):.4f}), ratio "
                         f"{mc / mf:.3f}; max |difference| {err:.2e}")
            print(lines[-1], flush=True)
            del T, C, K, out
        del eng
        torch.cuda.empty_cache()
    # end to end
    Ntr = 20000
    Xtr = rng.randn(Ntr, a.D)
    Ytr = np.sin(Xtr @ rng.randn(a.D, 1)) + 0.3 * rng.randn(Ntr, 1)
    for dtype in (torch.float64, torch.float32):
        m = p.t_SVGP(p.SquaredExponential(1.0, 2.0), p.Gaussian(0.1), Xtr[:a.M].copy(), compute_dtype=dtype, device=dev)
        for _ in range(2):
            m.natgrad_step((Xtr, Ytr), lr=0.8)
        for N in [int(s) for s in a.sizes.split(",")]:
            Xs = torch.as_tensor(rng.randn(N, a.D), device=dev)
            res = {}
            for name, fn in (("predict_f(full_cov=True)", lambda: m.predict_f(Xs, full_cov=True)),
                             ("predict_f_samples(S=100)", lambda: m.predict_f_samples(Xs, 100, draw=0))):
                fn()
                ts = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                res[name] = statistics.median(ts)
            lines.append(f"{B.suffix(dtype)} N* = {N}, M = {a.M}: " + ", ".join(f"{k} {v:.2f} ms" for k, v in res.items()))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
