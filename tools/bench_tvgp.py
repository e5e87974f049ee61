"""Time of one t_VGP update (``update_variational_parameters``) beside the same algebra in torch (HIP events).

Shapes: N = 4096, 8192, 16384 with D = 8, fp64, Gaussian likelihood.  Per N: warm-up updates, then ``--steps`` timed updates
between two events, then one update with per-kernel events (EStepEngine.profile): the system build, the factor-and-solve and
the row sweep, with the sweep's achieved bandwidth (it reads C [Np x Np] once) against 8 TB/s.  The torch line is the
reference's own sequence (tvgp.py:126-157) with ``torch.linalg.cholesky`` and ``solve_triangular`` on the device: K from the
difference form, B, L, T = L^-1 (s * K), alpha by two vector solves, the Gaussian site update.

    python tools/bench_tvgp.py [--sizes 4096,8192,16384] [--steps 3] [--warmup 1] [--out profiles/tvgp_bench.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tsvgp_amd as p  # noqa: E402

HBM_TBS = 8.0


def time_steps(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def torch_update(X, Y, l1, l2, variance, ls, s2, beta, jitter=1e-6):
    """tvgp.py:126-157 in torch, Gaussian likelihood; returns the new sites."""
    N = X.shape[0]
    Xs = X / ls
    K = variance * torch.exp(-0.5 * torch.cdist(Xs, Xs).square_())
    K.diagonal().add_(jitter)
    sW = torch.sqrt(torch.abs(l2))
    Bm = (sW @ sW.T) * K
    Bm.diagonal().add_(1.0)
    L = torch.linalg.cholesky(Bm)
    T = torch.linalg.solve_triangular(L, sW * K, upper=False)
    post_v = (K.diagonal() - (T * T).sum(dim=0)).reshape(N, 1)
    alpha = sW * torch.linalg.solve_triangular(L.T, torch.linalg.solve_triangular(L, sW * (l1 / l2), upper=False), upper=True)
    post_m = K @ alpha
    g0, g1 = (Y - post_m) / s2, -0.5 / s2
    return (1 - beta) * l1 + beta * (g0 - 2 * g1 * post_m), (1 - beta) * l2 + beta * (-2 * g1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192,16384")
    ap.add_argument("--D", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tvgp_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"# tools/bench_tvgp.py: one t_VGP update, D = {a.D}, fp64, Gaussian; {torch.cuda.get_device_name(dev)}; "
             f"steps = {a.steps}, warmup = {a.warmup}"]
    for N in (int(s) for s in a.sizes.split(",")):
        rng = np.random.RandomState(0)
        Xh = rng.randn(N, a.D)
        Yh = np.sin(Xh @ rng.randn(a.D, 1)) + np.sqrt(0.1) * rng.randn(N, 1)
        m = p.t_VGP((Xh, Yh), p.SquaredExponential(1.0, 1.0), p.Gaussian(0.1), device=dev)
        step = lambda: m.update_variational_parameters(beta=0.5)
        ms = time_steps(step, a.steps, a.warmup)
        eng = m._get_engine()
        eng.profile = {}
        step()
        prof = eng.profile_summary()
        eng.profile = None
        kern_ms = {k: round(sum(v[5]), 3) for k, v in prof.items()}
        Np = (N + 127) // 128 * 128
        rows_ms = kern_ms.get("tsvgp_vgp_rows", 0.0)
        row = dict(model="t_VGP (HIP)", N=N, D=a.D, update_ms=round(ms, 3), kernels_ms=kern_ms,
                   potrf_solve_TFLOPs=round((N ** 3 / 3 + N ** 3) / max(kern_ms.get("tsvgp_potrf", 0.0), 1e-9) / 1e9, 2),
                   rows_TBps=round(Np * Np * 8 / (rows_ms * 1e-3) / 1e12, 3) if rows_ms > 0 else None)
        row["rows_fraction_of_8TBps"] = round(row["rows_TBps"] / HBM_TBS, 3) if rows_ms > 0 else None
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
        l1n, l2n = m.lambda_1.value.clone(), m.lambda_2.value.clone()
        del m, eng, step
        torch.cuda.empty_cache()
        X, Y = torch.as_tensor(Xh, device=dev), torch.as_tensor(Yh, device=dev)
        ls = torch.ones(a.D, dtype=torch.float64, device=dev)
        state = [torch.zeros((N, 1), dtype=torch.float64, device=dev), torch.full((N, 1), 1e-6, dtype=torch.float64, device=dev)]

        def tstep():
            state[0], state[1] = torch_update(X, Y, state[0], state[1], 1.0, ls, 0.1, 0.5)

        tms = time_steps(tstep, a.steps, a.warmup)
        # both sides have now taken warmup + steps + 1 updates (the HIP side's profiled one): bring torch level and compare
        tstep()
        err = max(float((state[0] - l1n).abs().max() / l1n.abs().max()), float((state[1] - l2n).abs().max() / l2n.abs().max()))
        row = dict(model="torch (linalg.cholesky + solve_triangular)", N=N, D=a.D, update_ms=round(tms, 3),
                   sites_rel_diff_to_hip=float(f"{err:.3e}"))
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
        del X, Y, state
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
