"""Time of one ``t_VGP.elbo_and_grads()`` beside ``elbo()`` alone and beside torch autograd through the same ELBO (HIP events).

Shapes: N = 4096, 8192, 16384 with D = 8, fp64, Gaussian likelihood, after two site updates.  Per N: warm-up calls, then
``--steps`` timed calls between two events, then one call with per-kernel events (EStepEngine.profile): the share of
``tsvgp_vgp_kernel_grad_f64`` in the call and its achieved bandwidth (it reads the lower block triangle of W [Np x Np] once)
against 8 TB/s.  The torch line is the reference's own sequence (tvgp.py:77-111) in torch ops on the device with
``requires_grad`` on the variance, the lengthscales and the noise variance, forward + backward.

    python tools/bench_tvgp_grad.py [--sizes 4096,8192,16384] [--steps 3] [--warmup 1] [--out profiles/tvgp_grad_bench.txt]
"""
import argparse
import json
import math
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


def torch_elbo(X, Y, l1, l2, variance, ls, s2, jitter=1e-6):
    """tvgp.py:77-111 in torch, Gaussian likelihood."""
    N = X.shape[0]
    Xs = X / ls
    sq = (Xs * Xs).sum(1)
    K = variance * torch.exp(-0.5 * torch.clamp(sq[:, None] + sq[None, :] - 2.0 * Xs @ Xs.T, min=0.0))
    K = K + jitter * torch.eye(N, dtype=K.dtype, device=K.device)
    sW = torch.sqrt(torch.abs(l2))
    pseudo_y = l1 / l2
    L = torch.linalg.cholesky((sW @ sW.T) * K + torch.eye(N, dtype=K.dtype, device=K.device))
    T = torch.linalg.solve_triangular(L, sW * K, upper=False)
    post_v = (K.diagonal() - (T * T).sum(dim=0)).reshape(N, 1)
    alpha = sW * torch.linalg.solve_triangular(L.T, torch.linalg.solve_triangular(L, sW * pseudo_y, upper=False), upper=True)
    post_m = K @ alpha
    ve = torch.sum(-0.5 * math.log(2.0 * math.pi) - 0.5 * torch.log(s2) - 0.5 * ((Y - post_m) ** 2 + post_v) / s2)
    eqt = -torch.sum(0.5 * l2 * ((pseudo_y - post_m) ** 2 + post_v))
    log_Z = -0.5 * (pseudo_y * alpha).sum() - torch.log(L.diagonal()).sum()
    return log_Z - eqt + ve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192,16384")
    ap.add_argument("--D", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tvgp_grad_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"# tools/bench_tvgp_grad.py: one t_VGP.elbo_and_grads(), D = {a.D}, fp64, Gaussian; {torch.cuda.get_device_name(dev)}; "
             f"steps = {a.steps}, warmup = {a.warmup}"]
    for N in (int(s) for s in a.sizes.split(",")):
        rng = np.random.RandomState(0)
        Xh = rng.randn(N, a.D)
        Yh = np.sin(Xh @ rng.randn(a.D, 1)) + np.sqrt(0.1) * rng.randn(N, 1)
        m = p.t_VGP((Xh, Yh), p.SquaredExponential(1.0, np.ones(a.D)), p.Gaussian(0.1), device=dev)
        for _ in range(2):
            m.update_variational_parameters(beta=0.5)
        elbo_ms = time_steps(m.elbo, a.steps, a.warmup)
        grad_ms = time_steps(m.elbo_and_grads, a.steps, a.warmup)
        eng = m._get_engine()
        eng.profile = {}
        elbo, grads = m.elbo_and_grads()
        prof = eng.profile_summary()
        eng.profile = None
        kern_ms = {k: round(sum(v[5]), 3) for k, v in prof.items()}
        Np = (N + 127) // 128 * 128
        kg = kern_ms.get("tsvgp_vgp_kernel_grad", 0.0)
        read = (Np // 128) * (Np // 128 + 1) // 2 * 128 * 128 * 8
        row = dict(model="t_VGP (HIP)", N=N, D=a.D, elbo_ms=round(elbo_ms, 3), elbo_and_grads_ms=round(grad_ms, 3), kernels_ms=kern_ms,
                   kernel_grad_share=round(kg / grad_ms, 4), kernel_grad_TBps=round(read / (kg * 1e-3) / 1e12, 3) if kg > 0 else None)
        row["kernel_grad_fraction_of_8TBps"] = round(row["kernel_grad_TBps"] / HBM_TBS, 3) if kg > 0 else None
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
        l1, l2 = m.lambda_1.value.clone(), m.lambda_2.value.clone()
        hip = {k: v.detach().clone() for k, v in grads.items()}
        hip_elbo = float(elbo)
        del m, eng, grads
        torch.cuda.empty_cache()
        X, Y = torch.as_tensor(Xh, device=dev), torch.as_tensor(Yh, device=dev)
        par = [torch.tensor(1.0, dtype=torch.float64, device=dev, requires_grad=True),
               torch.ones(a.D, dtype=torch.float64, device=dev, requires_grad=True),
               torch.tensor(0.1, dtype=torch.float64, device=dev, requires_grad=True)]

        def tstep():
            for q in par:
                q.grad = None
            e = torch_elbo(X, Y, l1, l2, *par)
            e.backward()
            return e

        tms = time_steps(tstep, a.steps, a.warmup)
        e = tstep()
        diff = max(float((par[0].grad - hip["variance"]).abs() / hip["variance"].abs()),
                   float((par[1].grad - hip["lengthscales"]).abs().max() / hip["lengthscales"].abs().max()),
                   float((par[2].grad - hip["likelihood_variance"]).abs() / hip["likelihood_variance"].abs()))
        row = dict(model="torch autograd (linalg.cholesky + solve_triangular, forward + backward)", N=N, D=a.D,
                   elbo_and_grads_ms=round(tms, 3), grads_rel_diff_to_hip=float(f"{diff:.3e}"),
                   elbo_rel_diff_to_hip=float(f"{abs(float(e) - hip_elbo) / abs(hip_elbo):.3e}"))
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
        del X, Y, par, l1, l2, e
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
