"""The input gradient of the marginal prediction beside the M-step gradient kernel and beside torch autograd (HIP events; writes
profiles/predict_vjp_bench.txt).

Two shapes, X = randn, Z = X[:M], SE kernel with unit lengthscales, a t_SVGP after two E-steps on 65536 rows:

    fp64   N* = 1e6, M = 1024, D = 8
    C3     N* = 1e6, M = 1024, D = 16, fp32 compute dtype

(a) the launch alone, on the same (N, M, D) operands (K(X, Z) filled, U = K Q in the engine's buffer):
        moments_vjp     ``EStepEngine.moments_vjp``  (``tsvgp_moments_vjp_*``)
        kernel_grad     ``EStepEngine.kernel_grad``  (``tsvgp_kernel_grad_*``, the allocation of its partials and their host sums)
    as engine calls, and each C-ABI launch ALONE between the engine's own events (``EStepEngine.profile``): the launch-to-launch
    ratio is taken from those; and the time N Mp sizeof(T) bytes of U take at 8 TB/s.
(b) ``predict_f`` with a Xnew that requires grad (forward) and ``backward`` of (mean cm + var cv).sum(), and the backward's
    split into its fill, its GEMM U = K Q and the vjp launch (``EStepEngine.profile`` events for the two kernels, events around a
    stand-alone ``torch.mm`` of the same operands for the GEMM).
(c) forward + backward beside torch autograd through the same sums written in torch ops (the profile of the expanded squared
    distance, mean = K beta, var = variance - rowsum((K Q) * K)) in chunks of ``--chunk`` rows, the largest that fit for torch.

Warm-up calls, then ``--repeats`` calls of each, interleaved in one process, every call between two events on the stream; median
and range.  Wall-clock times of a device that sets its own clock under load: ratios within one run are steadier than the times.

    python tools/bench_predict_vjp.py [--rows 1000000] [--m 1024] [--chunk 65536] [--warmup 1] [--repeats 5]
                                      [--out profiles/predict_vjp_bench.txt]
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


def torch_forward_backward(X, Z, inv_ls, variance, beta, Q, cm, cv, chunk):
    """dX [N, D] fp64 by torch autograd through the dense formulas in the dtype of X, ``chunk`` rows at a time."""
    zt = Z * inv_ls
    z2 = (zt * zt).sum(dim=1)
    dX = torch.empty_like(X)
    for r in range(0, X.shape[0], chunk):
        Xc = X[r:r + chunk].detach().requires_grad_()
        xt = Xc * inv_ls
        s = ((xt * xt).sum(dim=1)[:, None] + z2[None, :] - 2.0 * (xt @ zt.t())).clamp_min(0.0)
        K = variance * torch.exp(-0.5 * s)  # [R, M]
        mean = K @ beta
        var = variance - ((K @ Q) * K).sum(dim=1, keepdim=True)
        (mean * cm[r:r + chunk] + var * cv[r:r + chunk]).sum().backward()
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
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_vjp_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N, M = a.rows, a.m
    say(f"# tools/bench_predict_vjp.py: N* = {N}, M = {M}, SE kernel, X = randn, Z = X[:M]; torch autograd in chunks of {a.chunk} rows")
    say(f"# per line: median (min .. max) of {a.repeats} calls after {a.warmup} warm-up call(s), interleaved, HIP events around each call; "
        "wall-clock times at the device's own clock: compare within this run")
    for tag, D, T in (("fp64 D=8", 8, torch.float64), ("C3 fp32 D=16", 16, torch.float32)):
        rng = np.random.RandomState(0)
        Xh = rng.randn(N, D)
        Yh = np.sin(Xh @ rng.randn(D, 1)) + np.sqrt(0.1) * rng.randn(N, 1)
        model = p.t_SVGP(p.SquaredExponential(1.0, 1.0), p.Gaussian(0.1), Xh[:M].copy(), num_data=65536, compute_dtype=T)
        for _ in range(2):
            model.natgrad_step((Xh[:65536], Yh[:65536]), lr=0.8)
        eng = model._get_engine()
        kernel = model.kernel
        X = torch.as_tensor(Xh, device=dev)
        Xc = X.to(T)
        Z = model._Z()
        cm, cv = torch.as_tensor(rng.randn(N, 1), device=dev), torch.as_tensor(rng.randn(N, 1), device=dev)
        beta, Q = model._predict_operands()
        beta, Q = beta.clone(), Q.clone()
        Np, Mp = p._backend.round_up(N), p._backend.round_up(M)
        esz = 8 if T == torch.float64 else 4
        # (a) operands in the engine's buffers
        Kfu, U = eng._get("Kfu", (Np, Mp), T), eng._get("U", (Np, Mp), T)
        eng.se_fill(Xc, Z.to(T), kernel.inv_lengthscales(D, T, dev), kernel.variance.item(), Kfu, kernel.kind)
        Qp = torch.zeros((Mp, Mp), dtype=T, device=dev)
        Qp[:M, :M] = Q[0]
        torch.mm(Kfu, Qp, out=U)
        cmT, cvT = torch.zeros((Np, 1), dtype=T, device=dev), torch.zeros((Np, 1), dtype=T, device=dev)
        cmT[:N], cvT[:N] = cm, cv
        dX = torch.empty((N, D), dtype=torch.float64, device=dev)
        Xg = X.clone().requires_grad_()
        split = {}

        def forward_backward():
            Xg.grad = None
            mean, var = model.predict_f(Xg)
            (mean * cm + var * cv).sum().backward()
            return Xg.grad

        def backward_profiled():
            """forward outside the events, backward with the engine's per-launch events on"""
            Xg.grad = None
            mean, var = model.predict_f(Xg)
            loss = (mean * cm + var * cv).sum()
            torch.cuda.synchronize()
            eng.profile = {}
            ms, _ = timed(loss.backward)
            for k, v in eng.profile_summary().items():
                split.setdefault(k, []).append(sum(v[5]))
            eng.profile = None
            return ms

        def launch_ms(name, fn):
            """the C-ABI launch inside ``fn`` alone: the engine's own events around it (no allocation, no host sum)"""
            eng.profile, eng.profile_only = {}, {name}
            fn()
            ms = sum(eng.profile_summary()[name][5])
            eng.profile, eng.profile_only = None, None
            return ms

        fns = {"moments_vjp": lambda: eng.moments_vjp(Xc, Z, kernel, U, cmT[:N, 0], cvT[:N, 0], beta[:, 0], dX),
               "kernel_grad": lambda: eng.kernel_grad(Xc, Z, kernel, U, cmT[:, 0], cvT[:, 0], beta[:, 0]),
               "gemm U = K Q": lambda: torch.mm(Kfu, Qp, out=U),
               "forward": lambda: model.predict_f(Xg),
               "forward+backward": forward_backward,
               "torch fwd+bwd": lambda: torch_forward_backward(Xc, Z.to(T), kernel.inv_lengthscales(D, T, dev), kernel.variance.item(),
                                                               beta.to(T), Q[0].to(T), cm.to(T), cv.to(T), a.chunk)}
        for fn in fns.values():
            for _ in range(a.warmup):
                fn()
        backward_profiled()
        split.clear()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        times["backward"], times["moments_vjp launch"], times["kernel_grad launch"] = [], [], []
        outs = {}
        for _ in range(a.repeats):
            for k, fn in fns.items():
                if k == "gemm U = K Q":
                    continue
                ms, outs[k] = timed(fn)
                times[k].append(ms)
            times["backward"].append(backward_profiled())
            times["moments_vjp launch"].append(launch_ms("tsvgp_moments_vjp", fns["moments_vjp"]))
            times["kernel_grad launch"].append(launch_ms("tsvgp_kernel_grad", fns["kernel_grad"]))
            # the GEMM last in the round: it rewrites U with the values the two launches above read (the same ones)
            ms, _ = timed(fns["gemm U = K Q"])
            times["gemm U = K Q"].append(ms)
        med = {k: statistics.median(ts) for k, ts in times.items()}
        for k, ts in times.items():
            say(f"{tag:13s} {k:18s} {med[k]:9.2f} ms ({min(ts):.2f} .. {max(ts):.2f})")
        for k, ts in sorted(split.items()):
            say(f"{tag:13s} backward: {k:22s} {statistics.median(ts):9.2f} ms ({min(ts):.2f} .. {max(ts):.2f})")
        floor = N * Mp * esz / 8e12 * 1e3
        kg = times["kernel_grad launch"]
        gap = float((outs["forward+backward"] - outs["torch fwd+bwd"].double()).abs().max())
        say(f"{tag:13s} launch alone: moments_vjp / kernel_grad = {med['moments_vjp launch'] / med['kernel_grad launch']:.3f} "
            f"(kernel_grad's own spread {(max(kg) - min(kg)) / med['kernel_grad launch']:.3f}); engine calls (kernel_grad with its "
            f"allocations and the host sums of its partials): {med['moments_vjp'] / med['kernel_grad']:.3f}; N Mp sizeof(T) bytes at "
            f"8 TB/s = {floor:.2f} ms, moments_vjp launch / that = {med['moments_vjp launch'] / floor:.2f}")
        say(f"{tag:13s} backward / forward = {med['backward'] / med['forward']:.3f}; forward+backward / torch fwd+bwd = "
            f"{med['forward+backward'] / med['torch fwd+bwd']:.3f}; max |dX - torch| = {gap:.2e} (max |dX| "
            f"{float(outs['forward+backward'].abs().max()):.2f})")
        del outs, model, eng, Kfu, U, X, Xc, Xg, Qp, dX
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
