"""Time of the two LinearCoregionalization launches (``tsvgp_lmc_mix_*``, ``tsvgp_lmc_unmix_*``) at N rows, through the C-ABI: each
launch alone between two HIP events, at (L, P) = (2, 8) and (8, 8), fp64 and fp32 arrays, and the HBM bandwidth it achieves
against the bytes it has to move -- 2 N (L + P) sizeof(T) for either launch (mix: mean_g, var_g in, Fmu, Fvar out; un-mix:
g0_f, g1_f in, g0_g, g1_g out) -- and against 8 TB/s.  Then one E-step (``natgrad_step``, eager) at the C5 shape (M = 1024, D = 8,
P = 8 Gaussian outputs) with ``LinearCoregionalization`` over L = 2 latents beside ``SeparateIndependent`` with one latent per
output, in the same run.

    python tools/bench_lmc.py [--rows 1000000] [--steps 50] [--warmup 5] [--estep-steps 5] [--out profiles/lmc_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as p  # noqa: E402

B = p._backend
HBM_BYTES_PER_S = 8e12


def _median_us(call, name, steps, warmup):
    for _ in range(warmup):
        B.check(call(), name)
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in events:
        e0.record()
        B.check(call(), name)
        e1.record()
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in events)
    return us[len(us) // 2], us[0], us[-1]


def launches(a, dev, lines):
    lib = B.lib()
    N = a.rows
    Np = B.round_up(N)
    g = torch.Generator(device=dev).manual_seed(0)
    s = torch.cuda.current_stream().cuda_stream
    for L, P in ((2, 8), (8, 8)):
        W = torch.randn(P, L, generator=g, device=dev, dtype=torch.float64)
        for dtype, sfx in ((torch.float64, "f64"), (torch.float32, "f32")):
            mean_g = torch.randn(N, L, generator=g, device=dev, dtype=dtype)
            var_g = torch.rand(N, L, generator=g, device=dev, dtype=dtype) + 0.05
            Fmu, Fvar = torch.empty(N, P, device=dev, dtype=dtype), torch.empty(N, P, device=dev, dtype=dtype)
            g0_f, g1_f = torch.zeros(Np, P, device=dev, dtype=dtype), torch.zeros(Np, P, device=dev, dtype=dtype)
            g0_f[:N].normal_(generator=g)
            g1_f[:N].normal_(generator=g)
            g0_g, g1_g = torch.empty(Np, L, device=dev, dtype=dtype), torch.empty(Np, L, device=dev, dtype=dtype)
            bad = torch.empty(Np // 128, device=dev, dtype=torch.int32)
            part = torch.empty(Np // 128, P, L, device=dev, dtype=torch.float64)
            mix, unmix = getattr(lib, f"tsvgp_lmc_mix_{sfx}"), getattr(lib, f"tsvgp_lmc_unmix_{sfx}")
            calls = {
                "mix": lambda: mix(mean_g.data_ptr(), var_g.data_ptr(), W.data_ptr(), Fmu.data_ptr(), Fvar.data_ptr(), bad.data_ptr(),
                                   N, Np, L, P, s),
                "un-mix": lambda: unmix(g0_f.data_ptr(), g1_f.data_ptr(), W.data_ptr(), 0, g0_g.data_ptr(), g1_g.data_ptr(), None, None,
                                        None, N, Np, L, P, s),
                "un-mix + dW": lambda: unmix(g0_f.data_ptr(), g1_f.data_ptr(), W.data_ptr(), B.LIK_NOCROP, g0_g.data_ptr(),
                                             g1_g.data_ptr(), mean_g.data_ptr(), var_g.data_ptr(), part.data_ptr(), N, Np, L, P, s),
            }
            esz = mean_g.element_size()
            for name, call in calls.items():
                # (the dW form reads every input a second time for the block sums and writes N / 128 P L doubles)
                nbytes = 2 * N * (L + P) * esz + ((2 * N * (L + P)) * esz + (Np // 128) * P * L * 8 if "dW" in name else 0)
                floor_us = nbytes / HBM_BYTES_PER_S * 1e6
                med, lo, hi = _median_us(call, name, a.steps, a.warmup)
                lines.append(f"L={L} P={P} {sfx} {name:12s} {med:9.1f} us ({lo:.1f} .. {hi:.1f})   {nbytes / med / 1e3:8.1f} GB/s   "
                             f"{med / floor_us:6.1f} x the {floor_us:.1f} us of 8 TB/s")
    if 2 * N * 16 * 8 < 256 * 2 ** 20:
        lines.append("(the arrays of one call fit the 256 MiB Infinity Cache and the timed calls repeat on them: a figure above the "
                     "HBM rate would be cache bandwidth)")


def esteps(a, dev, lines):
    N, M, D, P, L = a.rows, a.m, 8, 8, 2
    rng = np.random.RandomState(0)
    X = rng.randn(N, D)
    Wgen = rng.randn(P, L)
    Y = np.sin(X @ rng.randn(D, L)) @ Wgen.T + np.sqrt(0.1) * rng.randn(N, P)
    Z = X[:M].copy()
    Xd, Yd = torch.as_tensor(X, device=dev), torch.as_tensor(Y, device=dev)
    kern = lambda n: [p.SquaredExponential(1.0, float(l)) for l in np.linspace(0.8, 1.5, n)]
    models = {
        f"LinearCoregionalization, L = {L} latents": (p.LinearCoregionalization(kern(L), Wgen), L),
        f"SeparateIndependent, {P} latents": (p.SeparateIndependent(kern(P)), P),
    }
    lines.append(f"one eager natgrad_step, N = {N}, M = {M}, D = {D}, P = {P} Gaussian outputs, fp64: median of {a.estep_steps} after 2 "
                 f"warm-up steps, between two HIP events around the call (which ends with the step's own status read)")
    for name, (kernel, nl) in models.items():
        m = p.t_SVGP(kernel, p.Gaussian(0.1), p.SharedIndependentInducingVariables(Z), num_latent_gps=nl, num_data=N, device=dev,
                     use_graph=False)
        ms = []
        for i in range(2 + a.estep_steps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m.natgrad_step((Xd, Yd), lr=0.8)
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        ms.sort()
        med = ms[len(ms) // 2]
        lines.append(f"{name:44s} {med:9.2f} ms ({ms[0]:.2f} .. {ms[-1]:.2f})   {1e3 / med:7.2f} E-steps/s   batched launches: "
                     f"{m._get_engine().last_batched}")
        del m
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--estep-steps", type=int, default=5)
    ap.add_argument("--no-estep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"LinearCoregionalization launches, N = {a.rows}; each of {a.steps} timed launches alone between two HIP events after "
             f"{a.warmup} warm-up launches: median (min .. max); HBM peak taken as 8 TB/s"]
    launches(a, dev, lines)
    if not a.no_estep:
        esteps(a, dev, lines)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
