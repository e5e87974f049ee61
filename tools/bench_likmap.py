"""Time of the scalar likelihood map (``tsvgp_lik_map_scalar_*``: StudentT, Poisson) beside ``tsvgp_lik_map_*`` (Bernoulli) on one
column of N rows, through the C-ABI (HIP events), and the HBM bandwidth each achieves against the 5 N sizeof(T) bytes the map has
to move (mean, var, Y in; g0, g1 out).

    python tools/bench_likmap.py [--rows 1000000] [--steps 50] [--warmup 5] [--out profiles/likmap_bench.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as p  # noqa: E402

B = p._backend


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = B.lib()
    N = a.rows
    Np = B.round_up(N)
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"likelihood maps on one column, N = {N}, {a.steps} timed calls after {a.warmup} (HIP events); bytes = 5 N sizeof(T)"]
    for dtype, sfx in ((torch.float64, "f64"), (torch.float32, "f32")):
        mean = torch.randn(N, 1, generator=g, device=dev, dtype=dtype)
        var = torch.rand(N, 1, generator=g, device=dev, dtype=dtype) * 2.0 + 0.05
        counts = torch.poisson(torch.exp(mean.double())).to(dtype)
        labels = (torch.rand(N, 1, generator=g, device=dev) < 0.5).to(dtype)
        g0, g1 = torch.empty(Np, 1, device=dev, dtype=dtype), torch.empty(Np, 1, device=dev, dtype=dtype)
        ve = torch.empty(Np // 128, device=dev, dtype=torch.float64)
        dpar = torch.empty(Np // 128, device=dev, dtype=torch.float64)
        bad = torch.empty(Np // 128, device=dev, dtype=torch.int32)
        s = torch.cuda.current_stream().cuda_stream
        scalar, plain = getattr(lib, f"tsvgp_lik_map_scalar_{sfx}"), getattr(lib, f"tsvgp_lik_map_{sfx}")
        calls = {
            "StudentT (scalar map)": lambda: scalar(mean.data_ptr(), var.data_ptr(), counts.data_ptr(), 1, B.LIK_STUDENT_T, 0.7, 3.0,
                                                    g0.data_ptr(), g1.data_ptr(), 1, ve.data_ptr(), dpar.data_ptr(), bad.data_ptr(), N,
                                                    Np, s),
            "Poisson (scalar map)": lambda: scalar(mean.data_ptr(), var.data_ptr(), counts.data_ptr(), 1, B.LIK_POISSON, 1.0, 0.0,
                                                   g0.data_ptr(), g1.data_ptr(), 1, ve.data_ptr(), None, bad.data_ptr(), N, Np, s),
            "Bernoulli (tsvgp_lik_map)": lambda: plain(mean.data_ptr(), var.data_ptr(), labels.data_ptr(), B.LIK_BERNOULLI, 0.0,
                                                       g0.data_ptr(), g1.data_ptr(), ve.data_ptr(), bad.data_ptr(), N, Np, 1, s),
        }
        nbytes = 5 * N * mean.element_size()
        for name, call in calls.items():
            for _ in range(a.warmup):
                B.check(call(), name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                B.check(call(), name)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.steps
            lines.append(f"{sfx} {name:28s} {ms * 1e3:9.1f} us   {nbytes / ms / 1e6:8.1f} GB/s")
    if 5 * N * 8 < 256 * 2 ** 20:
        lines.append("(the arrays of one call fit the 256 MiB Infinity Cache and the timed calls repeat on them: a figure above the "
                     "HBM rate is cache bandwidth)")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
