"""Time of the Ordinal map (``tsvgp_lik_map_ordinal_*``) and of the Gamma arm of ``tsvgp_lik_map_scalar_*`` beside the StudentT arm
of the same entry, in one run on one column of N rows, through the C-ABI: each launch alone between two HIP events, and the HBM
bandwidth it achieves against the 5 N sizeof(T) bytes the map has to move (mean, var, Y in; g0, g1 out) and against 8 TB/s.
The Ordinal map evaluates the 20 nodes StudentT evaluates, with two erfc, two exp and a log per node where StudentT has a log1p
and two divisions: it is expected to be of StudentT's order, not of the closed forms'.

    python tools/bench_ordinal.py [--rows 1000000] [--bins 5] [--steps 50] [--warmup 5] [--out profiles/ordinal_bench.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as p  # noqa: E402

B = p._backend
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--bins", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = B.lib()
    N, K = a.rows, a.bins
    Np = B.round_up(N)
    g = torch.Generator(device=dev).manual_seed(0)
    edges = torch.linspace(-2.0, 2.0, K - 1, dtype=torch.float64, device=dev)
    lines = [f"likelihood maps on one column, N = {N}, Ordinal over {K} bins; each of {a.steps} timed launches alone between two HIP "
             f"events after {a.warmup} warm-up launches: median (min .. max); bytes = 5 N sizeof(T), HBM peak taken as 8 TB/s"]
    for dtype, sfx in ((torch.float64, "f64"), (torch.float32, "f32")):
        mean = torch.randn(N, 1, generator=g, device=dev, dtype=dtype)
        var = torch.rand(N, 1, generator=g, device=dev, dtype=dtype) * 2.0 + 0.05
        labels = torch.randint(0, K, (N, 1), generator=g, device=dev).to(dtype)
        amounts = torch.exp(torch.randn(N, 1, generator=g, device=dev, dtype=torch.float64)).to(dtype)
        g0, g1 = torch.empty(Np, 1, device=dev, dtype=dtype), torch.empty(Np, 1, device=dev, dtype=dtype)
        ve = torch.empty(Np // 128, device=dev, dtype=torch.float64)
        dpar = torch.empty(Np // 128, device=dev, dtype=torch.float64)
        bad = torch.empty(Np // 128, device=dev, dtype=torch.int32)
        s = torch.cuda.current_stream().cuda_stream
        scalar, ordinal = getattr(lib, f"tsvgp_lik_map_scalar_{sfx}"), getattr(lib, f"tsvgp_lik_map_ordinal_{sfx}")
        outs = (ve.data_ptr(), dpar.data_ptr(), bad.data_ptr(), N, Np, s)
        calls = {
            f"Ordinal, {K} bins": lambda: ordinal(mean.data_ptr(), var.data_ptr(), labels.data_ptr(), 1, B.LIK_ORDINAL, edges.data_ptr(),
                                                  K - 1, 0.7, g0.data_ptr(), g1.data_ptr(), 1, *outs),
            "Gamma (scalar map)": lambda: scalar(mean.data_ptr(), var.data_ptr(), amounts.data_ptr(), 1, B.LIK_GAMMA, 2.5, 0.0,
                                                 g0.data_ptr(), g1.data_ptr(), 1, *outs),
            "StudentT (scalar map)": lambda: scalar(mean.data_ptr(), var.data_ptr(), amounts.data_ptr(), 1, B.LIK_STUDENT_T, 0.7, 3.0,
                                                    g0.data_ptr(), g1.data_ptr(), 1, *outs),
        }
        nbytes = 5 * N * mean.element_size()
        floor_us = nbytes / HBM_BYTES_PER_S * 1e6
        for name, call in calls.items():
            for _ in range(a.warmup):
                B.check(call(), name)
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
            for e0, e1 in events:
                e0.record()
                B.check(call(), name)
                e1.record()
            torch.cuda.synchronize()
            us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in events)
            med = us[len(us) // 2]
            lines.append(f"{sfx} {name:24s} {med:9.1f} us ({us[0]:.1f} .. {us[-1]:.1f})   {nbytes / med / 1e3:8.1f} GB/s   "
                         f"{med / floor_us:6.1f} x the {floor_us:.1f} us of 8 TB/s")
    if 5 * N * 8 < 256 * 2 ** 20:
        lines.append("(the arrays of one call fit the 256 MiB Infinity Cache and the timed calls repeat on them: a figure above the "
                     "HBM rate would be cache bandwidth)")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
