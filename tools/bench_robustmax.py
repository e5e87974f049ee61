"""The MultiClass / RobustMax map beside the Softmax map (HIP events; writes profiles/robustmax_bench.txt).

Both maps on the same moments at N = 1e6 rows, C in {3, 10}, fp64 and fp32 arrays, through the C-ABI alone (no model around
them): ``tsvgp_lik_map_robustmax_*`` (20 nodes x (C - 1) classes of erf and exp per row, evaluated twice) and
``tsvgp_lik_map_softmax_*`` (S = 100 in-kernel draws x C classes of exp per row).  Warm-up calls, then ``--calls`` calls between
two events, repeated ``--repeats`` times, the two maps interleaved window by window in one process; median and range per call,
and the bytes each call moves (4 N C elements in and out) against the time.

    python tools/bench_robustmax.py [--rows 1000000] [--calls 10] [--warmup 3] [--repeats 5] [--out profiles/robustmax_bench.txt]
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


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robustmax_bench.txt"))
    a = ap.parse_args()
    B = p._backend
    lib = B.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N = a.rows
    Np = B.round_up(N)
    say(f"# tools/bench_robustmax.py: N = {N}, the maps alone through the C-ABI; mean ~ 1.5 randn, var log-uniform in [1e-4, 4]")
    say(f"# per line: median (min .. max) per call of {a.repeats} windows of {a.calls} calls after {a.warmup} warm-up calls, HIP events")
    rng = np.random.RandomState(0)
    for C in (3, 10):
        mean64 = torch.as_tensor(1.5 * rng.randn(N, C), device=dev)
        var64 = torch.as_tensor(np.exp(rng.uniform(np.log(1e-4), np.log(4.0), (N, C))), device=dev)
        y64 = torch.as_tensor(rng.randint(0, C, (N, 1)).astype(np.float64), device=dev)
        state = torch.tensor([1, 0], dtype=torch.int64, device=dev)
        ve = torch.empty(Np // B.TILE, dtype=torch.float64, device=dev)
        nonpos = torch.empty(Np // B.TILE, dtype=torch.int32, device=dev)
        for dtype in (torch.float64, torch.float32):
            sfx = B.suffix(dtype)
            mean, var, y = mean64.to(dtype), var64.to(dtype), y64.to(dtype)
            g0, g1 = torch.empty((Np, C), dtype=dtype, device=dev), torch.empty((Np, C), dtype=dtype, device=dev)
            ptrs = (mean.data_ptr(), var.data_ptr(), y.data_ptr())
            outs = (g0.data_ptr(), g1.data_ptr(), ve.data_ptr(), nonpos.data_ptr())
            robust, soft = getattr(lib, f"tsvgp_lik_map_robustmax_{sfx}"), getattr(lib, f"tsvgp_lik_map_softmax_{sfx}")
            maps = {
                "robustmax": lambda: B.check(robust(*ptrs, B.LIK_MULTICLASS, C, 1e-3, *outs, N, Np, stream), "tsvgp_lik_map_robustmax"),
                "softmax": lambda: B.check(soft(*ptrs, B.LIK_SOFTMAX, C, 100, state.data_ptr(), 0, None, *outs, N, Np, stream),
                                           "tsvgp_lik_map_softmax"),
            }
            for fn in maps.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in maps}
            for _ in range(a.repeats):  # interleaved: both maps see the same clock state window by window
                for k, fn in maps.items():
                    times[k].append(window(fn, a.calls))
            nbytes = (4 * N * C + N) * mean.element_size()
            for k, ts in times.items():
                med = statistics.median(ts)
                say(f"C = {C:2d} {str(dtype):14s} {k:10s} {med:9.4f} ms ({min(ts):.4f} .. {max(ts):.4f})  "
                    f"{nbytes / med / 1e6:8.1f} GB/s over {nbytes / 1e6:.0f} MB")
            say(f"C = {C:2d} {str(dtype):14s} robustmax / softmax = {statistics.median(times['robustmax']) / statistics.median(times['softmax']):.4f}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
