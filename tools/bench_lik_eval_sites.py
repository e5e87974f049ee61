"""Time of the launches that evaluate ``lik_eval`` (csrc/tsvgp_device.h) outside the moments kernels, Bernoulli likelihood (the arm
that reads the Gauss-Hermite tables), through the C-ABI with HIP events: ``tsvgp_lik_map_*`` and ``tsvgp_diag_site_step_*`` in both
types and ``tsvgp_vgp_rows_f64``.  One line per entry point: min / median / max over the timed launches.  For an A/B of two
builds run it once per build in a fresh process (``TSVGP_HIP_LIB=<library>``), alternating (profiles/split_units_ab.txt).

    python tools/bench_lik_eval_sites.py [--rows 1000000] [--steps 30] [--warmup 5]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as p  # noqa: E402

B = p._backend


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--vgp-rows", type=int, default=16384, help="N of the tsvgp_vgp_rows_f64 line (C is N x N)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = B.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(0)
    calls = {}
    keep = []  # the operands stay alive behind the lambdas
    N, Np = a.rows, B.round_up(a.rows)
    for dtype, sfx in ((torch.float64, "f64"), (torch.float32, "f32")):
        mean = torch.randn(N, 1, generator=g, device=dev, dtype=dtype)
        var = torch.rand(N, 1, generator=g, device=dev, dtype=dtype) * 2.0 + 0.05
        y = (torch.rand(N, 1, generator=g, device=dev) < 0.5).to(dtype)
        g0, g1 = torch.empty(Np, 1, device=dev, dtype=dtype), torch.empty(Np, 1, device=dev, dtype=dtype)
        l1, l2 = torch.zeros(Np, 1, device=dev, dtype=torch.float64), torch.full((Np, 1), -0.5, device=dev, dtype=torch.float64)
        l1c, l2c = l1.to(dtype), l2.to(dtype)
        ve = torch.empty(Np // 128, device=dev, dtype=torch.float64)
        bad = torch.empty(Np // 128, device=dev, dtype=torch.int32)
        keep += [mean, var, y, g0, g1, l1, l2, l1c, l2c, ve, bad]
        lik_map, site_step = getattr(lib, f"tsvgp_lik_map_{sfx}"), getattr(lib, f"tsvgp_diag_site_step_{sfx}")
        calls[f"tsvgp_lik_map_{sfx}"] = lambda f=lik_map, m=mean, v=var, y=y, g0=g0, g1=g1, ve=ve, bad=bad: f(
            m.data_ptr(), v.data_ptr(), y.data_ptr(), B.LIK_BERNOULLI, 0.0, g0.data_ptr(), g1.data_ptr(), ve.data_ptr(), bad.data_ptr(),
            N, Np, 1, s)
        extra = () if dtype == torch.float64 else (l1c.data_ptr(), l2c.data_ptr())
        calls[f"tsvgp_diag_site_step_{sfx}"] = lambda f=site_step, m=mean, v=var, y=y, l1=l1, l2=l2, ve=ve, bad=bad, extra=extra: f(
            m.data_ptr(), v.data_ptr(), y.data_ptr(), B.LIK_BERNOULLI, 0.0, 0.5, l1.data_ptr(), l2.data_ptr(), *extra, ve.data_ptr(),
            bad.data_ptr(), N, Np, 1, s)
    Nv = a.vgp_rows
    Nvp = B.round_up(Nv)
    C = torch.randn(Nvp, Nvp, generator=g, device=dev, dtype=torch.float64) * (0.5 / Nvp ** 0.5)  # q ~ 0.25 < kdiag
    z = torch.randn(Nvp, generator=g, device=dev, dtype=torch.float64)
    yv = (torch.rand(Nv, generator=g, device=dev) < 0.5).double()
    l1v, l2v = torch.zeros(Nvp, device=dev, dtype=torch.float64), torch.full((Nvp,), -0.5, device=dev, dtype=torch.float64)
    vev, eqt = torch.empty(Nvp // 128, device=dev, dtype=torch.float64), torch.empty(Nvp // 128, device=dev, dtype=torch.float64)
    badv = torch.empty(Nvp // 128, device=dev, dtype=torch.int32)
    calls["tsvgp_vgp_rows_f64"] = lambda: lib.tsvgp_vgp_rows_f64(
        C.data_ptr(), Nvp, z.data_ptr(), yv.data_ptr(), l1v.data_ptr(), l2v.data_ptr(), 4.0, B.LIK_BERNOULLI, 0.0, 0.0, None, None,
        vev.data_ptr(), eqt.data_ptr(), badv.data_ptr(), Nv, Nvp, Nvp, s)  # beta = 0: the sites are not written
    print(f"{os.environ.get('TSVGP_HIP_LIB', B.LIB_PATH)}: Bernoulli, N = {N} (vgp_rows: {Nv}), {a.steps} timed launches after "
          f"{a.warmup}, HIP events, microseconds")
    for name, call in calls.items():
        for _ in range(a.warmup):
            B.check(call(), name)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        for e0, e1 in ev:
            e0.record()
            B.check(call(), name)
            e1.record()
        torch.cuda.synchronize()
        us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
        print(f"  {name:28s} min {us[0]:9.1f}  median {statistics.median(us):9.1f}  max {us[-1]:9.1f}", flush=True)


if __name__ == "__main__":
    main()
