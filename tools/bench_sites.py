"""E-step time of t_SVGP_sites beside t_SVGP_white and t_SVGP on the same data (HIP events).

Shapes: the headline (N = 1e6, M = 1024, D = 8, fp64, Gaussian) and C3 (D = 16, Bernoulli, fp32).  Per model: warm-up
steps, then ``--steps`` timed E-steps between two events, then one step with per-kernel events (EStepEngine.profile) for the
share of the site map (tsvgp_diag_site_step) and its achieved bandwidth against 8 TB/s.  t_SVGP_sites runs with and without
``skip_unused_variance`` (Gaussian only).  The map's traffic per row: mean, var, Y in the compute dtype, the two fp64 sites
read and written, and their fp32 copies written in fp32.

    python tools/bench_sites.py [--rows 1000000] [--M 1024] [--steps 5] [--warmup 2] [--shapes headline,c3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as p  # noqa: E402

SHAPES = {"headline": dict(D=8, lik="gaussian", dtype=torch.float64), "c3": dict(D=16, lik="bernoulli", dtype=torch.float32)}
HBM_TBS = 8.0


def map_bytes(N, dtype, with_var=True):
    t = torch.empty((), dtype=dtype).element_size()
    return N * ((3 if with_var else 2) * t + 4 * 8 + (2 * t if dtype == torch.float32 else 0))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="headline,c3")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, M = a.rows, a.M
    for shape in a.shapes.split(","):
        cfg = SHAPES[shape]
        D, dtype = cfg["D"], cfg["dtype"]
        rng = np.random.RandomState(0)
        Xh = rng.randn(N, D)
        f = np.sin(Xh @ rng.randn(D, 1))
        Yh = f + np.sqrt(0.1) * rng.randn(N, 1)
        if cfg["lik"] == "bernoulli":
            Yh = (Yh > 0).astype(np.float64)
        Z = Xh[:M].copy()
        X = torch.as_tensor(Xh, device=dev, dtype=dtype)
        Y = torch.as_tensor(Yh, device=dev, dtype=dtype)
        lik = (lambda: p.Gaussian(0.1)) if cfg["lik"] == "gaussian" else (lambda: p.Bernoulli())
        kern = lambda: p.SquaredExponential(1.0, 1.0)
        variants = [("t_SVGP_sites", dict())]
        if cfg["lik"] == "gaussian":
            variants.append(("t_SVGP_sites", dict(skip_unused_variance=True)))
        variants += [("t_SVGP_white", dict()), ("t_SVGP", dict())]
        for name, kw in variants:
            if name == "t_SVGP_sites":
                m = p.t_SVGP_sites((X, Y), kern(), lik(), Z, compute_dtype=dtype, device=dev, **kw)
                step = lambda: m.natgrad_step(lr=0.5)
            elif name == "t_SVGP_white":
                m = p.t_SVGP_white(kern(), lik(), Z, num_data=N, compute_dtype=dtype, device=dev)
                step = lambda: m.natgrad_step((X, Y), lr=0.5)
            else:
                m = p.t_SVGP(kern(), lik(), Z, num_data=N, compute_dtype=dtype, device=dev, use_graph=False)
                step = lambda: m.natgrad_step((X, Y), lr=0.5)
            ms = time_steps(step, a.steps, a.warmup)
            eng = m._get_engine()
            eng.profile = {}
            step()
            prof = eng.profile_summary()
            eng.profile = None
            kern_ms = {k: (v[0], round(sum(v[5]), 4)) for k, v in prof.items()}
            row = dict(shape=shape, model=name, **{k: v for k, v in kw.items()}, N=N, M=M, D=D, dtype=str(dtype), lik=cfg["lik"],
                       step_ms=round(ms, 3), e_steps_per_s=round(1000.0 / ms, 2), kernels_ms=kern_ms)
            if name == "t_SVGP_sites":
                row["route"] = "two-product" if m._two_product else ("direct" if m._use_direct() else "whitened")
                mp_ms = sum(prof.get("tsvgp_diag_site_step", (0, 0, 0, 0, 0, []))[5])
                nbytes = map_bytes(N, dtype, with_var=not (kw.get("skip_unused_variance") and cfg["lik"] == "gaussian"))
                row["map_ms"] = round(mp_ms, 4)
                row["map_share_of_profiled_step"] = round(mp_ms / max(sum(sum(v[5]) for v in prof.values()), 1e-9), 4)
                row["map_TBps"] = round(nbytes / (mp_ms * 1e-3) / 1e12, 3) if mp_ms > 0 else None
                row["map_fraction_of_8TBps"] = round(row["map_TBps"] / HBM_TBS, 3) if mp_ms > 0 else None
            print(json.dumps(row), flush=True)
            del m, eng, step
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
