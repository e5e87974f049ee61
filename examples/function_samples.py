#!/usr/bin/env python3
"""Posterior FUNCTION draws on the 1-D regression of examples/posterior_samples.py (X in [-1, 1], Y = sin(15 X) + noise, 32
inducing points on a grid, lengthscale 0.1): 8 E-steps, then 8 functions from ``sample_functions`` -- each one object that can be
evaluated anywhere, any number of times.  They are read on a 200-point grid and on a 1e6-point grid in row chunks (no 1e6 x 1e6
covariance, which would be 8 TB), and the abscissae the two grids share get the same values bit for bit: it is the same draw.
The draws are put beside ``predict_f``'s mean and marginal 95 % band.  Writes .npy files; plot them with whatever is at hand.

    python examples/function_samples.py [--out function_samples] [--draws 8] [--features 1024] [--fine 1000000] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as gp  # noqa: E402  (alias of the package directory t-svgp_amd/)


def c1_problem(N=1000, M=32, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.rand(N, 1) * 2 - 1
    Y = np.sin(15 * X) + rng.randn(N, 1)
    Z = np.linspace(X.min(), X.max(), M)[:, None]
    return X, Y, Z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="function_samples")
    ap.add_argument("--draws", type=int, default=8)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--fine", type=int, default=1000000)
    ap.add_argument("--chunk", type=int, default=1 << 18)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    X, Y, Z = c1_problem()
    model = gp.t_SVGP(gp.SquaredExponential(variance=0.3, lengthscales=0.1), gp.Gaussian(variance=1.0), Z, num_data=X.shape[0])
    for _ in range(8):
        model.natgrad_step((X, Y), lr=0.8)
    fs = model.sample_functions(args.draws, args.features, seed=args.seed)
    fine = np.linspace(-1.0, 1.0, args.fine)[:, None]
    step = (args.fine - 1) // 199
    coarse = fine[::step][:200]  # 200 abscissae of the fine grid
    f_coarse = fs(coarse)  # [draws, 200, 1]
    f_fine = torch.cat([fs(fine[r:r + args.chunk]) for r in range(0, args.fine, args.chunk)], dim=1)  # [draws, fine, 1], in row chunks
    same = torch.equal(f_fine[:, ::step][:, :200], f_coarse)
    mean, var = model.predict_f(coarse)
    mean, sd = mean.cpu().numpy()[:, 0], np.sqrt(var.cpu().numpy()[:, 0])
    draws = f_coarse.cpu().numpy()[:, :, 0]
    os.makedirs(args.out, exist_ok=True)
    for name, arr in (("grid", coarse[:, 0]), ("mean", mean), ("band_lo", mean - 1.96 * sd), ("band_hi", mean + 1.96 * sd),
                      ("draws", draws), ("fine_grid", fine[:, 0]), ("fine_draws", f_fine.cpu().numpy()[:, :, 0])):
        np.save(os.path.join(args.out, name + ".npy"), arr)
    inside = np.mean(np.abs(draws - mean[None]) <= 1.96 * sd[None])
    argmax = fine[f_fine[:, :, 0].argmax(dim=1).cpu().numpy(), 0]  # a statistic of each draw no 200-point grid resolves
    print(f"{args.draws} function draws ({args.features} features): {100 * inside:.1f} % of their values on the 200-point grid inside "
          f"predict_f's marginal 95 % band; the {args.fine}-point grid (chunks of {args.chunk} rows) agrees with it bit for bit on the "
          f"shared abscissae: {same}; arg max of each draw: {np.array2string(argmax, precision=4)}; files in {args.out}/")
    if not same:
        raise SystemExit("the two grids disagree on shared abscissae")


if __name__ == "__main__":
    main()
