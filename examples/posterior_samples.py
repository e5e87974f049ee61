#!/usr/bin/env python3
"""Joint posterior draws on the C1 1-D regression (tests/helpers.c1_problem: X in [-1, 1], Y = sin(15 X) + noise, 32 inducing
points on a grid, lengthscale 0.1): 8 E-steps, then on a 400-point grid the posterior mean, the marginal 95 % band and 10 JOINT
function draws (``predict_f_samples``: smooth curves, where draws from the marginals would be white noise around the mean).
Writes .npy files; plot them with whatever is at hand.

    python examples/posterior_samples.py [--out posterior_samples] [--draws 10] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np

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
    ap.add_argument("--out", default="posterior_samples")
    ap.add_argument("--draws", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    X, Y, Z = c1_problem()
    model = gp.t_SVGP(gp.SquaredExponential(variance=0.3, lengthscales=0.1), gp.Gaussian(variance=1.0), Z, num_data=X.shape[0])
    for _ in range(8):
        model.natgrad_step((X, Y), lr=0.8)
    grid = np.linspace(-1.0, 1.0, 400)[:, None]
    mean, var = model.predict_f(grid)
    _, cov = model.predict_f(grid, full_cov=True)  # [1, 400, 400]
    draws = model.predict_f_samples(grid, args.draws, seed=args.seed)  # [draws, 400, 1], joint over the grid
    mean, sd = mean.cpu().numpy()[:, 0], np.sqrt(var.cpu().numpy()[:, 0])
    os.makedirs(args.out, exist_ok=True)
    for name, arr in (("grid", grid[:, 0]), ("mean", mean), ("band_lo", mean - 1.96 * sd), ("band_hi", mean + 1.96 * sd),
                      ("cov", cov.cpu().numpy()[0]), ("draws", draws.cpu().numpy()[:, :, 0])):
        np.save(os.path.join(args.out, name + ".npy"), arr)
    inside = np.mean(np.abs(draws.cpu().numpy()[:, :, 0] - mean[None]) <= 1.96 * sd[None])
    print(f"ELBO {float(model.elbo((X, Y))):.3f}; {args.draws} joint draws on {grid.shape[0]} points, {100 * inside:.1f} % of their "
          f"values inside the marginal 95 % band; files in {args.out}/")


if __name__ == "__main__":
    main()
