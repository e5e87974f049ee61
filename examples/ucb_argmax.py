#!/usr/bin/env python3
"""Acquisition functions written in ordinary torch code on top of ``predict_f`` / ``predict_y``, maximised over a continuous input
space by gradient ascent (the companion of examples/thompson_argmax.py, which climbs function DRAWS; this climbs the MOMENTS).

1. Regression, the 2-D problem of examples/thompson_argmax.py (X uniform in [-1, 1]^2, Y = sin(5 x0) cos(4 x1) + noise, 8 x 8
   inducing points, lengthscale 0.3): the upper confidence bound

       ucb(x) = mean(x) + kappa sqrt(var(x)),      (mean, var) = model.predict_f(x).

2. Classification, the same inputs with labels sign(sin(5 x0) cos(4 x1)) under a Bernoulli likelihood: the predictive entropy

       H(x) = -p log p - (1 - p) log(1 - p),       p = model.predict_y(x)[0],

   whose maxima are the points the classifier is least sure of (uncertainty sampling).

In both, R random starts sit in ONE tensor X that requires grad; ``predict_f(X)`` then has a ``grad_fn`` whose backward is one
K(X, Z) fill, one GEMM and one HIP launch per latent (``tsvgp_moments_vjp_*``), and ``torch.optim.Adam`` ascends the sum over the
rows (every row's acquisition depends on that row alone).  The best end points are printed next to the best point of a 200 x 200
grid evaluated with the same model: the ascent should reach at least the grid's value, at a position the grid resolves to 0.01.

    python examples/ucb_argmax.py [--starts 64] [--steps 200] [--lr 0.02] [--kappa 2.0] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as gp  # noqa: E402  (alias of the package directory t-svgp_amd/)


def c2_problem(N=2000, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.rand(N, 2) * 2 - 1
    F = np.sin(5 * X[:, :1]) * np.cos(4 * X[:, 1:])
    g = np.linspace(-1.0, 1.0, 8)
    Z = np.stack(np.meshgrid(g, g), axis=-1).reshape(64, 2)
    return X, F + 0.3 * rng.randn(N, 1), (F + 0.3 * rng.randn(N, 1) > 0).astype(np.float64), Z


def ascend(acquisition, device, starts, steps, lr, seed):
    """Adam on ``starts`` rows at once; returns (end points [R, 2], their values [R]) and the grid's (best point, best value)."""
    rng = np.random.RandomState(seed)
    X = torch.tensor(rng.rand(starts, 2) * 2 - 1, device=device, requires_grad=True)
    opt = torch.optim.Adam([X], lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        (-acquisition(X).sum()).backward()
        opt.step()
        with torch.no_grad():
            X.clamp_(-1.0, 1.0)
    with torch.no_grad():
        end = acquisition(X)
        g = np.linspace(-1.0, 1.0, 200)
        grid = torch.tensor(np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2), device=device)
        vals = acquisition(grid)
        at = int(vals.argmax())
    return X.detach().cpu().numpy(), end.cpu().numpy(), grid[at].cpu().numpy(), float(vals[at])


def report(name, x_end, v_end, x_grid, v_grid, top=5):
    order = np.argsort(-v_end)[:top]
    print(f"{name}: the {top} best of {len(v_end)} ascents beside the best of a 200 x 200 grid")
    print("  ascent: end point               value      ascent - grid")
    for i in order:
        print(f"  ({x_end[i, 0]:+.5f}, {x_end[i, 1]:+.5f})   {v_end[i]:+.6f}   {v_end[i] - v_grid:+.2e}")
    print(f"  grid:   ({x_grid[0]:+.5f}, {x_grid[1]:+.5f})   {v_grid:+.6f}")
    print(f"  the best ascent is {'at or above' if v_end[order[0]] >= v_grid else 'BELOW'} the grid's best value")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--kappa", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    X, Y, Yc, Z = c2_problem()

    reg = gp.t_SVGP(gp.SquaredExponential(variance=0.5, lengthscales=0.3), gp.Gaussian(variance=0.09), Z, num_data=X.shape[0])
    for _ in range(8):
        reg.natgrad_step((X, Y), lr=0.8)

    def ucb(x):
        mean, var = reg.predict_f(x)
        return (mean + a.kappa * torch.sqrt(var))[:, 0]

    report(f"UCB, kappa = {a.kappa}", *ascend(ucb, reg.device, a.starts, a.steps, a.lr, a.seed + 1))

    clf = gp.t_SVGP(gp.SquaredExponential(variance=2.0, lengthscales=0.3), gp.Bernoulli(), Z, num_data=X.shape[0])
    for _ in range(12):
        clf.natgrad_step((X, Yc), lr=0.5)

    def entropy(x):
        p = clf.predict_y(x)[0][:, 0].clamp(1e-12, 1.0 - 1e-12)
        return -(p * torch.log(p) + (1.0 - p) * torch.log1p(-p))

    report("predictive entropy of the Bernoulli model", *ascend(entropy, clf.device, a.starts, a.steps, a.lr, a.seed + 2))


if __name__ == "__main__":
    main()
