#!/usr/bin/env python3
"""The arg max of posterior FUNCTION draws in a continuous input space, by gradient ascent on the draws themselves (what Thompson
sampling needs at every round).  The 2-D analogue of the regression of examples/function_samples.py: X uniform in [-1, 1]^2,
Y = sin(5 x0) cos(4 x1) + noise, 8 x 8 inducing points on a grid, lengthscale 0.3.  After 8 E-steps, S = 8 functions are drawn
with ``sample_functions``; every draw gets R random starts, all S R rows sit in ONE tensor X, and ``torch.optim.Adam`` ascends

    sum_s sum_{rows of s} fs(X)[s, row]

through autograd: ``fs(X)`` has a ``grad_fn`` whose backward is one HIP launch per latent (``tsvgp_pathwise_vjp_f64``), exact and
with no N-sized matrix.  Each draw's best end point is printed next to the best point of a 200 x 200 grid evaluated with the same
``fs``: the ascent should reach at least the grid's value, at a position the grid can only resolve to 0.01.

    python examples/thompson_argmax.py [--draws 8] [--starts 32] [--features 1024] [--steps 200] [--lr 0.02] [--seed 0]
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
    Y = np.sin(5 * X[:, :1]) * np.cos(4 * X[:, 1:]) + 0.3 * rng.randn(N, 1)
    g = np.linspace(-1.0, 1.0, 8)
    Z = np.stack(np.meshgrid(g, g), axis=-1).reshape(64, 2)
    return X, Y, Z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=8)
    ap.add_argument("--starts", type=int, default=32)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    S, R = args.draws, args.starts
    X, Y, Z = c2_problem()
    model = gp.t_SVGP(gp.SquaredExponential(variance=0.5, lengthscales=0.3), gp.Gaussian(variance=0.09), Z, num_data=X.shape[0])
    for _ in range(8):
        model.natgrad_step((X, Y), lr=0.8)
    fs = model.sample_functions(S, args.features, seed=args.seed)

    rng = np.random.RandomState(args.seed + 1)
    Xs = torch.tensor(rng.rand(S * R, 2) * 2 - 1, device=model.device, requires_grad=True)  # rows s R .. s R + R - 1 belong to draw s
    draw_of, row = torch.arange(S, device=model.device).repeat_interleave(R), torch.arange(S * R, device=model.device)
    opt = torch.optim.Adam([Xs], lr=args.lr)
    for _ in range(args.steps):
        opt.zero_grad()
        (-fs(Xs)[draw_of, row, 0].sum()).backward()  # every row climbs its own draw; the others' cotangents are zeros
        opt.step()
        with torch.no_grad():
            Xs.clamp_(-1.0, 1.0)
    with torch.no_grad():
        end = fs(Xs)[draw_of, row, 0].view(S, R)
        best = end.argmax(dim=1)
        x_asc = Xs.view(S, R, 2)[torch.arange(S), best].cpu().numpy()
        f_asc = end.max(dim=1).values.cpu().numpy()
        g = np.linspace(-1.0, 1.0, 200)
        grid = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
        fg = fs(grid)[:, :, 0]  # [S, 40000]
        f_grid, at = fg.max(dim=1)
        x_grid, f_grid = grid[at.cpu().numpy()], f_grid.cpu().numpy()
    print(f"{S} draws ({args.features} features), {R} starts each, {args.steps} Adam steps (lr {args.lr}) on one [{S * R}, 2] tensor")
    print("draw   ascent: arg max              value    |  200 x 200 grid: arg max      value    | ascent - grid")
    for s in range(S):
        print(f"{s:4d}   ({x_asc[s, 0]:+.5f}, {x_asc[s, 1]:+.5f})   {f_asc[s]:+.6f}  |  ({x_grid[s, 0]:+.5f}, {x_grid[s, 1]:+.5f})   {f_grid[s]:+.6f}  | "
              f"{f_asc[s] - f_grid[s]:+.2e}")
    print(f"the ascent is at or above the grid's best value for {int(np.sum(f_asc >= f_grid))} of {S} draws")


if __name__ == "__main__":
    main()
