#!/usr/bin/env python3
"""Choosing the inducing points on one MI355X: clustered 2-D data, t-SVGP with Z = X[:M] (the first rows all sit in one tight
cluster) and with the greedy conditional-variance selection ``select_inducing_points`` (pivoted Cholesky of K(X, X) on the device).
Prints, for both choices, the residual trace tr(K_ff - Q_ff), the condition estimate of K_uu + 1e-6 I the models' route gates
look at (``util.cond2_estimate``) and the ELBO after the same natural-gradient E-steps.

    python examples/inducing_selection.py [--n 2000] [--m 64] [--steps 5]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as gpf  # noqa: E402  (alias of the package directory t-svgp_amd/)


def cross(kernel, A, B):
    """K(A, B) of a stationary kernel as a dense torch expression (small N only: the example's own check)."""
    ls = kernel.lengthscales.value
    diff = (A / ls)[:, None, :] - (B / ls)[None, :, :]
    return kernel.variance.value * kernel._profile(torch.sum(diff * diff, dim=-1))


def residual_trace(kernel, X, Z):
    Kuu = cross(kernel, Z, Z) + 1e-10 * torch.eye(Z.shape[0], dtype=X.dtype, device=X.device)
    A = torch.linalg.solve_triangular(torch.linalg.cholesky(Kuu), cross(kernel, Z, X), upper=False)
    return float(torch.clamp(kernel.variance.value - (A * A).sum(dim=0), min=0.0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.RandomState(7)
    X = rng.randn(args.n, 2)
    X[:args.n // 5] = 0.05 * rng.randn(args.n // 5, 2)  # the first fifth of the rows: one cluster of width 0.05
    Y = np.sin(2.0 * X[:, :1]) * np.cos(X[:, 1:]) + np.sqrt(0.1) * rng.randn(args.n, 1)

    kernel = gpf.SquaredExponential(variance=1.0, lengthscales=1.0)
    sel = gpf.select_inducing_points(X, kernel, args.m)
    print(f"selected {sel.count} of {args.n} rows; pivots {float(sel.pivots[0]):.3f} .. {float(sel.pivots[-1]):.3e}; "
          f"residual trace {float(sel.trace):.4f}", flush=True)
    Xd = torch.as_tensor(X, device=sel.Z.device)
    for name, Z in (("Z = X[:M]", Xd[:args.m]), ("Z = selection", sel.Z)):
        M = Z.shape[0]
        Kuu = cross(kernel, Z, Z) + 1e-6 * torch.eye(M, dtype=Z.dtype, device=Z.device)
        cond = float(gpf.util.cond2_estimate(Kuu))
        line = f"{name:14s} tr(K_ff - Q_ff) = {residual_trace(kernel, Xd, Z):10.4f}   cond(K_uu + 1e-6 I) ~ {cond:.3e}   "
        try:
            model = gpf.t_SVGP(kernel, gpf.Gaussian(variance=0.1), Z)
            for _ in range(args.steps):
                model.natgrad_step((X, Y), lr=0.8)
            line += f"ELBO after {args.steps} E-steps = {float(model.elbo((X, Y))):.3f}"
        except FloatingPointError as e:  # an ill-conditioned K_uu can end a step this way
            line += f"E-step failed: {e}"
        print(line, flush=True)


if __name__ == "__main__":
    main()
