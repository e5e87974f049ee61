#!/usr/bin/env python3
"""Four ways to choose the inducing points on one MI355X, on the clustered 2-D data of examples/inducing_selection.py (the first
fifth of the rows sits in one cluster of width 0.05): Z = X[:M], the greedy conditional-variance selection
``select_inducing_points``, Lloyd's k-means ``kmeans_inducing_points`` started from the first rows, and k-means started from the
greedy selection.  Prints, for each, the residual trace tr(K_ff - Q_ff) and the ELBO after the same natural-gradient E-steps; for
the two clusterings also the iterations and the inertia.

    python examples/kmeans_inducing.py [--n 2000] [--m 64] [--steps 8]
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
    ap.add_argument("--steps", type=int, default=8)
    args = ap.parse_args()
    rng = np.random.RandomState(7)
    X = rng.randn(args.n, 2)
    X[:args.n // 5] = 0.05 * rng.randn(args.n // 5, 2)  # the first fifth of the rows: one cluster of width 0.05
    Y = np.sin(2.0 * X[:, :1]) * np.cos(X[:, 1:]) + np.sqrt(0.1) * rng.randn(args.n, 1)

    kernel = gpf.SquaredExponential(variance=1.0, lengthscales=1.0)
    ls = kernel.lengthscales.value
    sel = gpf.select_inducing_points(X, kernel, args.m)
    choices = [("Z = X[:M]", None, None), ("greedy selection", sel.Z, None)]
    km_first = gpf.kmeans_inducing_points(X, args.m, init="first", lengthscales=ls)
    choices.append(("k-means from X[:M]", km_first.Z, km_first))
    if sel.count == args.m:
        km_sel = gpf.kmeans_inducing_points(X, args.m, init=sel, lengthscales=ls)
        choices.append(("k-means from greedy", km_sel.Z, km_sel))
    else:
        print(f"the selection stopped at {sel.count} < {args.m} rows: k-means from it is left out", flush=True)
    Xd = torch.as_tensor(X, device=sel.Z.device)
    for name, Z, km in choices:
        Z = Xd[:args.m] if Z is None else Z
        line = f"{name:20s} tr(K_ff - Q_ff) = {residual_trace(kernel, Xd, Z):10.4f}   "
        try:
            model = gpf.t_SVGP(kernel, gpf.Gaussian(variance=0.1), Z)
            for _ in range(args.steps):
                model.natgrad_step((X, Y), lr=0.8)
            line += f"ELBO after {args.steps} E-steps = {float(model.elbo((X, Y))):10.3f}"
        except FloatingPointError as e:  # an ill-conditioned K_uu can end a step this way
            line += f"E-step failed: {e}"
        if km is not None:
            line += (f"   ({km.n_iter} iterations, {'converged' if km.converged else 'not converged'}, inertia "
                     f"{float(km.inertia):.3f}, smallest cluster {int(km.counts.min())} rows)")
        print(line, flush=True)


if __name__ == "__main__":
    main()
