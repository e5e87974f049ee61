#!/usr/bin/env python3
"""k-means++ seeding as the start of Lloyd's k-means on one MI355X, on the clustered 2-D data of examples/kmeans_inducing.py (the
first fifth of the rows sits in one cluster of width 0.05, so Z = X[:M] and a k-means started there are poor): Z = X[:M], the
greedy conditional-variance selection, k-means from the greedy selection, and k-means from ``init="k-means++"`` for seeds 0 .. 4
-- the one good start that needs no kernel.  Prints, for each, the residual trace tr(K_ff - Q_ff) and the ELBO after the same
natural-gradient E-steps; for the clusterings also the iterations and the inertia, for the seeded ones the potential the seeding
itself left (the inertia of its M rows taken as centres).

    python examples/kmeanspp_inducing.py [--n 2000] [--m 64] [--steps 8] [--out profiles/kmeanspp_example.txt]
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
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    rng = np.random.RandomState(7)
    X = rng.randn(args.n, 2)
    X[:args.n // 5] = 0.05 * rng.randn(args.n // 5, 2)  # the first fifth of the rows: one cluster of width 0.05
    Y = np.sin(2.0 * X[:, :1]) * np.cos(X[:, 1:]) + np.sqrt(0.1) * rng.randn(args.n, 1)

    kernel = gpf.SquaredExponential(variance=1.0, lengthscales=1.0)
    ls = kernel.lengthscales.value
    sel = gpf.select_inducing_points(X, kernel, args.m)
    km_first = gpf.kmeans_inducing_points(X, args.m, init="first", lengthscales=ls)
    choices = [("Z = X[:M]", None, None), ("k-means from X[:M]", km_first.Z, km_first), ("greedy selection", sel.Z, None)]
    if sel.count == args.m:
        km_sel = gpf.kmeans_inducing_points(X, args.m, init=sel, lengthscales=ls)
        choices.append(("k-means from greedy", km_sel.Z, km_sel))
    for seed in range(5):
        km = gpf.kmeans_inducing_points(X, args.m, init="k-means++", seed=seed, lengthscales=ls)
        choices.append((f"k-means from k-means++ (seed {seed})", km.Z, km))
    Xd = torch.as_tensor(X, device=sel.Z.device)
    lines = [f"# examples/kmeanspp_inducing.py: N = {args.n}, M = {args.m}, {args.steps} E-steps, SquaredExponential(1, 1), Gaussian(0.1)"]
    print(lines[0], flush=True)
    for name, Z, km in choices:
        Z = Xd[:args.m] if Z is None else Z
        line = f"{name:34s} tr(K_ff - Q_ff) = {residual_trace(kernel, Xd, Z):10.4f}   "
        try:
            model = gpf.t_SVGP(kernel, gpf.Gaussian(variance=0.1), Z)
            for _ in range(args.steps):
                model.natgrad_step((X, Y), lr=0.8)
            line += f"ELBO after {args.steps} E-steps = {float(model.elbo((X, Y))):10.3f}"
        except FloatingPointError as e:  # an ill-conditioned K_uu can end a step this way
            line += f"E-step failed: {e}"
        if km is not None:
            line += (f"   ({km.n_iter} iterations, {'converged' if km.converged else 'not converged'}, inertia "
                     f"{float(km.inertia):.3f}, smallest cluster {int(km.counts.min())} rows")
            if km.seeding is not None:
                line += f"; seeding potential {float(km.seeding.potential):.3f}, {km.seeding.n_local_trials} trials per centre"
            line += ")"
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
