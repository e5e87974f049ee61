#!/usr/bin/env python3
"""The exact model beside the sparse one on the 1-D regression of the reference's regression_1D notebook (N = 200, X in [-1, 1],
Y = sin(15 X) + unit noise, SE kernel with variance 0.3 and lengthscale 0.1, M = 20 inducing points on a grid): ``t_VGP`` keeps one
site per datum and factors the N x N system, ``t_SVGP`` projects onto the inducing points.  Five natural-gradient steps of 0.9
each, as the notebook takes; under a Gaussian likelihood t_VGP's ELBO then sits at the exact log marginal likelihood, which is the
ceiling of t_SVGP's.  Prints both ELBOs and how far the sparse posterior is from the exact one on a 100-point grid.
``--train K`` then trains the kernel and the noise variance of the exact model for K iterations of ``training.em_fit_vgp``
(E-steps on the sites, Adam M-steps on ``t_VGP.elbo_and_grads``) and prints the ELBO per iteration and the parameters found.

    python examples/exact_vgp.py [--steps 5] [--lr 0.9] [--seed 0] [--train 0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as gp  # noqa: E402  (alias of the package directory t-svgp_amd/)


def regression_1d(N=200, M=20, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.rand(N, 1) * 2 - 1
    Y = np.sin(15 * X) + rng.randn(N, 1)
    return X, Y, np.linspace(X.min(), X.max(), M).reshape(-1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--train", type=int, default=0, help="iterations of em_fit_vgp on the exact model (0: the kernel stays as given)")
    args = ap.parse_args()
    X, Y, Z = regression_1d(seed=args.seed)
    kernel = lambda: gp.SquaredExponential(variance=0.3, lengthscales=0.1)
    exact = gp.t_VGP((X, Y), kernel(), gp.Gaussian(variance=1.0))
    sparse = gp.t_SVGP(kernel(), gp.Gaussian(variance=1.0), Z, num_data=X.shape[0])
    for _ in range(args.steps):
        exact.update_variational_parameters(beta=args.lr)
        sparse.natgrad_step((X, Y), lr=args.lr)
    grid = np.linspace(-1.0, 1.0, 100)[:, None]
    (me, ve), (ms, vs) = exact.predict_f(grid), sparse.predict_f(grid)
    print(f"t_VGP  ELBO {float(exact.elbo()):.4f}   (N = {X.shape[0]} sites)")
    print(f"t_SVGP ELBO {float(sparse.elbo((X, Y))):.4f}   (M = {Z.shape[0]} inducing points)")
    print(f"on {grid.shape[0]} grid points: max |mean difference| {float((me - ms).abs().max()):.4f}, "
          f"max |sd difference| {float((ve.sqrt() - vs.sqrt()).abs().max()):.4f}")
    if args.train > 0:
        from tsvgp_amd import training

        logf, _ = training.em_fit_vgp(exact, args.train, n_e_steps=2, n_m_steps=20, beta=args.lr, adam_lr=0.05)
        print("t_VGP  ELBO per training iteration: " + " ".join(f"{e:.4f}" for e in logf))
        print(f"trained: variance {exact.kernel.variance.item():.4f}, lengthscale {float(exact.kernel.lengthscales.value):.4f}, "
              f"noise variance {exact.likelihood.variance.item():.4f}")


if __name__ == "__main__":
    main()
