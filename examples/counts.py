#!/usr/bin/env python3
"""A Poisson rate on a 1-D grid with t-SVGP on one MI355X: counts y_n ~ Poisson(binsize * exp(f(x_n))), each observed over an
exposure of ``binsize`` (gpflow.likelihoods.Poisson [ext] with its exp link, whose variational expectations are closed form),
natural-gradient E-steps and Adam on the kernel; prints the posterior rate beside the true one at a few grid points.  The log rate
is of order one, as the zero-mean prior says: the undamped natural-gradient step on an exp link overshoots from a start that is
several prior standard deviations away (a base rate far from 1 belongs into ``binsize``).

    python examples/counts.py [--n 500] [--m 25] [--iters 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as gpf  # noqa: E402  (alias of the package directory t-svgp_amd/)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--m", type=int, default=25)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    X = np.linspace(0.0, 10.0, args.n)[:, None]
    binsize = 2.0
    rate = np.exp(np.sin(X) + 0.5 * np.cos(0.5 * X))  # events per unit exposure
    Y = rng.poisson(rate * binsize).astype(np.float64)
    Z = np.linspace(0.0, 10.0, args.m)[:, None]

    m = gpf.t_SVGP(gpf.SquaredExponential(1.0, 1.0), gpf.Poisson(binsize=binsize), Z, num_data=args.n)
    logf, _ = gpf.training.em_fit(m, (X, Y), iterations=args.iters, n_e_steps=8, n_m_steps=10, nat_lr=0.5, adam_lr=0.05)
    print("ELBO per iteration:", [round(v, 3) for v in logf], flush=True)
    mean, var = m.predict_y(X)  # counts per bin
    for i in range(0, args.n, max(args.n // 8, 1)):
        print(f"x = {X[i, 0]:5.2f}: rate {rate[i, 0]:7.2f}, posterior {float(mean[i, 0]) / binsize:7.2f} "
              f"+- {float(torch.sqrt(var[i, 0])) / binsize:6.2f} (one bin's predictive sd)")
    print("mean log predictive density", float(torch.mean(m.predict_log_density((X, Y)))))


if __name__ == "__main__":
    main()
