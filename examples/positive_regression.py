#!/usr/bin/env python3
"""Regression on strictly positive targets with t-SVGP on one MI355X: 1-D amounts drawn from a Gamma distribution whose scale
follows a smooth function, the Gamma likelihood (gpflow.likelihoods.Gamma [ext], exp link) against the usual workaround, a Gaussian
likelihood fitted to log y.  Both models run the E/M loop of ``training.em_fit``; the test NLPD is reported for y itself, so the
log-scale model's density carries the Jacobian -log y.

    python examples/positive_regression.py [--n 500] [--m 20] [--iters 8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as gpf  # noqa: E402  (alias of the package directory t-svgp_amd/)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--m", type=int, default=20)
    ap.add_argument("--iters", type=int, default=8)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    f = lambda x: np.sin(2.0 * x) + 0.3 * x
    shape = 2.0
    X = np.sort(rng.uniform(-3, 3, (args.n, 1)), axis=0)
    Y = rng.gamma(shape, np.exp(f(X)))
    Xt = np.linspace(-3, 3, 300)[:, None]
    Yt = rng.gamma(shape, np.exp(f(Xt)))
    Z = np.linspace(-3, 3, args.m)[:, None]

    lik = gpf.Gamma(shape=1.0)
    m = gpf.t_SVGP(gpf.SquaredExponential(1.0, 1.0), lik, Z.copy(), num_data=args.n)
    logf, nlpd = gpf.training.em_fit(m, (X, Y), iterations=args.iters, n_e_steps=8, n_m_steps=20, nat_lr=0.5, adam_lr=0.05,
                                     test_data=(Xt, Yt))
    print(f"Gamma: ELBO {logf[-1]:.3f}, shape {lik.shape.item():.4f} (data: {shape}), test NLPD {nlpd[-1]:.4f}", flush=True)

    lik = gpf.Gaussian(variance=1.0)
    m = gpf.t_SVGP(gpf.SquaredExponential(1.0, 1.0), lik, Z.copy(), num_data=args.n)
    logf, nlpd = gpf.training.em_fit(m, (X, np.log(Y)), iterations=args.iters, n_e_steps=8, n_m_steps=20, nat_lr=0.5, adam_lr=0.05,
                                     test_data=(Xt, np.log(Yt)))
    jac = float(np.mean(np.log(Yt)))  # p(y) = p(log y) / y
    print(f"Gaussian on log y: ELBO (of log y) {logf[-1]:.3f}, variance {lik.variance.item():.4f}, test NLPD of y {nlpd[-1] + jac:.4f}",
          flush=True)


if __name__ == "__main__":
    main()
