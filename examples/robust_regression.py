#!/usr/bin/env python3
"""Robust regression with t-SVGP on one MI355X: 1-D data with a few gross outliers, the Student-t likelihood
(gpflow.likelihoods.StudentT [ext]) against the Gaussian one on the same kernel and inducing points.  Both models run the E/M
loop of ``training.em_fit`` (natural-gradient E-steps, Adam on the kernel, the likelihood's noise parameter and Z) and print the
negative log predictive density of clean test data: the outliers inflate the Gaussian noise variance, the Student-t scale stays
at the size of the bulk.

    python examples/robust_regression.py [--n 400] [--m 20] [--iters 10]
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
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--m", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    f = lambda x: np.sin(2.0 * x) + 0.3 * x
    X = np.sort(rng.uniform(-3, 3, (args.n, 1)), axis=0)
    Y = f(X) + 0.2 * rng.randn(args.n, 1)
    out = rng.choice(args.n, max(args.n // 25, 1), replace=False)
    Y[out] += rng.choice([-1.0, 1.0], (len(out), 1)) * rng.uniform(5.0, 10.0, (len(out), 1))  # gross outliers
    Xt = np.linspace(-3, 3, 200)[:, None]
    Yt = f(Xt) + 0.2 * rng.randn(200, 1)
    Z = np.linspace(-3, 3, args.m)[:, None]

    for name, lik in (("StudentT", gpf.StudentT(scale=1.0, df=3.0)), ("Gaussian", gpf.Gaussian(variance=1.0))):
        m = gpf.t_SVGP(gpf.SquaredExponential(1.0, 1.0), lik, Z.copy(), num_data=args.n)
        logf, nlpd = gpf.training.em_fit(m, (X, Y), iterations=args.iters, n_e_steps=8, n_m_steps=20, nat_lr=0.5,
                                         adam_lr=0.05, test_data=(Xt, Yt))
        noise = f"scale {lik.scale.item():.4f}" if name == "StudentT" else f"variance {lik.variance.item():.4f}"
        mu, _ = m.predict_f(Xt)
        rmse = float(torch.sqrt(torch.mean((mu.cpu() - torch.as_tensor(f(Xt))) ** 2)))
        print(f"{name}: ELBO {logf[-1]:.3f}, {noise}, test NLPD {nlpd[-1]:.4f}, RMSE to the clean function {rmse:.4f}", flush=True)


if __name__ == "__main__":
    main()
