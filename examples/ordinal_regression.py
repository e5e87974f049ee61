#!/usr/bin/env python3
"""Ordinal regression with t-SVGP on one MI355X: 1-D synthetic ratings in 5 ordered bins, the Ordinal likelihood
(gpflow.likelihoods.Ordinal [ext]: one latent, the bins cut it at fixed edges) beside MultiClass(5) (five latents, the order of
the classes forgotten) on the same data, kernel and inducing points.  Both models run the E/M loop of ``training.em_fit``
(natural-gradient E-steps, Adam on the kernel, Z and -- Ordinal -- the link's sigma) and print the ELBO and the negative log
predictive density of held-out ratings.

    python examples/ordinal_regression.py [--n 600] [--m 20] [--iters 8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as gpf  # noqa: E402  (alias of the package directory t-svgp_amd/)

EDGES = np.array([-1.2, -0.4, 0.4, 1.2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=600)
    ap.add_argument("--m", type=int, default=20)
    ap.add_argument("--iters", type=int, default=8)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    f = lambda x: 1.6 * np.sin(1.5 * x) + 0.2 * x
    rate = lambda x: np.sum((f(x) + 0.4 * rng.randn(*x.shape))[..., None] > EDGES, axis=-1).astype(np.float64)
    X = np.sort(rng.uniform(-3, 3, (args.n, 1)), axis=0)
    Y = rate(X)
    Xt = np.linspace(-3, 3, 300)[:, None]
    Yt = rate(Xt)
    Z = np.linspace(-3, 3, args.m)[:, None]
    print(f"{args.n} ratings, counts per bin {np.bincount(Y[:, 0].astype(int), minlength=5).tolist()}", flush=True)

    for name, lik, P in (("Ordinal", gpf.Ordinal(EDGES), 1), ("MultiClass(5)", gpf.MultiClass(5), 5)):
        m = gpf.t_SVGP(gpf.SquaredExponential(1.0, 1.0), lik, Z.copy(), num_latent_gps=P, num_data=args.n)
        logf, nlpd = gpf.training.em_fit(m, (X, Y), iterations=args.iters, n_e_steps=8, n_m_steps=20, nat_lr=0.5, adam_lr=0.05,
                                         test_data=(Xt, Yt))
        extra = f", sigma {lik.sigma.item():.4f}" if name == "Ordinal" else ""
        print(f"{name}: {P} latent GP(s), ELBO {logf[-1]:.3f}, test NLPD {nlpd[-1]:.4f}{extra}", flush=True)


if __name__ == "__main__":
    main()
