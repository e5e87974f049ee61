#!/usr/bin/env python3
"""Correlated multi-output regression with t-SVGP on one MI355X: P = 8 outputs generated as linear mixtures of 2 smooth latent
functions, fitted twice on the same data and inducing points -- with ``LinearCoregionalization`` (L = 2 latent GPs, the mixing
matrix W [8, 2] trained by the M-step beside the kernels) and with ``SeparateIndependent`` (8 latent GPs, one per output, nothing
shared between the outputs).  Both run the E/M loop of ``training.em_fit`` and print the ELBO, the negative log predictive
density of held-out rows and the wall time of the fit.

    python examples/multioutput_lmc.py [--n 2000] [--m 32] [--iters 6]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as gpf  # noqa: E402  (alias of the package directory t-svgp_amd/)

P, L = 8, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--iters", type=int, default=6)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    Wtrue = rng.randn(P, L)
    latents = lambda x: np.concatenate([np.sin(2.0 * x), np.cos(1.3 * x) * x / 3.0], axis=1)
    draw = lambda x: latents(x) @ Wtrue.T + 0.3 * rng.randn(x.shape[0], P)
    X = np.sort(rng.uniform(-3, 3, (args.n, 1)), axis=0)
    Y = draw(X)
    Xt = np.linspace(-3, 3, 400)[:, None]
    Yt = draw(Xt)
    Z = np.linspace(-3, 3, args.m)[:, None]
    kernels = lambda n: [gpf.SquaredExponential(1.0, 1.0) for _ in range(n)]
    models = (
        (f"LinearCoregionalization (L = {L})", gpf.LinearCoregionalization(kernels(L), 0.5 * rng.randn(P, L)), L),
        (f"SeparateIndependent ({P} latents)", gpf.SeparateIndependent(kernels(P)), P),
    )
    # one throwaway E/M iteration first: library handles and work buffers are created once per process, and the first fit timed
    # would pay for them
    warm = gpf.t_SVGP(gpf.SeparateIndependent(kernels(2)), gpf.Gaussian(0.5), gpf.SharedIndependentInducingVariables(Z.copy()),
                      num_latent_gps=2, num_data=args.n)
    gpf.training.em_fit(warm, (X, Y[:, :2]), iterations=1, n_e_steps=2, n_m_steps=2)
    for name, kernel, nl in models:
        m = gpf.t_SVGP(kernel, gpf.Gaussian(0.5), gpf.SharedIndependentInducingVariables(Z.copy()), num_latent_gps=nl,
                       num_data=args.n)
        t0 = time.perf_counter()
        logf, nlpd = gpf.training.em_fit(m, (X, Y), iterations=args.iters, n_e_steps=4, n_m_steps=10, nat_lr=0.8, adam_lr=0.05,
                                         test_data=(Xt, Yt))
        wall = time.perf_counter() - t0
        print(f"{name}: ELBO {logf[-1]:.2f}, test NLPD {nlpd[-1]:.4f} per row of {P} outputs, noise variance "
              f"{m.likelihood.variance.item():.4f}, {wall:.2f} s for {args.iters} E/M iterations", flush=True)


if __name__ == "__main__":
    main()
