#!/usr/bin/env python3
"""Heteroskedastic regression with t-SVGP (reference docs/notebooks/heteroskedastic.py:40-152) on synthetic data, on one
MI355X: two latent GPs with one SE kernel each on shared inducing points -- f0 the mean, f1 the log noise scale of
y ~ Normal(f0, exp(f1)) -- then the notebook's loop: per iteration 2 natural-gradient E-steps (lr 0.5) and one Adam step
(lr 0.1) on the kernels' parameters, and predict_y at the end.

    python examples/heteroskedastic.py [--n 1000] [--m 50] [--iters 100]
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
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--m", type=int, default=50)
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    X = np.sort(rng.uniform(0, 10, (args.n, 1)), axis=0)
    Y = np.sin(X) + np.exp(0.6 * np.cos(0.7 * X) - 1.0) * rng.randn(args.n, 1)
    Y /= Y.std()
    N = len(X)

    likelihood = gpf.HeteroskedasticTFPConditional()  # Normal(loc=f0, scale=exp(f1)), the notebook's arguments
    kernel = gpf.SeparateIndependent([gpf.SquaredExponential(), gpf.SquaredExponential()])
    Z = np.linspace(X.min(), X.max(), args.m)[:, None]
    inducing_variable = gpf.SharedIndependentInducingVariables(gpf.InducingPoints(Z))
    m = gpf.t_SVGP(kernel, likelihood, inducing_variable, num_data=N, num_latent_gps=2)

    # M-step of the notebook: Adam on kernel.trainable_variables (variance and lengthscales of both kernels; GPflow keeps them
    # behind a softplus), the inducing inputs and the sites fixed
    params = {f"kernels.{p}.{n}": getattr(k, n) for p, k in enumerate(m.kernel.kernels) for n in ("variance", "lengthscales")}
    opt = gpf.training.Adam(0.1)
    softplus_inv = lambda x: x + torch.log(-torch.expm1(-x))
    for r in range(args.iters):
        for _ in range(2):
            m.natgrad_step((X, Y), lr=0.5)
        _, grads = m.elbo_and_grads((X, Y))
        u = {n: softplus_inv(par.value.detach().to(torch.float64)) for n, par in params.items()}
        gu = {n: -grads[n].reshape(u[n].shape) * torch.sigmoid(u[n]) for n in params}
        opt.step(u, gu)
        for n, par in params.items():
            par.assign(torch.nn.functional.softplus(u[n]))
        if r % 10 == 0:
            print(r, float(m.elbo((X, Y))), flush=True)

    Ymean, Yvar = m.predict_y(X)
    print("final ELBO", float(m.elbo((X, Y))))
    print("predictive std at x = 0, 5, 10:",
          [round(float(torch.sqrt(Yvar[i, 0])), 4) for i in (0, N // 2, N - 1)])
    print("mean log predictive density", float(torch.mean(m.predict_log_density((X, Y)))))


if __name__ == "__main__":
    main()
