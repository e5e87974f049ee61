#!/usr/bin/env python3
"""A separable model with a Product kernel beside a single ARD kernel, on one MI355X.

y = rough(x0) * smooth(x1, x2) + noise (a "time" profile modulating a smooth "space" surface), N = 2000, M = 64.  Two t-SVGP
models take the same E/M loop (``training.em_fit``: natural-gradient E-steps on the sites, Adam M-steps on the kernel parameters,
the noise and Z):

    product   Matern52(active_dims=[0]) * SquaredExponential(active_dims=[1, 2])   one fused K(X, Z) fill per step, one fused
                                                                                    gradient contraction per M-step evaluation
    ard       Matern52 with one lengthscale per column

and the ELBO and the test NLPD of both are printed per iteration.

    python examples/product_kernels.py [--iters 4]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as gp  # noqa: E402  (alias of the package directory t-svgp_amd/)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    N, M, NT = 2000, 64, 500
    X = rng.uniform(-2.0, 2.0, size=(N + NT, 3))
    rough = 1.0 + 0.6 * np.sign(np.sin(4.0 * X[:, 0])) * np.abs(np.sin(4.0 * X[:, 0])) ** 0.5
    smooth = np.sin(1.5 * X[:, 1]) * np.cos(X[:, 2])
    Y = (rough * smooth)[:, None] + 0.1 * rng.randn(N + NT, 1)
    (X, Xt), (Y, Yt) = (X[:N], X[N:]), (Y[:N], Y[N:])
    dev = torch.device("cuda:0")
    Xd, Yd = torch.as_tensor(X, device=dev), torch.as_tensor(Y, device=dev)
    kernels = {
        "product": gp.Matern52(variance=1.0, lengthscales=0.5, active_dims=[0])
        * gp.SquaredExponential(variance=1.0, lengthscales=[1.0, 1.0], active_dims=[1, 2]),
        "ard": gp.Matern52(variance=1.0, lengthscales=np.ones(3)),
    }
    for name, kernel in kernels.items():
        model = gp.t_SVGP(kernel, gp.Gaussian(variance=0.5), X[:M].copy(), num_data=N)
        logf, nlpd = gp.training.em_fit(model, (Xd, Yd), iterations=args.iters, n_e_steps=8, n_m_steps=20, nat_lr=0.8,
                                        adam_lr=0.05, test_data=(Xt, Yt))
        for i, (e, n) in enumerate(zip(logf, nlpd)):
            print(f"{name:8s} iteration {i}: ELBO {e:10.3f}   test NLPD {n:.4f}")
        for pname, (par, _) in gp.training.trainable_parameters(model).items():
            if pname != "Z":
                print(f"{name:8s}   {pname} = {np.round(par.numpy(), 3).tolist()}")


if __name__ == "__main__":
    main()
