#!/usr/bin/env python3
"""Multi-class classification with t-SVGP and the deterministic MultiClass likelihood (RobustMax link, 20-point Gauss-Hermite):
the loop of examples/multiclass.py on the same synthetic data, with ``gpf.MultiClass`` in place of the Monte Carlo ``gpf.Softmax``.
One shared Matern-5/2 ARD kernel over C = 10 latent GPs, M = 100 inducing points at the first M inputs; per iteration 8 minibatch
natural-gradient E-steps and 20 Adam M-steps (kernel variance, lengthscales and inducing inputs) on minibatches of 200.  Nothing
is drawn, so the ELBO of the fixed evaluation batch printed after each E-block is a number, not an estimate; the test NLPD and
accuracy follow the M-block.

    python examples/multiclass_robustmax.py [--n 10000] [--d 16] [--iters 20] [--epsilon 1e-3]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as gpf  # noqa: E402  (alias of the package directory t-svgp_amd/)
from multiclass import e_steps, evaluate, m_steps, make_data  # noqa: E402  (the same data and the same loop)


def make_model(X, c, m, num_data, epsilon=1e-3, **kw):
    d = X.shape[1]
    Z = X[:m].copy()
    kernel = gpf.Matern52(variance=1.0, lengthscales=np.full(d, float(np.sqrt(d))))
    model = gpf.t_SVGP(kernel, gpf.MultiClass(c, epsilon=epsilon), Z, num_data=num_data, num_latent_gps=c, **kw)
    return model, Z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--n-test", type=int, default=2000)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--m", type=int, default=100)
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--e-steps", type=int, default=8)
    ap.add_argument("--m-steps", type=int, default=20)
    ap.add_argument("--nat-lr", type=float, default=0.1)
    ap.add_argument("--adam-lr", type=float, default=0.02)
    ap.add_argument("--epsilon", type=float, default=1e-3)
    args = ap.parse_args()
    X, Y, Xt, Yt = make_data(args.n, args.n_test, args.d, args.classes)
    model, _ = make_model(X, args.classes, args.m, args.n, epsilon=args.epsilon)
    opt = gpf.training.Adam(args.adam_lr)
    rng = np.random.RandomState(1)
    Xe, Ye = X[:2000], Y[:2000]  # the batch the ELBO is reported on
    for it in range(args.iters):
        e_steps(model, X, Y, args.batch, args.e_steps, args.nat_lr, rng)
        elbo = float(model.elbo((Xe, Ye)))
        m_steps(model, X, Y, args.batch, args.m_steps, opt, rng)
        nlpd, acc = evaluate(model, Xt, Yt)
        print(f"{it:3d}  ELBO after the E-steps {elbo:12.3f}  test NLPD {nlpd:.4f}  accuracy {acc:.4f}", flush=True)


if __name__ == "__main__":
    main()
