#!/usr/bin/env python3
"""Multi-class classification with t-SVGP: the t-SVGP branch of the reference's docs/notebooks/mnist.py on synthetic 10-class data
generated here, on one MI355X.  One shared Matern-5/2 ARD kernel over C = 10 latent GPs, the Softmax likelihood (Monte Carlo, 100
draws made inside the kernel), M = 100 inducing points at the first M inputs; per iteration 8 minibatch natural-gradient E-steps
and 20 Adam M-steps (kernel variance, lengthscales and inducing inputs) on minibatches of 200, then the ELBO of a fixed
evaluation batch, the test NLPD and the test accuracy.

    python examples/multiclass.py [--n 10000] [--d 16] [--iters 20]        # --d 784: the MNIST input size (large-D fill)
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tsvgp_amd as gpf  # noqa: E402  (alias of the package directory t-svgp_amd/)


def make_data(n, n_test, d, c, seed=0):
    """Inputs in [0, 1]^d (as scaled pixels), labels = argmax of c smooth random scores; (X, Y [n, 1], Xtest, Ytest)."""
    rng = np.random.RandomState(seed)
    X = rng.rand(n + n_test, d)
    W, b = rng.randn(d, c) * (4.0 / np.sqrt(d)), rng.rand(c) * 2 * np.pi
    scores = np.sin(X @ W + b) + 0.1 * rng.randn(n + n_test, c)
    Y = np.argmax(scores, axis=1)[:, None].astype(np.float64)
    return X[:n], Y[:n], X[n:], Y[n:]


def make_model(X, c, m, num_data, seed=0, **kw):
    d = X.shape[1]
    Z = X[:m].copy()  # the notebook's choice
    kernel = gpf.Matern52(variance=1.0, lengthscales=np.full(d, float(np.sqrt(d))))  # ARD; sqrt(d): unit scale per unit distance
    model = gpf.t_SVGP(kernel, gpf.Softmax(c, seed=seed), Z, num_data=num_data, num_latent_gps=c, **kw)
    return model, Z


def e_steps(model, X, Y, batch, steps, lr, rng, on_batch=None):
    for _ in range(steps):
        idx = rng.choice(len(X), min(batch, len(X)), replace=False)
        if on_batch is not None:
            on_batch(idx)
        model.natgrad_step((X[idx], Y[idx]), lr=lr)


def m_steps(model, X, Y, batch, steps, opt, rng):
    for _ in range(steps):
        idx = rng.choice(len(X), min(batch, len(X)), replace=False)
        gpf.training.m_step(model, (X[idx], Y[idx]), opt, steps=1)


def evaluate(model, Xt, Yt):
    nlpd = -float(torch.mean(model.predict_log_density((Xt, Yt))))
    pred = model.predict_y(Xt)[0].argmax(dim=1).cpu().numpy()
    return nlpd, float(np.mean(pred == Yt[:, 0]))


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
    args = ap.parse_args()
    X, Y, Xt, Yt = make_data(args.n, args.n_test, args.d, args.classes)
    model, _ = make_model(X, args.classes, args.m, args.n)
    opt = gpf.training.Adam(args.adam_lr)
    rng = np.random.RandomState(1)
    Xe, Ye = X[:2000], Y[:2000]  # the batch the ELBO is reported on
    for it in range(args.iters):
        e_steps(model, X, Y, args.batch, args.e_steps, args.nat_lr, rng)
        m_steps(model, X, Y, args.batch, args.m_steps, opt, rng)
        nlpd, acc = evaluate(model, Xt, Yt)
        print(f"{it:3d}  ELBO {float(model.elbo((Xe, Ye))):12.3f}  test NLPD {nlpd:.4f}  accuracy {acc:.4f}", flush=True)


if __name__ == "__main__":
    main()
