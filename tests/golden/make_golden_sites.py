"""Regenerates the t_SVGP_sites fixtures under tests/golden/sites/ from the NumPy restatement (tests/sites_ref.py):
    python -m tests.golden.make_golden_sites
Each file holds the problem (X, Y, Z, hyperparameters, lr) and the sites after steps 1, 2 and 10 with the ELBO there."""
import os

import numpy as np

from oracle import tsvgp_oracle as O
from tests.helpers import synthetic
from tests.sites_ref import t_SVGP_sites

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sites")
STEPS = (1, 2, 10)


def make(lik, N=400, M=24, D=2, lr=0.7, seed=3):
    X, Y, _ = synthetic(N, M, D, 1, lik, seed=seed)
    Z = X[::N // M][:M].copy()
    kern = O.SquaredExponential(variance=1.0, lengthscales=1.0)
    L = O.Gaussian(variance=0.1) if lik == "gaussian" else O.Bernoulli()
    m = t_SVGP_sites((X, Y), kern, L, Z)
    out = dict(X=X, Y=Y, Z=Z, lr=lr, variance=1.0, lengthscales=1.0, noise=0.1, steps=np.array(STEPS))
    for s in range(1, max(STEPS) + 1):
        m.natgrad_step(lr=lr)
        if s in STEPS:
            out[f"lambda_1_{s}"], out[f"lambda_2_{s}"], out[f"elbo_{s}"] = m.lambda_1, m.lambda_2, m.elbo()
    return out


if __name__ == "__main__":
    os.makedirs(HERE, exist_ok=True)
    for lik in ("gaussian", "bernoulli"):
        path = os.path.join(HERE, f"sites_{lik}_d2.npz")
        np.savez_compressed(path, **make(lik))
        print(path, os.path.getsize(path))
