"""Writes tests/golden/softmax/c3_steps.npz: four natural-gradient steps (lr 0.5) and the ELBO of the C = 3 problem of
tests/softmax_problem.py from the oracle driven by the NumPy restatement of the Softmax likelihood (tests/softmax_ref.py,
seed 3, draws 0 .. 4).  Run from the repository root:  python tests/golden/softmax/make_golden.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

from oracle import tsvgp_oracle as O  # noqa: E402
from tests.softmax_problem import problem  # noqa: E402
from tests.softmax_ref import Softmax, normals  # noqa: E402

X, Y, Z = problem()
ora = O.t_SVGP(O.Matern52(1.0, 1.5), Softmax(3, seed=3), Z, num_latent_gps=3, num_data=len(X))
l1, L2 = [], []
for _ in range(4):
    ora.natgrad_step((X, Y), lr=0.5)
    l1.append(ora.lambda_1.copy())
    L2.append(ora.lambda_2.copy())
elbo = ora.elbo((X, Y))
np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "c3_steps.npz"), X=X, Y=Y, Z=Z, lambda_1=np.stack(l1),
         lambda_2=np.stack(L2), elbo=elbo, normals=normals(3, 2, np.arange(5, 9), 4, 3))
