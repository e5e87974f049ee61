"""The target-shape rule in front of ``EStepEngine.lik_map`` (``EStepEngine._check_y``) for all seven likelihood ids, and the one
``num_latent_gps`` check of ``t_SVGP``: host logic, no GPU."""
import numpy as np
import pytest
import torch

from tests.helpers import pkg

N = 10


def _coupled():
    """(lik_id, lik_param as the model passes it, latent_dim) of every coupled likelihood."""
    p = pkg()
    B = p._backend
    return [(B.LIK_HETERO, 0.0, 2), (B.LIK_SOFTMAX, p.Softmax(3), 3), (B.LIK_SOFTMAX, p.Softmax(5), 5), (B.LIK_MULTICLASS, p.MultiClass(3), 3)]


def _uncoupled():
    p = pkg()
    B = p._backend
    return [(B.LIK_GAUSSIAN, 0.1), (B.LIK_BERNOULLI, 0.0), (B.LIK_STUDENT_T, (1.0, 3.0)), (B.LIK_POISSON, (1.0, 0.0))]


def test_the_cases_cover_every_likelihood_id():
    B = pkg()._backend
    ids = {c[0] for c in _coupled()} | {c[0] for c in _uncoupled()}
    assert ids == {B.LIK_GAUSSIAN, B.LIK_BERNOULLI, B.LIK_HETERO, B.LIK_SOFTMAX, B.LIK_STUDENT_T, B.LIK_POISSON, B.LIK_MULTICLASS}
    assert {c[0] for c in _coupled()} == set(B.COUPLED_LIKS)


@pytest.mark.parametrize("nocrop", [False, True])
def test_check_y_coupled(nocrop):
    p = pkg()
    check, B = p.estep.EStepEngine._check_y, p._backend
    y = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    for lik_id, lik_param, C in _coupled():
        lik_id |= B.LIK_NOCROP if nocrop else 0
        check(y(N, 1), N, C, lik_id, lik_param)  # one target column for C latents
        for P in (1, C - 1, C + 1):
            with pytest.raises(ValueError, match="latent GPs"):
                check(y(N, 1), N, P, lik_id, lik_param)
        for bad in (y(N, 2), y(N, C), y(N), y(N - 1, 1), None):
            with pytest.raises(ValueError, match=r"Y \[N, 1\]"):
                check(bad, N, C, lik_id, lik_param)


def test_check_y_messages_name_the_likelihood():
    p = pkg()
    check, B = p.estep.EStepEngine._check_y, p._backend
    Y = torch.zeros(N, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"the heteroskedastic likelihood needs 2 latent GPs .* got P = 3 and Y \(10, 1\)"):
        check(Y, N, 3, B.LIK_HETERO, 0.0)
    with pytest.raises(ValueError, match=r"the Softmax likelihood needs 3 latent GPs \(its latent_dim\)"):
        check(Y, N, 2, B.LIK_SOFTMAX, p.Softmax(3))
    with pytest.raises(ValueError, match="the MultiClass likelihood needs 3 latent GPs"):
        check(Y, N, 2, B.LIK_MULTICLASS, p.MultiClass(3))


@pytest.mark.parametrize("nocrop", [False, True])
def test_check_y_uncoupled(nocrop):
    p = pkg()
    check, B = p.estep.EStepEngine._check_y, p._backend
    y = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    for lik_id, lik_param in _uncoupled():
        lik_id |= B.LIK_NOCROP if nocrop else 0
        for P in (1, 2, 3):
            check(y(N, P), N, P, lik_id, lik_param)  # one target column per latent
        for bad in (y(N, 1), y(N, 3), y(N), y(N - 1, 2)):
            with pytest.raises(ValueError, match=r"Y must be \[N, P\]"):
                check(bad, N, 2, lik_id, lik_param)


def test_model_checks_num_latent_gps_once_for_every_coupled_likelihood():
    p = pkg()
    Z = np.random.RandomState(0).randn(6, 2)
    with pytest.raises(ValueError, match=r"the heteroskedastic likelihood needs num_latent_gps = 2 \(its latent_dim\), got 3"):
        p.t_SVGP(p.SquaredExponential(), p.HeteroskedasticTFPConditional(), Z, num_latent_gps=3)
    with pytest.raises(ValueError, match=r"the heteroskedastic likelihood .*latent_dim"):
        p.t_SVGP(p.SquaredExponential(), p.HeteroskedasticTFPConditional(), Z, num_latent_gps=1)
    for lik, name in ((p.Softmax(3), "Softmax"), (p.MultiClass(3), "MultiClass")):
        with pytest.raises(ValueError, match=rf"the {name} likelihood needs num_latent_gps = 3 \(its latent_dim\), got 2"):
            p.t_SVGP(p.SquaredExponential(), lik, Z, num_latent_gps=2)
    p.t_SVGP(p.SquaredExponential(), p.HeteroskedasticTFPConditional(), Z, num_latent_gps=2)
    p.t_SVGP(p.SquaredExponential(), p.StudentT(), Z, num_latent_gps=3)  # uncoupled: any number of latents
