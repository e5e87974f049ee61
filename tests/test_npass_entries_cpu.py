"""``estep.per_latent``, the selection of one latent's operand from the forms the models hand to ``EStepEngine.run``: host logic,
no GPU."""
import torch

from tests.helpers import pkg

P, M = 3, 4


def test_per_latent_takes_the_five_forms():
    estep = pkg().estep
    per_latent = estep.per_latent
    mats = [torch.full((M, M), float(p)) for p in range(P)]
    stacked, shared = torch.stack(mats), torch.full((M, M), 9.0)
    for p in range(P):
        assert per_latent(None, p) is None
        assert per_latent(mats, p) is mats[p]
        assert per_latent(tuple(mats), p) is mats[p]
        assert per_latent(stacked, p).shape == (M, M) and torch.equal(per_latent(stacked, p), mats[p])
        assert per_latent(shared, p) is shared
    # per-latent routes: a list may hold None for a latent that works on K(X, Z) itself
    assert per_latent([None, mats[1]], 0) is None and per_latent([None, mats[1]], 1) is mats[1]
    assert estep.EStepEngine._per_latent is per_latent  # the alias full_cov and _batch_plan use
