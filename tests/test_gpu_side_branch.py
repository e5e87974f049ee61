"""The owner of side-stream work (t-svgp_amd/side_branch.py through ``EStepEngine.fork`` / ``start_fill`` / ``project_diag`` /
``private_buffers``): what a branch holds and for how long, eagerly and inside a hipGraph capture, the stale-fill rule, the
ticket checks.  N = 300, M = 40: neither a multiple of 128, so padding rows and columns exist.  Everything here asserts the sound
behaviour; equalities are bit for bit (the same kernels in the same order on each stream, and they use no atomics)."""
import gc
import weakref
from importlib import import_module

import numpy as np
import pytest
import torch

from tests.helpers import pkg, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, M, D = 300, 40, 3


def _engine(dtype=torch.float64):
    return import_module("t-svgp_amd.estep").EStepEngine(dtype)


def _problem():
    """X, Y, Z on the device (fp64), a kernel, and moment operands small enough that every predictive variance is positive."""
    p = pkg()
    X, Y, Z = (torch.as_tensor(a, dtype=torch.float64, device=DEV) for a in synthetic(N, M, D, seed=3))
    rng = np.random.RandomState(5)
    Tm = torch.as_tensor(np.triu(rng.rand(1, M, M)) * (0.3 / M), dtype=torch.float64, device=DEV)
    gamma = torch.as_tensor(rng.randn(M, 1) / M, dtype=torch.float64, device=DEV)
    return X, Y, Z, p.SquaredExponential(variance=1.0, lengthscales=0.8), Tm, gamma


def _run(eng, prob, **kw):
    B = pkg()._backend
    X, Y, Z, kernel, Tm, gamma = prob
    return eng.run(X, Y, Z, kernel, moment_Tm=Tm, moment_mode=B.TRI_UPPER, gamma=gamma, lik_id=B.LIK_GAUSSIAN, lik_param=0.1,
                   sites=True, want_moments=True, **kw)


def _fork_then_reallocate(eng, dtype, out):
    """Steps 1-6 of the lifetime check: a tensor of the current stream is handed to a branch and dropped by the caller; the next
    allocation of that size on the current stream must get another block, because the branch still reads this one."""
    t = torch.full((out.numel(),), 3.0, dtype=dtype, device=DEV)
    ptr = t.data_ptr()
    with eng.fork(reads=(t,)) as branch:
        out.copy_(t)
    del t
    u = torch.empty(out.numel(), dtype=dtype, device=DEV)
    u.fill_(-1.0)  # work of the forking stream between fork and join: in a replay it runs beside the branch
    assert u.data_ptr() != ptr
    branch.join()
    return u


@pytest.mark.parametrize("mode, dtype", [("capture", torch.float64), ("capture", torch.float32), ("eager", torch.float64)],
                         ids=["capture-fp64", "capture-fp32", "eager-fp64"])
def test_fork_keeps_what_it_reads_allocated_until_join(mode, dtype):
    eng = _engine(dtype)
    out = torch.zeros(1000, dtype=dtype, device=DEV)
    assert not eng.side_open
    with eng.fork() as first:  # (opens the side stream outside any capture)
        pass
    first.join()
    assert eng.side_open
    torch.cuda.synchronize()
    if mode == "capture":
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            u = _fork_then_reallocate(eng, dtype, out)
        out.zero_()
        torch.cuda.synchronize()
        graph.replay()
    else:
        u = _fork_then_reallocate(eng, dtype, out)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 3.0))
    assert torch.equal(u, torch.full_like(u, -1.0))


def test_references_are_released_at_join():
    eng = _engine()
    out = torch.zeros(1000, dtype=torch.float64, device=DEV)
    t = torch.ones(1000, dtype=torch.float64, device=DEV)
    ref = weakref.ref(t)
    with eng.fork(reads=(t,)) as branch:
        out.copy_(t)
    assert ref() is not None
    del t
    gc.collect()
    assert ref() is not None
    branch.join()
    gc.collect()
    assert ref() is None
    branch.join()  # a second join does nothing
    torch.cuda.synchronize()
    assert torch.equal(out, torch.ones_like(out))


def test_stale_fill_does_not_reach_the_next_pass():
    prob = _problem()
    X, _, Z, kernel = prob[:4]
    want = _run(_engine(), prob)
    eng = _engine()
    assert eng.start_fill(X, Z, kernel) is not None  # started and never consumed
    in_line = _run(eng, prob)
    ticket = eng.start_fill(X, Z, kernel)
    assert ticket is not None
    prefilled = _run(eng, prob, prefill=ticket)
    torch.cuda.synchronize()
    for got in (in_line, prefilled):
        for name in ("acc2", "acc1", "mean", "var"):
            assert torch.equal(getattr(got, name), getattr(want, name)), name


def test_foreign_tickets_are_refused():
    prob = _problem()
    X, _, Z, kernel, Tm, gamma = prob
    B = pkg()._backend
    mine, other = _engine(), _engine()
    ticket = mine.start_fill(X, Z, kernel)
    with pytest.raises(RuntimeError, match="prefill ticket does not belong to this pass"):
        _run(other, prob, prefill=ticket)
    ticket.join()
    w = torch.zeros((B.round_up(N), 1), dtype=torch.float64, device=DEV)
    w[:N] = 1.0
    _, _, ticket = mine.project_diag(X, Z, kernel, w, w)
    kw = dict(whiten_T=None, moment_Tm=Tm, moment_mode=B.TRI_UPPER, gamma=gamma)
    with pytest.raises(RuntimeError, match="needs the ticket of this engine's last project_diag"):
        other.diag_sites_moments(X, Z, kernel, ticket, **kw)
    mean, var = mine.diag_sites_moments(X, Z, kernel, ticket, **kw)  # its own engine takes it
    torch.cuda.synchronize()
    assert mean.shape == (N, 1) and bool(torch.isfinite(mean).all()) and bool((var > 0).all())


def test_private_buffers_restores_the_engines_own_on_error():
    prob = _problem()
    eng = _engine()
    _run(eng, prob, b_tag=("warm", 1))
    buf, tag, kfu = eng._buf, eng._b_tag, eng._buf["Kfu"]
    assert tag is not None
    with pytest.raises(ValueError, match="inside"):
        with eng.private_buffers() as private:
            assert private is eng._buf and private is not buf and not private and eng._b_tag is None
            _run(eng, prob, b_tag=("warm", 2))
            assert private["Kfu"] is not kfu and eng._b_tag is not None
            raise ValueError("inside")
    assert eng._buf is buf and eng._b_tag is tag and eng._buf["Kfu"] is kfu
    torch.cuda.synchronize()
