"""Side-stream work of the E-step: the one place that forks work off the current stream, joins it again and keeps its tensors
alive in between.  The only code of the package beside the profiling event pool of ``EStepEngine`` that creates a stream or
an event, waits for one or calls ``record_stream``.

The E-step overlaps two pieces of work with the main stream: the N-sized K(X, Z) fill beside the M x M prelude
(``EStepEngine.start_fill``) and the epilogue's three M^3 GEMMs beside the moments kernel (``t_SVGP._site_operands``).  Both
also run inside hipGraph captures, where the side stream JOINS the capture: it waits for an event recorded on the capturing
stream (the fork) and the consumer waits for the branch's end event (the join) inside the same capture, so a replayed step
overlaps exactly what an eager one does.

The lifetime rule.  Every tensor a branch reads or writes must stay allocated until the consuming stream has waited for the
branch.  Eagerly ``record_stream`` sees to that.  Inside a capture nothing does: ``record_stream`` means nothing to a graph's
private pool, a block freed between fork and join goes straight back to that pool, the next allocation on the capturing stream
takes it, and in the replayed graph that kernel runs BESIDE the branch still reading the block.  So the branch object itself
holds a reference to every tensor of ``reads`` and ``writes`` until ``join`` -- in both modes: the lifetime does not depend on
who else happens to hold the tensor.

The rule was broken twice while it was a convention of the call sites.  Round 4, the fp32 copy of Z in ``start_fill``, found by
the two-rank fp32 test of BASELINE configs[3] (fp32: Z [M, D] is converted into a temporary; fp64 passes its tensors through,
which is why three rounds of fp64 tests never saw it): the state after four replayed steps was off by 1e-5 ... 0.4, differently
on every run (profiles/r04_c4_fork_capture_race.txt).  Round 5, L^T of ``_site_operands``, read by the forked L L^T: the state
off by 0.21.  tests/test_gpu_side_branch.py makes a violation deterministic: the allocator must not hand out a held block.
"""
from __future__ import annotations

import contextlib
import time

import torch


class SideBranch:
    """One forked piece of work and the ticket for it.  ``name`` / ``buf`` / ``key``: what a consumer checks before it takes the
    result -- the engine's buffer the branch wrote, the name it is cached under and, for the shared-kernel fill, what it was
    filled from.  A branch that never left the current stream (``SideBranch.inline``) is the same ticket."""

    def __init__(self, device, consumer, held=(), name=None, buf=None, key=None):
        self.device, self.name, self.buf, self.key = device, name, buf, key
        self._consumer = consumer  # the stream that forked: ``produced`` tensors are its to read
        self._held = tuple(held)
        self._event = None
        self._eager = not torch.cuda.is_current_stream_capturing()  # record_stream means nothing to a graph's private pool

    @classmethod
    def inline(cls, device, reads=(), **payload):
        """A branch that ends here on the current stream: an event on that stream plus the payload."""
        stream = torch.cuda.current_stream(device)
        branch = cls(device, stream, reads, **payload)
        branch._end(stream)
        return branch

    def _end(self, stream):
        self._event = torch.cuda.Event()
        self._event.record(stream)

    def produced(self, *tensors):
        """Tensors allocated inside the body that the joining stream will consume (blocks of the side stream's pool)."""
        if self._eager:
            for t in tensors:
                t.record_stream(self._consumer)

    def join(self):
        """The current stream waits for the branch's end; the held references are dropped.  A second call does nothing."""
        if self._event is not None:
            torch.cuda.current_stream(self.device).wait_event(self._event)
            self._event, self._held = None, ()

    def take(self, name, buf):
        """``join`` for a consumer about to read ``buf``, cached as ``name``: the ticket must be the one of that buffer."""
        if self.name != name or self.buf is not buf:
            raise RuntimeError("prefill ticket does not belong to this pass")
        self.join()


class SideStream:
    """The side stream of one engine, created by the first fork."""

    def __init__(self, device):
        self.device = device
        self.stream = None

    @contextlib.contextmanager
    def fork(self, reads=(), writes=(), **payload):
        """``with fork(reads, writes) as branch:`` runs the body on the side stream, behind everything the current stream holds
        at this point (the buffers' last readers, conversions of the inputs), and ends the branch behind it.  The branch keeps
        ``reads`` and ``writes`` alive until ``branch.join()`` (the module's docstring has the rule and its history)."""
        main = torch.cuda.current_stream(self.device)
        if self.stream is None:
            self.stream = torch.cuda.Stream(self.device)
        side = self.stream
        branch = SideBranch(self.device, main, tuple(reads) + tuple(writes), **payload)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            yield branch
            branch._end(side)
        if branch._eager:
            for t in branch._held:  # blocks of the main stream's allocator pool that the side stream touches
                t.record_stream(side)

    def wait_stale(self):
        """A branch started for a pass that never ran must not land on top of the one about to start in line (a capture begins
        synchronised)."""
        if self.stream is not None and not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(self.device).wait_stream(self.stream)


def poll_current_stream(device):
    """Returns when everything enqueued on the current stream has retired, by polling an event instead of sleeping on an
    interrupt.  The poll yields between queries: other Python threads (loaders, logging) keep running."""
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    while not ev.query():
        time.sleep(0)  # gives up the GIL and the time slice
