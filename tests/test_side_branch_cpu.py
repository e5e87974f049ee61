"""Side-stream work has one owner (t-svgp_amd/side_branch.py): nothing else in the package creates a stream or an event, waits
for one or calls ``record_stream``, except the pools of profiling events; no model reaches into the engine's stream or swaps its
buffers by hand."""
import glob
import os
import re

STREAM_CALLS = re.compile(r"record_stream|wait_event|wait_stream|torch\.cuda\.Event\(|torch\.cuda\.Stream\(")


def _lines(path):
    with open(path) as f:
        return list(enumerate(f.read().split("\n"), 1))


def test_models_leave_streams_and_engine_buffers_to_the_engine(repo_root):
    pattern = re.compile(STREAM_CALLS.pattern + r"|eng\._side|eng\._buf =|eng\._b_tag|dict\(event=")
    files = sorted(glob.glob(os.path.join(repo_root, "t-svgp_amd", "models", "*.py")))
    assert files
    hits = [(os.path.basename(f), n, line.strip()) for f in files for n, line in _lines(f) if pattern.search(line)]
    assert not hits, hits


def test_engine_touches_events_only_in_its_profiling_pool(repo_root):
    inside, hits = None, []
    for n, line in _lines(os.path.join(repo_root, "t-svgp_amd", "estep.py")):
        m = re.match(r"\s+def (\w+)\(", line)
        inside = m.group(1) if m else inside
        if (STREAM_CALLS.search(line) or "dict(event=" in line) and inside not in ("_event", "reserve_events"):
            hits.append((n, inside, line.strip()))
    assert not hits, hits
