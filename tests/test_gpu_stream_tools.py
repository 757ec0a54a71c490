"""GPU test of the stream timing tools (tools/stream_*.py on tools/stream_timing.py): each runs as a fresh process with arguments so
small that a run takes seconds -- every case still has two buckets or more per stream --, and the nested keys of the JSON line it
prints are held to tests/golden/stream_tools_keys.json, recorded from the tools as they stood before they shared a harness.  The
tools' own answers checks (the library's answer against the recipe's) must be true; their "met" / "MISSED" verdicts are about timing
and are not asserted at these sizes."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stream_tools_keys.json")
SMALL = ["--minutes", "0.01", "--clips", "4", "--clip-seconds", "0.05", "--reps", "2"]
ARGS = {"stream_measure": SMALL, "stream_digest": SMALL, "stream_quiet": SMALL, "stream_histogram": SMALL, "stream_relate": SMALL, "stream_compare": SMALL,
        "stream_windows": ["--minutes", "0.05", "--tracks", "2", "--track-minutes", "0.02", "--windows", "4", "--window-seconds", "0.1", "--reps", "2"]}


def key_structure(v):
    """the keys of a JSON value, nested as it nests them; a leaf is null, a list the structure of its elements"""
    if isinstance(v, dict):
        return {k: key_structure(x) for k, x in v.items()}
    if isinstance(v, list):
        return [key_structure(x) for x in v]
    return None


def answers(v, found=None):
    """every answers check of a tool's result: the values under answers_equal, answers and exact, wherever they nest"""
    found = [] if found is None else found
    if isinstance(v, dict):
        for k, x in v.items():
            if k in ("answers_equal", "answers", "exact"):
                found += list(x.values()) if isinstance(x, dict) else [x]
            else:
                answers(x, found)
    return found


def run_tool(name):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name + ".py"), *ARGS[name]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


@pytest.mark.parametrize("name", sorted(ARGS))
def test_the_tool_prints_the_keys_it_printed(name):
    result = run_tool(name)
    got = answers(result)
    assert got and all(a is True for a in got), got
    with open(GOLDEN) as f:
        assert key_structure(result) == json.load(f)[name]
