"""GPU test of the timing tool of the mix calls (tools/stream_mix.py on tools/stream_timing.py): it runs as a fresh process with
arguments so small that a run takes seconds, its own answers checks (the library's answer against the recipe's) must be true, and the
nested keys of the JSON line it prints are held to tests/golden/stream_mix_keys.json.  Its "met" / "MISSED" verdicts are about timing
and are not asserted at these sizes."""
import json
import os
import subprocess
import sys

import pytest

from test_gpu_stream_tools import SMALL, answers, key_structure

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stream_mix_keys.json")


def test_the_tool_prints_its_keys_and_its_answers_are_equal():
    assert SMALL == ["--minutes", "0.01", "--clips", "4", "--clip-seconds", "0.05", "--reps", "2"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stream_mix.py"), *SMALL], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    result = json.loads(r.stdout.splitlines()[-1])
    got = answers(result)
    assert len(got) == 5 and all(a is True for a in got), got
    with open(GOLDEN) as f:
        assert key_structure(result) == json.load(f)
