"""GPU tests of the tools of the resample calls.  The command line tool's -Z writes the file Context.resample_streams writes.  The timing
tool (tools/stream_resample.py on tools/stream_timing.py) runs as a fresh process with arguments so small that a run takes seconds: its
own answers checks (the library's answer against the torch float64 conv1d recipe's) must be true, and the nested keys of the JSON line
it prints are held to tests/golden/stream_resample_keys.json.  Its "met" / "MISSED" verdicts are about timing and are not asserted at
these sizes."""
import json
import os
import subprocess
import sys

import pytest

import linne_amd
from signals import music
from stream_consumers import encoded
from test_cli_cpu import CLI
from test_gpu_stream_tools import SMALL, answers, key_structure

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stream_resample_keys.json")


def test_the_tool_prints_its_keys_and_its_answers_are_equal():
    assert SMALL == ["--minutes", "0.01", "--clips", "4", "--clip-seconds", "0.05", "--reps", "2"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stream_resample.py"), *SMALL], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    result = json.loads(r.stdout.splitlines()[-1])
    got = answers(result)
    assert len(got) == 4 and all(a is True for a in got), got
    with open(GOLDEN) as f:
        assert key_structure(result) == json.load(f)


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_command_line_tool(ctx, oracle, tmp_path):
    src, dst = tmp_path / "a.lnn", tmp_path / "b.lnn"
    two = encoded(ctx, oracle, music(2, 3 * 1024 + 300, 16, seed=92), 16, 5, True, "2ch")
    three = encoded(ctx, oracle, music(3, 2 * 1024 + 77, 24, seed=93), 24, 0, False, "3ch")
    for t, spec, rate, taps in ((two, "16000", 16000, 32), (two, "48000,16", 48000, 16), (three, "22050,64", 22050, 64), (two, "44100,1", 44100, 1)):
        src.write_bytes(t.stream)
        r = subprocess.run([CLI, "-Z", spec, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        want, = ctx.resample_streams([t.dev], rate, taps=taps)
        assert dst.read_bytes() == bytes(want.cpu().numpy().tobytes()), spec
    for t in (two, three):
        t.index.close()
