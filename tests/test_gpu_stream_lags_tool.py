"""GPU tests of the tools of the lag call.  The command line tool's -A prints the lag Context.align_streams finds.  The timing tool
(tools/stream_lags.py on tools/stream_timing.py) runs as a fresh process with arguments so small that a run takes seconds: its own
answers checks (the library's tables against the torch recipes') must be true, and the JSON line it prints has the keys of
tests/golden/stream_lags_keys.json.  Its "met" / "MISSED" verdicts are about timing and are not asserted at these sizes."""
import json
import os
import re
import subprocess
import sys

import pytest

from signals import music
from stream_consumers import encoded
from test_cli_cpu import CLI
from test_gpu_stream_tools import SMALL, answers, key_structure

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = ["--lags", "40", "--wide-lags", "300", "--needle-seconds", "0.01", "--unfold-lags", "64"]


def test_the_tool_prints_its_keys_and_its_answers_are_equal():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stream_lags.py"), *OWN, *SMALL], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    result = json.loads(r.stdout.splitlines()[-1])
    got = answers(result)
    assert len(got) >= 3 and all(a is True for a in got), got
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "stream_lags_keys.json")))
    assert key_structure(result) == want
    cases = [result["one_stream"]["needle_against_the_stream_pm_40"], result["one_stream"]["needle_against_the_stream_pm_300"], result["clips"]["each_against_its_neighbour_pm_40"]]
    assert [c["probes"] for c in cases] == [1, 1, 4] and [c["lags"] for c in cases] == [81, 601, 81]
    for c in cases:
        assert c["criteria"]["faster_than_the_recipe_beyond_the_spread"].startswith(("met: ", "MISSED: ")) and c["recipe_is"] in ("recipe_int64_unfold", "recipe_float64_conv1d")


def test_command_line_tool(ctx, oracle, tmp_path):
    assert os.path.exists(CLI), "linne_amd_cli is not built (python -c 'import __graft_entry__ as g; g.build()')"
    src, other = tmp_path / "a.lnn", tmp_path / "b.lnn"
    a = encoded(ctx, oracle, music(2, 3 * 1024 + 300, 16, seed=92), 16, 5, True, "2ch")
    delayed = ctx.splice_streams([[(a.dev, a.index, 1700, 1234), (a.dev, a.index, 0, None)]])[0]
    src.write_bytes(a.stream)
    other.write_bytes(bytes(delayed.cpu().numpy().tobytes()))
    for spec, kw in ((f"{other},2000,0,1500", dict(max_lag=2000, needle=(0, 1500))), (f"{other},1300", dict(max_lag=1300)), (str(other), dict(max_lag=4096))):
        r = subprocess.run([CLI, "-A", spec, str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        (lag, coef), = ctx.align_streams([(a.dev, delayed)], kw["max_lag"], needle=kw.get("needle"))
        lines = r.stdout.splitlines()
        assert len(lines) == 3 and lines[0].startswith("channel 0: lag ") and lines[1].startswith("channel 1: lag ")
        m = re.fullmatch(r"all 2 channels: lag (-?\d+) correlation (\S+) ", lines[2])
        assert m and int(m.group(1)) == lag == 1234 and abs(float(m.group(2)) - coef) < 1e-8, (spec, r.stdout)
    a.index.close()
