"""GPU tests of the tools of the project call.  The command line tool's -F prints the sums Context.spectrum_streams returns.  The timing
tool (tools/stream_project.py on tools/stream_timing.py) runs as a fresh process with arguments so small that a run takes seconds: its
own answers checks (the library's tables against the torch recipe's) must be true, and the JSON line it prints has the keys of
tests/golden/stream_project_keys.json.  Its "met" / "MISSED" verdicts are about timing and are not asserted at these sizes."""
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


def test_the_tool_prints_its_keys_and_its_answers_are_equal():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stream_project.py"), *SMALL], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    result = json.loads(r.stdout.splitlines()[-1])
    got = answers(result)
    assert len(got) == 3 and all(a is True for a in got), got
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "stream_project_keys.json")))
    assert key_structure(result) == want
    cases = [result["one_stream"]["stft_512_hop_128"], result["one_stream"]["bank_64x400_hop_160_at_16_kHz"], result["clips"]["stft_512_hop_128_float32_rows_first"]]
    assert [c["windows"] for c in cases] == [1, 1, 4] and [c["rows"] for c in cases] == [514, 64, 514]
    for c in cases:
        assert all(v.startswith(("met: ", "MISSED: ")) for v in c["criteria"].values())


def test_command_line_tool(ctx, oracle, tmp_path):
    assert os.path.exists(CLI), "linne_amd_cli is not built (python -c 'import __graft_entry__ as g; g.build()')"
    src = tmp_path / "a.lnn"
    a = encoded(ctx, oracle, music(2, 3 * 1024 + 300, 16, seed=92), 16, 5, True, "2ch")
    src.write_bytes(a.stream)
    for spec, n_fft, hop in (("64,16", 64, 16), ("512,128", 512, 128), ("100", 100, 25), ("1", 1, 1)):
        r = subprocess.run([CLI, "-F", spec, str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        want, = ctx.spectrum_streams([a.dev], n_fft, hop)
        lines = r.stdout.splitlines()
        assert len(lines) == n_fft // 2 + 1
        for j, line in enumerate(lines):
            m = re.fullmatch(r"bin (\d+) (\S+) Hz: (\d+) (\d+) ", line)
            assert m and int(m.group(1)) == j and abs(float(m.group(2)) - j * 44100 / n_fft) < 1e-5 and [int(m.group(3)), int(m.group(4))] == [want[0][j], want[1][j]], (spec, line)
    # a range of samples: the frames that begin in it, which the Python form names
    r = subprocess.run([CLI, "-F", "64,16,40,2000", str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    z = ctx.stft_windows([(a.dev, a.index, 40, 2000)], 64, 16).cpu().numpy().astype(object)
    want = (z ** 2).sum(axis=(2, 4))[0]
    got = [[int(v) for v in line.split(": ")[1].split()] for line in r.stdout.splitlines()]
    assert got == [[int(want[c][j]) for c in range(2)] for j in range(33)]
    a.index.close()
