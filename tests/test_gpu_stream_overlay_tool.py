"""GPU tests of the tools of the overlay calls.  The command line tool's -J writes the file Context.crossfade_streams writes.  The timing
tool (tools/stream_overlay.py on tools/stream_timing.py) runs as a fresh process with arguments so small that a run takes seconds: its
own answers checks (the library's answer against the torch recipe's) must be true, and the JSON line it prints has its cases, their
figures and their criteria.  Its "met" / "MISSED" verdicts are about timing and are not asserted at these sizes."""
import json
import os
import subprocess
import sys

import pytest

from signals import music
from stream_consumers import encoded
from test_cli_cpu import CLI
from test_gpu_stream_tools import SMALL, answers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = {"median_ms", "min_ms", "max_ms", "spread_ms"}


def test_the_tool_prints_its_keys_and_its_answers_are_equal():
    assert SMALL == ["--minutes", "0.01", "--clips", "4", "--clip-seconds", "0.05", "--reps", "2"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stream_overlay.py"), *SMALL], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    result = json.loads(r.stdout.splitlines()[-1])
    got = answers(result)
    assert len(got) == 3 and all(a is True for a in got), got
    assert {"config", "reps", "statistic", "one_stream", "clips"} <= set(result)
    cases = [result["one_stream"]["with_itself_a_second_later_int32"], result["clips"]["under_the_next_clip_float32_channels_last"]]
    for case in cases:
        assert {"streams", "outputs", "sources_per_output", "output", "output_bytes", "answers_equal", "peak_memory", "decoded_pcm_bytes", "kind_101_bytes_moved", "criteria"} <= set(case)
        for name in ("overlay_windows", "recipe", "kind_101_one_unity_source", "kind_101_two_sources", "kind_101_the_case", "kind_100_identity_1_tap", "kind_59_k_wx_place",
                     "kind_59_k_wx_place_into_the_images", "overlay_windows_device_ms"):
            assert set(case[name]) == STATS, name
        assert set(case["peak_memory"]) == {"overlay_windows", "recipe"} and all("peak_bytes" in v for v in case["peak_memory"].values())
        assert set(case["criteria"]) == {"faster_than_the_recipe_beyond_the_spread", "lower_peak_memory_than_the_recipe", "one_source_under_kind_100s_floor", "two_sources_under_twice_one",
                                         "against_the_copy_kernel"}
        assert all(v.startswith(("met: ", "MISSED: ")) for k, v in case["criteria"].items() if k != "against_the_copy_kernel")
    assert cases[0]["outputs"] == 1 and cases[1]["outputs"] == 4 and cases[0]["sources_per_output"] == cases[1]["sources_per_output"] == 2
    join = result["clips"]["join"]
    assert {"streams", "overlap_samples", "answers_equal", "stream_bytes", "peak_memory", "crossfade_streams", "recipe", "criteria"} <= set(join) and join["streams"] == 4
    assert set(join["criteria"]) == {"not_slower_than_the_recipe_beyond_the_spread", "lower_peak_memory_than_the_recipe"}


def test_command_line_tool(ctx, oracle, tmp_path):
    assert os.path.exists(CLI), "linne_amd_cli is not built (python -c 'import __graft_entry__ as g; g.build()')"
    src, other, dst = tmp_path / "a.lnn", tmp_path / "b.lnn", tmp_path / "c.lnn"
    two = encoded(ctx, oracle, music(2, 3 * 1024 + 300, 16, seed=92), 16, 5, True, "2ch")
    more = encoded(ctx, oracle, music(2, 2 * 1024 + 77, 24, seed=94), 24, 2, False, "2ch, 24 bits")
    three = encoded(ctx, oracle, music(3, 2 * 1024 + 77, 24, seed=93), 24, 0, False, "3ch")
    for a, b, overlap in ((two, more, None), (two, more, 0), (two, more, 1), (more, two, 257), (two, two, 3 * 1024 + 300), (three, three, 1000), (two, more, 2 * 1024 + 77)):
        src.write_bytes(a.stream)
        other.write_bytes(b.stream)
        spec = str(other) if overlap is None else f"{other},{overlap}"
        r = subprocess.run([CLI, "-J", spec, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        want = ctx.crossfade_streams([a.dev, b.dev], overlap or 0)
        assert dst.read_bytes() == bytes(want.cpu().numpy().tobytes()), spec
    for t in (two, more, three):
        t.index.close()
