"""GPU tests of finding the quiet runs of sample windows of resident .lnn streams (Context.quiet_windows, quiet_streams, the command
line tool's -S; include/linne_amd.h LINNEAmd_QuietWindowsDevice).  Every expected record, count and answer is computed with numpy
(test_stream_quiet_cpu.expected_quiet) from the oracle's decode of the same bytes, never from the library under test, and everything
must be equal.  Streams hold at most 8 blocks of 1024 samples, except the long stream of SILENT blocks."""
import os
import re
import subprocess

import numpy as np
import pytest

import linne_amd
from signals import music
import stream_consumers as sc
from stream_consumers import Stream, crc_damaged, encoded, to_device
from test_cli_cpu import CLI
from test_stream_quiet_cpu import (BASE_B, LONG_BLOCKS, MIXED_PLANTS, NS, S, TAIL, answer, expected_quiet, long_signal, made_loud, mixed_planted,
                                   planted_runs, planted_signal)

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CORRUPTION = 0, 1, 6
COMPRESS, SILENT, RAW = 0, 1, 2
SHAPES = [(nch, preset) for nch in (1, 2, 3) for preset in (0, 5)]
THRESHOLDS = [0, 3, 1 << 31]
MINS = [0, 1, 2, 64, 65, 257, 5000]
SENTINEL = 0x5A5A5A5A5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def streams(ctx, oracle):
    """1, 2 (MS) and 3 channels, presets 0 and 5, 3 blocks and a tail of 300, with planted silences"""
    out = {(nch, preset): encoded(ctx, oracle, planted_signal(nch, 30 + nch), 16, preset, nch == 2, f"{nch}ch -m {preset}") for nch, preset in SHAPES}
    yield out
    for t in out.values():
        t.index.close()


@pytest.fixture(scope="module")
def mixed(ctx, oracle):
    """stereo, 8 blocks: music, two SILENT, music, two RAW, music, a tail of 300; zeros planted across the blocks' ends"""
    t = encoded(ctx, oracle, mixed_planted(), 16, 5, True, "mixed")
    assert [b[2] for b in t.bl] == [COMPRESS, SILENT, SILENT, COMPRESS, RAW, RAW, COMPRESS, COMPRESS] and t.bl[-1][3] == TAIL
    yield t
    t.index.close()


@pytest.fixture(scope="module")
def long(ctx, oracle):
    t = encoded(ctx, oracle, long_signal(), 16, 0, True, "long")
    assert [b[2] for b in t.bl] == [COMPRESS] + [SILENT] * LONG_BLOCKS + [COMPRESS]
    yield t
    t.index.close()


def check(t, wins, thr, mins, got):
    for (first, n), th, mn, q in zip(wins, thr, mins, got):
        want = expected_quiet(t.full, first, n, th, mn)
        assert answer(q) == want, (t.name, first, n, th, mn)
        assert tuple(q.runs.shape) == (len(want[0]), 2)


def raw_call(ctx, items, group_frames=0):
    """LINNEAmd_QuietWindowsDevice itself.  items: (stream, index, first, n, threshold, min_samples, capacity, what is wrong with d_out);
    every window's table lies in one buffer of sentinels, a sentinel record in front of, between and behind the tables ->
    (ret, codes, answers as tuples, the buffer (records, 2) as numpy, the tables' first records)"""
    import torch
    offs, at = [], 1
    for it in items:
        offs.append(at)
        at += it[6] + 1
    buf = torch.full((at, 2), SENTINEL, dtype=torch.int64, device="cuda")
    W = len(items)
    w, sp, an = (linne_amd.Window * W)(), (linne_amd.QuietSpec * W)(), (linne_amd.Quiet * W)()
    for j, (dev, index, first, n, thr, mn, cap, wrong) in enumerate(items):
        w[j].index, w[j].d_stream, w[j].first_sample, w[j].num_samples, w[j].d_pcm, w[j].pcm_stride, w[j].result = index.h, dev.data_ptr(), first, n, None, 0, -1
        sp[j].threshold, sp[j].min_samples, sp[j].capacity = thr, mn, cap
        sp[j].d_out = buf.data_ptr() + 16 * offs[j] + (4 if wrong == "misaligned" else 0)
        if wrong == "null":
            sp[j].d_out = None
        an[j].num_runs = an[j].quiet_samples = an[j].lead_samples = an[j].trail_samples = SENTINEL
    torch.cuda.synchronize()
    ret = linne_amd.lib.LINNEAmd_QuietWindowsDevice(ctx.h, w, sp, an, W, group_frames)
    answers = [(int(a.num_runs), int(a.quiet_samples), int(a.lead_samples), int(a.trail_samples)) for a in an]
    return ret, [w[j].result for j in range(W)], answers, buf.cpu().numpy(), offs


def want_buffer(records, offs, tables):
    """sentinels but the given tables' records"""
    buf = np.full((records, 2), SENTINEL, dtype=np.int64)
    for off, runs in zip(offs, tables):
        for k, r in enumerate(runs):
            buf[off + k] = r
    return buf


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,preset", SHAPES)
def test_exactness(ctx, streams, nch, preset):
    t = streams[(nch, preset)]
    assert expected_quiet(t.full, 0, t.ns, 3, 1)[0] == planted_runs(3)
    spans = [(0, t.ns), (BASE_B, 1500), (S - 1, 2), (t.ns - 1, 1)]
    combos = [(w, th, mn) for w in spans for th in THRESHOLDS for mn in MINS]
    wins, thr, mins = [c[0] for c in combos], [c[1] for c in combos], [c[2] for c in combos]
    got = ctx.quiet_windows([(t.dev, t.index, a, n) for a, n in wins], thr, mins)
    check(t, wins, thr, mins, got)
    again = ctx.quiet_windows([(t.dev, t.index, a, n) for a, n in wins], thr, mins, group_frames=1)
    assert [answer(q) for q in again] == [answer(q) for q in got]
    one = ctx.quiet_windows([(t.dev, t.index, BASE_B, 1500)] * 2, 3, 2)                        # one value for every window
    check(t, [(BASE_B, 1500)] * 2, [3, 3], [2, 2], one)


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_block_types(ctx, mixed):
    t = mixed
    bl = t.bl
    assert expected_quiet(t.full, 0, t.ns, 0, 1)[0] == [(a, b - a) for a, b in MIXED_PLANTS]
    wins = [(0, t.ns)]
    for k in (0, 1, 2, 4, 5, 7):                                 # a window inside a block of every type, and across its ends
        wins += [(bl[k][4] + 10, bl[k][3] - 20), (bl[k][4] - 5 if k else 0, bl[k][3] + 10 if k < 7 else bl[k][3])]
    wins += [(bl[1][4] + 100, 2 * S - 150), (bl[2][4] + 500, 3 * S), (bl[4][4] + 3, 2 * S - 7), (bl[3][4] + 1000, 1 * S + 30), (t.ns - TAIL + 7, TAIL - 7),
             (S - 41, 2 * S + 67), (S - 40, 2 * S + 65), (4 * S - 31, 52), (6 * S - 20, 70)]
    for th, mn in ((0, 1), (0, 50), (0, 51), (0, 2 * S + 65), (0, 2 * S + 66), (40, 1), (1 << 15, 1), (1 << 15, 3 * S)):
        got = ctx.quiet_windows([(t.dev, t.index, a, n) for a, n in wins], th, mn)
        check(t, wins, [th] * len(wins), [mn] * len(wins), got)


def test_zeros_behind_the_last_block(ctx, oracle, mixed):
    """the mixed stream cut behind its sixth block: the header names 7 * S + TAIL samples, the blocks hold 6 * S (the last of them
    RAW); the zeros behind `covered` join the run in front of them"""
    u = Stream(ctx, oracle, mixed.stream[:mixed.bl[6][0]], "mixed, cut")
    cov = 6 * S
    assert u.ns == mixed.ns and len(u.bl) == 6 and np.array_equal(u.full[:, :cov], mixed.full[:, :cov]) and not u.full[:, cov:].any()
    assert expected_quiet(u.full, 0, u.ns, 0, 1)[0][-1] == (cov - 15, S + TAIL + 15)
    wins = [(0, u.ns), (cov - 100, 400), (cov, S + TAIL), (cov + 300, 1), (cov - 1, 2), (cov - 16, 17), (4 * S + 5, 2 * S + 900), (u.ns - 1, 1)]
    for mn in (1, 15, 16, S + TAIL + 15, S + TAIL + 16):
        got = ctx.quiet_windows([(u.dev, u.index, a, n) for a, n in wins], 0, mn)
        check(u, wins, [0] * len(wins), [mn] * len(wins), got)
    u.index.close()


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_long_runs(ctx, long):
    t = long
    L = LONG_BLOCKS * S
    assert L == 65536 and expected_quiet(t.full, 0, t.ns, 0, 1)[0] == [(S, L)]
    wins, mins = [], []
    for mn in (1, L - 1, L, L + 1):                              # one run that spans several commit workgroups (16384 frames each)
        wins += [(0, t.ns), (S - 3, L + 6), (S, L)]
        mins += [mn] * 3
    for mn in (16385, 20000, 40001):                             # min_samples beyond one commit chunk, on runs of min - 1, min, min + 1
        for n in (mn - 1, mn, mn + 1):
            wins += [(S + 2000, n), (S - 5, n + 5), (S + L - n, n + 7)]
            mins += [mn] * 3
    got = ctx.quiet_windows([(t.dev, t.index, a, n) for a, n in wins], 0, mins)
    check(t, wins, [0] * len(wins), mins, got)
    assert [q.num_runs for q in got[:12]] == [1] * 9 + [0] * 3
    again = ctx.quiet_windows([(t.dev, t.index, a, n) for a, n in wins], 0, mins, group_frames=1)
    assert [answer(q) for q in again] == [answer(q) for q in got]


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_capacity(ctx, streams):
    t = streams[(2, 5)]
    runs, num, quiet, lead, trail = expected_quiet(t.full, 0, t.ns, 0, 1)
    assert num > 12
    items = [(t.dev, t.index, 0, t.ns, 0, 1, cap, wrong) for cap, wrong in ((0, "null"), (0, None), (num - 1, None), (num, None), (num + 3, None), (1, None))]
    ret, codes, answers, buf, offs = raw_call(ctx, items)
    assert ret == OK and codes == [OK] * len(items)
    assert answers == [(num, quiet, lead, trail)] * len(items)   # the full answer, whatever fitted
    assert np.array_equal(buf, want_buffer(len(buf), offs, [runs[:it[6]] for it in items]))      # and not a byte behind the records that fitted
    # the Python form: a capacity is kept, the default grows
    few = ctx.quiet_windows([(t.dev, t.index, 0, t.ns)] * 2, 0, capacity=[5, 0])
    assert [q.cpu() for q in few] == [runs[:5], []] and [q.num_runs for q in few] == [num, num]
    default, linne_amd.QUIET_DEFAULT_CAPACITY = linne_amd.QUIET_DEFAULT_CAPACITY, 4
    try:
        a, b = ctx.quiet_windows([(t.dev, t.index, 0, t.ns), (t.dev, t.index, 0, 40)], 0)
        assert num > 4 and answer(a) == (runs, num, quiet, lead, trail) and answer(b) == expected_quiet(t.full, 0, 40, 0, 1)
    finally:
        linne_amd.QUIET_DEFAULT_CAPACITY = default
    assert answer(ctx.quiet_windows([(t.dev, t.index, 0, t.ns)], 0)[0]) == (runs, num, quiet, lead, trail)


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_many_windows_and_failures_stay_in_their_window(ctx, streams, mixed):
    ts = [streams[(1, 0)], streams[(2, 5)], streams[(3, 0)], mixed]
    t = streams[(2, 5)]
    bad, k = crc_damaged(t)
    assert 0 < k < len(t.bl) - 1
    d_bad = to_device(bad)
    bad_index = ctx.index_stream(d_bad)
    rng = np.random.default_rng(4)
    items, owner = [], []
    for i in range(64):
        u = ts[i % 4]
        first = int(rng.integers(0, u.ns))
        n = int(rng.integers(1, u.ns - first + 1)) if i % 7 else 0
        th, mn = [0, 3, 1 << 31, 40][i % 4 if i % 5 else 1], MINS[i % len(MINS)]
        cap = [0, 1, 3, 40][(i // 4) % 4]
        items.append((u.dev, u.index, first, n, th, mn, cap, None))
        owner.append(u)
    special = {9: (d_bad, bad_index, t.bl[k][4] + 3, 600, 0, 1, 8, None, CORRUPTION),           # a failing window between good ones
               10: (d_bad, bad_index, 0, t.bl[k][4] - 24, 0, 1, 40, None, OK),                  # in front of the damaged block
               20: (t.dev, t.index, 0, 1000, 0, 1, 8, "misaligned", INVALID_ARGUMENT),
               30: (t.dev, t.index, 0, 1000, 0, 1, 8, "null", INVALID_ARGUMENT),
               40: (t.dev, t.index, 1, t.ns, 0, 1, 8, None, INVALID_ARGUMENT)}                  # a range beyond num_samples
    want_codes = [OK] * 64
    for i, sp in special.items():
        items[i], owner[i], want_codes[i] = sp[:8], t, sp[8]
    ret, codes, answers, buf, offs = raw_call(ctx, items)
    assert codes == want_codes and ret == CORRUPTION             # the lowest failing window's
    assert linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode().startswith(f"window 9: block {k} ")
    tables = []
    for i, it in enumerate(items):
        if want_codes[i] != OK:
            assert answers[i] == (SENTINEL,) * 4, i              # a failing window's answers are not written
            tables.append([])
            continue
        runs, *rest = expected_quiet(owner[i].full, it[2], it[3], it[4], it[5])
        assert answers[i] == tuple(rest), (i, it[2:7])
        tables.append(runs[:it[6]])
    assert np.array_equal(buf, want_buffer(len(buf), offs, tables))      # the tables, and sentinels everywhere else
    ret2, codes2, answers2, buf2, _ = raw_call(ctx, items, group_frames=2)
    assert (ret2, codes2, answers2) == (ret, codes, answers) and np.array_equal(buf2, buf)
    for i in (9, 20, 30):                                        # alone: the same code, nothing written
        ret1, codes1, answers1, buf1, offs1 = raw_call(ctx, [items[i]])
        assert (ret1, codes1, answers1) == (want_codes[i], [want_codes[i]], [(SENTINEL,) * 4]) and np.array_equal(buf1, want_buffer(len(buf1), offs1, [[]])), i
    # the Python form
    four = [it[:4] for it in items[8:12]]
    got, pcodes = ctx.quiet_windows(four, [it[4] for it in items[8:12]], [it[5] for it in items[8:12]], return_codes=True)
    assert pcodes == want_codes[8:12] and got[1] is None
    for j in (0, 2, 3):
        assert answer(got[j]) == expected_quiet(owner[8 + j].full, *items[8 + j][2:6])
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.quiet_windows(four, 0)
    assert e.value.code == CORRUPTION and e.value.codes == pcodes and "window 1:" in str(e.value)
    assert ctx.quiet_windows([], 0) == [] and ctx.quiet_windows([], 0, return_codes=True) == ([], [])
    bad_index.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(mixed, streams):
    header = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    extra = int(re.search(r"#define\s+LINNE_AMD_QUIET_EXTRA_LAUNCHES\s+(\d+)", header).group(1))
    quiet = sc.CONSUMERS["quiet"]
    assert extra == len(quiet.kinds) - 1
    sc.launch_counts(quiet, mixed, streams[(3, 0)], ((0, 2), {"capacity": 64}), lambda t, w, q: check(t, [w], [0], [2], [q]))


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_composition_with_splice(ctx, oracle):
    """quiet_streams -> sound_segments -> splice_streams: the sound of a stream, cut out on the device.  -m 0: an edge block must hold
    more than 32 samples, and every segment here begins and ends 40 samples or more from a block's end"""
    x = made_loud(music(2, 4 * S, 16, seed=9))
    for a, b in ((0, 200), (1000, 1100), (2500, 2600), (4 * S - 196, 4 * S)):
        x[:, a:b] = 0
    t = encoded(ctx, oracle, x, 16, 0, True, "composition")
    q, = ctx.quiet_streams([t.dev], 0, min_samples=50)
    assert answer(q) == expected_quiet(t.full, 0, t.ns, 0, 50) and q.num_runs == 4 and (q.lead_samples, q.trail_samples) == (200, 196)
    segments = linne_amd.sound_segments(t.ns, q.cpu())
    assert segments == [(200, 800), (1100, 1400), (2600, 4 * S - 196 - 2600)]
    outs = ctx.splice_streams([[(t.dev, t.index, a, n)] for a, n in segments])
    for (a, n), out in zip(segments, outs):
        ret, full, _ = oracle.decode_whole(out.cpu().numpy().tobytes())
        assert ret == OK and np.array_equal(full, t.full[:, a:a + n]), (a, n)
    inside = ctx.quiet_streams(outs, 0, min_samples=50)
    assert [(r.num_runs, r.cpu(), r.lead_samples, r.trail_samples) for r in inside] == [(0, [], 0, 0)] * 3
    together, = ctx.splice_streams([[(t.dev, t.index, a, n) for a, n in segments]])           # one stream of all the sound
    assert ctx.quiet_streams([together], 0, min_samples=50)[0].num_runs == 0
    t.index.close()


# 8 ------------------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^run (\d+): first (\d+) samples (\d+) seconds (\S+) $")
SUMMARY = re.compile(r"^runs (\d+) quiet_samples (\d+) lead (\d+) trail (\d+) $")


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_command_line_tool(tmp_path, streams, mixed):
    path = tmp_path / "a.lnn"
    for t, spec, th, mn in ((mixed, "0,100", 0, 100), (streams[(2, 5)], "3", 3, 1), (streams[(2, 5)], "0,5000", 0, 5000)):
        path.write_bytes(t.stream)
        r = subprocess.run([CLI, "-S", spec, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        runs, num, quiet, lead, trail = expected_quiet(t.full, 0, t.ns, th, mn)
        *lines, last = r.stdout.splitlines()
        got = [LINE.match(x) for x in lines]
        assert all(got) and [(int(m.group(1)), int(m.group(2)), int(m.group(3))) for m in got] == [(k, a, n) for k, (a, n) in enumerate(runs)], r.stdout
        assert all(abs(float(m.group(4)) - int(m.group(3)) / 44100) <= 1e-6 for m in got)
        assert tuple(int(v) for v in SUMMARY.match(last).groups()) == (num, quiet, lead, trail)
    bad, k = crc_damaged(mixed)
    path.write_bytes(bad)
    r = subprocess.run([CLI, "-S", "0,100", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and not r.stdout and f"block {k} " in r.stderr, r.stderr
