"""GPU tests of measuring sample windows of resident .lnn streams (Context.measure_windows, measure_streams, the command line tool's
-M; include/linne_amd.h LINNEAmd_MeasureWindowsDevice).  Every expected record -- min, max, sum and the 128-bit sum of squares per
channel and bucket -- is computed with numpy and Python integers (test_stream_measure_cpu.expected_measure) from the oracle's decode
of the same bytes, never from the library under test, and every field must be equal.  Streams hold at most 8 blocks of 1024 samples,
except the carry stream, whose sum of squares passes 2^64."""
import os
import re
import subprocess

import numpy as np
import pytest

import linne_amd
from signals import music
import stream_consumers as sc
from stream_consumers import Stream, encoded
from stream_refs import CARRY_NS, CARRY_PEAK, carry_stream, expected_measure, measure_table as table, mixed_signal
from test_cli_cpu import CLI

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CORRUPTION, NG = 0, 1, 6, 7
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300
BUCKETS = [0, 1, 7, 64, 255, 256, 257, 1000, 1024, 5000]
SHAPES = [(nch, preset) for nch in (1, 2, 3) for preset in (0, 5)]
MEASURE = sc.CONSUMERS["measure"]


@pytest.fixture(scope="module")
def streams(ctx, oracle):
    """1, 2 (MS) and 3 channels, presets 0 and 5, 3 blocks and a tail of 300"""
    out = {(nch, preset): encoded(ctx, oracle, music(nch, 3 * S + TAIL, 16, seed=20 + 8 * nch + preset), 16, preset, nch == 2, f"{nch}ch -m {preset}")
           for nch, preset in SHAPES}
    yield out
    for t in out.values():
        t.index.close()


@pytest.fixture(scope="module")
def mixed(ctx, oracle):
    """stereo, 8 blocks: music, two SILENT, music, two RAW, music, a tail of 300"""
    t = encoded(ctx, oracle, mixed_signal(2, 16, 7 * S + TAIL, seed=11, block=S), 16, 5, True, "mixed")
    assert [b[2] for b in t.bl] == [COMPRESS, SILENT, SILENT, COMPRESS, RAW, RAW, COMPRESS, COMPRESS] and t.bl[-1][3] == TAIL
    yield t
    t.index.close()


def check(t, wins, buckets, got):
    for (first, n), b, m in zip(wins, buckets, got):
        want = expected_measure(t.full, first, n, b)
        assert table(m) == want, (t.name, first, n, b)
        nb = len(want[0])
        assert tuple(m.min.shape) == tuple(m.sum.shape) == tuple(m.sumsq_hi.shape) == (t.nch, nb)
        e = np.array([[float(r[4]) * 2.0 ** 64 + float(r[3]) for r in row] for row in want]).reshape(t.nch, nb)
        assert np.array_equal(m.energy().cpu().numpy(), e)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,preset", SHAPES)
def test_exactness_over_buckets(ctx, streams, nch, preset):
    t = streams[(nch, preset)]
    spans = [(0, t.ns), (517, 1500), (S - 1, 2), (t.ns - 1, 1)]
    wins = [w for w in spans for _ in BUCKETS]
    buckets = BUCKETS * len(spans)
    got = ctx.measure_windows([(t.dev, t.index, a, n) for a, n in wins], bucket_samples=buckets)
    check(t, wins, buckets, got)
    again = ctx.measure_windows([(t.dev, t.index, a, n) for a, n in wins], bucket_samples=buckets, group_frames=1)
    assert [table(m) for m in again] == [table(m) for m in got]
    one = ctx.measure_windows([(t.dev, t.index, 517, 1500)], bucket_samples=257)     # one value for every window
    check(t, [(517, 1500)], [257], one)


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_block_types(ctx, mixed):
    t = mixed
    bl = t.bl
    wins = [(0, t.ns)]
    for k in (0, 1, 2, 4, 5, 7):                                 # a window inside a block of every type, and across its ends
        wins += [(bl[k][4] + 10, bl[k][3] - 20), (bl[k][4] - 5 if k else 0, bl[k][3] + 10 if k < 7 else bl[k][3])]
    wins += [(bl[1][4] + 100, 2 * S - 150), (bl[2][4] + 500, 3 * S), (bl[4][4] + 3, 2 * S - 7), (bl[3][4] + 1000, 1 * S + 30), (t.ns - TAIL + 7, TAIL - 7)]
    for b in (0, 1, 100, 256, 300, 1000, 1025):                  # 100, 300, 1000, 1025: buckets straddle the blocks' boundaries
        got = ctx.measure_windows([(t.dev, t.index, a, n) for a, n in wins], bucket_samples=b)
        check(t, wins, [b] * len(wins), got)


def test_zeros_behind_the_last_block(ctx, oracle, mixed):
    """the mixed stream cut behind its sixth block: the header names 7 * S + TAIL samples, the blocks hold 6 * S (the last of them
    RAW); the windows reaching beyond `covered` count the rest's zeros"""
    u = Stream(ctx, oracle, mixed.stream[:mixed.bl[6][0]], "mixed, cut")
    cov = 6 * S
    assert u.ns == mixed.ns and len(u.bl) == 6 and np.array_equal(u.full[:, :cov], mixed.full[:, :cov]) and not u.full[:, cov:].any()
    wins = [(0, u.ns), (cov - 100, 400), (cov, S + TAIL), (cov + 300, 1), (cov - 1, 2), (4 * S + 5, 2 * S + 900), (u.ns - 1, 1)]
    for b in (0, 1, 64, 256, 333):
        got = ctx.measure_windows([(u.dev, u.index, a, n) for a, n in wins], bucket_samples=b)
        check(u, wins, [b] * len(wins), got)
    u.index.close()


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_carry_into_the_high_word(ctx, oracle):
    t = Stream(ctx, oracle, carry_stream(oracle), "carry")
    assert t.ns == CARRY_NS and all(b[2] == RAW for b in t.bl)
    whole, halves = ctx.measure_windows([(t.dev, t.index, 0, None)] * 2, bucket_samples=[0, 1 << 18])
    (rec,), = table(whole)
    assert rec == expected_measure(t.full, 0, CARRY_NS, 0)[0][0]
    assert rec[4] >= 1 and rec[4] * (1 << 64) + rec[3] == CARRY_NS * CARRY_PEAK ** 2
    assert table(halves) == expected_measure(t.full, 0, CARRY_NS, 1 << 18)
    assert float(whole.energy()[0, 0]) == float(CARRY_NS * CARRY_PEAK ** 2)
    t.index.close()


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_many_windows_of_mixed_shapes_in_one_call(ctx, streams):
    ts = [streams[(1, 0)], streams[(2, 5)], streams[(3, 0)]]
    rng = np.random.default_rng(4)
    wins, buckets, owner = [], [], []
    for i in range(64):
        t = ts[i % 3]
        first = int(rng.integers(0, t.ns))
        n = int(rng.integers(1, t.ns - first + 1))
        if i in (10, 11, 40):                                    # repeated windows, with other buckets
            first, n = wins[i - 3][2], wins[i - 3][3]
        wins.append((t.dev, t.index, first, n))
        buckets.append([0, 1, 7, 64, 255, 256, 257, 1000, 1024, 5000, 33][i % 11])
        owner.append(t)
    got = ctx.measure_windows(wins, bucket_samples=buckets)
    for i in range(64):
        alone = ctx.measure_windows([wins[i]], bucket_samples=buckets[i])[0]
        assert table(got[i]) == table(alone) == expected_measure(owner[i].full, wins[i][2], wins[i][3], buckets[i]), i
    assert [table(m) for m in ctx.measure_windows(wins, bucket_samples=buckets, group_frames=2)] == [table(m) for m in got]
    assert ctx.measure_windows([]) == [] and ctx.measure_windows([], return_codes=True) == ([], [])
    empty = ctx.measure_windows([(ts[2].dev, ts[2].index, 100, 0)], bucket_samples=5)[0]      # no samples: no buckets
    assert tuple(empty.min.shape) == (3, 0)


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_failures_stay_in_their_window_and_nothing_else_is_written(ctx, product, streams, mixed):
    """64 windows of four stream shapes with mixed bucket lengths, failing ones among them; the buffer byte for byte"""
    t, u = streams[(2, 5)], streams[(3, 0)]
    crc, rice = sc.damaged(ctx, product, t)
    (d_bad, bad_index, k), good = crc, (t.dev, t.index, 0, 1000, 2)
    special = {**sc.rice_windows(t, rice, [(100,), (7,), (441,)]),
               9: (d_bad, bad_index, t.bl[k][4] + 3, 600, 2, 100, None, CORRUPTION),
               10: (d_bad, bad_index, 0, t.bl[k][4] - 24, 2, 64, None, OK),                        # before the damaged block
               11: (d_bad, bad_index, t.bl[k + 1][4], 200, 2, 0, None, CORRUPTION),                # behind it
               20: good + (256, "misaligned", INVALID_ARGUMENT),
               21: good + (100, "stride", INVALID_ARGUMENT),
               22: good + (0, "null", INVALID_ARGUMENT),
               40: (t.dev, t.index, 1, t.ns, 2, 500, None, INVALID_ARGUMENT),                      # a range beyond num_samples
               41: (t.dev, t.index, 100, 2000, 2, 300, None, OK)}                                  # a good one, alone too
    items, tracks, codes = sc.many_windows(MEASURE, ctx, [streams[(1, 0)], t, u, mixed], t, lambda i: (BUCKETS[(i * 3 + i // 16) % 10],), special, crc, rice)
    for i in (2, 3, 43, 62):                                     # good windows of other shapes alone: the same code, the same bytes
        ret1, codes1, buf1, offs1, nbs1 = sc.raw_call(MEASURE, ctx, [items[i]])
        assert (ret1, codes1) == (OK, [OK]) and buf1.tobytes() == sc.want_buffer(MEASURE, len(buf1), [items[i]], [tracks[i]], [OK], offs1, nbs1).tobytes(), i


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(mixed, streams):
    sc.launch_counts(MEASURE, mixed, streams[(3, 0)], ((), {"bucket_samples": 441}), lambda t, w, m: check(t, [w], [441], [m]))


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_measure_streams(ctx, streams, mixed):
    ts = [streams[(2, 5)], mixed, streams[(3, 0)]]
    for b in (0, 441, [100, 0, 1024]):
        got = ctx.measure_streams([t.dev for t in ts], bucket_samples=b)
        bs = b if isinstance(b, list) else [b] * 3
        for t, m, bb in zip(ts, got, bs):
            assert table(m) == expected_measure(t.full, 0, t.ns, bb), (t.name, bb)
    assert table(ctx.measure_streams([ts[0].stream], group_frames=1)[0]) == expected_measure(ts[0].full, 0, ts[0].ns, 0)      # bytes are taken too
    assert ctx.measure_streams([]) == []


LINE = re.compile(r"^(?:bucket (\d+) )?channel (\d+): samples (\d+) min (-?\d+) max (-?\d+) sum (-?\d+) sumsq_hi (\d+) sumsq_lo (\d+) mean (\S+) rms (\S+) $")


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_command_line_tool(tmp_path, streams, mixed):
    for t in (streams[(2, 5)], mixed):
        path = tmp_path / "a.lnn"
        path.write_bytes(t.stream)
        for b in (0, 1000):
            r = subprocess.run([CLI, "-M"] + ([str(b)] if b else []) + [str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, r.stderr
            want = expected_measure(t.full, 0, t.ns, b)
            lines = [LINE.match(x) for x in r.stdout.splitlines()]
            assert all(lines) and len(lines) == t.nch * len(want[0]), r.stdout
            for m in lines:
                k, ch = int(m.group(1) or 0), int(m.group(2))
                assert (m.group(1) is not None) == (b > 0)
                mn, mx, sm, lo, hi = want[ch][k]
                cnt = min(b, t.ns - k * b) if b else t.ns
                assert tuple(int(m.group(j)) for j in range(3, 9)) == (cnt, mn, mx, sm, hi, lo), m.group(0)
                assert abs(float(m.group(9)) - sm / cnt) <= 1e-6 and abs(float(m.group(10)) - ((hi * 2 ** 64 + lo) / cnt) ** 0.5) <= 1e-6 * (1 + abs(mx) + abs(mn))
