"""GPU tests of histogramming the sample levels of windows of resident .lnn streams (Context.histogram_windows, histogram_streams,
level_threshold, the command line tool's -L; include/linne_amd.h LINNEAmd_HistogramWindowsDevice).  Every expected count is computed
with numpy.bincount (test_stream_histogram_cpu.expected_histogram) from the oracle's decode of the same bytes, never from the library
under test, and everything must be equal.  Streams hold at most 8 blocks of 1024 samples, except the two long ones."""
import os
import re
import subprocess

import numpy as np
import pytest

import linne_amd
from signals import music
import stream_consumers as sc
from stream_consumers import Stream, crc_damaged, encoded
from stream_refs import CARRY_NS, bins_of, carry_stream, expected_histogram, expected_quiet, mixed_signal
from test_cli_cpu import CLI
from test_stream_histogram_cpu import CONSTANT, S, TAIL, constant_signal
from test_stream_quiet_cpu import planted_signal

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CORRUPTION = 0, 1, 6
COMPRESS, SILENT, RAW = 0, 1, 2
SHAPES = [(nch, preset) for nch in (1, 2, 3) for preset in (0, 5)]
HISTOGRAM = sc.CONSUMERS["histogram"]
# (num_bins, shift, log2, bucket_samples): every bin count of {1, 2, 33, 64, 65, 1024}, every shift of {0, 4, 15, 31}, both scales, every
# bucket length of {0, 1, 7, 255, 256, 257, 441, 1024, 5000}; a bucket of one sample goes with few bins, so that a table stays small
SPECS = [(1, 0, False, 0), (2, 0, True, 255), (33, 0, True, 441), (64, 4, False, 256), (65, 4, True, 257), (1024, 0, False, 0), (1024, 4, False, 7), (1024, 15, False, 1024),
         (33, 31, True, 1), (64, 31, False, 5000), (2, 15, True, 7), (65, 0, False, 1), (1024, 0, True, 441), (33, 4, True, 0), (64, 15, True, 1024), (1, 31, True, 257)]


@pytest.fixture(scope="module")
def streams(ctx, oracle):
    """1, 2 (MS) and 3 channels, presets 0 and 5, 3 blocks and a tail of 300"""
    out = {(nch, preset): encoded(ctx, oracle, music(nch, 3 * S + TAIL, 16, seed=50 + 8 * nch + preset), 16, preset, nch == 2, f"{nch}ch -m {preset}")
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


def call(ctx, t, wins, specs, **kw):
    return ctx.histogram_windows([(t.dev, t.index, a, n) for a, n in wins], [s[0] for s in specs], [s[1] for s in specs], [s[2] for s in specs], [s[3] for s in specs], **kw)


def check(t, wins, specs, got):
    for (first, n), (bins, shift, log2, b), h in zip(wins, specs, got):
        want = expected_histogram(t.full, first, n, bins, shift, log2, b)
        have = h.cpu()
        assert have.shape == want.shape and have.dtype == np.int64, (t.name, first, n, bins, shift, log2, b)
        assert np.array_equal(have, want), (t.name, first, n, bins, shift, log2, b)
        # the bins of a (channel, bucket) add up to the bucket's samples
        step = b if b > 0 else n
        assert np.array_equal(have.sum(axis=2), np.tile(np.minimum(step, n - step * np.arange(want.shape[1])), (t.nch, 1)))
        assert (h.num_bins, h.shift, h.log2, h.bucket_samples) == (bins, shift, log2, b)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,preset", SHAPES)
def test_exactness(ctx, streams, nch, preset):
    t = streams[(nch, preset)]
    # the whole stream; starting and ending inside a block; across a block's end; one sample; 255, 256 and 257 samples across the
    # boundary of two pieces (a block's samples 256 j .. 256 j + 255 are one piece)
    spans = [(0, t.ns), (517, 1500), (S - 1, 2), (t.ns - 1, 1), (200, 255), (S + 130, 256), (2 * S + 255, 257)]
    wins = [w for w in spans for _ in SPECS]
    specs = SPECS * len(spans)
    got = call(ctx, t, wins, specs)
    check(t, wins, specs, got)
    again = call(ctx, t, wins, specs, group_frames=1)
    assert all(np.array_equal(a.cpu(), b.cpu()) for a, b in zip(again, got))
    one = ctx.histogram_windows([(t.dev, t.index, 517, 1500)] * 2, 33, 2, True, 257)               # one value for every window
    check(t, [(517, 1500)] * 2, [(33, 2, True, 257)] * 2, one)
    plain = ctx.histogram_windows([(t.dev, t.index, 0, None)], 64)                                 # the defaults: linear, no shift, one bucket
    check(t, [(0, t.ns)], [(64, 0, False, 0)], plain)


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_eight_channels_and_1024_bins(ctx, oracle):
    """one block of eight channels: the kernel's whole histogram in LDS, 8 x 1024 counters"""
    t = encoded(ctx, oracle, music(8, S, 16, seed=77), 16, 0, False, "8ch")
    assert len(t.bl) == 1 and t.bl[0][2] == COMPRESS
    wins = [(0, S), (0, S), (0, S), (3, S - 5), (0, S)]
    specs = [(1024, 5, False, 0), (1024, 0, True, 0), (1024, 5, False, 300), (1024, 3, False, 256), (1024, 0, False, 100)]
    assert len(np.flatnonzero(expected_histogram(t.full, 0, S, 1024, 5)[7, 0])) > 100                # the bins are in use, up to the last channel's
    check(t, wins, specs, call(ctx, t, wins, specs))
    t.index.close()


# 3 ------------------------------------------------------------------------------------------------------------------------------
BLOCK_SPECS = [(1024, 4, False, 0), (33, 0, True, 1), (64, 9, False, 100), (2, 0, True, 256), (1024, 0, False, 300), (65, 3, True, 1000), (1, 0, False, 1025)]


def test_block_types(ctx, mixed):
    t = mixed
    bl = t.bl
    wins = [(0, t.ns)]
    for k in (0, 1, 2, 4, 5, 7):                                 # a window inside a block of every type, and across its ends
        wins += [(bl[k][4] + 10, bl[k][3] - 20), (bl[k][4] - 5 if k else 0, bl[k][3] + 10 if k < 7 else bl[k][3])]
    wins += [(bl[1][4] + 100, 2 * S - 150), (bl[2][4] + 500, 3 * S), (bl[4][4] + 3, 2 * S - 7), (bl[3][4] + 1000, 1 * S + 30), (t.ns - TAIL + 7, TAIL - 7)]
    for spec in BLOCK_SPECS:                                     # 100, 300, 1000, 1025: buckets straddle the blocks' boundaries
        check(t, wins, [spec] * len(wins), call(ctx, t, wins, [spec] * len(wins)))
    mix = [BLOCK_SPECS[i % len(BLOCK_SPECS)] for i in range(len(wins))]
    check(t, wins, mix, call(ctx, t, wins, mix, group_frames=2))


def test_zeros_behind_the_last_block(ctx, oracle, mixed):
    """the mixed stream cut behind its sixth block: the header names 7 * S + TAIL samples, the blocks hold 6 * S (the last of them
    RAW); the windows reaching beyond `covered` count the rest's zeros in bin 0"""
    u = Stream(ctx, oracle, mixed.stream[:mixed.bl[6][0]], "mixed, cut")
    cov = 6 * S
    assert u.ns == mixed.ns and len(u.bl) == 6 and np.array_equal(u.full[:, :cov], mixed.full[:, :cov]) and not u.full[:, cov:].any()
    wins = [(0, u.ns), (cov - 100, 400), (cov, S + TAIL), (cov + 300, 1), (cov - 1, 2), (4 * S + 5, 2 * S + 900), (u.ns - 1, 1)]
    for spec in ((1024, 4, False, 0), (33, 0, True, 1), (64, 0, False, 64), (2, 0, True, 256), (65, 7, False, 333)):
        got = call(ctx, u, wins, [spec] * len(wins))
        check(u, wins, [spec] * len(wins), got)
    assert int(got[2].cpu()[:, :, 0].sum()) == 2 * (S + TAIL)
    u.index.close()


@pytest.mark.parametrize("bits,nch", [(8, 1), (24, 2)])
def test_other_sample_widths(ctx, oracle, bits, nch):
    """the values are the decoded int32, not the bytes a WAV file holds: 8-bit samples are signed, 24-bit ones reach 2^23"""
    x = music(nch, 2 * S + TAIL, bits, seed=60 + bits)
    x[0, 5], x[0, 6] = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    t = encoded(ctx, oracle, x, bits, 2, nch == 2, f"{bits} bits")
    wins = [(0, t.ns), (100, 2000), (0, t.ns), (0, t.ns), (S - 3, 700)]
    specs = [(1024, bits - 8, False, 0), (33, 0, True, 441), (2, bits - 1, False, 256), (64, 0, True, 7), (65, bits - 6, False, 257)]
    got = call(ctx, t, wins, specs)
    check(t, wins, specs, got)
    assert got[2].cpu()[0, 0, 1] >= 1                            # sample 5, of magnitude 2^(bits - 1)
    t.index.close()


# 4 ------------------------------------------------------------------------------------------------------------------------------
def crowded_signal():
    """stereo, four blocks.  The kernel adds up the lanes of a wave (64 consecutive samples of a block) that share a bin before it
    touches its histogram, from eight lanes on and for four bins at the most.  Block 0: eight equal values in every 64; block 1: seven;
    block 2: every other sample equal; block 3: five values twelve times each in every 64.  The rest is music"""
    x = music(2, 4 * S + TAIL, 16, seed=91)
    i = np.arange(S)
    x[:, 0 * S:1 * S][:, i % 64 < 8] = CONSTANT
    x[:, 1 * S:2 * S][:, i % 64 < 7] = -CONSTANT
    x[:, 2 * S:3 * S][:, i % 2 == 0] = CONSTANT
    for g in range(5):
        x[:, 3 * S:4 * S][:, (i % 64) // 12 == g] = 100 * (g + 1) * (-1) ** g
    return x


def test_one_bin_takes_everything(ctx, oracle, streams):
    # a constant track: every lane of every wave in one bin
    t = encoded(ctx, oracle, constant_signal(2, 3 * S + TAIL), 16, 0, True, "constant")
    assert [b[2] for b in t.bl] == [COMPRESS] * 4
    wins = [(0, t.ns), (0, t.ns), (0, t.ns), (7, 3000), (0, t.ns), (1, 1)]
    specs = [(1024, 0, False, 0), (33, 0, True, 0), (1024, 0, False, 441), (2, 0, True, 100), (1, 0, False, 257), (1024, 0, False, 0)]
    got = call(ctx, t, wins, specs)
    check(t, wins, specs, got)
    assert got[0].cpu()[:, 0, CONSTANT].tolist() == [t.ns] * 2 and got[1].cpu()[:, 0, 10].tolist() == [t.ns] * 2
    t.index.close()
    # log2 with two bins on music: nearly every lane in bin 1, a few in bin 0
    m = streams[(2, 5)]
    want = expected_histogram(m.full, 0, m.ns, 2, 0, True)
    assert (want[:, 0, 1] > 0.9 * m.ns).all()
    check(m, [(0, m.ns)] * 2, [(2, 0, True, 0), (2, 0, True, 256)], call(ctx, m, [(0, m.ns)] * 2, [(2, 0, True, 0), (2, 0, True, 256)]))
    # waves partly crowded: the lanes added up in the wave and the lanes that count one by one, in one wave
    c = encoded(ctx, oracle, crowded_signal(), 16, 0, False, "crowded")
    wins = [(0, c.ns), (0, c.ns), (5, c.ns - 9), (0, c.ns), (0, c.ns), (3 * S - 30, S)]
    specs = [(1024, 1, False, 0), (1024, 0, False, 64), (1024, 2, False, 300), (33, 0, True, 0), (1024, 0, False, 1), (1024, 0, False, 31)]
    check(c, wins, specs, call(ctx, c, wins, specs))
    c.index.close()


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_long_buckets(ctx, oracle):
    """48 COMPRESS blocks of stereo music in one bucket (8 slots), and 257 RAW blocks of 24-bit mono in one bucket: its 2^18 + 1024
    samples take all 64 slots.  Then buckets of 4097 samples: no multiple of a piece, nor of a block"""
    t = encoded(ctx, oracle, music(2, 48 * S, 16, seed=83), 16, 0, True, "48 blocks")
    assert len(t.bl) == 48 and all(b[2] == COMPRESS for b in t.bl)
    wins = [(0, t.ns)] * 5 + [(S + 7, 40 * S)]
    specs = [(1024, 5, False, 0), (33, 0, True, 0), (1024, 5, False, 4097), (2, 0, True, 4097), (64, 8, False, t.ns // 2), (65, 0, True, 0)]
    check(t, wins, specs, call(ctx, t, wins, specs))
    check(t, wins, specs, call(ctx, t, wins, specs, group_frames=5))
    t.index.close()
    c = Stream(ctx, oracle, carry_stream(oracle), "257 RAW blocks")
    assert c.ns == CARRY_NS >= 64 * 4096 and all(b[2] == RAW for b in c.bl)
    wins = [(0, c.ns)] * 4 + [(3, c.ns - 5)]
    specs = [(1024, 13, False, 0), (33, 0, True, 0), (1024, 14, False, 4097), (33, 0, True, 4097), (2, 22, False, 1 << 17)]
    got = call(ctx, c, wins, specs)
    check(c, wins, specs, got)
    assert got[0].cpu()[0, 0, 1023] == c.ns and got[1].cpu()[0, 0, 23] == c.ns                   # every sample has magnitude 2^23 - 1
    c.index.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_many_windows_and_failures_stay_in_their_window(ctx, product, streams, mixed):
    """64 windows of four stream shapes and of specs that differ in every field, failing ones among them"""
    t = streams[(2, 5)]
    crc, rice = sc.damaged(ctx, product, t)
    (d_bad, bad_index, k), good = crc, (t.dev, t.index, 0, 1000, 2)
    special = {**sc.rice_windows(t, rice, [(64, 4, 0, 100), (33, 0, 1, 7), (1024, 2, 0, 441)]),
               9: (d_bad, bad_index, t.bl[k][4] + 3, 600, 2, 64, 4, 0, 100, None, CORRUPTION),     # a failing window between good ones
               10: (d_bad, bad_index, 0, t.bl[k][4] - 24, 2, 1024, 2, 0, 64, None, OK),            # in front of the damaged block
               11: (d_bad, bad_index, t.bl[k + 1][4], 200, 2, 33, 0, 1, 0, None, CORRUPTION),      # behind it
               20: good + (64, 0, 0, 256, "misaligned", INVALID_ARGUMENT),
               21: good + (64, 0, 0, 100, "stride", INVALID_ARGUMENT),
               22: good + (64, 0, 0, 0, "null", INVALID_ARGUMENT),
               30: good + (0, 0, 0, 0, None, INVALID_ARGUMENT),                                     # num_bins
               31: good + (1025, 0, 0, 0, None, INVALID_ARGUMENT),
               32: good + (64, 32, 0, 0, None, INVALID_ARGUMENT),                                   # shift
               33: good + (64, 0, 2, 0, None, INVALID_ARGUMENT),                                    # scale
               34: good + (64, 0, 0, 0, "reserved", INVALID_ARGUMENT),
               40: (t.dev, t.index, 1, t.ns, 2, 64, 0, 0, 500, None, INVALID_ARGUMENT),             # a range beyond num_samples
               41: good + (1024, 31, 1, 1000, None, OK), 42: good + (1, 0, 0, 1, None, OK)}         # the specs' extremes

    def fields(i):
        bins, shift, log2, b = SPECS[(i * 5 + i // 16) % len(SPECS)]
        return bins, shift, int(log2), b if b != 1 else 3

    sc.many_windows(HISTOGRAM, ctx, [streams[(1, 0)], streams[(2, 5)], streams[(3, 0)], mixed], t, fields, special, crc, rice,
                    faults={"reserved": lambda sp: setattr(sp, "reserved", 1)})
    _, pcodes = ctx.histogram_windows([good[:4]] * 3, [64, 1025, 0], return_codes=True)             # a refused num_bins gets no table
    assert pcodes == [OK, INVALID_ARGUMENT, INVALID_ARGUMENT]


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(mixed, streams):
    sc.launch_counts(HISTOGRAM, mixed, streams[(3, 0)], ((65, 3, False, 441), {}), lambda t, w, h: check(t, [w], [(65, 3, False, 441)], [h]))


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_agreement_with_the_quiet_call(ctx, oracle):
    """on a mono stream a frame is quiet when its one sample is: the quiet samples at threshold T = ((j + 1) << shift) - 1 are the linear
    histogram's counts up to bin j"""
    t = encoded(ctx, oracle, planted_signal(1, 31), 16, 0, False, "mono")
    wins = [(0, t.ns), (517, 1500)]
    for shift in (0, 3):
        hs = call(ctx, t, wins, [(64, shift, False, 0)] * 2)
        for (a, n), h in zip(wins, hs):
            cum = np.cumsum(h.cpu()[0, 0])
            for j in (0, 1, 5, 62):
                T = ((j + 1) << shift) - 1
                q, = ctx.quiet_windows([(t.dev, t.index, a, n)], T, 1, capacity=0)
                assert q.quiet_samples == cum[j] == expected_quiet(t.full, a, n, T, 1)[2], (a, n, shift, j)
    # end to end: the level that half of the samples stay below, as the quiet call's threshold
    h, = ctx.histogram_streams([t.dev], 1024, shift=6)
    assert np.array_equal(h.cpu(), expected_histogram(t.full, 0, t.ns, 1024, 6))
    T = linne_amd.level_threshold(h.cpu()[0, 0], 0.5, shift=6)
    median = int(np.sort(np.abs(t.full[0].astype(np.int64)))[-(-t.ns // 2) - 1])
    assert T is not None and T == (((median >> 6) + 1) << 6) - 1
    q, = ctx.quiet_streams([t.dev], T)
    assert 2 * q.quiet_samples >= t.ns and (q.cpu(), q.num_runs, q.quiet_samples, q.lead_samples, q.trail_samples) == expected_quiet(t.full, 0, t.ns, T, 1)
    many = ctx.histogram_streams([t.dev, t.stream], [33, 2], log2=True, bucket_samples=[441, 0], group_frames=1)    # bytes are taken too
    assert np.array_equal(many[0].cpu(), expected_histogram(t.full, 0, t.ns, 33, 0, True, 441)) and np.array_equal(many[1].cpu(), expected_histogram(t.full, 0, t.ns, 2, 0, True))
    assert ctx.histogram_streams([], 64) == []
    t.index.close()


# 9 ------------------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^ch (\d+) bin (\d+) (\d+)\.\.(\d+|inf) (\d+) $")


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_command_line_tool(tmp_path, streams, mixed):
    path = tmp_path / "a.lnn"
    for t, spec, bins, shift, log2 in ((mixed, "1024,4", 1024, 4, False), (streams[(2, 5)], "33,0,log2", 33, 0, True), (streams[(3, 0)], "8", 8, 0, False),
                                       (streams[(2, 5)], "6,3,log2", 6, 3, True), (mixed, "64,9,linear", 64, 9, False)):
        path.write_bytes(t.stream)
        r = subprocess.run([CLI, "-L", spec, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        want = expected_histogram(t.full, 0, t.ns, bins, shift, log2)[:, 0]
        *lines, last = r.stdout.splitlines()
        got = [LINE.match(x) for x in lines]
        assert all(got) and last == f"samples {t.ns} ", r.stdout
        assert [(int(m.group(1)), int(m.group(2)), int(m.group(5))) for m in got] == [(ch, j, int(want[ch, j])) for ch in range(t.nch) for j in range(bins) if want[ch, j]]
        for m in got:                                            # the bin's edges: the least and the greatest |v| that fall into it
            j, lo = int(m.group(2)), int(m.group(3))
            assert int(bins_of([lo], bins, shift, log2)[0]) == j and (lo == 0 or int(bins_of([lo - 1], bins, shift, log2)[0]) == j - 1)
            if j == bins - 1:
                assert m.group(4) == "inf"
            else:
                hi = int(m.group(4))
                assert int(bins_of([hi], bins, shift, log2)[0]) == j and int(bins_of([hi + 1], bins, shift, log2)[0]) == j + 1
    bad, k = crc_damaged(mixed)
    path.write_bytes(bad)
    r = subprocess.run([CLI, "-L", "64", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and not r.stdout and f"block {k} " in r.stderr, r.stderr
