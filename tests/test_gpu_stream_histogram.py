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
from stream_refs import expected_quiet
from test_cli_cpu import CLI
from test_gpu_stream_compare import Stream, encoded
from test_gpu_stream_windows import crc_damaged, to_device
from test_stream_histogram_cpu import CONSTANT, S, TAIL, bins_of, constant_signal, expected_histogram
from test_stream_measure_cpu import CARRY_NS, carry_stream
from test_stream_quiet_cpu import mixed_signal, planted_signal

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CORRUPTION = 0, 1, 6
COMPRESS, SILENT, RAW = 0, 1, 2
SHAPES = [(nch, preset) for nch in (1, 2, 3) for preset in (0, 5)]
SENTINEL = 0x5A5A5A5A5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
PAD = 1                                                          # buckets a padded channel_stride leaves between the channels' rows
GAP = 3                                                          # sentinel words in front of, between and behind the tables


def raw_call(ctx, items, group_frames=0):
    """LINNEAmd_HistogramWindowsDevice itself.  items: (stream, index, first, n, channels, num_bins, shift, scale, bucket_samples, what
    is wrong with the spec); every window's table lies in one buffer of sentinels, its channels' rows PAD buckets apart -> (ret, codes,
    the buffer as numpy, the tables' first words, the bucket counts, the bins a table has room for)"""
    import torch
    offs, nbs, rooms, at = [], [], [], GAP
    for dev, index, first, n, nch, bins, shift, scale, b, wrong in items:
        nb = 0 if n == 0 else (1 if b == 0 else -(-n // b))
        room = bins if 1 <= bins <= 1024 else 4
        offs.append(at)
        nbs.append(nb)
        rooms.append(room)
        at += nch * (nb + PAD) * room + GAP
    buf = torch.full((at,), SENTINEL, dtype=torch.int64, device="cuda")
    W = len(items)
    w, sp = (linne_amd.Window * W)(), (linne_amd.HistogramSpec * W)()
    for j, (dev, index, first, n, nch, bins, shift, scale, b, wrong) in enumerate(items):
        w[j].index, w[j].d_stream, w[j].first_sample, w[j].num_samples, w[j].d_pcm, w[j].pcm_stride, w[j].result = index.h, dev.data_ptr(), first, n, None, 0, -1
        sp[j].bucket_samples, sp[j].num_bins, sp[j].shift, sp[j].scale, sp[j].reserved = b, bins, shift, scale, 1 if wrong == "reserved" else 0
        sp[j].d_out, sp[j].channel_stride = buf.data_ptr() + 8 * offs[j] + (4 if wrong == "misaligned" else 0), nbs[j] + PAD
        if wrong == "null":
            sp[j].d_out = None
        elif wrong == "stride":
            sp[j].channel_stride = nbs[j] - 1
    torch.cuda.synchronize()
    ret = linne_amd.lib.LINNEAmd_HistogramWindowsDevice(ctx.h, w, sp, W, group_frames)
    return ret, [w[j].result for j in range(W)], buf.cpu().numpy(), offs, nbs, rooms


def want_buffer(words, items, fulls, codes, offs, nbs):
    """sentinels but the OK windows' counts"""
    buf = np.full(words, SENTINEL, dtype=np.int64)
    for it, full, code, off, nb in zip(items, fulls, codes, offs, nbs):
        if code != OK or it[3] == 0:
            continue
        _, _, first, n, nch, bins, shift, scale, b, _ = it
        want = expected_histogram(full, first, n, bins, shift, bool(scale), b)
        for ch in range(nch):
            at = off + ch * (nb + PAD) * bins
            buf[at:at + nb * bins] = want[ch].reshape(-1)
    return buf


def test_many_windows_and_failures_stay_in_their_window(ctx, streams, mixed):
    """64 windows of four stream shapes and of specs that differ in every field, failing ones among them.  (Of the argument errors of a
    window, nb > 2^32 - 1 cannot be reached: a stream's header holds a 32-bit sample count and a bucket has a sample or more.)"""
    ts = [streams[(1, 0)], streams[(2, 5)], streams[(3, 0)], mixed]
    t = streams[(2, 5)]
    bad, k = crc_damaged(t)
    assert 0 < k < len(t.bl) - 1
    d_bad = to_device(bad)
    bad_index = ctx.index_stream(d_bad)
    rng = np.random.default_rng(4)
    items, fulls = [], []
    for i in range(64):
        u = ts[i % 4]
        first = int(rng.integers(0, u.ns))
        n = int(rng.integers(1, u.ns - first + 1)) if i % 7 else 0
        bins, shift, log2, b = SPECS[(i * 5 + i // 16) % len(SPECS)]
        items.append((u.dev, u.index, first, n, u.nch, bins, shift, int(log2), b if b != 1 else 3, None))
        fulls.append(u.full)
    good = (t.dev, t.index, 0, 1000, 2)
    special = {9: (d_bad, bad_index, t.bl[k][4] + 3, 600, 2, 64, 4, 0, 100, None, CORRUPTION),     # a failing window between good ones
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
    want_codes = [OK] * 64
    for i, sp in special.items():
        items[i], fulls[i], want_codes[i] = sp[:10], t.full, sp[10]
    ret, codes, buf, offs, nbs, _ = raw_call(ctx, items)
    assert codes == want_codes and ret == CORRUPTION             # the lowest failing window's
    text = linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode()
    assert text.startswith(f"window 9: block {k} ")
    assert np.array_equal(buf, want_buffer(len(buf), items, fulls, want_codes, offs, nbs))          # the tables, and sentinels everywhere else
    ret2, codes2, buf2, *_ = raw_call(ctx, items, group_frames=2)
    assert (ret2, codes2) == (ret, codes) and np.array_equal(buf2, buf)
    # codes and text are the decode call's
    _, dcodes = ctx.decode_windows([it[:4] for it in items[8:12]], return_codes=True)
    assert dcodes == want_codes[8:12] and linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode() == text.replace("window 9:", "window 1:")
    for i in sorted(special):                                    # alone: the same code, nothing written by a failing one
        ret1, codes1, buf1, offs1, nbs1, _ = raw_call(ctx, [items[i]])
        assert (ret1, codes1) == (want_codes[i], [want_codes[i]]), i
        assert np.array_equal(buf1, want_buffer(len(buf1), [items[i]], [fulls[i]], [want_codes[i]], offs1, nbs1)), i
        if want_codes[i] == INVALID_ARGUMENT and i != 40:
            assert linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode().startswith("window 0: HistogramWindowsDevice: "), i
    # the Python form
    four = [it[:4] for it in items[8:12]]
    spec4 = [[it[j] for it in items[8:12]] for j in (5, 6, 7, 8)]
    got, pcodes = ctx.histogram_windows(four, *spec4, return_codes=True)
    assert pcodes == want_codes[8:12] and got[1] is None and got[3] is None
    for j in (0, 2):
        it = items[8 + j]
        assert np.array_equal(got[j].cpu(), expected_histogram(fulls[8 + j], it[2], it[3], it[5], it[6], bool(it[7]), it[8]))
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.histogram_windows(four, 64)
    assert e.value.code == CORRUPTION and e.value.codes == pcodes and "window 1:" in str(e.value)
    _, pcodes = ctx.histogram_windows([good[:4]] * 3, [64, 1025, 0], return_codes=True)             # a refused num_bins gets no table
    assert pcodes == [OK, INVALID_ARGUMENT, INVALID_ARGUMENT]
    assert ctx.histogram_windows([], 64) == [] and ctx.histogram_windows([], 64, return_codes=True) == ([], [])
    empty = ctx.histogram_windows([(ts[2].dev, ts[2].index, 100, 0)], 64, bucket_samples=5)[0]      # no samples: no buckets
    assert tuple(empty.counts.shape) == (3, 0, 64)
    bad_index.close()


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(mixed, streams):
    three = streams[(3, 0)]
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        c.enable_timing(True)
        counts = {}
        for t in (mixed, three):
            index = c.index_stream(t.dev)
            for nw in (1, 64):
                spans = [(0, t.ns)] + [(37 * i, t.ns - 53 * i) for i in range(1, nw)]
                for gf in (0, 2):
                    c.decode_windows([(t.dev, index, a, n) for a, n in spans], group_frames=gf)
                    dec = {k: c.last_launches(k) for k in (28, 56, 57, 58, 59)}
                    got = c.histogram_windows([(t.dev, index, a, n) for a, n in spans], 65, 3, False, 441, group_frames=gf)
                    his = {k: c.last_launches(k) for k in (28, 56, 57, 58, 59, 79, 80, 81, 82, 83, 86, 87, 92, 93, 94)}
                    assert np.array_equal(got[-1].cpu(), expected_histogram(t.full, spans[-1][0], spans[-1][1], 65, 3, False, 441))
                    assert his[59] == 0 and all(his[k] == 0 for k in (79, 80, 81, 82, 83, 86, 87)) and his[92] == dec[59] >= 1, (t.name, nw, gf, dec, his)
                    assert all(his[k] == dec[k] for k in (28, 56, 57, 58)), (t.name, nw, gf, dec, his)
                    assert his[93] == 1 and his[94] == 1, (t.name, nw, gf, his)                  # the two launches per call
                    assert c.last_ms(92) > 0
                    counts[(t.name, nw, gf)] = his
                assert counts[(t.name, nw, 0)][92] == 1
            assert counts[(t.name, 1, 0)] == counts[(t.name, 64, 0)]          # not a launch more for 64 windows than for one
            assert counts[(t.name, 1, 2)][92] > 1                             # the window spans passes
            index.close()
    finally:
        c.close()


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
