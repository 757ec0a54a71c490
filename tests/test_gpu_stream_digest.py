"""GPU tests of digesting sample windows of resident .lnn streams (Context.digest_windows, digest_streams, same_audio, the command
line tool's -D; include/linne_amd.h LINNEAmd_DigestWindowsDevice).  Every expected digest is zlib.crc32 of the byte string numpy builds
(test_stream_digest_cpu.expected_digest) from the oracle's decode of the same bytes, never from the library under test, and every
digest must be equal: no tolerance is involved.  Streams hold a handful of blocks of 1024 samples, except the two long ones whose
single bucket many workgroups fold into."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import linne_amd
from signals import music
import stream_consumers as sc
from stream_consumers import Stream, crc_damaged, encoded, to_device
from stream_refs import CARRY_NS, carry_stream, digest_table as table, expected_digest, mixed_signal
from test_cli_cpu import CLI
from test_stream_digest_cpu import wav_data

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CORRUPTION, NG = 0, 1, 6, 7
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300
BUCKETS = [0, 1, 7, 255, 256, 257, 441, 1024, 1025, 100000]
DIGEST = sc.CONSUMERS["digest"]
SHAPES = [(8, 1, False), (8, 2, False), (16, 1, False), (16, 2, True), (16, 8, False), (24, 1, False), (24, 2, True)]   # bits, channels, mid/side


@pytest.fixture(scope="module")
def streams(ctx, oracle):
    """8, 16 and 24 bits, 1, 2 (one of them mid/side) and 8 channels: music, two SILENT blocks, music, two RAW, music, a tail of 300"""
    out = {}
    for bits, nch, ms in SHAPES:
        t = encoded(ctx, oracle, mixed_signal(nch, bits, 7 * S + TAIL, seed=bits + nch, block=S), bits, 5, ms, f"{bits} bits {nch}ch")
        assert {COMPRESS, SILENT, RAW} <= {b[2] for b in t.bl} and t.bl[1][2] == SILENT and t.bl[-1][3] == TAIL, t.name
        t.bits = bits
        out[(bits, nch)] = t
    yield out
    for t in out.values():
        t.index.close()


def spans_of(t):
    """whole; starting and ending inside a block; 1 sample; 255 / 256 / 257 samples across the piece boundary at 256 samples into the
    fourth block; inside one SILENT block; across every block type"""
    at = t.bl[3][4]
    return [(0, t.ns), (517, 1500), (S - 1, 2), (t.ns - 1, 1), (at + 130, 255), (at + 1, 256), (at + 255, 257), (t.bl[1][4] + 10, S - 20), (S + 500, 5 * S)]


def check(t, wins, buckets, got):
    for (first, n), b, d in zip(wins, buckets, got):
        want = expected_digest(t.full, t.bits, first, n, b)
        assert table(d) == want, (t.name, first, n, b)
        assert tuple(d.crc32.shape) == tuple(d.num_bytes.shape) == (len(want),)
        assert d.crc32.cpu().tolist() == [w[0] for w in want] and d.num_bytes.cpu().tolist() == [w[1] for w in want]


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,nch,ms", SHAPES)
def test_exactness_over_windows_and_buckets(ctx, streams, bits, nch, ms):
    t = streams[(bits, nch)]
    spans = spans_of(t)
    wins = [w for w in spans for _ in BUCKETS]
    buckets = BUCKETS * len(spans)
    got = ctx.digest_windows([(t.dev, t.index, a, n) for a, n in wins], bucket_samples=buckets)
    check(t, wins, buckets, got)
    for gf in (1, 2):                                            # the windows span passes: the same answers
        again = ctx.digest_windows([(t.dev, t.index, a, n) for a, n in wins], bucket_samples=buckets, group_frames=gf)
        assert [table(d) for d in again] == [table(d) for d in got], gf
    twice = ctx.digest_windows([(t.dev, t.index, a, n) for a, n in wins], bucket_samples=buckets)      # the same call once more
    assert [table(d) for d in twice] == [table(d) for d in got]
    one = ctx.digest_windows([(t.dev, t.index, 517, 1500)], bucket_samples=257)                        # one value for every window
    check(t, [(517, 1500)], [257], one)


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,nch", [(8, 2), (16, 2), (24, 1)])
def test_zeros_behind_the_last_block(ctx, oracle, streams, bits, nch):
    """the stream cut behind its sixth block: the header names 7 * S + TAIL samples, the blocks hold 6 * S; the windows reaching beyond
    `covered` hash the rest's zeros (8 bits: 0x80 bytes)"""
    whole = streams[(bits, nch)]
    u = Stream(ctx, oracle, whole.stream[:whole.bl[6][0]], f"{whole.name}, cut")
    u.bits = bits
    cov = 6 * S
    assert u.ns == whole.ns and len(u.bl) == 6 and np.array_equal(u.full[:, :cov], whole.full[:, :cov]) and not u.full[:, cov:].any()
    wins = [(0, u.ns), (cov - 100, 400), (cov, S + TAIL), (cov + 300, 1), (cov + 10, 700), (cov - 1, 2), (4 * S + 5, 2 * S + 900), (u.ns - 1, 1)]
    for b in (0, 1, 64, 256, 333):
        got = ctx.digest_windows([(u.dev, u.index, a, n) for a, n in wins], bucket_samples=b)
        check(u, wins, [b] * len(wins), got)
    if bits == 8:
        assert table(got[3]) == [(zlib.crc32(b"\x80" * nch), nch)]
    u.index.close()


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_one_bucket_many_workgroups(ctx, oracle):
    """48 COMPRESS blocks of stereo music in one bucket (8 slots), and 257 RAW blocks of 24-bit mono in one bucket: its 2^18 + 1024
    samples take all 64 slots.  Halves, and buckets that are no multiple of a piece, beside them"""
    t = encoded(ctx, oracle, music(2, 48 * S, 16, seed=83), 16, 0, True, "48 blocks")
    t.bits = 16
    assert len(t.bl) == 48 and all(b[2] == COMPRESS for b in t.bl)
    wins, buckets = [(0, t.ns)] * 4 + [(S + 7, 40 * S)], [0, t.ns // 2, 8192, 10000, 0]
    check(t, wins, buckets, ctx.digest_windows([(t.dev, t.index, a, n) for a, n in wins], bucket_samples=buckets))
    check(t, wins, buckets, ctx.digest_windows([(t.dev, t.index, a, n) for a, n in wins], bucket_samples=buckets, group_frames=5))
    t.index.close()
    c = Stream(ctx, oracle, carry_stream(oracle), "257 RAW blocks")
    c.bits = 24
    assert c.ns == CARRY_NS >= 64 * 4096 and all(b[2] == RAW for b in c.bl)
    wins, buckets = [(0, c.ns)] * 3 + [(3, c.ns - 5)], [0, 1 << 17, 100001, 0]
    check(c, wins, buckets, ctx.digest_windows([(c.dev, c.index, a, n) for a, n in wins], bucket_samples=buckets))
    c.index.close()


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_many_windows_of_mixed_shapes_in_one_call(ctx, streams):
    ts = [streams[k] for k in ((8, 1), (16, 2), (24, 2), (16, 8), (8, 2))]
    rng = np.random.default_rng(4)
    wins, buckets, owner = [], [], []
    for i in range(64):
        t = ts[i % len(ts)]
        first = int(rng.integers(0, t.ns))
        n = int(rng.integers(1, t.ns - first + 1))
        if i in (10, 11, 40):                                    # repeated windows, with other buckets
            first, n = wins[i - 5][2], wins[i - 5][3]
        wins.append((t.dev, t.index, first, n))
        buckets.append([0, 1, 7, 64, 255, 256, 257, 441, 1024, 1025, 100000][i % 11])
        owner.append(t)
    got = ctx.digest_windows(wins, bucket_samples=buckets)
    want = [expected_digest(owner[i].full, owner[i].bits, wins[i][2], wins[i][3], buckets[i]) for i in range(64)]
    assert [table(d) for d in got] == want
    for i in (0, 10, 33, 63):
        assert table(ctx.digest_windows([wins[i]], bucket_samples=buckets[i])[0]) == want[i], i
    assert [table(d) for d in ctx.digest_windows(wins, bucket_samples=buckets, group_frames=2)] == want
    assert ctx.digest_windows([]) == [] and ctx.digest_windows([], return_codes=True) == ([], [])
    empty = ctx.digest_windows([(ts[2].dev, ts[2].index, 100, 0)], bucket_samples=5)[0]      # no samples: no buckets
    assert tuple(empty.crc32.shape) == (0,)


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_failures_stay_in_their_window_and_nothing_else_is_written(ctx, product, streams):
    """64 windows of five stream shapes with mixed bucket lengths, failing ones among them; the buffer byte for byte"""
    t, u = streams[(16, 2)], streams[(8, 1)]
    crc, rice = sc.damaged(ctx, product, t)
    (d_bad, bad_index, k), good = crc, (t.dev, t.index, 0, 1000, 2)
    special = {**sc.rice_windows(t, rice, [(100,), (7,), (441,)]),
               9: (d_bad, bad_index, t.bl[k][4] + 3, 600, 2, 100, None, CORRUPTION),
               10: (d_bad, bad_index, 0, t.bl[k][4] - 24, 2, 64, None, OK),                        # before the damaged block
               11: (d_bad, bad_index, t.bl[k + 1][4], 200, 2, 0, None, CORRUPTION),                # behind it
               20: good + (256, "misaligned", INVALID_ARGUMENT),
               22: good + (0, "null", INVALID_ARGUMENT),
               40: (t.dev, t.index, 1, t.ns, 2, 500, None, INVALID_ARGUMENT),                      # a range beyond num_samples
               41: (t.dev, t.index, 100, 2000, 2, 300, None, OK)}                                  # a good one, alone too
    ts = [streams[key] for key in ((8, 1), (16, 2), (24, 2), (16, 8), (8, 2))]
    items, tracks, codes = sc.many_windows(DIGEST, ctx, ts, t, lambda i: ([0, 1, 7, 64, 255, 256, 257, 441, 1024, 1025, 100000][(i * 3 + i // 16) % 11],), special, crc, rice)
    for i in (2, 3, 43, 62):                                     # good windows of other shapes alone: the same code, the same bytes
        ret1, codes1, buf1, offs1, nbs1 = sc.raw_call(DIGEST, ctx, [items[i]])
        assert (ret1, codes1) == (OK, [OK]) and buf1.tobytes() == sc.want_buffer(DIGEST, len(buf1), [items[i]], [tracks[i]], [OK], offs1, nbs1).tobytes(), i


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(streams):
    sc.launch_counts(DIGEST, streams[(16, 2)], streams[(8, 1)], ((), {"bucket_samples": 441}), lambda t, w, d: check(t, [w], [441], [d]))


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_the_same_audio_in_other_streams(ctx, oracle):
    """-m 0 and -m 7, blocks of 1024 and 4096, mid/side or not: equal digests, whole and per bucket; one LSB changes one bucket; a
    splice of the whole stream digests as its source"""
    x = mixed_signal(2, 16, 7 * S + TAIL, seed=77, block=S)
    forms = [oracle.encode_whole(x, 16, 44100, S, 0, False), oracle.encode_whole(x, 16, 44100, S, 7, True), oracle.encode_whole(x, 16, 44100, 4096, 7, True),
             oracle.encode_whole(x, 16, 44100, 4096, 0, True)]
    devs = [to_device(bytes(f)) for f in forms]
    assert len({bytes(f) for f in forms}) == 4
    for b in (0, 441):
        want = expected_digest(x, 16, 0, x.shape[1], b)
        assert [table(d) for d in ctx.digest_streams(devs, bucket_samples=b)] == [want] * 4
        for d in devs[1:]:
            assert ctx.same_audio(devs[0], d, bucket_samples=b) == (True, None)
    at = 3 * S + 123
    y = x.copy()
    y[1, at] += 1 if y[1, at] < 32767 else -1
    other = to_device(bytes(oracle.encode_whole(y, 16, 44100, 4096, 7, True)))
    a, b = ctx.digest_streams([devs[0], other], bucket_samples=441)
    assert [i for i, (p, q) in enumerate(zip(table(a), table(b))) if p != q] == [at // 441] and table(b) == expected_digest(y, 16, 0, y.shape[1], 441)
    assert ctx.same_audio(devs[0], other, bucket_samples=441) == (False, at // 441)
    assert ctx.same_audio(devs[0], other) == (False, 0) and ctx.same_audio(other, other) == (True, None)
    shorter = to_device(bytes(oracle.encode_whole(x[:, :-1], 16, 44100, S, 0, False)))
    mono = to_device(bytes(oracle.encode_whole(x[:1], 16, 44100, S, 0, False)))
    assert ctx.same_audio(devs[0], shorter) == (False, None) and ctx.same_audio(devs[0], mono, bucket_samples=100) == (False, None)
    index = ctx.index_stream(devs[1])
    spliced, = ctx.splice_streams([[(devs[1], index, 0, None)]])
    cut, = ctx.splice_streams([[(devs[1], index, 700, 3000)]])
    index.close()
    assert table(ctx.digest_streams([spliced], bucket_samples=441)[0]) == expected_digest(x, 16, 0, x.shape[1], 441)
    assert table(ctx.digest_streams([cut])[0]) == expected_digest(x, 16, 700, 3000, 0)
    assert ctx.same_audio(spliced, devs[0], bucket_samples=1024) == (True, None)
    assert table(ctx.digest_streams([bytes(forms[0])], group_frames=1)[0]) == expected_digest(x, 16, 0, x.shape[1], 0)      # bytes are taken too
    assert ctx.digest_streams([]) == []


LINE = re.compile(r"^crc32 ([0-9a-f]{8}) bytes (\d+) $")


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
@pytest.mark.parametrize("bits,nch", [(8, 2), (16, 2), (24, 1)])
def test_command_line_tool(ctx, tmp_path, streams, bits, nch):
    """digest_streams = zlib.crc32 of the `data` chunk of the WAV file linne_amd_cli -d writes, and -D prints it, whole and bucketed"""
    t = streams[(bits, nch)]
    lnn, wav = tmp_path / "a.lnn", tmp_path / "a.wav"
    lnn.write_bytes(t.stream)
    r = subprocess.run([CLI, "-d", "-q", str(lnn), str(wav)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    data = wav_data(wav)
    assert table(ctx.digest_streams([t.dev])[0]) == [(zlib.crc32(data), len(data))] == expected_digest(t.full, bits, 0, t.ns, 0)
    for b in (0, 1000):
        r = subprocess.run([CLI, "-D"] + ([str(b)] if b else []) + [str(lnn)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        lines = [LINE.match(x) for x in r.stdout.splitlines()]
        assert all(lines), r.stdout
        assert [(int(m.group(1), 16), int(m.group(2))) for m in lines] == expected_digest(t.full, bits, 0, t.ns, b)
    bad, _ = crc_damaged(t)
    lnn.write_bytes(bad)
    r = subprocess.run([CLI, "-D", str(lnn)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and not r.stdout and "Failed to digest" in r.stderr
