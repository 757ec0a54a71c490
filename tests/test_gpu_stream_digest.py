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
from test_cli_cpu import CLI
from test_gpu_stream_compare import Stream, encoded
from test_gpu_stream_windows import crc_damaged, mixed_signal, to_device
from test_stream_digest_cpu import expected_digest, table, wav_data
from test_stream_measure_cpu import CARRY_NS, carry_stream

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CORRUPTION, NG = 0, 1, 6, 7
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300
BUCKETS = [0, 1, 7, 255, 256, 257, 441, 1024, 1025, 100000]
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
SENTINEL = 0x5A5A5A5A5A5A5A5A


def test_failures_stay_in_their_window_and_nothing_else_is_written(ctx, streams):
    import torch
    t, u = streams[(16, 2)], streams[(8, 1)]
    bad, k = crc_damaged(t)
    assert 0 < k < len(t.bl) - 1
    d_bad = to_device(bad)
    bad_index = ctx.index_stream(d_bad)
    at_k = t.bl[k][4]
    # (stream, index, first, n, bucket, track, expected code, what is wrong with its spec)
    cases = [(t.dev, t.index, 100, 2000, 300, t, OK, None),
             (d_bad, bad_index, 0, at_k - 24, 64, t, OK, None),                      # before the damaged block
             (d_bad, bad_index, at_k + 3, 600, 100, t, CORRUPTION, None),
             (d_bad, bad_index, t.bl[k + 1][4], 200, 0, t, CORRUPTION, None),        # behind it
             (t.dev, t.index, 0, 1000, 256, t, INVALID_ARGUMENT, "misaligned"),
             (t.dev, t.index, 0, 1000, 0, t, INVALID_ARGUMENT, "null"),
             (t.dev, t.index, 1, t.ns, 500, t, INVALID_ARGUMENT, None),              # a range beyond num_samples
             (u.dev, u.index, 517, 1500, 0, u, OK, None),
             (u.dev, u.index, 0, u.ns, 1000, u, OK, None)]
    W = len(cases)
    nbs = [1 if b == 0 else -(-n // b) for _, _, _, n, b, *_ in cases]
    offs, at = [], 1
    for nb in nbs:
        offs.append(at)                                          # (a sentinel record in front of, between and behind the tables)
        at += nb + 1
    total = at

    def call(which):
        buf = torch.full((total, 2), SENTINEL, dtype=torch.int64, device="cuda")
        w, sp = (linne_amd.Window * len(which))(), (linne_amd.DigestSpec * len(which))()
        for j, i in enumerate(which):
            dev, index, first, n, b, _, _, wrong = cases[i]
            w[j].index, w[j].d_stream, w[j].first_sample, w[j].num_samples, w[j].d_pcm, w[j].pcm_stride, w[j].result = index.h, dev.data_ptr(), first, n, None, 0, -1
            sp[j].bucket_samples, sp[j].d_out = b, buf.data_ptr() + 16 * offs[i]
            if wrong == "misaligned":
                sp[j].d_out = buf.data_ptr() + 16 * offs[i] + 4
            elif wrong == "null":
                sp[j].d_out = None
        torch.cuda.synchronize()
        ret = linne_amd.lib.LINNEAmd_DigestWindowsDevice(ctx.h, w, sp, len(which), 0)
        return ret, [w[j].result for j in range(len(which))], buf.cpu().numpy().view(linne_amd.DIGEST_DTYPE).reshape(total)

    def want_buffer(which):
        """every record of the buffer: sentinels but the OK windows' buckets"""
        buf = np.full((total, 2), SENTINEL, dtype=np.int64).view(linne_amd.DIGEST_DTYPE).reshape(total)
        for i in which:
            _, _, first, n, b, tr, code, _ = cases[i]
            if code != OK:
                continue
            for j, (crc, size) in enumerate(expected_digest(tr.full, tr.bits, first, n, b)):
                buf[offs[i] + j] = (crc, 0, size)
        return buf

    ret, codes, buf = call(range(W))
    assert codes == [c[6] for c in cases]
    assert ret == CORRUPTION                                     # the lowest failing window's
    assert linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode().startswith(f"window 2: block {k} ")
    assert buf.tobytes() == want_buffer(range(W)).tobytes()      # byte for byte: the tables, and sentinels everywhere else
    for i in range(W):                                           # and every window alone: the same code, the same bytes
        ret1, codes1, buf1 = call([i])
        assert (ret1, codes1) == (cases[i][6], [cases[i][6]]), i
        assert buf1.tobytes() == want_buffer([i]).tobytes(), i
    # the Python form: codes, None for a failing window
    four = [c[:4] for c in cases[:4]]
    got, pcodes = ctx.digest_windows(four, bucket_samples=[c[4] for c in cases[:4]], return_codes=True)
    assert pcodes == [OK, OK, CORRUPTION, CORRUPTION] and got[2] is None and got[3] is None
    for i in (0, 1):
        assert table(got[i]) == expected_digest(t.full, 16, cases[i][2], cases[i][3], cases[i][4])
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.digest_windows(four, bucket_samples=7)
    assert e.value.code == CORRUPTION and e.value.codes == pcodes and "window 2:" in str(e.value)
    bad_index.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(streams):
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        c.enable_timing(True)
        counts = {}
        for t in (streams[(16, 2)], streams[(8, 1)]):
            index = c.index_stream(t.dev)
            for nw in (1, 64):
                spans = [(0, t.ns)] + [(37 * i, t.ns - 53 * i) for i in range(1, nw)]
                for gf in (0, 2):
                    c.decode_windows([(t.dev, index, a, n) for a, n in spans], group_frames=gf)
                    dec = {k: c.last_launches(k) for k in (28, 56, 57, 58, 59)}
                    got = c.digest_windows([(t.dev, index, a, n) for a, n in spans], bucket_samples=441, group_frames=gf)
                    dig = {k: c.last_launches(k) for k in (28, 56, 57, 58, 59, 79, 80, 81, 82, 83, 84, 85)}
                    assert table(got[-1]) == expected_digest(t.full, t.bits, spans[-1][0], spans[-1][1], 441)
                    assert dig[59] == dig[79] == dig[80] == dig[81] == dig[82] == 0 and dig[83] == dec[59] >= 1, (t.name, nw, gf, dec, dig)   # a launch per placing pass
                    assert all(dig[k] == dec[k] for k in (28, 56, 57, 58)), (t.name, nw, gf, dec, dig)
                    assert dig[84] == 1 and dig[85] == 1, (t.name, nw, gf, dig)                                   # the two launches per call
                    assert c.last_ms(83) > 0
                    counts[(t.name, nw, gf)] = dig
                assert counts[(t.name, nw, 0)][83] == 1
            assert counts[(t.name, 1, 0)] == counts[(t.name, 64, 0)]          # not a launch more for 64 windows than for one
            assert counts[(t.name, 1, 2)][83] > 1                             # the window spans passes
            index.close()
    finally:
        c.close()


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
