"""What the GPU tests of the windows consumers share (tests/test_gpu_stream_{measure,digest,quiet,histogram,relate}.py, the history
runner of tests/test_gpu_stream_history.py): the consumers as a table, the material helpers, and the scaffold that every bucket consumer
is held in -- the C entry point on tables that lie in one buffer of sentinels, the launch counts, and the 64 windows among which
failing ones must stay in their window.  A consumer is a row of CONSUMERS plus what is truly its own, which stays in its test file.

Quiet's tables have another shape (a capacity, runs instead of buckets, answers beside the table): its raw_call and want_buffer stay in
tests/test_gpu_stream_quiet.py; it shares the table, the material and launch_counts."""
import os
import re
from collections import namedtuple

import numpy as np

import linne_amd
from relate_refs import expected_relate
from stream_refs import be, blocks, crc16, expected_digest, expected_histogram, expected_measure, expected_quiet

OK, INVALID_ARGUMENT, CORRUPTION, NG = 0, 1, 6, 7
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
SENTINEL = 0x5A5A5A5A5A5A5A5A
PAD = 1                                     # buckets a padded stride leaves between the rows of a table
GAP = 3                                     # sentinel words in front of, between and behind the tables
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "linne_amd.h")).read(), flags=re.S)
KIND = {name: int(v) for name, v in re.findall(r"\bLINNE_AMD_(\w*T_\w+)\s*=\s*(\d+)", HEADER)}       # the kernel kinds, by their names less LINNE_AMD_
DECODE_KINDS = [KIND[k] for k in ("T_RICE_DECODE", "T_WX_GATHER", "T_WX_PARAMS", "T_WX_RICE_CHECK")]   # what every windows call has of the decode call


# ---- the consumers ----
# name; method: the Python form; entry: the C entry point; spec: its spec struct; stride: the spec's stride field; fields: how many
# fields of its own a window's spec has (the last is bucket_samples); rows(channels): the rows of a window's table; words(fields): the
# 64-bit words of a bucket; reference: what a window's table must hold; table(track, first, n, *fields): that as int64 (rows, buckets,
# words); fill(spec, *fields); python(list of fields) and scalar: the Python form's arguments, per window and one for all ->
# (args, keywords); empty(result of a window without samples, channels): its shape; kinds: pass, then what a call launches once
Consumer = namedtuple("Consumer", "name method entry spec stride fields rows words reference table fill python scalar empty kinds")


def bucket_fill(sp, b):
    sp.bucket_samples = b


def histogram_fill(sp, bins, shift, scale, b):
    sp.bucket_samples, sp.num_bins, sp.shift, sp.scale = b, bins, shift, scale


def records(dtype):
    """[row][bucket] of tuples, or a structured array (rows, buckets) -> int64 (rows, buckets, words)"""
    return lambda want: np.ascontiguousarray(np.array(want, dtype=dtype)).view(np.int64).reshape(len(want), -1, dtype.itemsize // 8)


def kinds(*names):
    return tuple(KIND[n] for n in names)


measure_words, relate_words = records(linne_amd.MEASURE_DTYPE), records(linne_amd.RELATION_DTYPE)
digest_words = records(linne_amd.DIGEST_DTYPE)
CONSUMERS = {c.name: c for c in (
    Consumer("place", "decode_windows", "LINNEAmd_DecodeWindowsDevice", None, None, 0, None, None, None, None, None, None, None, None, kinds("T_WX_PLACE")),
    Consumer("compare", "compare_windows", "LINNEAmd_CompareWindowsDevice", None, None, 0, None, None, None, None, None, None, None, None, kinds("COMPARE_T_COMPARE")),
    Consumer("measure", "measure_windows", "LINNEAmd_MeasureWindowsDevice", "MeasureSpec", "channel_stride", 1, lambda C: C, lambda b: 4, expected_measure,
             lambda t, first, n, b: measure_words(expected_measure(t.full, first, n, b)), bucket_fill,
             lambda f: ((), {"bucket_samples": [x[0] for x in f]}), ((), {"bucket_samples": 7}), lambda m, C: (tuple(m.min.shape), (C, 0)),
             kinds("MEASURE_T_MEASURE", "MEASURE_T_PRESET", "MEASURE_T_COMMIT")),
    Consumer("digest", "digest_windows", "LINNEAmd_DigestWindowsDevice", "DigestSpec", None, 1, lambda C: 1, lambda b: 2, expected_digest,
             lambda t, first, n, b: digest_words([[(crc, 0, size) for crc, size in expected_digest(t.full, t.bits, first, n, b)]]), bucket_fill,
             lambda f: ((), {"bucket_samples": [x[0] for x in f]}), ((), {"bucket_samples": 7}), lambda d, C: (tuple(d.crc32.shape), (0,)),
             kinds("DIGEST_T_DIGEST", "DIGEST_T_PRESET", "DIGEST_T_COMMIT")),
    Consumer("quiet", "quiet_windows", "LINNEAmd_QuietWindowsDevice", "QuietSpec", None, 3, None, None, expected_quiet, None, None, None, None, None,
             kinds("QUIET_T_QUIET", "QUIET_T_PRESET", "QUIET_T_COUNT", "QUIET_T_SCAN", "QUIET_T_STARTS", "QUIET_T_ENDS")),
    Consumer("histogram", "histogram_windows", "LINNEAmd_HistogramWindowsDevice", "HistogramSpec", "channel_stride", 4, lambda C: C,
             lambda bins, *_: bins if 1 <= bins <= 1024 else 4, expected_histogram,          # (a refused num_bins: room for four, which must stay sentinels)
             lambda t, first, n, bins, shift, scale, b: expected_histogram(t.full, first, n, bins, shift, bool(scale), b), histogram_fill,
             lambda f: (tuple([x[j] if j != 2 else bool(x[j]) for x in f] for j in range(4)), {}), ((64,), {}), lambda h, C: (tuple(h.counts.shape), (C, 0, 64)),
             kinds("HISTOGRAM_T_HISTOGRAM", "HISTOGRAM_T_PRESET", "HISTOGRAM_T_COMMIT")),
    Consumer("relate", "relate_windows", "LINNEAmd_RelateWindowsDevice", "RelateSpec", "pair_stride", 1, lambda C: C * (C + 1) // 2, lambda b: 4, expected_relate,
             lambda t, first, n, b: relate_words(expected_relate(t.full, first, n, b)), bucket_fill,
             lambda f: (([x[0] for x in f],), {}), ((), {"bucket_samples": 64}), lambda r, C: (tuple(r.records.shape), (C * (C + 1) // 2, 0, 4)),
             kinds("RELATE_T_RELATE", "RELATE_T_PRESET", "RELATE_T_COMMIT")),
)}
BUCKET_CONSUMERS = ("measure", "digest", "histogram", "relate")


def other_kinds(name):
    """every kind of every other row of the table: what a call of consumer `name` must not launch"""
    return sorted(k for c in CONSUMERS.values() if c.name != name for k in c.kinds)


# ---- the material ----
def to_device(stream):
    import torch
    return torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()


class Stream:
    """a stream, the oracle's decode of its bytes, its device copy and index"""

    def __init__(self, ctx, oracle, data, name=""):
        self.name, self.stream = name, bytes(data)
        ret, full, _ = oracle.decode_whole(self.stream)
        assert ret == OK, name
        self.full = np.ascontiguousarray(full, dtype=np.int32)
        self.nch, self.ns = self.full.shape
        self.bits = be(self.stream[22:24])
        self.bl = blocks(self.stream)
        self.dev = to_device(self.stream)
        self.index = ctx.index_stream(self.dev)


def encoded(ctx, oracle, x, bits, preset, ms, name=""):
    t = Stream(ctx, oracle, oracle.encode_whole(x, bits, 44100, S, preset, ms), name)
    assert np.array_equal(t.full, x), name
    return t


def crc_damaged(t):
    """(the track's stream with a payload byte of block k flipped, so that the block's CRC fails; k)"""
    k = len(t.bl) // 2
    off, size = t.bl[k][:2]
    bad = bytearray(t.stream)
    bad[off + size - 2] ^= 0x10
    return bytes(bad), k


def rice_damaged(product, t):
    """(t's stream with a bit in the Rice codes of COMPRESS block k flipped and the block's CRC16 made right again, such that the whole
    decode fails; k): the index finds nothing wrong with it, the device's Rice check does, and sets the window's fail word there"""
    rng = np.random.default_rng(77)
    for k in sorted((i for i, b in enumerate(t.bl[:-1]) if b[2] == COMPRESS and i > 0), reverse=True):      # the last such block that 64 flips can break
        off, size = t.bl[k][:2]
        for _ in range(64):
            bad = bytearray(t.stream)
            p = off + 11 + (size - 11) // 2 + int(rng.integers(0, (size - 11) // 2))   # the later half of the payload: Rice codes
            bad[p] ^= 1 << int(rng.integers(0, 8))
            bad[off + 6:off + 8] = crc16(bad[off + 8:off + size]).to_bytes(2, "big")
            if product.decode_whole(bytes(bad))[0] != OK:
                return bytes(bad), k
    raise AssertionError("no flip in 64 made the whole decode fail")


def last_error(ctx):
    return linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode()


# ---- the C entry point of a bucket consumer on tables between sentinels ----
def num_buckets(n, b):
    return 0 if n == 0 else (1 if b == 0 else -(-n // b))


def layout(c, items, pad=PAD, gap=GAP):
    """the tables' first words, their bucket counts and the buffer's words: every table's rows pad buckets apart, gap sentinel words in
    front of, between and behind the tables"""
    offs, nbs, at = [], [], gap
    for it in items:
        nb = num_buckets(it[3], it[4 + c.fields])
        offs.append(at)
        nbs.append(nb)
        at += c.rows(it[4]) * (nb + pad) * c.words(*it[5:5 + c.fields]) + gap
    return offs, nbs, at


def raw_call(c, ctx, items, group_frames=0, faults=None, pad=PAD, gap=GAP):
    """consumer c's C entry point itself.  items: (stream, index, first, n, channels, the spec's own fields ..., what is wrong with the
    spec): "misaligned", "null", "stride" (one short), or a key of faults, name -> what it does to the spec; every window's table lies
    in one buffer of sentinels -> (ret, codes, the buffer as numpy int64, the tables' first words, the bucket counts)"""
    import torch
    offs, nbs, words = layout(c, items, pad, gap)
    buf = torch.full((words,), SENTINEL, dtype=torch.int64, device="cuda")
    W = len(items)
    w, sp = (linne_amd.Window * W)(), (getattr(linne_amd, c.spec) * W)()
    for j, (dev, index, first, n, nch, *fields, wrong) in enumerate(items):
        w[j].index, w[j].d_stream, w[j].first_sample, w[j].num_samples, w[j].d_pcm, w[j].pcm_stride, w[j].result = index.h, dev.data_ptr(), first, n, None, 0, -1
        c.fill(sp[j], *fields)
        sp[j].d_out = None if wrong == "null" else buf.data_ptr() + 8 * offs[j] + (4 if wrong == "misaligned" else 0)
        if c.stride:
            setattr(sp[j], c.stride, nbs[j] - 1 if wrong == "stride" else nbs[j] + pad)
        if wrong in (faults or {}):
            faults[wrong](sp[j])
    torch.cuda.synchronize()
    ret = getattr(linne_amd.lib, c.entry)(ctx.h, w, sp, W, group_frames)
    return ret, [w[j].result for j in range(W)], buf.cpu().numpy(), offs, nbs


def want_buffer(c, words, items, tracks, codes, offs, nbs, pad=PAD):
    """sentinels but the OK windows' tables"""
    buf = np.full(words, SENTINEL, dtype=np.int64)
    for it, t, code, off, nb in zip(items, tracks, codes, offs, nbs):
        if code != OK or it[3] == 0:
            continue
        want = c.table(t, it[2], it[3], *it[5:5 + c.fields])
        assert want.shape[:2] == (c.rows(it[4]), nb)
        for r, row in enumerate(want):
            at = off + r * (nb + pad) * want.shape[2]
            buf[at:at + row.size] = row.reshape(-1)
    return buf


def as_words(result):
    """a Python form's result as want_buffer's table"""
    a = np.ascontiguousarray(result.cpu())
    return a.view(np.int64).reshape(a.shape + (-1,)) if a.dtype.names else a


# ---- the launches ----
def launch_counts(c, mixed, three, args, check_last):
    """what the launches of a call of consumer c must be: the decode call's with c's pass kind in place of kind 59, c's other kinds
    once each, none of any other consumer's, the same for one window and for 64.  args: (args, keywords) of the Python form behind its
    windows; check_last(track, (first, n), result) holds the last window's answer to its reference"""
    place, (run, *once) = CONSUMERS["place"].kinds[0], c.kinds
    ctx = linne_amd.Context(0, use_torch_stream=False)
    try:
        ctx.enable_timing(True)
        counts = {}
        for t in (mixed, three):
            index = ctx.index_stream(t.dev)
            for nw in (1, 64):
                spans = [(0, t.ns)] + [(37 * i, t.ns - 53 * i) for i in range(1, nw)]
                wins = [(t.dev, index, a, n) for a, n in spans]
                for gf in (0, 2):
                    ctx.decode_windows(wins, group_frames=gf)
                    dec = {k: ctx.last_launches(k) for k in DECODE_KINDS + [place]}
                    got = getattr(ctx, c.method)(wins, *args[0], group_frames=gf, **args[1])
                    mine = {k: ctx.last_launches(k) for k in DECODE_KINDS + list(c.kinds) + other_kinds(c.name)}
                    check_last(t, spans[-1], got[-1])
                    assert all(mine[k] == 0 for k in other_kinds(c.name)), (t.name, nw, gf, mine)           # kind 59 among them
                    assert mine[run] == dec[place] >= 1, (t.name, nw, gf, dec, mine)                         # a launch per placing pass
                    assert all(mine[k] == dec[k] for k in DECODE_KINDS), (t.name, nw, gf, dec, mine)
                    assert all(mine[k] == 1 for k in once), (t.name, nw, gf, mine)                           # the launches per call
                    assert ctx.last_ms(run) > 0
                    counts[(nw, gf)] = mine
                assert counts[(nw, 0)][run] == 1
            assert counts[(1, 0)] == counts[(64, 0)]                  # not a launch more for 64 windows than for one
            assert counts[(1, 2)][run] > 1                            # the window spans passes
            index.close()
    finally:
        ctx.close()


# ---- many windows, and failures stay in their window ----
def damaged(ctx, product, t):
    """t's CRC-damaged and Rice-damaged copies on the device, indexed: ((stream, index, block), (stream, index, block)).  The index
    takes the Rice-damaged stream: its block heads and CRCs are right"""
    out = []
    for data, k in (crc_damaged(t), rice_damaged(product, t)):
        dev = to_device(data)
        out.append((dev, ctx.index_stream(dev), k))
    assert 0 < out[0][2] < len(t.bl) - 1
    return out


def rice_windows(t, rice, fields):
    """windows 5 to 7 of every bucket consumer's list: over the Rice-damaged block -- the fail word is set on the device, the commit
    skips that window alone --, in front of it, and the whole damaged stream.  fields: the three windows' own spec fields"""
    dev, index, kr = rice
    return {5: (dev, index, t.bl[kr][4] + 10, 600, t.nch, *fields[0], None, NG),
            6: (dev, index, t.bl[kr - 1][4] + 10, 600, t.nch, *fields[1], None, OK),
            7: (dev, index, 0, t.ns, t.nch, *fields[2], None, NG)}


def many_windows(c, ctx, ts, t, fields_of, special, crc, rice, faults=None):
    """64 windows over the streams ts (a seventh of them without samples) with the spec fields fields_of(i), and `special`: window ->
    an item of raw_call and its code, on t and its damaged copies `crc` and `rice` (damaged()).  Windows 5 to 7 are rice_windows(),
    9 to 11 the CRC-damaged stream's, the first of them failing; a spec fault must have the code INVALID_ARGUMENT and, but for a range
    beyond the stream, the consumer's name in its text.  (Of the argument errors of a window, nb > 2^32 - 1 cannot be reached: a
    stream's header holds a 32-bit sample count and a bucket has a sample or more.) -> (items, tracks, codes)"""
    import pytest
    k, kr = crc[2], rice[2]
    rng = np.random.default_rng(4)
    items, tracks = [], []
    for i in range(64):
        u = ts[i % len(ts)]
        first = int(rng.integers(0, u.ns))
        n = int(rng.integers(1, u.ns - first + 1)) if i % 7 else 0
        items.append((u.dev, u.index, first, n, u.nch, *fields_of(i), None))
        tracks.append(u)
    want_codes = [OK] * 64
    for i, sp in special.items():
        items[i], tracks[i], want_codes[i] = sp[:-1], t, sp[-1]
    assert want_codes[5] == NG and want_codes[9] == CORRUPTION and all(code == OK for code in want_codes[:5] + [want_codes[8]])
    ret, codes, buf, offs, nbs = raw_call(c, ctx, items, faults=faults)
    assert codes == want_codes and ret == NG                     # the lowest failing window's
    text = last_error(ctx)
    assert text.startswith(f"window 5: block {kr} ")
    assert buf.tobytes() == want_buffer(c, len(buf), items, tracks, want_codes, offs, nbs).tobytes()    # byte for byte: the tables, and sentinels everywhere else
    ret2, codes2, buf2, *_ = raw_call(c, ctx, items, group_frames=2, faults=faults)
    assert (ret2, codes2) == (ret, codes) and np.array_equal(buf2, buf)
    # codes and text are the decode call's
    _, dcodes = ctx.decode_windows([it[:4] for it in items[8:12]], return_codes=True)
    assert dcodes == want_codes[8:12] and last_error(ctx).startswith(f"window 1: block {k} ")
    _, dcodes = ctx.decode_windows([it[:4] for it in items[4:8]], return_codes=True)
    assert dcodes == want_codes[4:8] and last_error(ctx) == text.replace("window 5:", "window 1:")
    for i in sorted(special):                                    # alone: the same code, the same bytes, nothing written by a failing one
        ret1, codes1, buf1, offs1, nbs1 = raw_call(c, ctx, [items[i]], faults=faults)
        assert (ret1, codes1) == (want_codes[i], [want_codes[i]]), i
        assert buf1.tobytes() == want_buffer(c, len(buf1), [items[i]], [tracks[i]], [want_codes[i]], offs1, nbs1).tobytes(), i
        if want_codes[i] == INVALID_ARGUMENT and items[i][2] + items[i][3] <= t.ns:
            assert last_error(ctx).startswith(f"window 0: {c.entry[len('LINNEAmd_'):]}: "), i
    # the Python form: codes, None for a failing window
    method = getattr(ctx, c.method)
    four = [it[:4] for it in items[8:12]]
    args, kw = c.python([it[5:5 + c.fields] for it in items[8:12]])
    got, pcodes = method(four, *args, return_codes=True, **kw)
    assert pcodes == want_codes[8:12] == [OK, CORRUPTION, OK, CORRUPTION]
    for j in range(4):
        it = items[8 + j]
        if pcodes[j] != OK:
            assert got[j] is None
        elif it[3]:
            assert np.array_equal(as_words(got[j]).reshape(-1), c.table(tracks[8 + j], it[2], it[3], *it[5:5 + c.fields]).reshape(-1)), j
    with pytest.raises(linne_amd.LinneAmdError) as e:
        method(four, *c.scalar[0], **c.scalar[1])                 # one value for every window
    assert e.value.code == CORRUPTION and e.value.codes == pcodes and "window 1:" in str(e.value)
    assert method([], *c.scalar[0], **c.scalar[1]) == [] and method([], *c.scalar[0], return_codes=True, **c.scalar[1]) == ([], [])
    u = ts[-1]
    empty = method([(u.dev, u.index, 100, 0)], *c.scalar[0], **dict(c.scalar[1], bucket_samples=5))[0]      # no samples: no buckets
    have, want = c.empty(empty, u.nch)
    assert have == want
    for _, index, _ in (crc, rice):
        index.close()
    return items, tracks, want_codes
