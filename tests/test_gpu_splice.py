"""GPU tests of cutting and joining resident .lnn streams (Context.splice_streams; include/linne_amd.h LINNEAmd_SpliceStreamsDevice):
every output's bytes against the numpy assembly of source blocks (from the index tables) and the oracle's edge blocks, the copy
kernel's alignment matrix behind sentinels, failing outputs among good ones with every code of the contract, one call against many,
and -a 1.  tests/test_splice_cpu.py holds the oracle to the real reference on such streams."""
import ctypes as C

import numpy as np
import pytest

import linne_amd
import splice_cases as sc
from signals import music

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, INSUFFICIENT_BUFFER, CORRUPTION = sc.OK, sc.INVALID_ARGUMENT, sc.INSUFFICIENT_BUFFER, sc.CORRUPTION
SENTINEL = 0xA5
CHUNK = 32768                                                  # linne_amd/csrc/lnn_splice.h SP_CHUNK_UNITS * 16
STREAM_KINDS = list(range(48, 69)) + [71, 72]                  # include/linne_amd.h: the stream-level kernels of windows, encode and splice


def as_bytes(t):
    return bytes(t.cpu().numpy())


class Source:
    """a PCM signal, its stream encoded on the device, the stream's index and block tables"""

    def __init__(self, ctx, x, bits, block, preset, rate=44100, data=None):
        self.x, self.bits, self.block, self.preset, self.rate = x, bits, block, preset, rate
        self.ms = x.shape[0] >= 2
        self.t = ctx.encode_stream(x, bits, rate, block, preset, self.ms).clone() if data is None else data
        self.bytes = as_bytes(self.t)
        self.index = ctx.index_stream(self.t)
        self.tables = tuple(list(int(v) for v in a) for a in self.index.blocks())


def expected(oracle, cuts, af_iters=0):
    """cuts = [(Source, first, n)] -> (bytes, copied, encoded, PCM): the index tables' blocks and the oracle's edge blocks"""
    out = [sc.with_num_samples(cuts[0][0].bytes[:sc.HEADER], sum(n for _, _, n in cuts))]
    copied = encoded = 0
    for s, lo, n in cuts:
        off, first, size, typ, nsmp = s.tables
        for p in sc.pieces(s.tables, lo, n):
            if p[0] == "copy":
                out.append(s.bytes[off[p[1]]:off[p[2] - 1] + size[p[2] - 1] + 6])
                copied += p[2] - p[1]
            else:
                out.append(oracle.encode_whole(s.x[:, p[1]:p[2]], s.bits, s.rate, s.block, s.preset, s.ms, af_iters=af_iters)[sc.HEADER:])
                encoded += 1
    return b"".join(out), copied, encoded, np.concatenate([s.x[:, lo:lo + n] for s, lo, n in cuts], axis=1)


def check_outputs(ctx, oracle, outputs, got, af_iters=0):
    for k, cuts in enumerate(outputs):
        want, copied, encoded, pcm = expected(oracle, cuts, af_iters)
        data = as_bytes(got[k])
        assert data == want, f"output {k}"
        assert ctx.last_splice_blocks[k] == (copied, encoded), f"output {k}"
        ret, back, _ = oracle.decode_whole(data)
        assert ret == OK and np.array_equal(back, pcm), f"output {k}: the oracle's decode"
        ix = ctx.index_stream(got[k])
        assert ix.failure()[0] == -1 and np.array_equal(ctx.decode_stream(got[k], index=ix).cpu().numpy(), pcm), f"output {k}: the product's decode"
        ix.close()


def branch_cuts(a, b):
    """outputs that hit every branch of the planner test, for two sources of one shape: 7 whole blocks and a ragged one each
    (every edge block longer than 128 samples at a block size of 256: inside the contract at every preset)"""
    S, total = a.block, a.x.shape[1]
    return [[(a, S + S // 4, S // 2 + S // 8)],                             # inside one block
            [(a, S, 3 * S)],                                                # on block boundaries: nothing re-encoded
            [(a, S + S // 2 - 12, 4 * S + S // 2 - 100)],                   # head and tail fragments
            [(a, 6 * S, total - 6 * S)],                                    # the ragged last block whole
            [(a, 7 * S, total - 7 * S)],                                    # ... alone
            [(a, 0, total)],                                                # the whole stream
            [(a, 0, 0), (a, S // 8, S - S // 8), (b, S // 2, 0), (b, S, 2 * S), (a, total, 0)],     # zero-sample cuts between others
            [(a, S // 4 + 7, 2 * S + S // 2), (b, 2 * S, 2 * S - S // 3), (a, 0, S)]]              # a join of two streams


@pytest.mark.parametrize("nch,bits,block,preset", [(1, 16, 256, 0), (2, 16, 1024, 7), (8, 24, 256, 7), (2, 24, 1024, 0)])
def test_bytes_of_every_planner_branch(ctx, oracle, nch, bits, block, preset):
    total = 7 * block + block // 2 + 9
    a = Source(ctx, music(nch, total, bits, seed=block + nch), bits, block, preset)
    b = Source(ctx, music(nch, total, bits, seed=block + nch + 50), bits, block, preset)
    assert a.index.num_blocks == 8
    outputs = branch_cuts(a, b)
    got = ctx.splice_streams([[(s.t, s.index, lo, n) for s, lo, n in cuts] for cuts in outputs])
    assert ctx.last_splice_blocks[1] == (3, 0) and ctx.last_splice_count(0) == len(outputs)
    check_outputs(ctx, oracle, outputs, got)
    assert ctx.last_splice_count(1) == sum(c for c, _ in ctx.last_splice_blocks) and ctx.last_splice_count(2) == sum(e for _, e in ctx.last_splice_blocks)
    # group_frames never changes a byte
    again = ctx.splice_streams([[(s.t, s.index, lo, n) for s, lo, n in cuts] for cuts in outputs], group_frames=3)
    assert [as_bytes(t) for t in again] == [as_bytes(t) for t in got]


def test_silent_and_raw_blocks(ctx, oracle):
    S = 1024
    rng = np.random.default_rng(5)
    noise = lambda n: rng.integers(-32768, 32768, size=(2, n), dtype=np.int64).astype(np.int32)
    parts = [music(2, S, 16, seed=1), np.zeros((2, 2 * S), np.int32), noise(2 * S), music(2, S, 16, seed=2), np.zeros((2, S), np.int32), music(2, S // 2, 16, seed=3)]
    src = Source(ctx, np.concatenate(parts, axis=1), 16, S, 7)
    assert src.tables[3] == [sc.COMPRESS, sc.SILENT, sc.SILENT, sc.RAW, sc.RAW, sc.COMPRESS, sc.SILENT, sc.COMPRESS]
    outputs = [[(src, S + 300, 3 * S)],                                     # from inside a SILENT block to inside a RAW block
               [(src, 2 * S, 2 * S)],                                       # a SILENT and a RAW block whole
               [(src, 3 * S + 200, 400), (src, 6 * S + 100, 500)],          # inside a RAW block, inside a SILENT block
               [(src, S, S), (src, 6 * S, S)]]                              # runs of one tiny SILENT block
    got = ctx.splice_streams([[(s.t, s.index, lo, n) for s, lo, n in cuts] for cuts in outputs])
    check_outputs(ctx, oracle, outputs, got)
    types = [sc.blocks_of(as_bytes(t))[3] for t in got]
    assert types[0][:3] == [sc.SILENT, sc.SILENT, sc.RAW] and len(types[0]) == 4 and types[2][1] == sc.SILENT and types[3] == [sc.SILENT, sc.SILENT]


def raw_call(ctx, outputs, group_frames=0):
    """LINNEAmd_SpliceStreamsDevice on the caller's own buffers: outputs = [(cuts, d_out, capacity)], cuts = [(tensor or None, index
    handle or None, first, n)] -> (return code, error text, the Splice array)"""
    arr = (linne_amd.Splice * max(len(outputs), 1))()
    keep = []
    for k, (cuts, d_out, capacity) in enumerate(outputs):
        cs = (linne_amd.Cut * max(len(cuts or []), 1))()
        for i, (t, h, first, n) in enumerate(cuts or []):
            cs[i].index, cs[i].d_stream, cs[i].first_sample, cs[i].num_samples = h, (t.data_ptr() if t is not None else None), first, n
        keep.append(cs)
        arr[k].cuts, arr[k].num_cuts, arr[k].d_out, arr[k].capacity = (cs if cuts is not None else None), (len(cuts) if cuts is not None else 1), d_out, capacity
        arr[k].out_bytes, arr[k].result = 12345, -1
    ctx._fence()
    ret = linne_amd.lib.LINNEAmd_SpliceStreamsDevice(ctx.h, arr, len(outputs), group_frames)
    return ret, linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode(), arr


def test_copy_kernel_alignment_matrix(ctx):
    """16 source alignments x 16 destination alignments of one run longer than four chunks, behind runs of 0 .. 15 tiny SILENT blocks,
    every output inside a sentinel-filled buffer"""
    import torch
    rng = np.random.default_rng(9)
    noise = rng.integers(-32768, 32768, size=(2, 8 * 4096), dtype=np.int64).astype(np.int32)
    big = Source(ctx, noise, 16, 4096, 0)
    quiet = Source(ctx, np.zeros((2, 16 * 4096), np.int32), 16, 4096, 0)
    assert set(big.tables[3]) == {sc.RAW} and quiet.tables[3] == [sc.SILENT] * 16 and quiet.tables[2] == [5] * 16      # 11-byte blocks
    n_big = len(big.bytes)
    assert n_big - sc.HEADER > 4 * CHUNK
    # the big stream again at byte offsets 0 .. 15 of one buffer
    pitch = (n_big + 15 + 63) & ~63
    srcbuf = torch.full((16 * pitch + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    base = (-srcbuf.data_ptr()) % 16
    views = []
    for i in range(16):
        v = srcbuf[base + i * pitch + i:base + i * pitch + i + n_big]
        v.copy_(big.t)
        views.append(v)
    assert [v.data_ptr() % 16 for v in views] == list(range(16))
    slot = (n_big + 16 * 11 + 64 + 63) & ~63
    outbuf = torch.full((256 * slot + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    obase = (-outbuf.data_ptr()) % 16 + 32
    image = np.full(outbuf.numel(), SENTINEL, dtype=np.uint8)
    outputs, pairs, sizes = [], set(), []
    for i in range(16):
        for j in range(16):
            at = obase + (16 * i + j) * slot + 4 * (i % 4)                 # outputs at 4-byte-aligned places of every residue
            cuts = ([(quiet.t, quiet.index.h, 0, 4096 * j)] if j else []) + [(views[i], big.index.h, 0, noise.shape[1])]
            want = sc.with_num_samples(big.bytes[:30], 4096 * j + noise.shape[1]) + quiet.bytes[30:30 + 11 * j] + big.bytes[30:]
            image[at:at + len(want)] = np.frombuffer(want, dtype=np.uint8)
            outputs.append((cuts, outbuf.data_ptr() + at, len(want)))       # exactly the room it needs
            sizes.append(len(want))
            pairs.add(((views[i].data_ptr() + 30) % 16, (outbuf.data_ptr() + at + 30 + 11 * j) % 16))
            if j:
                pairs.add(((quiet.t.data_ptr() + quiet.tables[0][0]) % 16, (outbuf.data_ptr() + at + 30) % 16))
    assert {s for s, _ in pairs} == set(range(16)) and {d for _, d in pairs} == set(range(16))
    assert len({(s, d) for s, d in pairs}) >= 256
    ret, msg, arr = raw_call(ctx, outputs)
    assert ret == OK, msg
    assert [(arr[k].result, arr[k].out_bytes, arr[k].encoded_blocks) for k in range(256)] == [(OK, sizes[k], 0) for k in range(256)]
    assert [arr[16 * i + j].copied_blocks for i in range(2) for j in range(16)] == [8 + j for _ in range(2) for j in range(16)]
    assert ctx.last_splice_count(3) == 256 + 240 and ctx.last_splice_count(4) == sum(sizes) - 30 * 256 and ctx.last_splice_count(2) == 0
    got = outbuf.cpu().numpy()
    bad = np.flatnonzero(got != image)
    assert bad.size == 0, f"first differing byte {bad[0]} (slot {(bad[0] - obase) // slot}, byte {(bad[0] - obase) % slot} of it)"
    assert bytes(srcbuf.cpu().numpy()[base:base + 30]) == big.bytes[:30]   # the sources are as they were
    for i in range(16):
        assert as_bytes(views[i]) == big.bytes


def test_isolation_and_codes(ctx, oracle):
    import torch
    S = 1024
    good = Source(ctx, music(2, 8 * S, 16, seed=40), 16, S, 0)
    other = Source(ctx, music(2, 8 * S, 16, seed=41), 16, S, 7)              # another preset
    mono = Source(ctx, music(1, 8 * S, 16, seed=42), 16, S, 0)
    hurt = bytearray(good.bytes)
    hurt[good.tables[0][5] + 40] ^= 0x10                                    # one flipped byte in block 5
    bad = Source(ctx, good.x, 16, S, 0, data=torch.from_numpy(np.frombuffer(bytes(hurt), dtype=np.uint8).copy()).cuda())
    assert bad.index.failure()[:2] == (5, CORRUPTION)
    room = 1 << 16
    buf = torch.full((16 * room,), SENTINEL, dtype=torch.uint8, device="cuda")
    at = lambda k: buf.data_ptr() + k * room + 64
    cut = lambda s, lo, n: (s.t, s.index.h, lo, n)
    need = len(expected(oracle, [(good, 100, 3500)])[0])
    outputs = [
        ([cut(bad, 0, 4 * S)], at(0), room - 64, OK),                       # blocks 0 - 3 of the damaged stream
        ([cut(bad, 4 * S, 2 * S + 100)], at(1), room - 64, CORRUPTION),     # touches block 6: the index's code
        ([cut(good, 100, 3500)], at(2), room - 64, OK),
        ([cut(bad, 6 * S, S)], at(3), room - 64, CORRUPTION),               # damage before the cut counts, as in DecodeStreamDevice
        ([cut(good, 100, 3500)], at(4), need - 1, INSUFFICIENT_BUFFER),
        ([cut(good, 100, 3500)], at(5), need, OK),
        ([cut(good, 0, S)], None, room, INVALID_ARGUMENT),                  # NULL d_out
        ([cut(good, 0, S)], at(7) + 2, room - 64, INVALID_ARGUMENT),        # misaligned d_out
        ([], at(8), room - 64, INVALID_ARGUMENT),                           # no cuts
        (None, at(8), room - 64, INVALID_ARGUMENT),                         # NULL cuts with a count
        ([cut(good, 5, 0), cut(good, 9, 0)], at(8), room - 64, INVALID_ARGUMENT),           # 0 samples in all
        ([cut(good, 8 * S - 10, 11)], at(8), room - 64, INVALID_ARGUMENT),  # beyond num_samples
        ([cut(good, 0, S), cut(other, 0, S)], at(8), room - 64, INVALID_ARGUMENT),          # presets differ
        ([cut(good, 0, S), cut(mono, 0, S)], at(8), room - 64, INVALID_ARGUMENT),           # channels differ
        ([(good.t, None, 0, S)], at(8), room - 64, INVALID_ARGUMENT),       # NULL index
        ([(None, good.index.h, 0, S)], at(8), room - 64, INVALID_ARGUMENT),                 # NULL d_stream
        ([cut(good, S - 20, S + 20)], at(8), room - 64, INVALID_ARGUMENT),  # an edge block outside the contract
        ([cut(good, 0, 2 * S)], at(9), room - 64, OK),
    ]
    ret, msg, arr = raw_call(ctx, [o[:3] for o in outputs])
    assert [arr[k].result for k in range(len(outputs))] == [o[3] for o in outputs]
    assert ret == CORRUPTION and msg.startswith("splice 1: ")
    assert [arr[k].out_bytes for k in range(len(outputs)) if outputs[k][3] not in (OK, INSUFFICIENT_BUFFER)] == [0] * 13
    assert arr[4].out_bytes == need and arr[5].out_bytes == need
    host = buf.cpu().numpy()
    image = np.full(host.size, SENTINEL, dtype=np.uint8)
    for k, cuts in ((0, [(bad, 0, 4 * S)]), (2, [(good, 100, 3500)]), (5, [(good, 100, 3500)]), (17, [(good, 0, 2 * S)])):
        want = expected(oracle, cuts)[0]
        lo = outputs[k][1] - buf.data_ptr()
        image[lo:lo + len(want)] = np.frombuffer(want, dtype=np.uint8)
        assert arr[k].out_bytes == len(want)
    assert np.array_equal(host, image)                                      # the good ones whole, nothing else touched
    # more than 2^32 - 1 samples in all: the whole stream 600000 times
    many = np.zeros((600000, 4), dtype=np.uint64)
    many[:] = (good.index.h, good.t.data_ptr(), 0, 8 * S)
    assert 600000 * 8 * S > 2 ** 32 - 1 and many.nbytes == 600000 * C.sizeof(linne_amd.Cut)
    one = (linne_amd.Splice * 1)()
    one[0].cuts, one[0].num_cuts, one[0].d_out, one[0].capacity = C.cast(many.ctypes.data, C.POINTER(linne_amd.Cut)), 600000, at(10), room - 64
    assert linne_amd.lib.LINNEAmd_SpliceStreamsDevice(ctx.h, one, 1, 0) == INVALID_ARGUMENT and one[0].result == INVALID_ARGUMENT
    assert "2^32" in linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode()
    # the whole-call argument errors
    assert linne_amd.lib.LINNEAmd_SpliceStreamsDevice(ctx.h, None, 1, 0) == INVALID_ARGUMENT
    assert linne_amd.lib.LINNEAmd_SpliceStreamsDevice(ctx.h, None, 0, 0) == OK
    assert np.array_equal(buf.cpu().numpy(), image)


def test_one_call_equals_many_calls(oracle):
    S = 1024
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        srcs = [Source(c, music(2, 8 * S, 16, seed=60 + i), 16, S, 7) for i in range(4)]
        outputs = [[(srcs[k % 4], S // 2, 5 * S)] for k in range(64)]                      # one shape, the same edge lengths everywhere
        spl = lambda which: [[(s.t, s.index, lo, n) for s, lo, n in outputs[k]] for k in which]
        c.splice_streams(spl(range(64)))                                   # warm: the scratch has grown
        c.enable_timing(True)
        census = []
        for which in ([7], list(range(64))):
            got = c.splice_streams(spl(which))
            census.append(({k: c.last_launches(k) for k in STREAM_KINDS}, c.last_splice_count(5)))
            assert c.last_ms(0) > 0
        c.enable_timing(False)
        assert census[0] == census[1], census
        assert census[0][1] == 1 and census[0][0][71] == 1 and census[0][0][72] == 1
        singles = [as_bytes(c.splice_streams(spl([k]))[0]) for k in range(64)]
        assert [as_bytes(t) for t in got] == singles
        for k in (0, 63):
            assert singles[k] == expected(oracle, outputs[k])[0]
    finally:
        c.close()


def test_edge_blocks_follow_the_contexts_af_iterations(oracle):
    S = 1024
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        src = Source(c, music(2, 4 * S, 16, seed=70), 16, S, 7)             # (encoded without -a)
        cuts = [(src, S // 2, 2 * S + 200)]
        plain = as_bytes(c.splice_streams([[(src.t, src.index, S // 2, 2 * S + 200)]])[0])
        c.set_af_iterations(1)
        got = as_bytes(c.splice_streams([[(src.t, src.index, S // 2, 2 * S + 200)]])[0])
        c.set_af_iterations(0)
        assert got == expected(oracle, cuts, af_iters=1)[0] and plain == expected(oracle, cuts)[0] and got != plain
    finally:
        c.close()
