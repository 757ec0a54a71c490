"""GPU tests of decoding many sample windows of resident .lnn streams in one call (Context.decode_windows; include/linne_amd.h
LINNEAmd_DecodeWindowsDevice): every window's PCM and code against the slice of LINNEDecoder_DecodeWhole's output and against
Context.decode_stream on that window alone -- mixed shapes, passes (group_frames), overlap, damaged streams whose failure must stay
in its window, bad arguments per window, the launch count, and the plumbing of torch tensors and streams.  Every window of every
test is compared."""
import numpy as np
import pytest

import linne_amd
from stream_consumers import crc_damaged, to_device
from stream_refs import blocks, crc16, mixed_signal

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CORRUPTION, NG = 0, 1, 6, 7
COMPRESS, SILENT, RAW = 0, 1, 2
NEW_KINDS = (56, 57, 58, 59)


class Track:
    def __init__(self, ctx, product, stream, name):
        self.name, self.stream = name, stream
        ret, self.full = product.decode_whole(stream)
        assert ret == OK, name
        self.full = np.ascontiguousarray(self.full, dtype=np.int32)
        self.ns = self.full.shape[1]
        self.bl = blocks(stream)
        self.dev = to_device(stream)
        self.index = ctx.index_stream(self.dev)

    def win(self, first, n):
        return (self.dev, self.index, first, n)


SHAPES = [  # nch, bits, block, preset, ms, ns, seed
    (1, 16, 4096, 0, False, 50000, 1),
    (2, 16, 4096, 5, True, 60000, 2),
    (2, 16, 4096, 5, True, 70001, 3),       # the shape of the one before
    (3, 24, 2048, 3, False, 30000, 4),
    (8, 16, 2048, 5, True, 20000, 5),
    (2, 8, 1023, 2, False, 30000, 6),
    (2, 24, 10240, 7, True, 100000, 7),
]


@pytest.fixture(scope="module")
def corpus(ctx, product):
    from test_gpu_parity import many_block_lengths, stream_of_blocks
    tracks = []
    for nch, bits, block, preset, ms, ns, seed in SHAPES:
        x = mixed_signal(nch, bits, ns, seed=seed, block=block)
        t = Track(ctx, product, product.encode_whole(x, bits, 44100, block, preset, ms), f"{nch}ch {bits}b {block} -m{preset}")
        assert np.array_equal(t.full, x)
        tracks.append(t)
    # the variable-block-length stream (48 distinct lengths); two of its blocks silent and two of full-scale noise, so that it too
    # holds all three block types
    x, lens = many_block_lengths()
    x = np.array(x, dtype=np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)])
    x[:, starts[5]:starts[7]] = 0
    x[:, starts[10]:starts[12]] = np.random.default_rng(9).integers(-32768, 32768, size=(2, int(starts[12] - starts[10])))
    t = Track(ctx, product, stream_of_blocks(product, x, 16, 44100, 4096, 7, True, lens), "variable block lengths")
    assert np.array_equal(t.full, x) and len({b[3] for b in t.bl}) >= 40
    tracks.append(t)
    for t in tracks:
        assert {COMPRESS, SILENT, RAW} <= {b[2] for b in t.bl}, t.name
    assert len(tracks) >= 6
    yield tracks
    for t in tracks:
        t.index.close()


def batch_of(tracks):
    """[(track, first, n)]: per stream the edge cases, then 200 seeded random windows over all streams"""
    cases = []
    for t in tracks:
        ns, bl = t.ns, t.bl
        cases += [(t, 0, 1), (t, ns - 1, 1), (t, 0, ns), (t, ns, 0), (t, 17, 0)]
        for off, size, typ, n, first in bl[1:6]:
            cases.append((t, first - 7, 20))                     # straddling a boundary
        for typ_want in (SILENT, RAW):
            b = next(b for b in bl if b[2] == typ_want)
            cases.append((t, b[4] + 5, b[3] - 10))               # inside the block
            cases.append((t, b[4] - 3, b[3] + 6))                # and across both its ends
    rng = np.random.default_rng(2026)
    for _ in range(200):
        t = tracks[int(rng.integers(0, len(tracks)))]
        a = int(rng.integers(0, t.ns))
        cases.append((t, a, int(rng.integers(1, min(t.ns - a, 30000) + 1))))
    return cases


def check(cases, got):
    assert len(got) == len(cases)
    for i, ((t, a, n), g) in enumerate(zip(cases, got)):
        assert tuple(g.shape) == (t.full.shape[0], n), (i, t.name, a, n)
        assert np.array_equal(g.cpu().numpy(), t.full[:, a:a + n]), (i, t.name, a, n)


def test_equal_to_the_single_call_mixed_corpus(ctx, corpus):
    import torch
    cases = batch_of(corpus)
    assert len(cases) >= 200 + 14 * len(corpus)
    got = ctx.decode_windows([t.win(a, n) for t, a, n in cases])
    check(cases, got)
    assert len({g.untyped_storage().data_ptr() for g in got}) == 1          # views of one allocation
    # None: to the end of the stream
    t = corpus[1]
    tail = ctx.decode_windows([(t.dev, t.index, t.ns - 777, None), (t.dev, t.index, 0, None)])
    assert np.array_equal(tail[0].cpu().numpy(), t.full[:, t.ns - 777:]) and np.array_equal(tail[1].cpu().numpy(), t.full)
    # against decode_stream on the window alone: every 7th window, at least 30
    sub = cases[::7]
    assert len(sub) >= 30
    for (t, a, n), g in zip(sub, got[::7]):
        alone = ctx.decode_stream(t.dev, a, n, index=t.index)
        assert torch.equal(alone, g), (t.name, a, n)
    # the out= form: windows of one size over the two streams that share a shape, as many as that subset
    rng = np.random.default_rng(5)
    n = 5000
    same = []
    for k in range(len(sub)):
        t = corpus[1 + (k & 1)]
        same.append((t, int(rng.integers(0, t.ns - n)), n))
    out = torch.full((len(same), 2, n), -99, dtype=torch.int32, device="cuda")
    back = ctx.decode_windows([t.win(a, m) for t, a, m in same], out=out)
    assert back is out
    check(same, list(out))
    # a (W, C, n) view whose rows are wider than n
    wide = torch.full((len(same), 2, n + 13), -99, dtype=torch.int32, device="cuda")
    ctx.decode_windows([t.win(a, m) for t, a, m in same], out=wide[:, :, 5:5 + n])
    check(same, list(wide[:, :, 5:5 + n]))
    assert bool((wide[:, :, :5] == -99).all()) and bool((wide[:, :, 5 + n:] == -99).all())


@pytest.mark.parametrize("group_frames", [1, 7, 64])
def test_passes_give_the_same_tensors(ctx, corpus, group_frames):
    import torch
    cases = batch_of(corpus)
    wins = [t.win(a, n) for t, a, n in cases]
    base = ctx.decode_windows(wins)
    got = ctx.decode_windows(wins, group_frames=group_frames)
    assert len(got) == len(base)
    for i, (b, g) in enumerate(zip(base, got)):
        assert torch.equal(b, g), (group_frames, i)
    check(cases, got)


def test_throughput_synthesis(ctx, corpus):
    """one shape, at least 1536 COMPRESS channel-frames in the batch: the synthesis takes its throughput form"""
    a, b = corpus[1], corpus[2]
    cases = []
    for k in range(45):
        cases += [(a, 3 * k, a.ns - 5 * k), (b, 2 * k, b.ns - 2 * k)]
    count = 0
    for t, first, n in cases:
        count += sum(1 for blk in t.bl if blk[2] == COMPRESS and blk[4] < first + n and blk[4] + blk[3] > first)
    assert count * 2 >= 1536, count
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        c.enable_timing(True)
        got = c.decode_windows([t.win(first, n) for t, first, n in cases])
        assert c.last_launches(32) == 0 and c.last_launches(33) >= 1          # not the pipelined latency form: the rows form
    finally:
        c.close()
    check(cases, got)


def test_overlap_and_repetition(ctx, corpus):
    t = corpus[1]
    cases = [(t, 10000, 9000)] * 50 + [(t, 20000 + k, 9000) for k in range(50)]
    check(cases, ctx.decode_windows([t.win(a, n) for t, a, n in cases]))


def codes_alone(ctx, wins):
    out = []
    for dev, index, a, n in wins:
        try:
            ctx.decode_stream(dev, a, n, index=index)
            out.append(OK)
        except linne_amd.LinneAmdError as e:
            out.append(e.code)
    return out


def test_damage_stays_in_its_window(ctx, corpus):
    import torch
    t, u, v = corpus[1], corpus[2], corpus[6]                    # all stereo
    bl = t.bl
    bad, k = crc_damaged(t)
    d_bad = to_device(bad)
    index = ctx.index_stream(d_bad)
    n = 900
    before, after = bl[k - 2], bl[k + 1]
    wins = [(d_bad, index, before[4] + 1, n), (d_bad, index, bl[k][4] + 3, n), (d_bad, index, after[4], n), u.win(4321, n), v.win(12345, n)]
    want = [t.full[:, before[4] + 1:before[4] + 1 + n], None, None, u.full[:, 4321:4321 + n], v.full[:, 12345:12345 + n]]
    for gf in (0, 1):
        out = torch.full((5, 2, n), -7777, dtype=torch.int32, device="cuda")
        back, codes = ctx.decode_windows(wins, out=out, group_frames=gf, return_codes=True)
        assert codes == [OK, CORRUPTION, CORRUPTION, OK, OK]
        assert codes == codes_alone(ctx, wins)
        for i in range(5):
            if want[i] is None:
                assert bool((out[i] == -7777).all()), i
            else:
                assert np.array_equal(out[i].cpu().numpy(), want[i]), i
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.decode_windows(wins)
    assert e.value.code == CORRUPTION and e.value.codes == [OK, CORRUPTION, CORRUPTION, OK, OK]
    assert "window 1:" in str(e.value) and f"block {k} " in str(e.value)
    index.close()


@pytest.fixture(scope="module")
def rice_damaged(ctx, product, corpus):
    """corpus[1] with a payload bit of COMPRESS block k flipped and the CRC16 made right again, such that DecodeWhole fails on it:
    (the stream on the device, its index, k, DecodeWhole's code)"""
    t = corpus[1]
    bl = t.bl
    k = max(i for i, b in enumerate(bl[:-1]) if b[2] == COMPRESS and bl[i - 1][2] == COMPRESS)
    off, size = bl[k][:2]
    rng = np.random.default_rng(77)
    found = None
    for _ in range(64):
        bad = bytearray(t.stream)
        p = off + 11 + (size - 11) // 2 + int(rng.integers(0, (size - 11) // 2))       # the later half of the payload: Rice codes
        bad[p] ^= 1 << int(rng.integers(0, 8))
        bad[off + 6:off + 8] = crc16(bad[off + 8:off + size]).to_bytes(2, "big")
        bad = bytes(bad)
        ret, _ = product.decode_whole(bad)
        if ret == OK:
            continue
        d_bad = to_device(bad)
        found = (d_bad, ctx.index_stream(d_bad), k, ret)
        break
    assert found is not None, "no flip in 64 made DecodeWhole fail"
    yield found
    found[1].close()


def test_the_consumption_check(ctx, corpus, rice_damaged):
    """a payload bit of a COMPRESS block flipped and the CRC16 made right again: the index finds nothing, the Rice decoder does"""
    import torch
    t, u = corpus[1], corpus[6]
    bl = t.bl
    d_bad, index, k, whole = rice_damaged
    assert whole != OK                                           # DecodeWhole's verdict on that stream
    n = 700
    wins = [(d_bad, index, bl[k][4] + 10, n), (d_bad, index, bl[k - 1][4] + 10, n), u.win(999, n), (d_bad, index, bl[k + 1][4], 50)]
    alone = codes_alone(ctx, wins)
    assert alone[0] == NG and alone[1:] == [OK, OK, OK]
    for gf in (0, 1):
        arr = torch.full((3, 2, n), -4242, dtype=torch.int32, device="cuda")
        back, codes = ctx.decode_windows(wins[:3], out=arr, group_frames=gf, return_codes=True)
        assert codes == alone[:3]
        assert bool((arr[0] == -4242).all())                     # untouched
        a1 = bl[k - 1][4] + 10
        assert np.array_equal(arr[1].cpu().numpy(), t.full[:, a1:a1 + n]) and np.array_equal(arr[2].cpu().numpy(), u.full[:, 999:999 + n])
    # a window wider than one pass over the damaged block and its neighbours: nothing of it is written either
    a0, a1 = bl[k - 1][4], bl[k + 1][4] + 50
    arr = torch.full((2, 2, a1 - a0), -4242, dtype=torch.int32, device="cuda")
    back, codes = ctx.decode_windows([(d_bad, index, a0, a1 - a0), t.win(a0, a1 - a0)], out=arr, group_frames=1, return_codes=True)
    assert codes == [alone[0], OK]
    assert bool((arr[0] == -4242).all()) and np.array_equal(arr[1].cpu().numpy(), t.full[:, a0:a1])
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.decode_windows(wins)
    assert e.value.code == alone[0] and e.value.codes == alone and "window 0:" in str(e.value)


def test_single_call_text_is_the_windows_text(ctx, corpus, rice_damaged):
    """one window of each kind of failure -- the index's, the consumption check's, an argument's: decode_windows reads "window 0: "
    and then exactly what decode_stream reads for that window.  The index's text is also held to what the separate single-call path
    gave before both calls shared one implementation, recorded from that build"""
    t = corpus[1]
    bad, kc = crc_damaged(t)
    d_crc = to_device(bad)
    crc_index = ctx.index_stream(d_crc)
    d_rice, rice_index, kr, _ = rice_damaged
    texts = {}
    for name, win, code in [("crc", (d_crc, crc_index, t.bl[kc][4] + 3, 900), CORRUPTION),
                            ("rice", (d_rice, rice_index, t.bl[kr][4] + 10, 700), NG),
                            ("argument", t.win(t.ns, 1), INVALID_ARGUMENT)]:
        dev, index, a, n = win
        with pytest.raises(linne_amd.LinneAmdError) as single:
            ctx.decode_stream(dev, a, n, index=index)
        with pytest.raises(linne_amd.LinneAmdError) as batch:
            ctx.decode_windows([win])
        assert single.value.code == code and batch.value.code == code and batch.value.codes == [code], name
        head_single, head_batch = f"DecodeStreamDevice -> {code}: ", f"DecodeWindowsDevice -> {code}: "
        assert str(single.value).startswith(head_single) and str(batch.value).startswith(head_batch), name
        text = str(single.value)[len(head_single):]
        assert text and "window" not in text, (name, text)
        assert str(batch.value)[len(head_batch):] == "window 0: " + text, name
        texts[name] = text
    assert texts["crc"] == f"block {kc} (byte {t.bl[kc][0]} of the stream): damaged or truncated stream"
    assert texts["rice"].startswith(f"block {kr} (byte {t.bl[kr][0]} of the stream): ") and "no encoder writes" in texts["rice"]
    crc_index.close()


def test_bad_arguments_per_window(ctx, corpus):
    t, u = corpus[0], corpus[3]
    ns = t.ns
    wins = [t.win(100, 50), t.win(ns, 1), u.win(5, 60), t.win(ns - 5, 6), t.win(0, ns + 1), t.win(ns, 0), u.win(u.ns - 9, 9)]
    want = [OK, INVALID_ARGUMENT, OK, INVALID_ARGUMENT, INVALID_ARGUMENT, OK, OK]
    pcm, codes = ctx.decode_windows(wins, return_codes=True)
    assert codes == want and codes == codes_alone(ctx, wins)
    for (dev, index, a, n), c, g, tr in zip(wins, codes, pcm, [t, t, u, t, t, t, u]):
        if c == OK:
            assert np.array_equal(g.cpu().numpy(), tr.full[:, a:a + n]), (a, n)
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.decode_windows(wins)
    assert e.value.code == INVALID_ARGUMENT and e.value.codes == want and "window 1:" in str(e.value)


def test_no_per_window_launches(corpus):
    t = corpus[1]
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        c.enable_timing(True)
        rng = np.random.default_rng(3)
        counts = []
        for nw in (1, 200):
            cases = [(t, int(a), 9000) for a in rng.integers(0, t.ns - 9000, size=nw)]
            cases[0] = (t, 100, 9000)                            # music: COMPRESS blocks
            got = c.decode_windows([t.win(a, n) for t, a, n in cases], group_frames=0)
            counts.append({k: c.last_launches(k) for k in NEW_KINDS + (28,)})
            assert c.last_ms(0) > 0
            check(cases, got)
        assert counts[0] == counts[1] and all(v >= 1 for v in counts[0].values()), counts
    finally:
        c.close()


def test_stream_view_at_an_odd_address(ctx, corpus):
    import torch
    for t in (corpus[1], corpus[5]):
        for shift in (1, 3, 8):
            big = torch.zeros(len(t.stream) + 40, dtype=torch.uint8, device="cuda")
            big[shift:shift + len(t.stream)] = t.dev
            view = big[shift:shift + len(t.stream)]
            assert view.data_ptr() % 16 == shift
            cases = [(t, 0, t.ns), (t, 1000, 5000), (t, t.ns - 3000, 3000)]
            check(cases, ctx.decode_windows([(view, t.index, a, n) for t, a, n in cases]))


@pytest.mark.parametrize("use_torch_stream", [True, False])
def test_torch_stream_ordering(corpus, use_torch_stream):
    import torch
    t, u = corpus[1], corpus[2]
    c = linne_amd.Context(0, use_torch_stream=use_torch_stream)
    try:
        it, iu = c.index_stream(t.dev), c.index_stream(u.dev)
        spans = [(t, it, 2000, 30000), (u, iu, 500, 30000), (t, it, 20000, 30000)]
        want = sum(int(tr.full[:, a:a + n].astype(np.int64).sum()) for tr, _, a, n in spans)
        for _ in range(3):
            ins = {}
            for tr in (t, u):
                ins[id(tr)] = torch.empty_like(tr.dev)
                ins[id(tr)].copy_(tr.dev)                        # written by torch just before the call
            out = torch.empty((3, 2, 30000), dtype=torch.int32, device="cuda")
            c.decode_windows([(ins[id(tr)], ix, a, n) for tr, ix, a, n in spans], out=out)
            assert int(out.to(torch.int64).sum().item()) == want              # read by torch right after it
            for v in ins.values():
                v.zero_()
        it.close(); iu.close()
    finally:
        c.close()


def test_empty_window_list(ctx):
    assert ctx.decode_windows([]) == []
    assert ctx.decode_windows([], return_codes=True) == ([], [])
