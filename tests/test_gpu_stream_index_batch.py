"""GPU tests of the block indexes of resident .lnn streams, many in one call (Context.index_streams; include/linne_amd.h
LINNEAmd_StreamIndexesCreate) or one (Context.index_stream, LINNEAmd_StreamIndexCreate: the same code on one stream).  The yardsticks:
index_cases.index_walk, a serial walk of the stream's bytes in plain Python that shares nothing with the device code and is itself
held to LINNEDecoder_DecodeWhole (tests/test_stream_index_walk_cpu.py) -- code, header, num_blocks, the blocks() tables, failure() of
both calls; the stream indexed alone on a private copy, which company in a call must not change; the walk blocks(stream) for
well-formed streams; and LINNEDecoder_DecodeWhole, whose code and PCM a whole decode and two inner ranges through the indexes must
give."""
import numpy as np
import pytest

import linne_amd
from index_cases import SILENT_BLOCKS, build_corpus, index_walk
from stream_consumers import to_device
from stream_refs import blocks, mixed_signal
from test_gpu_stream_windows import SHAPES

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, INVALID_FORMAT, INSUFFICIENT_DATA, CORRUPTION, NG = 0, 1, 2, 4, 6, 7
INDEX_KINDS = tuple(range(37, 45)) + (69, 70)


def index_facts(ix):
    """everything the accessors tell of an index"""
    return (dict(ix.header), ix.num_blocks, ix.nbytes, tuple(a.tolist() for a in ix.blocks()), ix.failure())


@pytest.fixture(scope="module")
def corpus(ctx, product):
    """the cases with their yardsticks: .walk = index_walk's answer, .alone = (code, facts of index_stream on a private copy),
    .whole = DecodeWhole's (code, PCM)"""
    cases = build_corpus(product)
    for c in cases:
        if c.data is None:
            c.walk, c.alone, c.whole, c.dev = None, (INVALID_ARGUMENT, None), None, None
            continue
        c.walk = index_walk(c.data)
        c.dev = to_device(c.data)
        try:
            ix = ctx.index_stream(to_device(c.data))
            c.alone = (OK, index_facts(ix))
            ix.close()
        except linne_amd.LinneAmdError as e:
            c.alone = (e.code, None)
        if c.alone[0] == OK:
            ret, pcm = product.decode_whole(c.data)
            c.whole = (ret, np.ascontiguousarray(pcm, dtype=np.int32))
        else:
            c.whole = None
    cases[-1].dev = cases[0].dev                                  # the same device bytes named twice
    return cases


def compare(ctx, cases, streams):
    """index_streams over `streams` (the cases' bytes on the device, in their order) against the three yardsticks"""
    got, codes = ctx.index_streams(streams, return_codes=True)
    assert len(got) == len(cases) and codes == [c.alone[0] for c in cases]
    wins, want = [], []
    for c, ix, dev in zip(cases, got, streams):
        if c.alone[0] != OK:
            assert ix is None, c.name
            continue
        assert index_facts(ix) == c.alone[1], c.name
        if c.well_formed:
            off, first, size, typ, nsmp = ix.blocks()
            walk = blocks(c.data)
            assert [(int(o), int(s) + 6, int(t), int(n), int(f)) for o, s, t, n, f in zip(off, size, typ, nsmp, first)] == walk, c.name
            assert ix.failure() == (-1, OK, 0), c.name
        ret, pcm = c.whole
        ns = ix.header["num_samples"]
        spans = [(0, ns)] + ([(ns // 3, ns // 5), (ns - ns // 7 - 1, ns // 7)] if ret == OK else [])
        for a, n in spans:
            wins.append((dev, ix, a, n))
            want.append((c, ret, pcm[:, a:a + n]))
    pcm, wcodes = ctx.decode_windows(wins, return_codes=True)
    for (c, ret, samples), g, code in zip(want, pcm, wcodes):
        assert code == ret, c.name
        if ret == OK:
            assert np.array_equal(g.cpu().numpy(), samples), c.name
    for ix in got:
        if ix is not None:
            ix.close()
    return codes


def walk_facts(c):
    """index_facts as index_walk gives them"""
    code, header, nb, tables, failure = c.walk
    return (header, nb, len(c.data), tuple(tables), failure)


def test_both_calls_equal_the_walk(ctx, corpus):
    """for every case, index_stream and index_streams give what the serial walk of the bytes gives: the code, and where an index is
    built its header, num_blocks, tables and failure triple"""
    cases = [c for c in corpus if c.data is not None]
    built, codes = ctx.index_streams([c.dev for c in cases], return_codes=True)
    for c, ix, code in zip(cases, built, codes):
        assert code == c.walk[0], c.name
        assert (ix is None) == (code != OK), c.name
        try:
            one, one_code = ctx.index_stream(to_device(c.data)), OK
        except linne_amd.LinneAmdError as e:
            one, one_code = None, e.code
        assert one_code == c.walk[0], c.name
        if code != OK:
            continue
        assert index_facts(ix) == walk_facts(c), c.name
        assert index_facts(one) == walk_facts(c), c.name
        ix.close()
        one.close()
    assert sum(1 for c in cases if c.walk[0] == OK and c.walk[4][0] >= 0) >= 20      # damaged streams that still have an index
    assert sum(1 for c in cases if c.walk[0] == OK and c.walk[2] == 0) >= 12         # ... and streams without a block


def test_single_call_text_is_the_stream_text(ctx, corpus):
    """raw calls: a header the single call refuses gives NULL, the code and the text it always gave; the batch call on that one
    stream gives the code and "stream 0: " before the same text.  A NULL stream is the single call's INVALID_ARGUMENT, a NULL result
    pointer is tolerated"""
    import ctypes as C
    lib = linne_amd.lib
    by = {c.name: c for c in corpus}
    want = {"fewer than 30 bytes": (INSUFFICIENT_DATA, "stream header: LINNEDecoder_DecodeHeader -> 4"),
            "bad signature": (INVALID_FORMAT, "stream header: LINNEDecoder_DecodeHeader -> 2"),
            "bad format version": (INVALID_FORMAT, "stream header: LINNEDecoder_SetHeader -> 2"),
            "the rest of that block head (no signature)": (INVALID_FORMAT, "stream header: LINNEDecoder_DecodeHeader -> 2")}
    for name, (code, text) in want.items():
        dev = by[name].dev
        res = C.c_int(-5)
        h = lib.LINNEAmd_StreamIndexCreate(ctx.h, C.c_void_p(dev.data_ptr()), dev.numel(), C.byref(res))
        assert not h and res.value == code, name
        assert lib.LINNEAmd_GetLastError(ctx.h).decode() == text, name
        assert not lib.LINNEAmd_StreamIndexCreate(ctx.h, C.c_void_p(dev.data_ptr()), dev.numel(), None), name      # NULL result: tolerated
        ptrs, sizes = (C.c_void_p * 1)(dev.data_ptr()), (C.c_uint64 * 1)(dev.numel())
        handles, codes = (C.c_void_p * 1)(0x77), (C.c_int32 * 1)(-5)
        assert lib.LINNEAmd_StreamIndexesCreate(ctx.h, ptrs, sizes, 1, handles, codes) == code, name
        assert not handles[0] and codes[0] == code, name
        assert lib.LINNEAmd_GetLastError(ctx.h).decode() == "stream 0: " + text, name
    good = by["1000 silent blocks"].dev
    res = C.c_int(-5)
    assert not lib.LINNEAmd_StreamIndexCreate(ctx.h, None, good.numel(), C.byref(res)) and res.value == INVALID_ARGUMENT
    assert not lib.LINNEAmd_StreamIndexCreate(ctx.h, None, good.numel(), None)
    assert not lib.LINNEAmd_StreamIndexCreate(None, C.c_void_p(good.data_ptr()), good.numel(), C.byref(res)) and res.value == INVALID_ARGUMENT
    h = lib.LINNEAmd_StreamIndexCreate(ctx.h, C.c_void_p(good.data_ptr()), good.numel(), None)                      # NULL result, a sound stream
    assert h and lib.LINNEAmd_StreamIndexNumBlocks(h) == SILENT_BLOCKS
    lib.LINNEAmd_StreamIndexDestroy(h)


def test_a_single_call_is_a_one_stream_call(corpus):
    """scratch grown and timing on: the single call on the silent stream counts as a call of one stream, and launches what
    index_streams([that stream]) launches"""
    silent = next(c for c in corpus if c.name == "1000 silent blocks")
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        c.enable_timing(True)
        c.index_streams([silent.dev])[0].close()                  # (grows the context's scratch)
        ix = c.index_streams([silent.dev])[0]
        batch = {k: c.last_launches(k) for k in INDEX_KINDS}
        assert [c.last_index_batch_count(w) for w in range(5)] == [1, 1, 10, 4, 1]
        facts = index_facts(ix)
        ix.close()
        ix = c.index_stream(silent.dev)
        assert [c.last_index_batch_count(w) for w in range(5)] == [1, 1, 10, 4, 1]
        assert {k: c.last_launches(k) for k in INDEX_KINDS} == batch and all(v >= 1 for v in batch.values()), batch
        assert c.last_ms(0) > 0
        assert index_facts(ix) == facts == walk_facts(silent)
        ix.close()
    finally:
        c.close()


def test_corpus_is_what_it_says(corpus):
    by = {c.name: c for c in corpus}
    assert len(corpus) >= 45
    assert by["fewer than 30 bytes"].alone[0] == INSUFFICIENT_DATA
    assert by["bad signature"].alone[0] == INVALID_FORMAT and by["bad format version"].alone[0] == INVALID_FORMAT
    assert by["the rest of that block head (no signature)"].alone[0] == INVALID_FORMAT
    for name in ("first", "middle", "last"):
        block, code, _ = by[f"CRC damage in the {name} block"].alone[1][4]
        assert code == CORRUPTION and block >= 0
    # the chain breaks: both outcomes at the place behind it
    mid = by["size field beyond the stream"].alone[1]
    assert mid[4][:2] == (mid[1], INSUFFICIENT_DATA)
    low = by["size field below 5"].alone[1]
    assert low[4][:2] == (low[1], INVALID_FORMAT)
    assert by["sync word damaged"].alone[1][4][1] == INVALID_FORMAT
    assert by["size field one less"].alone[1][4][1] == CORRUPTION
    assert by["false candidate in a RAW payload"].whole[0] == OK and by["false candidate in a RAW payload"].alone[1][4][0] == -1
    assert by["1000 silent blocks"].alone[1][1] == SILENT_BLOCKS
    assert sum(1 for c in corpus if c.well_formed) >= 9


def test_equal_to_the_single_call_in_both_orders(ctx, corpus):
    codes = compare(ctx, corpus, [c.dev for c in corpus])
    assert ctx.last_index_batch_count(0) == len(corpus)
    assert ctx.last_index_batch_count(1) == sum(1 for c in codes if c == OK)
    assert ctx.last_index_batch_count(2) == 10                  # 2^10 > 1000 candidates: the silent stream sets K
    back = corpus[::-1]
    compare(ctx, back, [c.dev for c in back])
    # without return_codes the first failing stream raises, with every stream's code
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.index_streams([c.dev for c in corpus])
    first = next(i for i, c in enumerate(corpus) if c.alone[0] != OK)
    assert e.value.code == corpus[first].alone[0] and e.value.codes == [c.alone[0] for c in corpus]
    assert f"stream {first}: stream header: " in str(e.value)
    with pytest.raises(linne_amd.LinneAmdError) as alone:
        ctx.index_stream(corpus[first].dev)
    assert str(e.value).endswith(f"stream {first}: " + str(alone.value).split(": ", 1)[1])
    assert ctx.index_streams([]) == [] and ctx.index_streams([], return_codes=True) == ([], [])


def test_call_level_arguments(ctx, corpus):
    """NULL arrays with a positive count are INVALID_ARGUMENT and touch nothing; no streams is OK whatever the arrays are"""
    import ctypes as C
    f = linne_amd.lib.LINNEAmd_StreamIndexesCreate
    dev = corpus[0].dev
    ptrs, sizes = (C.c_void_p * 2)(dev.data_ptr(), dev.data_ptr()), (C.c_uint64 * 2)(dev.numel(), dev.numel())
    handles, res = (C.c_void_p * 2)(0x77, 0x77), (C.c_int32 * 2)(-5, -5)
    for args in [(None, sizes, handles, res), (ptrs, None, handles, res), (ptrs, sizes, None, res), (ptrs, sizes, handles, None)]:
        assert f(ctx.h, args[0], args[1], 2, args[2], args[3]) == INVALID_ARGUMENT
    assert f(ctx.h, None, None, 0, None, None) == OK
    assert f(ctx.h, ptrs, sizes, 0, handles, res) == OK
    assert [handles[i] for i in range(2)] == [0x77, 0x77] and [res[i] for i in range(2)] == [-5, -5]       # untouched
    assert [ctx.last_index_batch_count(w) for w in range(5)] == [0] * 5
    assert ctx.last_index_batch_count(5) == -1 and ctx.last_index_batch_count(-1) == -1
    # a call whose every stream fails on its own is no whole-call failure: the codes come back
    got, codes = ctx.index_streams([None, corpus[0].dev[:29]], return_codes=True)
    assert got == [None, None] and codes == [INVALID_ARGUMENT, INSUFFICIENT_DATA]


def test_adjacent_views_of_one_buffer(ctx, corpus):
    """the corpus back to back in one buffer from byte 1 on, nothing between the streams: no read of a stream leaves its bytes"""
    import torch
    cases = [c for c in corpus if c.data is not None]
    total = sum(len(c.data) for c in cases)
    flat = torch.zeros(total + 2, dtype=torch.uint8, device="cuda")
    views, starts, at = [], [], 1
    for c in cases:
        flat[at:at + len(c.data)] = c.dev
        views.append(flat[at:at + len(c.data)])
        starts.append(at)
        at += len(c.data)
    assert sum(1 for v in views if v.data_ptr() % 2) >= 10 and len({v.data_ptr() % 16 for v in views}) >= 8
    k = next(i for i, c in enumerate(cases) if c.name == "silent cut inside a block head")
    assert bytes(flat[starts[k + 1] - 5:starts[k + 1] + 1].cpu().numpy()) == b"\xff\xff\x00\x00\x00\x05"
    compare(ctx, cases, views)


def test_counts_do_not_depend_on_the_number_of_streams(corpus):
    three = [corpus[1], corpus[6], corpus[3]]                     # two shapes and the silent stream
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        c.enable_timing(True)
        census = []
        for rep in (16, 1, 16):                                  # (the first call grows the context's scratch: two more allocations)
            cases = three * rep
            built, codes = c.index_streams([x.dev for x in cases], return_codes=True)
            assert codes == [OK] * len(cases)
            launches = {k: c.last_launches(k) for k in INDEX_KINDS}
            counts = [c.last_index_batch_count(w) for w in range(5)]
            assert c.last_ms(0) > 0
            for ix, x in zip(built, cases):
                assert index_facts(ix) == x.alone[1]
                ix.close()
            census.append((launches, counts))
        (l1, n1), (l16, n16) = census[1], census[2]
        assert l1 == l16 and all(v >= 1 for v in l1.values()), census
        assert l1[41] == n1[2] - 1 and n1[2] == 10
        assert n1[2:] == n16[2:] and (n1[0], n16[0]) == (3, 48) and (n1[1], n16[1]) == (3, 48)
        assert n1[3] == 4 and n1[4] == 1
    finally:
        c.close()


def test_lifetime_and_mixing_with_single_built_indexes(ctx, corpus):
    good = [c for c in corpus if c.well_formed]
    built = ctx.index_streams([c.dev for c in good])
    for ix in built[::2]:
        ix.close()
    single = {i: ctx.index_stream(good[i].dev) for i in range(0, len(good), 2)}
    wins, want = [], []
    for i, c in enumerate(good):
        ix = built[i] if i % 2 else single[i]
        ns = ix.header["num_samples"]
        for a, n in ((0, ns), (ns // 4, ns // 2)):
            wins.append((c.dev, ix, a, n))
            want.append(c.whole[1][:, a:a + n])
    for g, w in zip(ctx.decode_windows(wins), want):
        assert np.array_equal(g.cpu().numpy(), w)
    for ix in built[::-1] + list(single.values()):                # odd ones now, in reverse; closing twice is harmless
        ix.close()


def test_answers_do_not_depend_on_the_contexts_history(corpus):
    import torch
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        compare(c, corpus, [x.dev for x in corpus])
        tracks = []
        for k in (1, 5, 0):
            nch, bits, block, preset, ms, _, seed = SHAPES[k]
            x = mixed_signal(nch, bits, 7 * block + 500, seed=seed + 40, block=block)
            tracks.append((x, bits, block, preset, ms))
        streams = c.encode_streams([(torch.from_numpy(x).cuda(), bits, 44100, block, preset, ms) for x, bits, block, preset, ms in tracks])
        # encode_streams' outputs (views of one allocation) straight into index_streams
        built = c.index_streams(streams)
        for ix, s, (x, bits, block, preset, ms) in zip(built, streams, tracks):
            alone = c.index_stream(s.clone())
            assert index_facts(ix) == index_facts(alone)
            alone.close()
        pcm = c.decode_windows([(s, ix, 0, None) for s, ix in zip(streams, built)])
        for g, (x, *_) in zip(pcm, tracks):
            assert np.array_equal(g.cpu().numpy(), x)
        for ix in built:
            ix.close()
        compare(c, corpus, [x.dev for x in corpus])
    finally:
        c.close()
