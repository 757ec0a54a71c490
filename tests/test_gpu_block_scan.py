"""GPU tests of the block-head scan that Context.index_streams and Context.repair_streams share (include/linne_amd.h
LINNEAmd_StreamIndexesCreate, LINNEAmd_RepairStreamsDevice): on undamaged streams both calls see the same block chain, and one context
that takes the calls in turn, its buffers growing in between, answers as fresh contexts do.  tests/test_block_scan_cpu.py holds the
streams to what these tests need of them."""
import numpy as np
import pytest

import linne_amd
import repair_cases as rc
import scan_cases as sc

pytestmark = pytest.mark.gpu

OK = 0


def as_bytes(t):
    return bytes(t.cpu().numpy())


def facts(ix):
    return (dict(ix.header), ix.num_blocks, ix.nbytes, tuple(a.tolist() for a in ix.blocks()), ix.failure())


@pytest.fixture(scope="module")
def streams(oracle, product):
    return sc.undamaged_streams(oracle, product)


def test_index_and_repair_see_the_same_chain(ctx, product, streams):
    """every undamaged stream in one call of each kind: the blocks the repair call keeps are the blocks of the index -- their count,
    and the offsets, sizes, types and sample counts the repaired stream's own index names -- and the repaired stream is the input
    byte for byte.  The two stumps, a stream that ends before the first block's offset and one that ends at it: the header's code
    from both calls for the first; no block in the index and none kept for the second"""
    stumps = sc.stumps(product)
    data = [d for _, d in streams] + [d for _, d in stumps]
    dev = [ctx._stream_bytes(d) for d in data]
    built, icodes = ctx.index_streams(dev, return_codes=True)
    repaired, rcodes = ctx.repair_streams(dev, return_codes=True)
    again = ctx.index_streams([out for out, _ in repaired[:len(streams)]])
    for (name, d), ix, (out, report), back, icode, rcode in zip(streams, built, repaired, again, icodes, rcodes):
        assert icode == OK and rcode == OK and ix.failure() == (-1, OK, 0), name
        want = sc.blocks_of(d)
        assert [a.tolist() for a in ix.blocks()] == [list(w) for w in want], name
        assert report["kept_blocks"] == ix.num_blocks == len(want[0]) and report["fill_blocks"] == 0 and report["num_gaps"] == 0 and report["exact"] == 1, name
        assert facts(back) == facts(ix), name
        assert as_bytes(out) == d, name
    short, bare = len(streams), len(streams) + 1
    assert icodes[short] == rcodes[short] != OK and built[short] is None and repaired[short][0] is None, icodes
    assert icodes[bare] == OK and built[bare].num_blocks == 0 and rcodes[bare] == OK and repaired[bare][1]["kept_blocks"] == 0
    for ix in list(built) + list(again):
        if ix is not None:
            ix.close()


def test_calls_in_turn_on_one_context(oracle, streams):
    """index (one stream), repair (three, the largest of the table and damaged ones among them), index (five small ones), then windows
    on the indexes built: every answer is that of the same call on a fresh context, and the second index call, every buffer of
    which the repair call before it has sized, waits four times and allocates its tables and nothing else"""
    table = rc.build_cases(oracle)
    big = [table[n][0] for n in ("stereo/m0/ms/a", "stereo/m7/lr/j", "stereo/m7/ms/f")]
    small = [d for _, d in sorted(streams, key=lambda s: len(s[1]))[:5]]
    one = [dict(streams)["mono/m7/a"]]
    assert sum(len(d) for d in small) < min(len(d) for d in big)

    def index(c, data):
        got = c.index_streams([c._stream_bytes(d) for d in data])
        return got, [facts(ix) for ix in got], [c.last_index_batch_count(k) for k in range(5)]

    def repair(c, data):
        got, codes = c.repair_streams(data, return_codes=True)
        return [(as_bytes(out), report) for out, report in got], codes

    def windows(c, data, built):
        return [w.cpu().numpy() for w in c.decode_windows([(c._stream_bytes(d), ix, 0, ix.header["num_samples"]) for d, ix in zip(data, built)])]

    def fresh(call, *args):
        c = linne_amd.Context(0, use_torch_stream=False)
        try:
            return call(c, *args)
        finally:
            c.close()

    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        ix1, facts1, _ = index(c, one)
        rep = repair(c, big)
        ix5, facts5, census5 = index(c, small)
        pcm = windows(c, one + small, ix1 + ix5)
        assert census5[0] == 5 and census5[1] == 5 and census5[3:] == [4, 1], census5
        lone, lone_facts, _ = fresh(index, one)
        assert facts1 == lone_facts
        assert rep == fresh(repair, big) and rep[1] == [OK, OK, OK]
        five, five_facts, fresh_census = fresh(index, small)
        assert facts5 == five_facts and fresh_census[:3] == census5[:3]
        want = fresh(windows, one + small, lone + five)
        assert len(pcm) == len(want) == 6 and all(np.array_equal(a, b) for a, b in zip(pcm, want))
        for d, p in zip(one + small, pcm):
            ret, ref, _ = oracle.decode_whole(d)
            assert ret == OK and np.array_equal(p, ref)
        for ix in ix1 + ix5 + lone + five:
            ix.close()
    finally:
        c.close()
