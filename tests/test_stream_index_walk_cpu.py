"""The yardstick of the stream index tests against LINNEDecoder_DecodeWhole: index_cases.index_walk, the plain-Python walk the GPU
tests hold Context.index_stream and Context.index_streams to, must say of every stream what a whole decode says of it -- the code of
its lowest failing block where it reports one, OK where it reports none, a header's code where the header is refused -- and on
well-formed streams its tables are those of blocks(stream).

Two corpora.  The streams of SILENT and RAW blocks written in index_cases.host_corpus decode on the host alone and run everywhere.
The corpus of the GPU tests (index_cases.build_corpus) is encoded by the library and holds COMPRESS blocks, which the library decodes
on the device: that comparison needs the GPU and is marked so."""
import pytest

import index_cases as ic
from stream_refs import blocks


def agree(name, data, product):
    """index_walk(data) against product.decode_whole(data) -> the walk"""
    walk = ic.index_walk(data)
    ret, _ = product.decode_whole(data)
    code, header, nb, tables, failure = walk
    if code != ic.OK:
        assert ret == code and header is None, (name, ret, walk)
        return walk
    assert ret == failure[1], (name, ret, failure)
    off, first, size, typ, nsmp = tables
    assert len(off) == len(size) == len(typ) == len(nsmp) == nb and len(first) == nb + 1, name
    assert (failure[0] == -1 and failure[2] == 0) if failure[1] == ic.OK else 0 <= failure[0] <= nb, (name, failure)
    return walk


def test_the_walk_agrees_with_decode_whole_on_host_only_streams(product):
    cases = ic.host_corpus(product)
    seen = set()
    for name, data in cases:
        code, header, nb, tables, failure = agree(name, data, product)
        seen.add(code if code != ic.OK else failure[1])
        if name in ("whole", "trailing bytes"):
            assert failure == (-1, ic.OK, 0) and nb == 10, name
            off, first, size, typ, nsmp = tables
            assert [(o, s + 6, t, n, f) for o, s, t, n, f in zip(off, size, typ, nsmp, first)] == blocks(data), name
    by = {name: ic.index_walk(data) for name, data in cases}
    assert by["two damaged blocks"][4][:2] == (2, ic.CORRUPTION)                   # the lowest of the two
    assert by["cut at a block"][4] == (-1, ic.OK, 0) and by["cut at a block"][2] == 5
    assert by["cut inside a head"][4][:2] == (4, ic.INSUFFICIENT_DATA) and by["cut inside a head"][2] == 4
    assert by["more samples than the blocks hold"][4] == (-1, ic.OK, 0)
    assert {ic.OK, ic.INVALID_FORMAT, ic.INSUFFICIENT_BUFFER, ic.INSUFFICIENT_DATA, ic.CORRUPTION} <= seen, seen


@pytest.mark.gpu
def test_the_walk_agrees_with_decode_whole_on_the_corpus(product):
    """every case of the GPU tests' corpus takes part (the NULL pointer is no stream)"""
    cases = ic.build_corpus(product)
    assert len(cases) >= 45
    for c in cases:
        if c.data is None:
            continue
        code, header, nb, tables, failure = agree(c.name, c.data, product)
        if c.well_formed:
            assert code == ic.OK and failure == (-1, ic.OK, 0), c.name
            off, first, size, typ, nsmp = tables
            assert [(o, s + 6, t, n, f) for o, s, t, n, f in zip(off, size, typ, nsmp, first)] == blocks(c.data), c.name
