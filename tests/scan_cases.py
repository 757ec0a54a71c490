"""What the tests of the block-head scan that StreamIndexesCreate and RepairStreamsDevice share have in common
(tests/test_block_scan_cpu.py, tests/test_gpu_block_scan.py): the undamaged streams of the index and the repair corpora, and a few
streams of one to four blocks of a few hundred samples written here byte by byte."""
import ctypes as C

import numpy as np

import index_cases as ic
import repair_cases as rc
from refs import _RefHeader
from splice_cases import COMPRESS, HEADER, RAW, SILENT, blocks_of


def tiny_stream(product, nch, bits, S, lens, kinds, seed):
    """a stream of RAW and SILENT blocks of the given lengths, behind the header LINNEEncoder_EncodeHeader writes"""
    rng = np.random.default_rng(seed)
    body = [rc.silent_block(n) if k == SILENT else rc.raw_block(rng.integers(0, 255, size=bits // 8 * nch * n, dtype=np.uint8).tobytes(), n)
            for n, k in zip(lens, kinds)]
    hdr = _RefHeader(1, 2, nch, sum(lens), 44100, bits, S, 0, 0)
    out = np.zeros(HEADER, dtype=np.uint8)
    assert product.L.LINNEEncoder_EncodeHeader(C.byref(hdr), out.ctypes.data, out.size) == 0
    return out.tobytes() + b"".join(body)


def undamaged_streams(oracle, product):
    """[(name, bytes)]: every undamaged stream of repair_cases.build_cases (its cases a) and of index_cases.host_corpus (its whole
    stream), then streams of exactly one block, of two, of four blocks with a short last one"""
    out = [(name, data) for name, (data, clean) in sorted(rc.build_cases(oracle).items()) if name.endswith("/a")]
    out += [("host corpus " + name, data) for name, data in ic.host_corpus(product) if name == "whole"]
    out.append(("one RAW block", tiny_stream(product, 1, 16, 300, [300], [RAW], 1)))
    out.append(("one SILENT sample", tiny_stream(product, 2, 16, 256, [1], [SILENT], 2)))
    out.append(("two blocks", tiny_stream(product, 2, 8, 200, [200, 199], [SILENT, RAW], 3)))
    out.append(("four blocks", tiny_stream(product, 1, 24, 257, [257, 257, 257, 5], [RAW, SILENT, RAW, RAW], 4)))
    return out


def block_types(data):
    """the set of block types of an undamaged stream"""
    return set(blocks_of(data)[3])


def stumps(product):
    """[(name, bytes)]: a stream shorter than the first block's offset, and one that ends where the first block would begin"""
    s = tiny_stream(product, 1, 16, 300, [300], [RAW], 1)
    return [("shorter than the header", s[:HEADER - 1]), ("the header alone", s[:HEADER])]
