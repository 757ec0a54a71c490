"""CPU tests (-m "not gpu") of what the GPU tests of the windows consumers share (tests/stream_consumers.py) and of the stream tools'
harness (tools/stream_timing.py): the shared scaffold can still fail.  The arrays come from the reference functions on a small
synthetic stream -- 3 channels, 2 blocks of 256 and a tail of 100 -- with bucket lengths 0, 7 and 256: one bucket, many short buckets,
and a bucket boundary on a block boundary.  The want_buffer functions the four bucket consumers' tests had before they shared one are
copied here as what the generic one is compared against: the old code is the reference, not the code under test."""
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import linne_amd
import stream_consumers as sc
from relate_refs import expected_relate
from signals import music
from stream_consumers import OK, SENTINEL
from stream_refs import expected_digest, expected_histogram, expected_measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = SimpleNamespace(full=music(3, 2 * 256 + 100, 16, seed=3), bits=16, nch=3, ns=612)
CORRUPTION = 6
WINDOWS = [(0, 612), (200, 312), (255, 2), (611, 1), (256, 256), (17, 0)]
BUCKETS = [0, 7, 256]
FIELDS = {"measure": [(b,) for b in BUCKETS], "digest": [(b,) for b in BUCKETS], "relate": [(b,) for b in BUCKETS],
          "histogram": [(64, 4, 0, 0), (33, 0, 1, 7), (2, 9, 0, 256)]}


def items_of(name):
    """every window with every spec; the second window of each spec fails"""
    items, codes = [], []
    for f in FIELDS[name]:
        for j, (first, n) in enumerate(WINDOWS):
            items.append((None, None, first, n, 3, *f, None))
            codes.append(CORRUPTION if j == 1 else OK)
    return items, codes


# ---- the four old want_buffers ----
def old_relate(words, items, fulls, codes, offs, nbs, PAD=1):
    buf = np.full(words, SENTINEL, dtype=np.int64)
    for it, full, code, off, nb in zip(items, fulls, codes, offs, nbs):
        if code != OK or it[3] == 0:
            continue
        want = expected_relate(full, it[2], it[3], it[5])
        for p in range(want.shape[0]):
            at = off + 4 * p * (nb + PAD)
            buf[at:at + 4 * nb] = np.ascontiguousarray(want[p]).view(np.int64)
    return buf


def old_histogram(words, items, fulls, codes, offs, nbs, PAD=1):
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


def old_measure(total, cases, offs, nbs, PAD=2):
    """cases: (first, n, b, full, code); offs in records"""
    buf = np.full((total, 4), SENTINEL, dtype=np.int64).view(linne_amd.MEASURE_DTYPE).reshape(total)
    for i, (first, n, b, full, code) in enumerate(cases):
        if code != OK:
            continue
        for ch, row in enumerate(expected_measure(full, first, n, b)):
            for j, r in enumerate(row):
                buf[offs[i] + ch * (nbs[i] + PAD) + j] = r
    return buf


def old_digest(total, cases, offs):
    buf = np.full((total, 2), SENTINEL, dtype=np.int64).view(linne_amd.DIGEST_DTYPE).reshape(total)
    for i, (first, n, b, tr, code) in enumerate(cases):
        if code != OK:
            continue
        for j, (crc, size) in enumerate(expected_digest(tr.full, tr.bits, first, n, b)):
            buf[offs[i] + j] = (crc, 0, size)
    return buf


def generic(name, pad=sc.PAD, gap=sc.GAP):
    c = sc.CONSUMERS[name]
    items, codes = items_of(name)
    offs, nbs, words = sc.layout(c, items, pad, gap)
    return c, items, codes, offs, nbs, words, sc.want_buffer(c, words, items, [T] * len(items), codes, offs, nbs, pad)


@pytest.mark.parametrize("name", ["relate", "histogram"])
def test_want_buffer_is_the_old_one_words(name):
    c, items, codes, offs, nbs, words, got = generic(name)
    old = {"relate": old_relate, "histogram": old_histogram}[name](words, items, [T.full] * len(items), codes, offs, nbs)
    assert (got != SENTINEL).sum() > 1000 and np.array_equal(got, old)


def test_want_buffer_is_the_old_one_measure():
    """the old layout: records of four words, a sentinel record around the tables, the rows two records apart"""
    c, items, codes, offs, nbs, words, got = generic("measure", pad=2, gap=4)
    assert all(o % 4 == 0 for o in offs) and words % 4 == 0
    cases = [(it[2], it[3], it[5], T.full, code) for it, code in zip(items, codes)]
    old = old_measure(words // 4, [x for x in cases if x[1]], [o // 4 for o, x in zip(offs, cases) if x[1]], [nb for nb, x in zip(nbs, cases) if x[1]])
    assert got.tobytes() == old.tobytes()


def test_want_buffer_is_the_old_one_digest():
    c, items, codes, offs, nbs, words, got = generic("digest", pad=0, gap=2)
    cases = [(it[2], it[3], it[5], T, code) for it, code in zip(items, codes)]
    old = old_digest(words // 2, [x for x in cases if x[1]], [o // 2 for o, x in zip(offs, cases) if x[1]])
    assert got.tobytes() == old.tobytes()


@pytest.mark.parametrize("name", sc.BUCKET_CONSUMERS)
def test_a_wrong_buffer_compares_unequal(name):
    c, items, codes, offs, nbs, words, want = generic(name)
    assert np.array_equal(want, want.copy())
    word = want.copy()
    word[offs[0]] ^= 1                                           # a table word
    gap = want.copy()
    assert gap[offs[2] - 1] == np.int64(SENTINEL)
    gap[offs[2] - 1] = 0                                         # a sentinel in a gap
    failing = want.copy()
    assert codes[1] != OK and failing[offs[1]] == np.int64(SENTINEL)
    failing[offs[1]] = 5                                         # a word in a failing window's table
    stride = want.copy()
    if c.stride:
        at = offs[0] + nbs[0] * c.words(*items[0][5:5 + c.fields])
        assert stride[at] == np.int64(SENTINEL)
        stride[at] = 0                                           # the padding between two rows
    for bad in (word, gap, failing) + ((stride,) if c.stride else ()):
        assert not np.array_equal(bad, want) and bad.tobytes() != want.tobytes()


def test_the_table_knows_every_kind_the_old_lists_knew():
    """the hand-written "no other consumer's kernel ran" lists of the five test_launch_counts, as they stood"""
    old = {"measure": [59, 79], "digest": [59, 79, 80, 81, 82], "quiet": [59, 79, 80, 83], "histogram": [59, 79, 80, 81, 82, 83, 86, 87],
           "relate": [59, 79, 80, 81, 82, 83, 86, 87, 92, 93, 94]}
    for name, kinds in old.items():
        assert set(kinds) <= set(sc.other_kinds(name)), name
        assert not set(sc.CONSUMERS[name].kinds) & set(sc.other_kinds(name))
    every = sorted(k for c in sc.CONSUMERS.values() for k in c.kinds)
    assert every == [59] + list(range(79, 98)) and sc.DECODE_KINDS == [28, 56, 57, 58]
    assert sc.CONSUMERS["quiet"].kinds[1:] == (87, 88, 89, 90, 91)


def test_the_harness_statistic_is_the_tools():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import stream_timing as st
    finally:
        sys.path.pop(0)

    def stats(ts):                                               # as every tools/stream_*.py had it
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "spread_ms": round(max(ts) - min(ts), 3)}

    def verdict(ok, text):
        return ("met: " if ok else "MISSED: ") + text
    ts = [3.14159, 2.71828, 10.00049, 0.5, 7.77777, 2.0]
    assert st.stats(ts) == stats(ts) == {"median_ms": 2.93, "min_ms": 0.5, "max_ms": 10.0, "spread_ms": 9.5}
    assert st.stats(ts[:1]) == stats(ts[:1])
    assert [st.verdict(ok, "a b") for ok in (True, False)] == [verdict(ok, "a b") for ok in (True, False)] == ["met: a b", "MISSED: a b"]
