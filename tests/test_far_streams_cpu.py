"""CPU tests of what the far-stream GPU tests stand on (tests/far_streams.py): the builder's streams decode, at reduced scale, to what
FarPcm says under the oracle's whole decode; the references that walk runs of zeros and PCM equal the dense references of the sibling
tests on that decode; crc32_zeros equals zlib, once beyond 2^32 bytes; and the full-scale streams of 2^32 - 1 samples have, byte for byte,
the layout their description claims.  Nothing here touches a GPU or the library under test."""
import zlib

import numpy as np
import pytest

import far_streams as fs
from far_streams import A_START, B_START, CLOSING_SILENT, ISLAND, ISLAND_SAMPLES, N32, SHAPES
from index_cases import index_walk
from relate_refs import expected_relate
from splice_cases import COMPRESS, HEADER, RAW, SILENT
from stream_refs import expected_digest, expected_histogram, expected_measure, expected_quiet

OK = 0
NAMES = tuple(SHAPES)
BUCKETS = (0, 441, 65535, 65536)
SMALL_BUCKETS = (1, 7)


@pytest.fixture(scope="module")
def reduced(oracle):
    """name -> (stream, description, the oracle's whole decode): one or two SILENT blocks of 65535 samples in front of each island"""
    out = {}
    for name in NAMES:
        stream, d = fs.reduced_scale(oracle, name, gaps=(1, 2))
        ret, full, _ = oracle.decode_whole(stream)
        assert ret == OK and d.total < 2_000_000 and d.tail > 0
        out[name] = (stream, d, np.ascontiguousarray(full, dtype=np.int32))
    return out


def long_windows(d):
    (a, _, _, pa), (b, _, _, pb) = d.islands
    la, T = pa.shape[1], d.total
    return [(0, T), (1, T - 2), (a - 1000, la + 2000), (a + 100, 2000), (a, la), (a + la, b - a - la), (a + 500, b - a), (d.covered - 10, d.tail + 10),
            (T - 100, 100), (a - 1, la + 2), (b + 7, T - b - 7)]


def short_windows(d):
    (a, _, _, pa), (b, _, _, pb) = d.islands
    la, T = pa.shape[1], d.total
    return [(a - 20, 50), (a + la - 30, 60), (a + 1024 - 5, 12), (T - 40, 40), (d.covered - 5, 30), (b - 3, 3), (b, 1)]


def cases(d):
    """(first, n, bucket length): long windows under the long buckets and one longer than the window, short ones under 1 and 7 as well"""
    out = [(a, n, b) for a, n in long_windows(d) for b in BUCKETS + (n + 5,)]
    return out + [(a, n, b) for a, n in short_windows(d) for b in SMALL_BUCKETS + (0, n + 1)]


@pytest.mark.parametrize("name", NAMES)
def test_reduced_scale_decodes_to_the_virtual_pcm(reduced, name):
    """SILENT and unreached samples are zeros, and an island's blocks decode the same wherever they lie"""
    stream, d, full = reduced[name]
    assert full.shape == (d.nch, d.total) and np.array_equal(full, d.pcm.dense())
    assert not full[:, d.covered:].any() and [k for _, k in ISLAND] == [COMPRESS, COMPRESS, RAW, COMPRESS, COMPRESS]
    for start, k0, nb, pcm in d.islands:
        assert np.array_equal(full[:, start:start + pcm.shape[1]], pcm) and pcm.any()
        assert d.tables[1][k0] == start and d.tables[3][k0 - 1] == SILENT and 0 < d.tables[4][k0 - 1] < 65535      # a shorter SILENT block in front
    code, h, nblocks, tables, failure = index_walk(stream)
    assert code == OK and failure == (-1, OK, 0) and tuple(tables) == tuple(d.tables) and nblocks == len(d.tables[0])
    for a, n in long_windows(d) + short_windows(d):
        assert np.array_equal(d.pcm.slice(a, n), full[:, a:a + n])
        kinds = [k for k, _ in d.pcm.segments(a, n)]
        assert not any(x == y == "zeros" for x, y in zip(kinds, kinds[1:]))      # a run of zeros is whole
    with pytest.raises(AssertionError):
        fs.FarPcm([], 1, 1 << 25).slice(0, (1 << 24) + 1)


@pytest.mark.parametrize("name", NAMES)
def test_segment_references_equal_the_dense_ones(reduced, name):
    _, d, full = reduced[name]
    for a, n, b in cases(d):
        key = (name, a, n, b)
        if n <= 70000 or b in (0, 65535):                       # (the dense measure reference is a Python loop per sample)
            assert fs.far_measure(d.pcm, a, n, b) == expected_measure(full, a, n, b), key
        want = expected_relate(full, a, n, b)
        got = fs.far_relate(d.pcm, a, n, b)
        assert [[(int(r["dot_lo"]), int(r["dot_hi"]), int(r["num_equal"]), int(r["num_opposite"])) for r in row] for row in want] == got, key
        assert fs.far_digest(d.pcm, d.bits, a, n, b) == expected_digest(full, d.bits, a, n, b), key
        for bins, shift, log2 in ((64, 3, False), (33, 0, True), (1, 0, False), (1024, 6, False)):
            assert np.array_equal(np.array(fs.far_histogram(d.pcm, a, n, bins, shift, log2, b), dtype=np.int64), expected_histogram(full, a, n, bins, shift, log2, b)), key
    for a, n in long_windows(d) + short_windows(d):
        for thr in (0, 3, 1 << 12, 1 << 31):
            for mn in (0, 1, 2, 33, 3001, 65536, n, n + 1):
                assert fs.far_quiet(d.pcm, a, n, thr, mn) == expected_quiet(full, a, n, thr, mn), (name, a, n, thr, mn)


@pytest.mark.parametrize("name", NAMES)
def test_resample_view_is_the_window_of_the_whole(reduced, name):
    """resample_refs.expected_resample on the view's dense piece equals it on the whole decode"""
    from resample_refs import expected_resample, random_coef, resampled_length
    _, d, full = reduced[name]
    rng = np.random.default_rng(5)
    (a, _, _, pa), _ = d.islands
    for up, down, taps, before in ((1, 1, 64, 31), (147, 160, 16, 7), (160, 147, 64, 32), (1, 2, 64, 0), (2, 1, 33, 32)):
        coef = random_coef(rng, up, taps)
        L = resampled_length(d.total, up, down)
        for m0, n in ((0, 40), (a * up // down - 20, 45), ((a + pa.shape[1]) * up // down - 3, 9), (L - 30, 30), (L - 1, 1)):
            view, local = fs.resample_view(d.pcm, m0, n, up, down, before, taps)
            want = expected_resample(full, m0, n, coef, up, down, before, 15, 0)
            got = expected_resample(view, local, n, coef, up, down, before, 15, 0)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1], (name, up, down, m0, n)
            assert view.shape[1] <= taps + n * down // up + 2 * down + 2


def lag_cases(reduced):
    """(needle stream, first_a, n, haystack stream, first_b, lag_first, num_lags, pairs).  lag_refs.lag_sums is numpy while n * 2^(2 bits - 2)
    fits int64: needles of more than 2^17 samples go with the 16-bit stream alone"""
    d16, d24 = reduced["far16"][1], reduced["far24"][1]
    (a, _, _, pa), (b, _, _, pb) = d16.islands
    la, T = pa.shape[1], d16.total
    assert d24.total == T and [s for s, _, _, _ in d24.islands] == [a, b]
    both = b + la + 100 - (a - 50)
    return [("far16", a - 100, la + 300, "far16", a - 100, -300, 601, [(0, 0), (1, 1), (0, 1)]),          # a needle over an island, against itself
            ("far24", a - 7, la + 20, "far16", b, -100, 400, [(0, 1), (2, 0)]),                           # ... over the other stream's other island
            ("far16", a + 100, 2000, "far24", a, 0, 300, [(1, 2)]),                                       # a needle of PCM alone
            ("far16", a - 50, both, "far16", a - 50, -40, 81, [(0, 1), (1, 0)]),                          # a needle holding two islands
            ("far16", 0, T, "far16", 0, -30, 61, [(1, 1)]),                                               # a haystack range off both ends
            ("far24", b - 50, 5000, "far24", b, 0, 20000, [(2, 1)]),                                      # ... off the end, lags in the thousands
            ("far16", a, la, "far24", a, -a - 100, 300, [(0, 0)]),                                        # ... that starts at -100
            ("far16", a, la, "far24", T + 5, -(T + 5 - a) + 17, 200, [(0, 2), (1, 1)]),                    # first_b beyond the stream, the range inside it
            ("far16", a, la, "far24", (1 << 64) - 1, 5, 9, [(0, 0)]),                                     # a range that misses the stream
            ("far16", a, la, "far24", 0, -(1 << 63), 9, [(0, 0)]),
            ("far24", T - 40, 40, "far16", b + la - 10, -20, 50, [(0, 0)]), ("far24", T - 1, 1, "far24", a, 0, la, [(1, 1)]),
            ("far16", b + la - 1, 1, "far24", a, 0, la, [(1, 1)]), ("far24", a + 5, 1, "far16", a, -3, 1, [(2, 0)])]


def test_far_lags_equal_the_dense_reference(reduced):
    """far_streams.far_lags and far_lag_table against lag_refs.lag_sums and expected_lags on the oracle's whole decode"""
    from lag_refs import expected_lags, lag_sums
    nonzero = 0
    for key in lag_cases(reduced):
        na, first_a, n, nb, first_b, lag_first, num_lags, pairs = key
        (_, da, fa), (_, db, fb) = reduced[na], reduced[nb]
        for ca, cb in pairs:
            got = fs.far_lags(da.pcm, ca, first_a, n, db.pcm, cb, first_b, lag_first, num_lags)
            assert got == lag_sums(fa[ca], first_a, n, fb[cb], first_b, lag_first, num_lags), key[:7] + (ca, cb)
            nonzero += any(got[0])
        table, a_sq = fs.far_lag_table(da.pcm, first_a, n, db.pcm, first_b, lag_first, num_lags, pairs)
        want, want_sq = expected_lags(fa, first_a, n, fb, first_b, lag_first, num_lags, pairs)
        assert table.dtype == want.dtype and table.tobytes() == want.tobytes() and a_sq.dtype == want_sq.dtype and np.array_equal(a_sq, want_sq), key
    assert nonzero >= 12


@pytest.mark.parametrize("name", NAMES)
def test_far_project_equals_the_dense_reference(reduced, name):
    """far_streams.far_project against project_refs.expected_project on the oracle's whole decode: hops from 1 to beyond the frame and
    65536, `before` at 0 and N - 1, windows that start before an island, that hold both, that end behind the stream's last block and in
    the header's tail, and one of silence alone; every frame outside the returned indexes is zeros in the dense reference"""
    from project_refs import expected_project, project_length
    _, d, full = reduced[name]
    (a, _, _, pa), (b, _, _, pb) = d.islands
    la, T = pa.shape[1], d.total
    rng = np.random.default_rng(77)
    loud, k = 0, 0
    for N, K in ((70, 5), (1, 2), (512, 3)):
        basis = rng.integers(-32768, 32768, (K, N)).astype(np.int16)
        basis[0] = 32767
        for H in (1, 3, N, N + 5, 1000, 65536):
            F = project_length(T, H)
            spans = [(max((a - 300) // H, 0), min(-(-(la + 600) // H), 900)), ((a + la - 100) // H, min(40, F - (a + la - 100) // H)), (max(F - 50, 0), min(F, 50)),
                     ((d.covered - 200) // H, min(-(-400 // H), F - (d.covered - 200) // H)), (b // H, min(-(-(la + 3100) // H), 700, F - b // H)), (0, min(F, 30))]
            if H >= 1000:
                spans.append((0, F))                            # both islands and all the silence in one window
            for first, n in spans:
                for before in (0, N - 1):
                    shift, clip, f32 = (0, 15, 31, 7)[k % 4], (0, 16, 24)[k % 3], k % 5 == 1
                    idx, rows, sat = fs.far_project(d.pcm, first, n, basis, H, before, shift, clip, f32, 31 if f32 else 0)
                    want, wsat = expected_project(full, first, n, basis, H, before, shift, clip, f32, 31 if f32 else 0)
                    got = fs.dense_project(d.nch, n, K, idx, rows)
                    assert got.dtype == want.dtype and got.tobytes() == want.tobytes() and sat == wsat, (name, N, K, H, first, n, before)
                    assert idx.shape[0] <= n and (np.diff(idx) > 0).all() and (idx.shape[0] == 0 or (0 <= idx[0] and idx[-1] < n))
                    loud += bool(rows.any())
                    k += 1
    assert loud >= 60


def test_crc32_zeros_against_zlib():
    starts = (0, 1, 0xFFFFFFFF, 0xDEADBEEF, zlib.crc32(b"far streams"))
    for n in (0, 1, 255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24, (1 << 24) + 1):
        zeros = bytes(n)
        for crc in starts:
            assert fs.crc32_zeros(crc, n) == zlib.crc32(zeros, crc), (n, crc)
    # once beyond 2^32 bytes, fed to zlib in chunks: byte 4 of a length against an implementation that is not ours
    n, crc = (1 << 32) + 5, 0x12345678
    chunk = bytes(1 << 26)
    for _ in range(n >> 26):
        crc = zlib.crc32(chunk, crc)
    crc = zlib.crc32(bytes(n & ((1 << 26) - 1)), crc)
    assert fs.crc32_zeros(0x12345678, n) == crc
    assert fs.crc32_zeros(0x12345678, n) != fs.crc32_zeros(0x12345678, 5)


@pytest.mark.parametrize("name", NAMES)
def test_full_scale_layout(oracle, name):
    """the stream of 2^32 - 1 samples, bytes only: its size, every block head, the islands' places, the tail, and the serial index walk"""
    stream, d = fs.full_scale(oracle, name)
    off, first, size, typ, nsmp = d.tables
    assert d.total == N32 and fs.header_fields(stream)["num_samples"] == N32 and fs.header_fields(stream)["num_samples_per_block"] == 65535
    island_blocks = {k for _, k0, nb, _ in d.islands for k in range(k0, k0 + nb)}
    island_bytes = sum(size[k] + 6 for k in island_blocks)
    nsilent = len(off) - len(island_blocks)
    assert len(stream) == d.nbytes == HEADER + 11 * nsilent + island_bytes
    assert all(typ[k] == SILENT and size[k] == 5 for k in range(len(off)) if k not in island_blocks)
    raw = np.frombuffer(stream, dtype=np.uint8)
    o = np.array(off, dtype=np.int64)
    assert (raw[o] == 0xFF).all() and (raw[o + 1] == 0xFF).all() and np.array_equal(raw[o + 8], np.array(typ, dtype=np.uint8))
    assert np.array_equal(raw[o + 9].astype(np.int64) * 256 + raw[o + 10], np.array(nsmp, dtype=np.int64))
    field = (raw[o + 2].astype(np.int64) << 24) | (raw[o + 3].astype(np.int64) << 16) | (raw[o + 4].astype(np.int64) << 8) | raw[o + 5]
    assert np.array_equal(field, np.array(size, dtype=np.int64)) and np.array_equal(o[1:], o[:-1] + field[:-1] + 6) and o[0] == HEADER
    assert off[-1] + size[-1] + 6 == len(stream) and np.array_equal(np.diff(np.array(first, dtype=np.int64)), np.array(nsmp, dtype=np.int64))
    (a, ka, na, pa), (b, kb, nb, pb) = d.islands
    assert (a, b) == (A_START, B_START) == ((1 << 31) - 1500, N32 - 70000) and first[ka] == a and first[kb] == b
    assert a < 1 << 31 < a + pa.shape[1] and pa.shape[1] == ISLAND_SAMPLES and pb.shape[1] == ISLAND_SAMPLES + CLOSING_SILENT
    assert [typ[k] for k in range(kb, kb + nb)] == [COMPRESS, COMPRESS, RAW, COMPRESS, COMPRESS, SILENT] and kb + nb == len(off)
    assert [nsmp[k] for k in range(ka, ka + na)] == [n for n, _ in ISLAND] and nsmp[-1] == CLOSING_SILENT
    assert d.covered == first[-1] == b + ISLAND_SAMPLES + CLOSING_SILENT and d.tail == N32 - d.covered == 70000 - ISLAND_SAMPLES - CLOSING_SILENT
    assert 65537 <= len(off) < 65560 and nsilent * 11 < 730_000
    code, h, nblocks, tables, failure = index_walk(stream)
    assert code == OK and failure == (-1, OK, 0) and nblocks == len(off) and tuple(tables) == tuple(d.tables)
    assert list(d.pcm.segments(0, N32)) and [k for k, _ in d.pcm.segments(0, N32)] == ["zeros", "pcm", "zeros", "pcm", "zeros"]
    assert sum(v if k == "zeros" else v.shape[1] for k, v in d.pcm.segments(0, N32)) == N32
