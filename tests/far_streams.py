"""What the far-stream tests share (tests/test_far_streams_cpu.py, tests/test_gpu_stream_far.py): .lnn streams of up to 2^32 - 1
samples -- all the header's 32-bit sample count allows -- built from parts, and references of the windows calls that never allocate
such a stream.  A far stream is SILENT blocks of 65535 samples (11 bytes each) with a few `islands` of oracle-encoded blocks at chosen
sample positions and, behind its last block, the zeros of the header's tail.  Its decode is known without decoding it: an island's
blocks decode as they do in a short stream that the oracle decodes whole, everything else is zero (tests/test_far_streams_cpu.py holds
that to the oracle at reduced scale, and the island's bytes here are asserted equal to the short stream's).  FarPcm is that virtual
decode; the references for long windows walk its runs of zeros and of PCM in Python integers and numpy int64.  Nothing here touches a
GPU or the library under test."""
import zlib
from collections import namedtuple

import numpy as np

from relate_refs import MASK64, exact_dot, pairs
from signals import music
from splice_cases import COMPRESS, HEADER, RAW, SILENT, header_fields
from stream_refs import bins_of, pcm_bytes
from synth_records import CLOSING_SAMPLES, RATE, silent_block

SLICE_LIMIT = 1 << 24
N32 = (1 << 32) - 1

Far = namedtuple("Far", "nch bits preset ms total tables islands covered tail nbytes pcm")
# tables: (off, first, size, type, nsmp) as splice_cases.blocks_of gives them, `first` one longer; islands: [(start, first block, number of
# blocks, int32 [C][n])]; covered: the samples the blocks hold; tail: total - covered, the header's zeros; pcm: the FarPcm


def header(nch, total, bits, block, preset, ms):
    """the 30-byte stream header, as synth_records.write_stream writes one"""
    head = (b"IBRA" + (1).to_bytes(4, "big") + (2).to_bytes(4, "big") + nch.to_bytes(2, "big") + int(total).to_bytes(4, "big") +
            RATE.to_bytes(4, "big") + bits.to_bytes(2, "big") + block.to_bytes(4, "big") + bytes([preset, int(bool(ms))]))
    assert len(head) == HEADER
    h = header_fields(head)
    assert (h["num_channels"], h["num_samples"], h["bits_per_sample"], h["num_samples_per_block"], h["preset"], h["ch_process_method"]) == \
        (nch, total, bits, block, preset, int(bool(ms)))
    return head


def island_signal(nch, bits, blocks, seed):
    """the PCM an island's blocks are encoded from: music under COMPRESS blocks, full-scale noise under RAW ones, zeros under SILENT"""
    n = sum(length for length, _ in blocks)
    x = music(nch, n, bits, seed=seed).astype(np.int64)
    rng = np.random.default_rng(seed)
    lim, at = 1 << (bits - 1), 0
    for length, kind in blocks:
        if kind == RAW:
            x[:, at:at + length] = rng.integers(-lim, lim, size=(nch, length))
        elif kind == SILENT:
            x[:, at:at + length] = 0
        at += length
    return np.ascontiguousarray(x, dtype=np.int32)


def encode_blocks(oracle, x, bits, block, preset, ms, lengths):
    """one EncodeBlock of a fresh oracle encoder per entry of `lengths` -> the blocks' bytes"""
    enc = oracle.encoder(x.shape[0], bits, RATE, block, preset, ms)
    out, at = [], 0
    for n in lengths:
        out.append(enc.encode_block(x[:, at:at + n])[0])
        at += n
    enc.close()
    return out


def far_stream(oracle, nch, bits, preset, ms, islands, total, silent=65535):
    """islands: [(start sample, [(block length, kind), ...], seed)] in ascending order -> (the stream's bytes, its Far description).
    The header names `total` samples and blocks of 65535; SILENT blocks of `silent` samples (and one shorter, so that an island starts
    where it is asked to) lie between the islands; the blocks end behind the last island"""
    block = 65535
    assert 1 <= silent <= block and 0 < total <= N32
    full = silent_block(silent)
    parts = [header(nch, total, bits, block, preset, ms)]
    off, first, size, typ, nsmp = [], [0], [], [], []
    at = HEADER
    found = []

    def add(data, kind, n):
        nonlocal at
        parts.append(data)
        off.append(at); size.append(len(data) - 6); typ.append(kind); nsmp.append(n)
        first.append(first[-1] + n)
        at += len(data)

    for start, blocks, seed in islands:
        gap = start - first[-1]
        assert gap >= 0, "islands ascend and do not overlap"
        q, r = divmod(gap, silent)
        k0 = len(off)
        off += [at + 11 * i for i in range(q)]
        size += [5] * q; typ += [SILENT] * q; nsmp += [silent] * q
        first += [first[-1] + silent * (i + 1) for i in range(q)]
        parts.append(full * q)
        at += 11 * q
        assert len(off) == k0 + q and first[-1] == start - r
        if r:
            add(silent_block(r), SILENT, r)
        lengths = [n for n, _ in blocks]
        x = island_signal(nch, bits, blocks, seed)
        datas = encode_blocks(oracle, x, bits, block, preset, ms, lengths)
        # the same blocks under a short header: a stream the oracle decodes whole.  (A closing SILENT block keeps a COMPRESS block from
        # being the last thing in the data: synth_records.write_stream says why.)
        short_blocks = encode_blocks(oracle, x, bits, block, preset, ms, lengths)
        short = header(nch, x.shape[1] + CLOSING_SAMPLES, bits, block, preset, ms) + b"".join(short_blocks) + silent_block(CLOSING_SAMPLES)
        k0 = len(off)
        for data, (n, kind) in zip(datas, blocks):
            assert data[8] == kind and int.from_bytes(data[9:11], "big") == n, "the encoder chose another block type"
            add(data, kind, n)
        ret, pcm, _ = oracle.decode_whole(short)
        assert ret == 0 and pcm.shape == (nch, x.shape[1] + CLOSING_SAMPLES) and not pcm[:, -CLOSING_SAMPLES:].any()
        pcm = np.ascontiguousarray(pcm[:, :x.shape[1]], dtype=np.int32)
        assert np.array_equal(pcm, x), "the island does not decode to what it was encoded from"
        found.append((start, k0, len(blocks), pcm))
        stream_so_far = b"".join(parts[-len(blocks):])
        assert stream_so_far == short[HEADER:len(short) - 11], "the island's bytes differ from the short stream's"
    covered = first[-1]
    assert covered <= total
    stream = b"".join(parts)
    assert len(stream) == at
    far = FarPcm([(s, p) for s, _, _, p in found], nch, total)
    return stream, Far(nch, bits, preset, ms, total, (off, first, size, typ, nsmp), found, covered, total - covered, at, far)


class FarPcm:
    """the virtual decode of a far stream: islands (start, int32 [C][n]) in ascending order, zeros elsewhere, `total` samples"""

    def __init__(self, islands, nch, total):
        self.islands, self.nch, self.total = [(int(s), np.ascontiguousarray(p, dtype=np.int32)) for s, p in islands], nch, int(total)
        at = 0
        for s, p in self.islands:
            assert s >= at and p.shape[0] == nch
            at = s + p.shape[1]
        assert at <= self.total

    def segments(self, first, n):
        """the runs of window [first, first + n), in order: ("zeros", length) and ("pcm", int32 [C][length])"""
        first, n = int(first), int(n)
        assert 0 <= first and n >= 0 and first + n <= self.total
        at, end = first, first + n
        for s, p in self.islands:
            e = s + p.shape[1]
            if e <= at:
                continue
            if s >= end:
                break
            if s > at:
                yield ("zeros", s - at)
                at = s
            hi = min(e, end)
            yield ("pcm", p[:, at - s:hi - s])
            at = hi
        if at < end:
            yield ("zeros", end - at)

    def slice(self, first, n):
        """the dense int32 [C][n] of a window of at most 2^24 samples"""
        assert n <= SLICE_LIMIT, "a dense window of more than 2^24 samples"
        out = np.zeros((self.nch, n), dtype=np.int32)
        at = 0
        for kind, v in self.segments(first, n):
            if kind == "pcm":
                out[:, at:at + v.shape[1]] = v
                at += v.shape[1]
            else:
                at += v
        assert at == n
        return out

    def dense(self):
        """the whole decode, for the reduced scale"""
        return self.slice(0, self.total)


def buckets_of(first, n, b):
    """(first sample, length) of the buckets of window [first, first + n) with bucket length b (0: one bucket)"""
    step = b if b > 0 else max(n, 1)
    return [(first + at, min(step, n - at)) for at in range(0, n, step)]


# ---- the consumers' references over segments ----
def far_measure(pcm, first, n, b):
    """stream_refs.expected_measure for a window of any length: [channel][bucket] of (min, max, sum, sumsq_lo, sumsq_hi)"""
    out = [[] for _ in range(pcm.nch)]
    for a, m in buckets_of(first, n, b):
        lo, hi, s, q = [None] * pcm.nch, [None] * pcm.nch, [0] * pcm.nch, [0] * pcm.nch
        for kind, v in pcm.segments(a, m):
            for ch in range(pcm.nch):
                if kind == "zeros":
                    vmin = vmax = 0
                else:
                    row = v[ch].astype(np.int64)
                    vmin, vmax = int(row.min()), int(row.max())
                    s[ch] += int(row.sum())                     # (fewer than 2^24 values below 2^31: int64 holds it)
                    q[ch] += exact_dot(row, row)
                lo[ch] = vmin if lo[ch] is None else min(lo[ch], vmin)
                hi[ch] = vmax if hi[ch] is None else max(hi[ch], vmax)
        for ch in range(pcm.nch):
            out[ch].append((lo[ch], hi[ch], s[ch], q[ch] & MASK64, q[ch] >> 64))
    return out


def far_histogram(pcm, first, n, num_bins, shift=0, log2=False, b=0):
    """stream_refs.expected_histogram for a window of any length: Python integers [C][nb][num_bins]"""
    bk = buckets_of(first, n, b)
    out = [[[0] * num_bins for _ in bk] for _ in range(pcm.nch)]
    for k, (a, m) in enumerate(bk):
        for kind, v in pcm.segments(a, m):
            for ch in range(pcm.nch):
                if kind == "zeros":
                    out[ch][k][0] += v
                else:
                    for j, c in enumerate(np.bincount(bins_of(v[ch], num_bins, shift, log2), minlength=num_bins)):
                        out[ch][k][j] += int(c)
    return out


def far_relate(pcm, first, n, b=0):
    """relate_refs.expected_relate for a window of any length: [pair][bucket] of (dot_lo, dot_hi, num_equal, num_opposite), dot_hi signed"""
    pp = pairs(pcm.nch)
    out = [[] for _ in pp]
    for a, m in buckets_of(first, n, b):
        dot, eq, opp = [0] * len(pp), [0] * len(pp), [0] * len(pp)
        for kind, v in pcm.segments(a, m):
            for p, (i, j) in enumerate(pp):
                if kind == "zeros":
                    eq[p] += v
                    opp[p] += v
                else:
                    x, y = v[i].astype(np.int64), v[j].astype(np.int64)
                    dot[p] += exact_dot(x, y)
                    eq[p] += int((x == y).sum())
                    opp[p] += int((x + y == 0).sum())
        for p in range(len(pp)):
            out[p].append((dot[p] & MASK64, dot[p] >> 64, eq[p], opp[p]))
    return out


def far_quiet(pcm, first, n, threshold, min_samples):
    """stream_refs.expected_quiet for a window of any length: (runs, num_runs, quiet_samples, lead_samples, trail_samples)"""
    raw = []                                                    # maximal quiet runs [a, b) in window samples
    first_loud = last_loud = None

    def quiet(a, b):
        if raw and raw[-1][1] == a:
            raw[-1][1] = b
        else:
            raw.append([a, b])

    at = 0
    for kind, v in pcm.segments(first, n):
        if kind == "zeros":
            quiet(at, at + v)
            at += v
            continue
        q = (np.abs(v.astype(np.int64)) <= int(threshold)).all(axis=0)
        edge = np.diff(np.concatenate([[0], q.astype(np.int8), [0]]))
        for a, b in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)):
            quiet(at + int(a), at + int(b))
        loud = np.flatnonzero(~q)
        if loud.size:
            first_loud = at + int(loud[0]) if first_loud is None else first_loud
            last_loud = at + int(loud[-1])
        at += v.shape[1]
    m = max(int(min_samples), 1)
    runs = [(first + a, b - a) for a, b in raw if b - a >= m]
    lead, trail = (n, n) if first_loud is None else (first_loud, n - 1 - last_loud)
    return runs, len(runs), sum(r[1] for r in runs), lead, trail


# ---- CRC-32 over zeros ----
CRC_POLY = 0xEDB88320                                           # the reflected CRC-32 polynomial: bit 31 is x^0


def _mulmod(a, b):
    """a * b modulo the CRC-32 polynomial, both in the reflected form (bit 31 the coefficient of x^0)"""
    p = 0
    for k in range(31, -1, -1):
        if (a >> k) & 1:
            p ^= b
        b = (b >> 1) ^ CRC_POLY if b & 1 else b >> 1            # b * x
    return p


def crc32_zeros(crc, nbytes):
    """zlib.crc32(bytes(nbytes), crc) without the bytes: the register (crc ^ 0xFFFFFFFF) times x^(8 nbytes) by square-and-multiply"""
    nbytes = int(nbytes)
    assert nbytes >= 0
    power, x = 1 << 31, 1 << 23                                 # x^0, x^8
    while nbytes:
        if nbytes & 1:
            power = _mulmod(power, x)
        x = _mulmod(x, x)
        nbytes >>= 1
    return _mulmod(power, (int(crc) & 0xFFFFFFFF) ^ 0xFFFFFFFF) ^ 0xFFFFFFFF


def far_digest(pcm, bits, first, n, b):
    """stream_refs.expected_digest for a window of any length of a stream of 2 or more bytes per sample: [bucket] of (crc32, num_bytes)"""
    w = (bits + 7) // 8
    assert w >= 2, "a zero sample of an 8-bit stream is the byte 0x80: digest those densely"
    out = []
    for a, m in buckets_of(first, n, b):
        crc = 0
        for kind, v in pcm.segments(a, m):
            crc = crc32_zeros(crc, v * pcm.nch * w) if kind == "zeros" else zlib.crc32(pcm_bytes(v, bits, 0, v.shape[1]), crc)
        out.append((crc, m * pcm.nch * w))
    return out


# ---- resample: a dense view with the filter's halo ----
def resample_view(pcm, first, n, up, down, before, taps):
    """a window of output samples [first, first + n) of the stream resampled by up/down, for resample_refs.expected_resample: (full,
    local first) such that outputs [local first, local first + n) of `full` are the far stream's.  `full` begins at a multiple of
    `down` input samples -- shifting the input by j * down samples shifts the output by j * up, the phases stay -- at or before the first
    input sample the filter reads, and ends behind the last; where it ends short of that, the stream ends, and the reference's zeros
    before sample 0 and behind the last are the stream's"""
    lo_in = (first * down) // up - before
    hi_in = ((first + n - 1) * down) // up - before + taps
    lo = max(lo_in, 0) // down * down
    hi = min(max(hi_in, lo + 1), pcm.total)
    return pcm.slice(lo, hi - lo), first - lo // down * up


# ---- lags: a needle's runs of PCM against dense pieces of the haystack ----
def padded(pcm, ch, start, m):
    """row ch of the m <= 2^24 samples from `start` on -- any Python integer -- as int64, zeros where the stream has none"""
    start, m = int(start), int(m)
    assert 0 <= m <= SLICE_LIMIT, "a dense window of more than 2^24 samples"
    out = np.zeros(m, dtype=np.int64)
    lo, hi = max(start, 0), min(start + m, pcm.total)
    if lo < hi:
        out[lo - start:hi - start] = pcm.slice(lo, hi - lo)[ch]
    return out


def far_lags(pcm_a, ca, first_a, n, pcm_b, cb, first_b, lag_first, num_lags):
    """lag_refs.lag_sums for a needle of any length at any position: channel ca of pcm_a's [first_a, first_a + n) slid over channel cb of
    pcm_b from first_b + lag_first on -> (dots [num_lags], b_sq [num_lags], a_sq), Python integers.  The needle's zeros add nothing: per
    run of PCM at needle offset r, np.correlate against the haystack's dense piece [S + r, S + r + length + num_lags - 1) -- a run has
    fewer than 2^13 samples of at most 2^23 in magnitude, asserted, so that int64 holds every sum.  b_sq at the first lag from the
    haystack's runs over [S, S + n); from there on the square that enters less the square that leaves"""
    first_a, n, num_lags = int(first_a), int(n), int(num_lags)
    S = int(first_b) + int(lag_first)
    dots, a_sq, r = [0] * num_lags, 0, 0
    for kind, v in pcm_a.segments(first_a, n):
        if kind == "zeros":
            r += v
            continue
        x = v[ca].astype(np.int64)
        h = padded(pcm_b, cb, S + r, x.shape[0] + num_lags - 1)
        assert x.shape[0] < 1 << 13 and int(np.abs(x).max()) <= 1 << 23 and int(np.abs(h).max()) <= 1 << 23
        dots = [d + int(c) for d, c in zip(dots, np.correlate(h, x, mode="valid"))]
        a_sq += exact_dot(x, x)
        r += x.shape[0]
    assert r == n
    lo, hi = max(S, 0), min(S + n, pcm_b.total)
    first = 0
    if lo < hi:
        for kind, v in pcm_b.segments(lo, hi - lo):
            if kind == "pcm":
                first += exact_dot(v[cb], v[cb])
    b_sq = [first]
    if num_lags > 1:
        leave, enter = padded(pcm_b, cb, S, num_lags - 1), padded(pcm_b, cb, S + n, num_lags - 1)
        for e, l in zip((enter * enter).tolist(), (leave * leave).tolist()):
            b_sq.append(b_sq[-1] + e - l)
    assert min(b_sq) >= 0
    return dots, b_sq, a_sq


def far_lag_table(pcm_a, first_a, n, pcm_b, first_b, lag_first, num_lags, pairs):
    """lag_refs.expected_lags from far_lags: (lag_refs.table_of's table (P, num_lags), a_sq as uint64 (P, 2): low word, high word)"""
    import linne_amd
    once = {pair: far_lags(pcm_a, pair[0], first_a, n, pcm_b, pair[1], first_b, lag_first, num_lags) for pair in set(pairs)}
    t = np.zeros((len(pairs), num_lags), dtype=linne_amd.LAG_DTYPE)
    a_sq = np.zeros((len(pairs), 2), dtype=np.uint64)
    word = lambda vals, shift: np.array([(v >> shift) & MASK64 for v in vals], dtype=np.uint64)    # (two's complement: Python's >> and & do it)
    for p, pair in enumerate(pairs):
        dots, b_sq, e = once[tuple(pair)]
        t["dot_lo"][p], t["dot_hi"][p], t["b_sq_lo"][p], t["b_sq_hi"][p] = word(dots, 0), word(dots, 64).view(np.int64), word(b_sq, 0), word(b_sq, 64)
        a_sq[p] = (e & MASK64, e >> 64)
    return t, a_sq


# ---- project: the frames that touch an island, cut densely ----
def far_project(pcm, first, n, basis, hop, before=0, shift=0, clip_bits=0, f32=False, float_exp=0):
    """project_refs.expected_project for frames [first, first + n) of a stream of any length -> (idx, rows, saturated): idx the frames,
    counted from `first` and ascending, that read a sample of an island; rows what the call stores for them, (C, len(idx), K) int32 or
    float32.  Every other frame of the window reads zeros alone, and its row is zeros: a sum of 0 stays 0 under the rounding shift (the
    half that is added is shifted out again) and under any clip, and never saturates.  Frame f reads samples f * hop - before + (0 .. N);
    the frames that touch an island are runs of consecutive ones, and every run is cut from `padded` in pieces of at most 256 frames
    and goes through project_refs.projected_values as a stream of its own that begins at the piece's first sample"""
    from project_refs import projected_values
    first, n, hop, before = int(first), int(n), int(hop), int(before)
    basis = np.asarray(basis, dtype=np.int64)
    K, N = basis.shape
    touched = set()
    for s, p in pcm.islands:
        e = s + p.shape[1]
        lo = max((s - N + before) // hop + 1, first)                    # f * hop - before + N > s
        hi = min(-(-(e + before) // hop), first + n)                    # f * hop - before < e
        touched.update(range(lo, hi))
    idx = np.array(sorted(touched), dtype=np.int64)
    rows = np.zeros((pcm.nch, idx.shape[0], K), dtype=np.int64)
    sat, at = False, 0
    while at < idx.shape[0]:
        cnt = 1
        while at + cnt < idx.shape[0] and cnt < 256 and idx[at + cnt] == idx[at] + cnt and cnt * hop + N <= SLICE_LIMIT:
            cnt += 1
        start = int(idx[at]) * hop - before
        x = np.stack([padded(pcm, ch, start, (cnt - 1) * hop + N) for ch in range(pcm.nch)])
        rows[:, at:at + cnt], s = projected_values(x, 0, cnt, basis, hop, 0, shift, clip_bits)
        sat, at = sat or s, at + cnt
    idx -= first
    if not f32:
        return idx, rows.astype(np.int32), sat
    return idx, (rows.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -float_exp)).astype(np.float32), sat


def dense_project(nch, n, K, idx, rows):
    """far_project's answer as the table (C, n, K) of a window small enough to hold"""
    out = np.zeros((nch, n, K), dtype=rows.dtype)
    out[:, idx] = rows
    return out


# ---- the streams of the far tests ----
ISLAND = ((1024, COMPRESS), (777, COMPRESS), (300, RAW), (33, COMPRESS), (1024, COMPRESS))
ISLAND_SAMPLES = sum(n for n, _ in ISLAND)
CLOSING_SILENT = 3000
SHAPES = {"far16": (2, 16, 5, True), "far24": (3, 24, 0, False)}       # channels, bits, preset, MS
A_START, B_START = (1 << 31) - 1500, N32 - 70000


def full_scale(oracle, name):
    """the stream `name` of 2^32 - 1 samples: island A straddles 2^31, island B starts 70000 samples before the end and is followed by
    one SILENT block of 3000 samples; then the blocks end and the header's tail begins"""
    nch, bits, preset, ms = SHAPES[name]
    seed = 500 + bits
    return far_stream(oracle, nch, bits, preset, ms, [(A_START, list(ISLAND), seed), (B_START, list(ISLAND) + [(CLOSING_SILENT, SILENT)], seed + 1)], N32)


def reduced_scale(oracle, name, gaps=(3, 5), tail=4321):
    """the same builder with a handful of SILENT blocks in front of each island and a tail behind the last block"""
    nch, bits, preset, ms = SHAPES[name]
    seed = 500 + bits
    a = gaps[0] * 65535 + 34036                                 # (not on a block edge: a shorter SILENT block in front of it)
    b = a + ISLAND_SAMPLES + gaps[1] * 65535 + 17
    total = b + ISLAND_SAMPLES + CLOSING_SILENT + tail
    return far_stream(oracle, nch, bits, preset, ms, [(a, list(ISLAND), seed), (b, list(ISLAND) + [(CLOSING_SILENT, SILENT)], seed + 1)], total)
