"""The references the tests of the resident-stream calls hold the library to, in one place so that the per-feature tests and the
history scenarios (tests/stream_history.py) share them: what a windows call must answer for a window of a stream that decodes to
`full` -- numpy and Python integers on the oracle's decode, zlib.crc32 of the byte string numpy builds --, the block walk of a
well-formed stream, the block checksum, and the material with all three block types.  Nothing here touches a GPU or the library."""
import zlib

import numpy as np

from signals import music


def be(b):
    return int.from_bytes(bytes(b), "big")


def blocks(stream):
    """(offset, bytes, type, samples, first sample) of the blocks DecodeWhole walks in a well-formed stream"""
    ns, off, prog, out = be(stream[14:18]), 30, 0, []
    while prog < ns and off + 11 <= len(stream):
        size, typ, n = be(stream[off + 2:off + 6]), stream[off + 8], be(stream[off + 9:off + 11])
        out.append((off, size + 6, typ, n, prog))
        prog += n
        off += size + 6
    return out


def mixed_signal(nch, bits, ns, seed, block=4096):
    """music with a silent stretch (SILENT blocks) and a stretch of full-scale noise (RAW blocks), each two blocks long"""
    ns = max(ns, 7 * block)
    x = music(nch, ns, bits, seed=seed).astype(np.int64)
    x[:, block:3 * block] = 0
    rng = np.random.default_rng(seed)
    lim = 1 << (bits - 1)
    x[:, 4 * block:6 * block] = rng.integers(-lim, lim, size=(nch, 2 * block))
    return np.ascontiguousarray(x, dtype=np.int32)


def crc16(data):
    """CRC-16/ARC (reflected 0xA001, initial value 0, no final XOR): what a block's bytes 6..7 hold, big-endian, over everything
    behind them (lnn_entropy.c crc_init / lnn_crc16)"""
    crc = 0
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0xA001 if crc & 1 else crc >> 1
    return crc


# ---- compare ----
def expected_compare(full, first, n, held):
    """what the call must answer for window [first, first + n) of a stream that decodes to `full` against PCM that holds the values
    `held` (C, n)"""
    d = full[:, first:first + n].astype(np.int64) != np.asarray(held).astype(np.int64)
    if not d.any():
        return (0, 0, 0)
    s = int(np.flatnonzero(d.any(axis=0))[0])
    return (int(d.sum()), first + s, int(np.flatnonzero(d[:, s])[0]))


# ---- measure ----
def expected_measure(full, first, n, b):
    """the table LINNEAmd_MeasureWindowsDevice must write for window [first, first + n) of a stream that decodes to `full` (C, N),
    with bucket length b (0: one bucket): [channel][bucket] of (min, max, sum, sumsq_lo, sumsq_hi), Python integers"""
    out = []
    step = b if b > 0 else max(n, 1)
    for row in np.asarray(full)[:, first:first + n]:
        recs = []
        for at in range(0, n, step):
            v = [int(e) for e in row[at:at + step]]
            q = sum(e * e for e in v)
            recs.append((min(v), max(v), sum(v), q & ((1 << 64) - 1), q >> 64))
        out.append(recs)
    return out


def measure_table(m):
    """a Measurement's (or a structured array's) records in expected_measure's form"""
    a = m if isinstance(m, np.ndarray) else m.cpu()
    return [[(int(r["min"]), int(r["max"]), int(r["sum"]), int(r["sumsq_lo"]), int(r["sumsq_hi"])) for r in row] for row in a]


# ---- digest ----
def pcm_bytes(full, bits, first, n):
    """the byte string of samples [first, first + n) of a stream that decodes to `full` (C, N) with `bits` bits per sample:
    interleaved, ceil(bits / 8) little-endian bytes of the two's-complement value, truncated, 8-bit samples offset by 128"""
    w = (bits + 7) // 8
    x = np.ascontiguousarray(np.asarray(full)[:, first:first + n].T).astype(np.int64)       # (n, C)
    if w == 1:
        x = x + 128
    u = (x & 0xFFFFFFFF).astype("<u4")
    return np.ascontiguousarray(u.view(np.uint8).reshape(x.shape[0], x.shape[1], 4)[:, :, :w]).tobytes()


def expected_digest(full, bits, first, n, b):
    """the table LINNEAmd_DigestWindowsDevice must write for window [first, first + n) of a stream that decodes to `full` (C, N),
    with bucket length b (0: one bucket): [bucket] of (crc32, num_bytes)"""
    step = b if b > 0 else max(n, 1)
    out = []
    for at in range(0, n, step):
        s = pcm_bytes(full, bits, first + at, min(step, n - at))
        out.append((zlib.crc32(s), len(s)))
    return out


def digest_table(d):
    """a DigestTable's (or a structured array's) records in expected_digest's form"""
    a = d if isinstance(d, np.ndarray) else d.cpu()
    assert not a["reserved"].any()
    return [(int(r["crc32"]), int(r["num_bytes"])) for r in a]


# ---- quiet ----
def expected_quiet(full, first, n, threshold, min_samples):
    """what LINNEAmd_QuietWindowsDevice must answer for window [first, first + n) of a stream that decodes to `full` (C, N):
    (runs, num_runs, quiet_samples, lead_samples, trail_samples), runs the list of (first sample in the stream, length)"""
    x = np.abs(np.asarray(full)[:, first:first + n].astype(np.int64))
    q = (x <= int(threshold)).all(axis=0)
    edge = np.diff(np.concatenate([[0], q.astype(np.int8), [0]]))
    starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    m = max(int(min_samples), 1)
    runs = [(first + int(a), int(b - a)) for a, b in zip(starts, ends) if b - a >= m]
    loud = np.flatnonzero(~q)
    lead, trail = (n, n) if loud.size == 0 else (int(loud[0]), n - 1 - int(loud[-1]))
    return runs, len(runs), sum(r[1] for r in runs), lead, trail


def quiet_answer(q):
    """a QuietRuns in expected_quiet's form"""
    return q.cpu(), q.num_runs, q.quiet_samples, q.lead_samples, q.trail_samples


# ---- histogram ----
def bins_of(v, num_bins, shift, log2):
    """the bin of every sample of v (any shape): m = |v| >> shift in 64 bits, x = m or m's bit length, min(x, num_bins - 1)"""
    m = np.abs(np.asarray(v).astype(np.int64)) >> int(shift)
    x = np.searchsorted(np.int64(1) << np.arange(33, dtype=np.int64), m, side="right") if log2 else m       # powers of two <= m: the bit length
    return np.minimum(x, num_bins - 1)


def expected_histogram(full, first, n, num_bins, shift=0, log2=False, b=0):
    """the table LINNEAmd_HistogramWindowsDevice must write for window [first, first + n) of a stream that decodes to `full` (C, N),
    with bucket length b (0: one bucket): int64 (C, nb, num_bins)"""
    full = np.asarray(full)
    step = b if b > 0 else max(n, 1)
    nb = -(-n // step)
    out = np.zeros((full.shape[0], nb, num_bins), dtype=np.int64)
    for ch, row in enumerate(full[:, first:first + n]):
        x = bins_of(row, num_bins, shift, log2)
        for k in range(nb):
            out[ch, k] = np.bincount(x[k * step:(k + 1) * step], minlength=num_bins)
    return out


# ---- a stream whose sum of squares passes 2^64 ----
CARRY_BLOCK = 1024
CARRY_NS = (1 << 18) + 1024
CARRY_PEAK = (1 << 23) - 1


def carry_signal():
    """mono: a square wave between +-(2^23 - 1), 2^18 + 1024 samples -- its sum of squares is above 2^64"""
    i = np.arange(CARRY_NS)
    return np.where((i // 100) % 2 == 0, CARRY_PEAK, -CARRY_PEAK).astype(np.int32)[None, :]


def carry_stream(oracle):
    """carry_signal() as a 24-bit stream of RAW blocks of 1024 samples, written here: the header and the blocks' first two bytes are
    those of the oracle's encode of as many zeros; a RAW block holds its samples zig-zagged, three bytes each, big-endian, behind
    the size field (bytes 2..5: what follows them), the CRC16 over what follows it (bytes 6..7), the type and the sample count"""
    x = carry_signal()
    quiet = bytes(oracle.encode_whole(np.zeros_like(x), 24, 44100, CARRY_BLOCK, 0, False))
    out = bytearray(quiet[:30])
    for at in range(0, CARRY_NS, CARRY_BLOCK):
        v = x[0, at:at + CARRY_BLOCK].astype(np.int64)
        zz = np.where(v >= 0, 2 * v, -2 * v - 1)
        payload = b"".join(int(u).to_bytes(3, "big") for u in zz)
        body = bytes([2]) + len(v).to_bytes(2, "big") + payload
        out += quiet[30:32] + (len(body) + 2).to_bytes(4, "big") + crc16(body).to_bytes(2, "big") + body
    return bytes(out)
