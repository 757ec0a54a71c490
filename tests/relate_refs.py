"""The reference of the relate call's tests (tests/test_stream_relate_cpu.py, tests/test_gpu_stream_relate.py,
tests/test_gpu_stream_history.py): what LINNEAmd_RelateWindowsDevice must write, from numpy and Python integers on the
oracle's decode of a stream -- never from the library under test -- and the streams those tests write themselves."""
import numpy as np

import linne_amd
from stream_refs import CARRY_NS, CARRY_PEAK, carry_signal, crc16

RAW = 2
S = 1024
MASK64 = (1 << 64) - 1


def pairs(C):
    """the channel pairs (i, j), i <= j < C, in the table's order: the upper triangle row by row"""
    return [(i, j) for i in range(C) for j in range(i, C)]


def exact_dot(x, y):
    """the sum of x[s] * y[s] as a Python integer.  A product of two int32 fits int64 (at most 2^62); its halves -- q >> 32 and
    q & (2^32 - 1) -- are added up apart in int64, which fewer than 2^31 terms cannot overflow, and put together in Python"""
    q = np.asarray(x).astype(np.int64) * np.asarray(y).astype(np.int64)
    assert q.size < 1 << 31
    return (int((q >> 32).sum(dtype=np.int64)) << 32) + int((q & 0xFFFFFFFF).sum(dtype=np.int64))


def expected_relate(full, first, n, b=0):
    """the table for window [first, first + n) of a stream that decodes to `full` (C, N), with bucket length b (0: one bucket): a
    structured array (P, nb) of linne_amd.RELATION_DTYPE, dot_hi * 2^64 + dot_lo the 128-bit two's complement of the sum"""
    full = np.asarray(full)
    C = full.shape[0]
    step = b if b > 0 else max(n, 1)
    nb = -(-n // step)
    out = np.zeros((C * (C + 1) // 2, nb), dtype=linne_amd.RELATION_DTYPE)
    w = full[:, first:first + n].astype(np.int64)
    live = (np.arange(nb * step) < n).reshape(nb, step)         # the last bucket may be short: its missing frames count nowhere
    w = np.pad(w, ((0, 0), (0, nb * step - n))).reshape(C, nb, step)
    for p, (i, j) in enumerate(pairs(C)):
        x, y = w[i], w[j]
        q = x * y                                                # at most 2^62 in magnitude; its halves are added up apart (exact_dot)
        hi, lo = (q >> 32).sum(axis=1, dtype=np.int64), (q & 0xFFFFFFFF).sum(axis=1, dtype=np.int64)
        eq, opp = ((x == y) & live).sum(axis=1), ((x + y == 0) & live).sum(axis=1)
        for k in range(nb):
            d = (int(hi[k]) << 32) + int(lo[k])
            out[p, k] = ((d & MASK64), (d >> 64), int(eq[k]), int(opp[k]))      # (d >> 64 floors: the signed high word)
    return out


def dots(table):
    """the sums of a table as Python integers [P][nb]"""
    return [[(int(r["dot_hi"]) << 64) + int(r["dot_lo"]) for r in row] for row in table]


def bucket_lengths(n, b):
    step = b if b > 0 else max(n, 1)
    return [min(step, n - k * step) for k in range(-(-n // step))]


def carry_stereo_signal():
    """stereo: L a square wave between +-(2^23 - 1) over 2^18 + 1024 samples (the measure tests' carry_signal), R = -L"""
    x = carry_signal()
    return np.concatenate([x, -x], axis=0)


def carry_stereo_stream(oracle):
    """carry_stereo_signal() as a 24-bit stream of RAW blocks of 1024 sample frames, written as test_stream_measure_cpu.carry_stream
    writes its mono one: header and block heads from the oracle's encode of as many zeros (L/R, no MS); a RAW block holds its
    samples zig-zagged, three bytes each, big-endian, frame by frame"""
    x = carry_stereo_signal()
    quiet = bytes(oracle.encode_whole(np.zeros_like(x), 24, 44100, S, 0, False))
    out = bytearray(quiet[:30])
    for at in range(0, CARRY_NS, S):
        v = x[:, at:at + S].T.reshape(-1).astype(np.int64)          # interleaved
        zz = np.where(v >= 0, 2 * v, -2 * v - 1)
        payload = b"".join(int(u).to_bytes(3, "big") for u in zz)
        body = bytes([RAW]) + (len(v) // 2).to_bytes(2, "big") + payload
        out += quiet[30:32] + (len(body) + 2).to_bytes(4, "big") + crc16(body).to_bytes(2, "big") + body
    return bytes(out)


__all__ = ["CARRY_NS", "CARRY_PEAK", "pairs", "exact_dot", "expected_relate", "dots", "bucket_lengths", "carry_stereo_signal", "carry_stereo_stream"]
