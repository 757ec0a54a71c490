"""The reference of the lag tests (include/linne_amd.h LINNEAmd_LagWindowsDevice): the sliding sums of a needle over a haystack that is
zero outside its stream, from decoded PCM alone.  np.correlate on int64 where n * 2^(2 * bits - 2) fits int64 -- bits the width the
values really have --; otherwise Python integers for short needles and, for long ones, numpy on 16-bit limbs put together in Python
integers (limb_sums), which tests/test_stream_lags_cpu.py holds to the Python integers."""
import numpy as np

import linne_amd

MASK64 = (1 << 64) - 1


def haystack(b, first_b, lag_first, num_lags, n):
    """the num_lags - 1 + n samples of row b from first_b + lag_first on, zeros where the stream has none -> int64"""
    b = np.asarray(b, dtype=np.int64)
    start, m = int(first_b) + int(lag_first), int(num_lags) - 1 + int(n)
    out = np.zeros(m, dtype=np.int64)
    lo, hi = max(start, 0), min(start + m, b.shape[0])
    if lo < hi:
        out[lo - start:hi - start] = b[lo:hi]
    return out


def _bits(*arrays):
    return max(max(int(np.abs(v).max()) if v.size else 0 for v in arrays).bit_length() + 1, 2)


def lag_sums(a, first_a, n, b, first_b, lag_first, num_lags):
    """rows a and b of decoded PCM -> (dots [num_lags], b_sq [num_lags], a_sq), Python integers"""
    x = np.asarray(a, dtype=np.int64)[int(first_a):int(first_a) + int(n)]
    assert x.shape[0] == n >= 1
    h = haystack(b, first_b, lag_first, num_lags, n)
    if n * (1 << (2 * _bits(x, h) - 2)) < 1 << 63:
        dots = [int(v) for v in np.correlate(h, x, mode="valid")]
        cs = np.concatenate(([0], np.cumsum(h * h)))
        b_sq = [int(cs[l + n] - cs[l]) for l in range(num_lags)]
        return dots, b_sq, int(np.dot(x, x))
    if n > 4096:
        return limb_sums(x, h, n, num_lags)
    xs, hs = [int(v) for v in x], [int(v) for v in h]
    dots = [sum(p * q for p, q in zip(xs, hs[l:l + n])) for l in range(num_lags)]
    sq = [v * v for v in hs]
    b_sq = [sum(sq[:n])]
    for l in range(1, num_lags):
        b_sq.append(b_sq[-1] + sq[l - 1 + n] - sq[l - 1])
    return dots, b_sq, sum(v * v for v in xs)


def limb_sums(x, h, n, num_lags):
    """lag_sums for int32 values of any width and long needles, exact: every value is v1 * 2^16 + v0 with 0 <= v0 < 2^16 and
    |v1| <= 2^15, a product of two limbs lies below 2^32, and np.correlate's int64 holds n < 2^31 of them; the four limb correlations
    are put together in Python integers.  The squares are Python integers"""
    assert n < 1 << 31 and int(np.abs(x).max()) <= 1 << 31 and int(np.abs(h).max()) <= 1 << 31
    x0, x1, h0, h1 = x & 0xFFFF, x >> 16, h & 0xFFFF, h >> 16
    c = [[np.correlate(p, q, mode="valid") for q in (x0, x1)] for p in (h0, h1)]
    dots = [(int(hh) << 32) + ((int(hl) + int(lh)) << 16) + int(ll) for ll, lh, hl, hh in zip(c[0][0], c[0][1], c[1][0], c[1][1])]
    sq = h.astype(object) ** 2
    cs = np.concatenate(([0], np.cumsum(sq)))
    return dots, [int(cs[l + n] - cs[l]) for l in range(num_lags)], int((x.astype(object) ** 2).sum())


def expected_lags(full_a, first_a, n, full_b, first_b, lag_first, num_lags, pairs):
    """-> (the table, a LAG_DTYPE array (P, num_lags); a_sq, uint64 (P, 2): low word, high word)"""
    table = np.zeros((len(pairs), num_lags), dtype=linne_amd.LAG_DTYPE)
    a_sq = np.zeros((len(pairs), 2), dtype=np.uint64)
    for p, (ca, cb) in enumerate(pairs):
        dots, b_sq, e = lag_sums(full_a[ca], first_a, n, full_b[cb], first_b, lag_first, num_lags)
        for l in range(num_lags):
            d = dots[l] & ((1 << 128) - 1)
            table[p, l] = (d & MASK64, (d >> 64) - (1 << 64 if d >> 127 else 0), b_sq[l] & MASK64, b_sq[l] >> 64)
        a_sq[p] = (e & MASK64, e >> 64)
    return table, a_sq


def table_of(dots, b_sq):
    """[P][L] Python integers -> a LAG_DTYPE array, for the host helpers' tests"""
    t = np.zeros((len(dots), len(dots[0])), dtype=linne_amd.LAG_DTYPE)
    for p, row in enumerate(dots):
        for l, d in enumerate(row):
            u = d & ((1 << 128) - 1)
            t[p, l] = (u & MASK64, (u >> 64) - (1 << 64 if u >> 127 else 0), b_sq[p][l] & MASK64, b_sq[p][l] >> 64)
    return t
