"""GPU tests of sliding resident .lnn streams over each other (Context.lag_windows, align_streams; include/linne_amd.h
LINNEAmd_LagWindowsDevice).  Every element of every table is computed with numpy int64 or Python integers (lag_refs.expected_lags) from
the oracle's decode of the same bytes, never from the library under test, and everything must be equal: integers, no tolerance.  The
tables of a call lie in one buffer of sentinels, which must come back untouched around them.  Streams hold 3 blocks of 1024 samples and
a tail, or 21 blocks of 33; one mono stream holds 65537 + 300 samples for the needles at the chunk's edge, and one of 24-bit RAW blocks
written by hand holds 66 blocks of full-scale values.  Where a test is about which of the kernel's two summing paths a sub-tile takes,
it works that out from the reference's data under the kernel's staging rule (sub_tiles) and asserts its premise."""
import numpy as np
import pytest

import linne_amd
import synth_records as sr
from lag_refs import expected_lags, haystack
from relate_refs import CARRY_NS, CARRY_PEAK, carry_stereo_stream
from signals import music
import stream_consumers as sc
from stream_consumers import KIND, Stream, encoded, last_error
from stream_refs import crc16, mixed_signal
from test_stream_lags_cpu import BAD
from test_stream_relate_cpu import WIDE_SHAPE, wide_cases

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, NG = 0, 1, 7
S = 1024
TAIL = 300
SENTINEL = 0x5A5A5A5A5A5A5A5A
GAP = 3
LAGS_KIND, COMMIT_KIND, PLACE_KIND = KIND["LAGS_T_LAGS"], KIND["LAGS_T_COMMIT"], KIND["T_WX_PLACE"]


@pytest.fixture(scope="module")
def streams(ctx, oracle):
    out = {nch: encoded(ctx, oracle, music(nch, 3 * S + TAIL, 16, seed=40 + nch), 16, 5 if nch == 2 else 0, nch == 2, f"{nch}ch") for nch in (1, 2, 3, 8)}
    out["8bit"] = encoded(ctx, oracle, music(2, 2 * S + 77, 8, seed=61), 8, 0, False, "8 bits")
    out["24bit"] = encoded(ctx, oracle, music(2, 2 * S + 77, 24, seed=62), 24, 2, True, "24 bits")
    x = music(2, 20 * 33 + 5, 16, seed=17)
    out["small"] = Stream(ctx, oracle, oracle.encode_whole(x, 16, 44100, 33, 0, False), "blocks of 33")
    m = mixed_signal(2, 16, 7 * S + TAIL, seed=11, block=S)
    whole = bytes(oracle.encode_whole(m, 16, 44100, S, 5, True))
    out["cut"] = Stream(ctx, oracle, whole[:sc.blocks(whole)[6][0]], "mixed, cut")         # SILENT and RAW blocks, and a tail of zeros behind the blocks
    assert out["cut"].ns == 7 * S + TAIL and not out["cut"].full[:, 6 * S:].any()
    yield out
    for t in out.values():
        t.index.close()


@pytest.fixture(scope="module")
def long_mono(ctx, oracle):
    t = encoded(ctx, oracle, music(1, 65537 + TAIL, 16, seed=33), 16, 0, False, "65837 samples")
    yield t
    t.index.close()


def probe(a, first_a, n, b, first_b, lag_first, num_lags, pairs, a_sq=True, **over):
    return dict(a=a, first_a=first_a, n=n, b=b, first_b=first_b, lag_first=lag_first, num_lags=num_lags, pairs=pairs, a_sq=a_sq, over=over)


def raw_lags(ctx, probes, group_frames=0, pad=1):
    """LINNEAmd_LagWindowsDevice itself -> (ret, codes, the buffer as int64, per probe (the table's first word, its pair stride, the
    a_sq's first word or None))"""
    import torch
    places, at = [], GAP
    for q in probes:
        P, L = len(q["pairs"]), q["num_lags"]
        places.append((at, L + pad, at + 4 * P * (L + pad) + GAP if q["a_sq"] else None))
        at += 4 * P * (L + pad) + GAP + (2 * P + GAP if q["a_sq"] else 0)
    buf = torch.full((at,), SENTINEL, dtype=torch.int64, device="cuda")
    arr = (linne_amd.LagProbe * len(probes))()
    for k, q in enumerate(probes):
        a, b, (off, stride, sq) = q["a"], q["b"], places[k]
        f = dict(index_a=q["over"].get("index_a", a.index).h, d_stream_a=q["over"].get("dev_a", a.dev).data_ptr(), first_a=q["first_a"], num_samples=q["n"],
                 index_b=q["over"].get("index_b", b.index).h, d_stream_b=q["over"].get("dev_b", b.dev).data_ptr(), first_b=q["first_b"], lag_first=q["lag_first"],
                 num_lags=q["num_lags"], num_pairs=len(q["pairs"]), d_out=buf.data_ptr() + 8 * off, pair_stride=stride, d_a_sq=None if sq is None else buf.data_ptr() + 8 * sq, reserved=0, result=-1)
        f.update({x: y for x, y in q["over"].items() if x not in ("index_a", "dev_a", "index_b", "dev_b")})
        for x, y in f.items():
            setattr(arr[k], x, y)
        for p, (i, j) in enumerate(q["pairs"]):
            arr[k].chan_a[p], arr[k].chan_b[p] = i, j
        if "wrong_channel" in q:                                  # what no reference has: a channel not of its stream, a pointer 4 bytes on, a NULL index
            field, v = q["wrong_channel"]
            getattr(arr[k], field)[1] = 255 if v == 255 else (a if field == "chan_a" else b).nch
        if "four_bytes_on" in q:
            setattr(arr[k], q["four_bytes_on"], getattr(arr[k], q["four_bytes_on"]) + 4)
        if "null_index" in q:
            setattr(arr[k], q["null_index"], None)
    torch.cuda.synchronize()
    ret = linne_amd.lib.LINNEAmd_LagWindowsDevice(ctx.h, arr, len(probes), group_frames)
    return ret, [arr[k].result for k in range(len(probes))], buf.cpu().numpy(), places


def want_buffer(words, probes, codes, places):
    """sentinels but the OK probes' tables"""
    buf = np.full(words, SENTINEL, dtype=np.int64)
    for q, code, (off, stride, sq) in zip(probes, codes, places):
        if code != OK:
            continue
        table, e = expected_lags(q["a"].full, q["first_a"], q["n"], q["b"].full, q["first_b"], q["lag_first"], q["num_lags"], q["pairs"])
        w = np.ascontiguousarray(table).view(np.int64).reshape(len(q["pairs"]), q["num_lags"], 4)
        for p in range(len(q["pairs"])):
            buf[off + 4 * p * stride:off + 4 * (p * stride + q["num_lags"])] = w[p].reshape(-1)
        if sq is not None:
            buf[sq:sq + 2 * len(q["pairs"])] = e.view(np.int64).reshape(-1)
    return buf


def check(ctx, probes, codes=None, group_frames=0):
    ret, got_codes, buf, places = raw_lags(ctx, probes, group_frames)
    codes = [OK] * len(probes) if codes is None else codes
    assert got_codes == codes, (got_codes, last_error(ctx))
    assert ret == next((c for c in codes if c != OK), OK)
    want = want_buffer(buf.shape[0], probes, codes, places)
    bad = np.nonzero(buf != want)[0]
    assert bad.size == 0, (bad[:8], buf[bad[:8]], want[bad[:8]], places)
    return buf


# ---- shapes ----
@pytest.mark.parametrize("num_lags", [1, 255, 256, 257, 513])
def test_lag_counts(ctx, streams, num_lags):
    t, u = streams[2], streams["small"]
    check(ctx, [probe(t, 100, 33, t, 60, -7, num_lags, [(0, 0), (1, 1)]), probe(u, 3, 200, t, 1000, -num_lags // 2, num_lags, [(0, 1)]),
                probe(t, 0, 1, u, 0, -3, num_lags, [(1, 0)], a_sq=False)])


@pytest.mark.parametrize("n,num_lags", [(1, 5), (33, 40), (65535, 3), (65536, 2), (65537, 257)])
def test_needle_lengths(ctx, long_mono, n, num_lags):
    """the chunk of 65536 needle samples and its neighbours; the last is about 17 M products"""
    check(ctx, [probe(long_mono, 7, n, long_mono, 0, -100, num_lags, [(0, 0)])])


def test_ranges_off_the_haystack(ctx, streams):
    """negative, zero and positive lag_first; haystack ranges that start before sample 0, end behind the stream, do both, or miss it"""
    t, u = streams[2], streams[3]
    N = u.ns
    check(ctx, [probe(t, 10, 100, u, 0, -50, 120, [(0, 0)]), probe(t, 10, 100, u, N - 80, 0, 60, [(0, 2)]), probe(t, 0, t.ns, u, 0, -300, 601, [(1, 1)]),
                probe(t, 5, 64, u, 0, -400, 300, [(0, 0), (1, 1)]), probe(t, 5, 64, u, N, 0, 9, [(0, 0)]), probe(t, 5, 64, u, (1 << 64) - 1, 5, 9, [(1, 2)]),
                probe(t, 5, 64, u, 0, -(1 << 63), 9, [(0, 0)]), probe(t, 5, 64, u, 200, 17, 3, [(1, 0)]), probe(t, 5, 64, u, N - 1, 0, 1, [(1, 0)])])


def test_autocorrelation_and_channel_pairs(ctx, streams):
    """A == B with overlapping images; the pair (0, 1) of one stream; a channel named twice; 8 channels with 1 and 8 pairs"""
    t, e = streams[2], streams[8]
    check(ctx, [probe(t, 500, 700, t, 500, -300, 601, [(0, 0), (1, 1)]), probe(t, 0, t.ns, t, 0, 0, 1, [(0, 1)]), probe(t, 40, 90, t, 0, 0, 130, [(0, 0), (0, 1), (0, 0)]),
                probe(e, 10, 300, e, 0, -20, 70, [(7, 0)]), probe(e, 10, 300, e, 0, -20, 70, [(c, 7 - c) for c in range(8)]), probe(streams[1], 0, 50, e, 3, -1, 3, [(0, 5)])])


def test_widths_block_types_and_block_sizes(ctx, streams):
    """8-, 16- and 24-bit streams; blocks of 33 and of 1024 samples in one probe; SILENT blocks, RAW blocks and the tail's zeros"""
    b8, b24, sm, t, cut = streams["8bit"], streams["24bit"], streams["small"], streams[2], streams["cut"]
    check(ctx, [probe(b8, 0, b8.ns, b24, 0, -10, 21, [(0, 0), (1, 1)]), probe(b24, 100, 1500, b24, 0, 90, 21, [(0, 1)]), probe(sm, 30, 600, t, 900, -40, 300, [(0, 0), (1, 1)]),
                probe(t, 0, 2000, cut, 0, -100, 260, [(0, 0)]), probe(cut, S - 10, 5 * S + 600, cut, S, -30, 40, [(0, 1), (1, 1)]), probe(cut, 6 * S + 5, 200, t, 0, 0, 4, [(0, 0)])])


def test_narrow_sums_pass_two_to_the_64(ctx, oracle):
    """full-scale 24-bit stereo, R = -L, against itself: every value within +-2^23, the sums beyond 64 bits on both sides"""
    c = Stream(ctx, oracle, carry_stereo_stream(oracle), "257 RAW blocks, R = -L")
    try:
        buf = check(ctx, [probe(c, 0, CARRY_NS, c, 0, -1, 3, [(0, 0), (0, 1)])])
        assert CARRY_NS * CARRY_PEAK ** 2 > 1 << 64 and buf[GAP + 4 + 1] == 1 and buf[GAP + 4 * 4 + 4 + 1] == -2      # dot_hi at lag 0 of both pairs
    finally:
        c.index.close()


def test_wide_values(ctx, oracle):
    """a 16-bit stream whose crafted blocks decode to values over all of int32: (lo, hi) sums, with products of every sign"""
    w = Stream(ctx, oracle, sr.case_stream(WIDE_SHAPE, wide_cases()), "wide values")
    try:
        assert np.abs(w.full.astype(np.int64)).max() > 1 << 30
        n = min(w.ns - 40, 2500)
        check(ctx, [probe(w, 20, n, w, 20, -20, 41, [(0, 0), (0, 1), (1, 0)]), probe(w, 0, 300, w, 0, 0, 1, [(1, 1)])])
    finally:
        w.index.close()


# ---- the two summing paths: sub-tiles within +-2^23 in one int64, the others in (lo, hi) ----
CHUNK, SUB, LAGS, NARROW = 65536, 1024, 256, 1 << 23


def is_wide(v):
    """the kernel's rule (lnn_k_lags.h wxl_wide): -2^23 and 2^23 are narrow, -2^23 - 1 and 2^23 + 1 are wide"""
    return (v < -NARROW) | (v > NARROW)


def sub_tiles(x, h, l0, chunk):
    """what tile (chunk, l0) stages, from the reference's data: x the needle's samples, h = lag_refs.haystack(...), which is zero where the
    haystack's image has no word -> per sub-tile (its 1024 or fewer needle words, the 1279 haystack words under them at the tile's 256
    lags, whether one of them is wide)"""
    i0 = chunk * CHUNK
    length = min(x.shape[0] - i0, CHUNK)
    out = []
    for s0 in range(0, length, SUB):
        a = x[i0 + s0:i0 + min(s0 + SUB, length)]
        b = np.zeros(SUB + LAGS - 1, dtype=np.int64)
        piece = h[l0 + i0 + s0:l0 + i0 + s0 + SUB + LAGS - 1]
        b[:piece.shape[0]] = piece
        out.append((a, b, bool(is_wide(a).any() or is_wide(b).any())))
    return out


def raw24_stream(oracle, x):
    """x (2, a multiple of 1024 samples) as a 24-bit stream of RAW blocks, written as relate_refs.carry_stereo_stream writes its one: header
    and block heads from the oracle's encode of as many zeros; a RAW block holds its samples zig-zagged, three bytes each, big-endian,
    frame by frame"""
    assert x.shape[0] == 2 and x.shape[1] % S == 0 and np.abs(x.astype(np.int64) * 2 + 1).max() < 1 << 24
    quiet = bytes(oracle.encode_whole(np.zeros_like(x), 24, 44100, S, 0, False))
    out = bytearray(quiet[:30])
    for at in range(0, x.shape[1], S):
        v = x[:, at:at + S].T.reshape(-1).astype(np.int64)
        zz = np.where(v >= 0, 2 * v, -2 * v - 1)
        body = bytes([2]) + S.to_bytes(2, "big") + b"".join(int(u).to_bytes(3, "big") for u in zz)
        out += quiet[30:32] + (len(body) + 2).to_bytes(4, "big") + crc16(body).to_bytes(2, "big") + body
    return bytes(out)


@pytest.fixture(scope="module")
def wide(ctx, oracle):
    w = Stream(ctx, oracle, sr.case_stream(WIDE_SHAPE, wide_cases()), "wide values")
    yield w
    w.index.close()


@pytest.fixture(scope="module")
def full24(ctx, oracle):
    """66 RAW blocks of 24 bits: L alternates between -2^23 and 2^23 - 1, R is -2^23 throughout -- all of it narrow, by one"""
    n = 66 * S
    x = np.empty((2, n), dtype=np.int32)
    x[0, 0::2], x[0, 1::2], x[1] = -NARROW, NARROW - 1, -NARROW
    t = Stream(ctx, oracle, raw24_stream(oracle, x), "66 RAW blocks of 24 bits")
    assert np.array_equal(t.full, x) and not is_wide(t.full.astype(np.int64)).any()
    yield t
    t.index.close()


def test_wide_values_among_narrow_in_one_tile(ctx, long_mono, wide):
    """a 16-bit needle of 65537 samples (2 chunks) over the wide-value stream, 600 lags (3 lag tiles): tile (chunk 0, l0 256) sums some of
    its sub-tiles in one int64 and some in (lo, hi), and the int64 part, which the tile's end merges into (lo, hi) with its sign, is
    negative at some lag.  Probe 0 has the wide stream under needle samples 28000 to 34000, so no square enters or leaves its b^2: probe
    1 has it under the needle's first samples, where wide squares leave at every lag of the second and third lag tile.  Probe 2: the
    wide stream as the needle"""
    m, w, L, n = long_mono, wide, 600, 65537
    assert w.ns == 6115 and m.ns >= n and not is_wide(m.full.astype(np.int64)).any()
    x = m.full[0, :n].astype(np.int64)
    for S0, squares in ((-28300, False), (800, True)):
        for cb in (0, 1):
            h = haystack(w.full[cb], S0, 0, L, n)
            tiles = sub_tiles(x, h, 256, 0)
            kinds = [wd for _, _, wd in tiles]
            assert len(tiles) == 64 and any(kinds) and not all(kinds), (S0, cb)
            share = sum(np.correlate(b[:a.shape[0] + LAGS - 1], a, mode="valid") for a, b, wd in tiles if not wd)
            assert share.shape == (LAGS,) and share.min() < 0, (S0, cb)
            for l0 in (256, 512):
                lanes = np.arange(1, min(LAGS, L - l0))
                leave, enter = h[l0 + lanes - 1], h[l0 + lanes - 1 + n]
                assert (max(int((leave * leave).max()), int((enter * enter).max())) > 1 << 48) == squares, (S0, cb, l0)
    check(ctx, [probe(m, 0, n, w, 0, -28300, L, [(0, 0), (0, 1)]), probe(m, 0, n, w, 800, 0, L, [(0, 0), (0, 1)]),
                probe(w, 0, w.ns, m, 1000, -300, L, [(0, 0), (1, 0)])])


def test_wide_values_across_chunks(ctx, wide, full24):
    """a full-scale 24-bit needle of 66 blocks (2 chunks) over the wide-value stream, 300 lags (2 lag tiles): the wide values under chunk 0,
    under both chunks and under chunk 1 alone, so that the commit adds (lo, hi) parts of both kinds with carries; and the narrow path at
    its documented worst case, 65536 products of 2^46 in one int64: R against R is 2^62 per chunk, L against L nearly, at lags -1 .. 1"""
    r, w, L = full24, wide, 300
    n = r.ns
    assert n == CHUNK + 2 * S
    x = r.full[0].astype(np.int64)
    met = []
    for S0 in (-20000, -64000, -66000):
        h = haystack(w.full[0], S0, 0, L, n)
        met.append([any(wd for _, _, wd in sub_tiles(x, h, l0, c)) for c in (0, 1) for l0 in (0, 256)])
    assert met == [[True, True, False, False], [True, True, True, True], [False, False, True, True]]
    edge = CHUNK + S
    y = r.full[1, :edge].astype(np.int64)
    assert int(np.dot(y[:CHUNK], y[:CHUNK])) == 1 << 62 and (y == -NARROW).all()           # a chunk's share: all that one int64 is documented to hold
    assert -(1 << 62) < int(np.dot(x[:CHUNK], x[1:CHUNK + 1])) < -(1 << 62) + (1 << 41)
    check(ctx, [probe(r, 0, n, w, 0, S0, L, [(0, 0), (1, 1), (0, 1)]) for S0 in (-20000, -64000, -66000)] +
               [probe(r, 0, edge, r, 0, -1, 3, [(0, 0), (0, 1), (1, 1)])])


def test_boundary_of_the_narrow_rule(ctx, wide, full24):
    """-2^23, the least a 24-bit RAW block holds, is narrow; the wide-value stream's channel 0 grows through 2^23 between samples 1034 and
    1035, and its wide value of smallest magnitude is sample 2417, among wide neighbours.  A needle of 16 samples of -2^23 against
    haystack ranges that end just before and just behind each of the two: by the rule the first range is summed in one int64 and the
    other three in (lo, hi); the reference decides all four"""
    r, w = full24, wide
    v = w.full.astype(np.int64)
    beyond = np.where(is_wide(v), np.abs(v), 1 << 40)
    ch, at = np.unravel_index(np.argmin(beyond), beyond.shape)
    assert is_wide(v).any() and (int(ch), int(at), int(v[ch, at])) == (0, 2417, -8391482) and NARROW < 8391482 < NARROW + 3000
    assert int(v[0, 1034]) == 8212517 <= NARROW < int(v[0, 1035]) == 8816126 and not is_wide(v[0, :1035]).any()
    needle = r.full[1, :16].astype(np.int64)
    assert (needle == -NARROW).all() and not is_wide(needle).any() and is_wide(needle - 1).all() and not is_wide(-needle).any() and is_wide(1 - needle).all()
    ranges = [(1000, 20), (1000, 21), (2400, 2), (2400, 3)]           # (first_b, num_lags): the range ends at first_b + 16 + num_lags - 1
    assert [first + 16 + lags - 1 for first, lags in ranges] == [1035, 1036, 2417, 2418]
    paths = [sub_tiles(needle, haystack(v[0], first, 0, lags, 16), 0, 0) for first, lags in ranges]
    assert [[wd for _, _, wd in p] for p in paths] == [[False], [True], [True], [True]]
    assert int(paths[0][0][1].max()) == 8212517                  # (the narrow range's largest value lies 2 % below the bound)
    check(ctx, [probe(r, 0, 16, w, first, 0, lags, [(1, 0), (0, 0)]) for first, lags in ranges])


# ---- the call ----
def test_group_frames_never_change_a_byte(ctx, streams):
    t, u = streams[2], streams[3]
    ps = [probe(t, 0, t.ns, u, 0, -100, 201, [(0, 0), (1, 2)]), probe(u, 10, 2000, t, 0, 50, 30, [(2, 1)])]
    bufs = [check(ctx, ps, group_frames=g) for g in (0, 1, 3)]
    assert np.array_equal(bufs[0], bufs[1]) and np.array_equal(bufs[0], bufs[2])


def test_many_probes_and_failures_stay_in_their_probe(ctx, product, streams):
    """64 probes of mixed specs, with damaged needles, damaged haystacks and argument errors among them: failing probes' tables stay
    sentinels, the others are right"""
    t, u, sm = streams[2], streams[3], streams["small"]
    (cdev, cidx, ck), (rdev, ridx, rk) = sc.damaged(ctx, product, t)
    try:
        ps, codes = [], []
        for i in range(64):
            a, b = ((t, u), (u, t), (sm, t), (t, t))[i % 4]
            ps.append(probe(a, (7 * i) % 100, 50 + (31 * i) % 500, b, (13 * i) % 500, -10 * (i % 9), 1 + (37 * i) % 300, [(i % 2, (i + 1) % 2)] * (1 + i % 3), a_sq=bool(i % 5)))
            codes.append(OK)
        first_bad = t.bl[ck][4]
        special = {3: (dict(num_lags=0), INVALID_ARGUMENT), 6: (dict(reserved=1), INVALID_ARGUMENT), 9: (dict(num_pairs=9), INVALID_ARGUMENT), 12: (dict(pair_stride=0), INVALID_ARGUMENT),
                   15: (dict(num_samples=1 << 40), INVALID_ARGUMENT), 18: (dict(first_a=1 << 33), INVALID_ARGUMENT), 21: (dict(d_stream_b=None), INVALID_ARGUMENT)}
        for i, (over, code) in special.items():
            ps[i]["over"].update(over)
            codes[i] = code
        # every argument error of a probe's own (test_stream_lags_cpu.BAD), on probes 40 to 59: their tables and a_sq stay sentinels
        assert len(BAD) == 20
        for i, (fields, word) in enumerate(BAD, 40):
            a, b = ((t, u), (u, t))[i % 2]
            ps[i] = probe(a, 3, 10, b, 0, -5, 10, [(0, 0), (1, 1)])
            for k, v in fields.items():
                if k in ("chan_a", "chan_b"):
                    ps[i]["wrong_channel"] = (k, v)
                elif v == "four bytes on":
                    ps[i]["four_bytes_on"] = k
                elif k in ("index_a", "index_b"):
                    ps[i]["null_index"] = k
                else:
                    ps[i]["over"][k] = v
            codes[i], ps[i]["word"] = INVALID_ARGUMENT, word
        # the CRC-damaged copy as needle (a range over the damaged block) and as haystack; in front of the damage it is sound
        ps[24] = probe(t, first_bad + 5, 100, t, 0, 0, 4, [(0, 0)], dev_a=cdev, index_a=cidx)
        ps[27] = probe(u, 0, 100, t, first_bad, -50, 100, [(0, 0)], dev_b=cdev, index_b=cidx)
        ps[30] = probe(t, 0, 100, t, 0, 0, 4, [(0, 0)], dev_a=cdev, index_a=cidx)
        # the Rice-damaged copy: the device's check sets the fail word, needle and haystack
        r0 = t.bl[rk][4]
        ps[33] = probe(t, r0 + 10, 200, u, 0, 0, 8, [(1, 1)], dev_a=rdev, index_a=ridx)
        ps[36] = probe(u, 0, 200, t, r0, -10, 30, [(0, 1)], dev_b=rdev, index_b=ridx)
        ps[39] = probe(t, 0, 200, t, 0, 0, 8, [(1, 1)], dev_a=rdev, index_a=ridx)
        codes[33] = codes[36] = NG
        ret, got, buf, places = raw_lags(ctx, ps)
        codes[24] = codes[27] = got[24]                        # (the index's own code for its failing block, which must be a failure)
        assert got[24] not in (OK, INVALID_ARGUMENT) and got[27] == got[24]
        assert got == codes and ret == codes[3], (got, last_error(ctx))
        assert last_error(ctx).startswith("probe 3: LagWindowsDevice: num_lags 0")
        for i in range(40, 60):                                 # each alone: its own text
            ret1, got1, buf1, _ = raw_lags(ctx, [ps[i]])
            assert ret1 == INVALID_ARGUMENT and got1 == [INVALID_ARGUMENT] and last_error(ctx).startswith("probe 0: LagWindowsDevice: "), (i, last_error(ctx))
            assert (buf1 == SENTINEL).all(), i
        want = want_buffer(buf.shape[0], ps, codes, places)
        assert np.array_equal(buf, want)
    finally:
        cidx.close()
        ridx.close()


def test_launch_counts(ctx, streams):
    t, u = streams[2], streams[3]
    ctx.enable_timing(True)
    try:
        for ps in ([probe(t, 0, 100, u, 0, 0, 1, [(0, 0)])], [probe(t, i, 100 + i, u, 5 * i, -i, 1 + 20 * i, [(0, 0), (1, 1)]) for i in range(40)]):
            check(ctx, ps)
            assert ctx.last_launches(LAGS_KIND) == 1 and ctx.last_launches(COMMIT_KIND) == 1 and ctx.last_launches(PLACE_KIND) >= 1
            assert ctx.last_ms(LAGS_KIND) >= 0 and ctx.last_launches(KIND["OVERLAY_T_OVERLAY"]) <= 0 and ctx.last_launches(KIND["RELATE_T_RELATE"]) <= 0
    finally:
        ctx.enable_timing(False)


def test_the_call_among_its_siblings(ctx, streams):
    """the same probes before and after measure, quiet, mix, resample and overlay calls on one context: the same bytes, and right"""
    t, u = streams[2], streams[3]
    ps = [probe(t, 0, 3000, u, 0, -64, 129, [(0, 0), (1, 1)]), probe(u, 100, 900, t, 100, 0, 300, [(2, 0)])]
    first = check(ctx, ps)
    w = [(t.dev, t.index, 10, 2000)]
    ctx.measure_windows(w)
    ctx.quiet_windows(w, 100)
    ctx.mix_windows(w, ((1, 1),), shift=1)
    ctx.resample_windows(w, 3, 2)
    ctx.overlay_windows([(500, [(t.dev, t.index, 0, 500, 0, 1), (t.dev, t.index, 100, 400, 50, -1)])])
    assert np.array_equal(check(ctx, ps), first)
    ctx.relate_windows(w)
    check(ctx, ps[::-1])


def test_python_form_and_agreement_with_relate(ctx, streams):
    """lag_windows on the batch scaffold; at lag 0 of A == B, dot and b_sq of pair (c, c) are relate_windows' dot(c, c)"""
    t = streams[2]
    out = ctx.lag_windows([(t.dev, t.index, 100, 2000, t.dev, t.index, 100, -3, 7, None), (t.dev, t.index, 0, None, t.dev, t.index, 0, 0, 1, [(0, 1)])])
    want, e = expected_lags(t.full, 100, 2000, t.full, 100, -3, 7, [(0, 0), (1, 1)])
    assert np.array_equal(out[0].cpu(), want) and out[0].pairs == ((0, 0), (1, 1)) and out[0].lag_first == -3
    assert out[0].a_squares() == [(int(h) << 64) + int(l) for l, h in e]
    rel = linne_amd.relation_dots(ctx.relate_windows([(t.dev, t.index, 100, 2000)])[0])
    dots, energies = linne_amd.lag_dots(out[0]), linne_amd.lag_energies(out[0])
    for c in range(2):
        assert dots[c][3] == energies[c][3] == out[0].a_squares()[c] == rel[linne_amd.pair_index(2, c, c)][0]
    assert linne_amd.best_lag(out[0]) == (0, 1.0) and linne_amd.lag_correlation(out[0])[:, 3].tolist() == [1.0, 1.0]
    assert linne_amd.lag_dots(out[1])[0][0] == linne_amd.relation_dots(ctx.relate_windows([(t.dev, t.index, 0, None)])[0])[linne_amd.pair_index(2, 0, 1)][0]
    with pytest.raises(ValueError):
        ctx.lag_windows([(t.dev, t.index, 0, None, t.dev, t.index, 0, 0, 65537, None)])
    with pytest.raises(ValueError):
        ctx.lag_windows([(t.dev, t.index, 0, None, t.dev, t.index, 0, 0, 1, [(0, 2)])])
    res, codes = ctx.lag_windows([(t.dev, t.index, 0, 10, t.dev, t.index, 0, 0, 1, None)], return_codes=True)
    assert codes == [OK] and res[0] is not None


def test_align_streams_finds_a_known_delay(ctx, streams):
    """a stream and a copy delayed by 1234 samples through splice_streams: the lag is 1234, the coefficient 1.0, and overlaying the
    pair at that offset with gains +1 and -1 gives zeros on the overlap"""
    import torch
    a = streams[2]
    # the 1234 samples in front are samples of the same stream from further on, which the needle does not reach
    delayed = ctx.splice_streams([[(a.dev, a.index, 1700, 1234), (a.dev, a.index, 0, None)]])[0]
    (lag, r), = ctx.align_streams([(a.dev, delayed)], 2000, needle=(0, 1500))
    assert (lag, r) == (1234, 1.0)
    x = ctx.index_stream(delayed)
    try:
        n = a.ns
        pcm = ctx.overlay_windows([(lag + n, [(a.dev, a.index, 0, n, lag, 1), (delayed, x, 0, lag + n, 0, -1)])])[0]
        assert not pcm[:, lag:].any().item() and torch.equal(pcm[:, :lag].cpu(), -torch.from_numpy(a.full[:, 1700:1700 + 1234]))
    finally:
        x.close()
    with pytest.raises(ValueError):
        ctx.align_streams([(a.dev, delayed)], 40000)
