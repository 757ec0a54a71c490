"""GPU tests of relating the channels of windows of resident .lnn streams (Context.relate_windows, relate_streams, correlation,
channel_findings, the command line tool's -R; include/linne_amd.h LINNEAmd_RelateWindowsDevice).  Every expected number is computed
with numpy and Python integers (relate_refs.expected_relate) from the oracle's decode of the same bytes, never from the library under
test, and everything must be equal.  Streams hold at most 8 blocks of 1024 samples, except the 48-block stream, the two 257-block
streams and the wide-value stream (6 blocks)."""
import os
import re
import subprocess

import numpy as np
import pytest

import linne_amd
import synth_records as sr
from relate_refs import CARRY_NS, CARRY_PEAK, bucket_lengths, carry_stereo_stream, dots, expected_relate, pairs
from signals import music
import stream_consumers as sc
from stream_consumers import Stream, crc_damaged, encoded
from stream_refs import mixed_signal
from test_cli_cpu import CLI
from test_stream_relate_cpu import WIDE_SHAPE, first_wide_frame, wide_cases

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CORRUPTION, NG = 0, 1, 6, 7
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300
SHAPES = [(nch, preset) for nch in (1, 2, 3) for preset in (0, 5)]
BUCKETS = [0, 1, 7, 64, 255, 256, 257, 1000, 1024, 5000]
RELATE = sc.CONSUMERS["relate"]


@pytest.fixture(scope="module")
def streams(ctx, oracle):
    """1, 2 (MS) and 3 channels, presets 0 and 5, 3 blocks and a tail of 300"""
    out = {(nch, preset): encoded(ctx, oracle, music(nch, 3 * S + TAIL, 16, seed=50 + 8 * nch + preset), 16, preset, nch == 2, f"{nch}ch -m {preset}")
           for nch, preset in SHAPES}
    yield out
    for t in out.values():
        t.index.close()


@pytest.fixture(scope="module")
def mixed(ctx, oracle):
    """stereo, 8 blocks: music, two SILENT, music, two RAW, music, a tail of 300"""
    t = encoded(ctx, oracle, mixed_signal(2, 16, 7 * S + TAIL, seed=11, block=S), 16, 5, True, "mixed")
    assert [b[2] for b in t.bl] == [COMPRESS, SILENT, SILENT, COMPRESS, RAW, RAW, COMPRESS, COMPRESS] and t.bl[-1][3] == TAIL
    yield t
    t.index.close()


def call(ctx, t, wins, buckets, **kw):
    return ctx.relate_windows([(t.dev, t.index, a, n) for a, n in wins], buckets, **kw)


def check(t, wins, buckets, got):
    for (first, n), b, r in zip(wins, buckets, got):
        want = expected_relate(t.full, first, n, b)
        have = r.cpu()
        assert have.shape == want.shape and have.dtype == linne_amd.RELATION_DTYPE, (t.name, first, n, b)
        if not np.array_equal(have, want):
            bad = np.argwhere(have != want)[0]
            raise AssertionError(f"{t.name}: window ({first}, {n}), bucket length {b}: pair {bad[0]} bucket {bad[1]} is {have[tuple(bad)]}, not {want[tuple(bad)]}")
        assert r.bucket_samples == b and r.num_channels == t.nch
        for name in ("dot_lo", "dot_hi", "num_equal", "num_opposite"):   # the tensors are views of the same records
            assert np.array_equal(getattr(r, name).cpu().numpy().view(want[name].dtype), want[name])
        # (float64 of the two words, rounded word by word: within two units in the last place of the exact sum's float64)
        assert np.allclose(r.dot().cpu().numpy(), np.array([[float(d) for d in row] for row in dots(want)], dtype=np.float64).reshape(want.shape), rtol=2.0 ** -51, atol=0)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,preset", SHAPES)
def test_exactness_over_buckets(ctx, streams, nch, preset):
    t = streams[(nch, preset)]
    # the whole stream; mid-block to mid-block; two samples across a block's edge; the last sample
    spans = [(0, t.ns), (517, 1500), (S - 1, 2), (t.ns - 1, 1)]
    wins = [w for w in spans for _ in BUCKETS]
    buckets = BUCKETS * len(spans)
    got = call(ctx, t, wins, buckets)
    check(t, wins, buckets, got)
    again = call(ctx, t, wins, buckets, group_frames=1)
    check(t, wins, buckets, again)
    one = ctx.relate_windows([(t.dev, t.index, 517, 1500)] * 2, 257)                               # one value for every window
    check(t, [(517, 1500)] * 2, [257] * 2, one)
    plain = ctx.relate_windows([(t.dev, t.index, 0, None)])                                        # the default: one bucket
    check(t, [(0, t.ns)], [0], plain)


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_eight_channels(ctx, oracle):
    """blocks of 256 frames of eight channels: 36 pairs, the kernel's LDS tables at their largest"""
    x = music(8, 3 * 256 + 100, 16, seed=77)
    x[5] = x[2]                                                  # a duplicate and an inverted stem among the eight
    x[7] = -x[1]
    t = Stream(ctx, oracle, oracle.encode_whole(x, 16, 44100, 256, 0, False), "8ch")
    assert np.array_equal(t.full, x) and len(t.bl) == 4 and len(pairs(8)) == 36
    wins = [(0, t.ns)] * 4 + [(3, t.ns - 5), (255, 300)]
    buckets = [0, 1, 100, 256, 100, 256]
    got = call(ctx, t, wins, buckets)
    check(t, wins, buckets, got)
    f, = linne_amd.channel_findings(got[0])
    assert {p for p, v in f["pairs"].items() if v == "identical"} == {(2, 5)} and {p for p, v in f["pairs"].items() if v == "inverted"} == {(1, 7)}
    t.index.close()


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_block_types(ctx, mixed):
    t = mixed
    bl = t.bl
    wins = [(0, t.ns)]
    for k in (0, 1, 2, 4, 5, 7):                                 # a window inside a block of every type, and across its ends
        wins += [(bl[k][4] + 10, bl[k][3] - 20), (bl[k][4] - 5 if k else 0, bl[k][3] + 10 if k < 7 else bl[k][3])]
    wins += [(bl[1][4] + 100, 2 * S - 150), (bl[2][4] + 500, 3 * S), (bl[4][4] + 3, 2 * S - 7), (bl[3][4] + 1000, 1 * S + 30), (t.ns - TAIL + 7, TAIL - 7)]
    for b in (0, 1, 100, 256, 300, 1000, 1025):                  # 100, 300, 1000, 1025: buckets straddle the blocks' boundaries
        check(t, wins, [b] * len(wins), call(ctx, t, wins, [b] * len(wins)))
    mix = [(0, 1, 100, 256, 300, 1000, 1025)[i % 7] for i in range(len(wins))]
    check(t, wins, mix, call(ctx, t, wins, mix, group_frames=2))
    # the SILENT blocks' zeros are equal and opposite in every pair
    r, = call(ctx, t, [(bl[1][4], 2 * S)], [0])
    assert r.cpu()["num_equal"].tolist() == [[2 * S]] * 3 and r.cpu()["num_opposite"].tolist() == [[2 * S]] * 3 and dots(r.cpu()) == [[0]] * 3


def test_zeros_behind_the_last_block(ctx, oracle, mixed):
    """the mixed stream cut behind its sixth block: the header names 7 * S + TAIL samples, the blocks hold 6 * S (the last of them
    RAW); the windows reaching beyond `covered` count the rest's zeros as equal and opposite"""
    u = Stream(ctx, oracle, mixed.stream[:mixed.bl[6][0]], "mixed, cut")
    cov = 6 * S
    assert u.ns == mixed.ns and len(u.bl) == 6 and np.array_equal(u.full[:, :cov], mixed.full[:, :cov]) and not u.full[:, cov:].any()
    wins = [(0, u.ns), (cov - 100, 400), (cov, S + TAIL), (cov + 300, 1), (cov - 1, 2), (4 * S + 5, 2 * S + 900), (u.ns - 1, 1)]
    for b in (0, 1, 64, 256, 333):
        got = call(ctx, u, wins, [b] * len(wins))
        check(u, wins, [b] * len(wins), got)
    assert int(got[2].cpu()["num_equal"].sum()) == int(got[2].cpu()["num_opposite"].sum()) == 3 * (S + TAIL)
    u.index.close()


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_signed_carries(ctx, oracle):
    """257 RAW blocks of 24-bit stereo, R = -L at full scale: dot(0, 1) below -2^64, dot(0, 0) above 2^64, all 64 slots in use"""
    c = Stream(ctx, oracle, carry_stereo_stream(oracle), "257 RAW blocks, R = -L")
    assert c.ns == CARRY_NS >= 64 * 4096 and all(b[2] == RAW for b in c.bl)
    wins = [(0, c.ns), (0, c.ns), (3, c.ns - 5)]
    buckets = [0, 1 << 18, 1 << 17]
    got = call(ctx, c, wins, buckets)
    check(c, wins, buckets, got)
    whole = got[0].cpu()
    assert dots(whole) == [[CARRY_NS * CARRY_PEAK ** 2], [-CARRY_NS * CARRY_PEAK ** 2], [CARRY_NS * CARRY_PEAK ** 2]]
    assert dots(whole)[1][0] < -(1 << 64) and dots(whole)[0][0] > 1 << 64
    assert (int(whole[1, 0]["num_opposite"]), int(whole[1, 0]["num_equal"])) == (CARRY_NS, 0)
    assert got[1].cpu().shape == (3, 2) and linne_amd.channel_findings(got[1])[1]["pairs"] == {(0, 1): "inverted"}
    assert linne_amd.correlation(got[0])[0, 1, 0] == -1.0
    c.index.close()


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_wide_values(ctx, oracle):
    """a 16-bit stream whose crafted blocks decode to values over all of int32: the products are folded as one int64 only in the waves
    whose values say so.  The windows end behind the stream's first wide frame, which is then alone in a narrow wave; the buckets cut
    the waves that mix wide and narrow values"""
    t = Stream(ctx, oracle, sr.case_stream(WIDE_SHAPE, wide_cases()), "wide values")
    mag = np.abs(t.full.astype(np.int64))
    assert t.nch == 2 and (mag.max(axis=1) >= 1 << 24).all() and mag.max() > 1 << 30
    f = first_wide_frame(t.full)
    wins = [(0, t.ns)] * 6 + [(f - 300, 301), (f - 63, 64), (f - 10, 11), (f, 1), (f - 300, 301), (f - 100, 400), (f - 1, 1000)]
    buckets = [0, 1, 64, 100, 1023, 256, 0, 0, 0, 0, 64, 37, 255]
    got = call(ctx, t, wins, buckets)
    check(t, wins, buckets, got)
    check(t, wins, buckets, call(ctx, t, wins, buckets, group_frames=2))
    t.index.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_slots(ctx, oracle):
    """48 COMPRESS blocks of stereo music in one bucket (8 slots); 257 blocks of 256 frames in one bucket, whose pieces go round all 64
    slots; buckets of 8192 on the same stream (2 slots each)"""
    t = encoded(ctx, oracle, music(2, 48 * S, 16, seed=83), 16, 0, True, "48 blocks")
    assert len(t.bl) == 48 and all(b[2] == COMPRESS for b in t.bl)
    wins = [(0, t.ns), (0, t.ns), (S + 7, 40 * S), (0, t.ns)]
    buckets = [0, 8192, 0, t.ns // 2]
    check(t, wins, buckets, call(ctx, t, wins, buckets))
    check(t, wins, buckets, call(ctx, t, wins, buckets, group_frames=5))
    t.index.close()
    x = music(2, 257 * 256, 16, seed=84)
    u = Stream(ctx, oracle, oracle.encode_whole(x, 16, 44100, 256, 0, True), "257 blocks of 256")
    assert np.array_equal(u.full, x) and len(u.bl) == 257 and u.ns >= 64 * 1024
    wins = [(0, u.ns), (0, u.ns), (5, u.ns - 9)]
    buckets = [0, 8192, 8192]
    check(u, wins, buckets, call(ctx, u, wins, buckets))
    u.index.close()


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_many_windows_and_failures_stay_in_their_window(ctx, product, streams, mixed):
    """64 windows over three streams (and damaged copies of one) with mixed bucket lengths, failing ones among them"""
    t = streams[(2, 5)]
    crc, rice = sc.damaged(ctx, product, t)
    (d_bad, bad_index, k), good = crc, (t.dev, t.index, 0, 1000, 2)
    special = {**sc.rice_windows(t, rice, [(100,), (7,), (441,)]),
               9: (d_bad, bad_index, t.bl[k][4] + 3, 600, 2, 100, None, CORRUPTION),               # CRC damage between good windows: refused on the host
               10: (d_bad, bad_index, 0, t.bl[k][4] - 24, 2, 64, None, OK),                        # in front of the damaged block
               11: (d_bad, bad_index, t.bl[k + 1][4], 200, 2, 0, None, CORRUPTION),                # behind it
               20: good + (256, "misaligned", INVALID_ARGUMENT),
               21: good + (100, "stride", INVALID_ARGUMENT),                                       # pair_stride one short
               22: good + (0, "null", INVALID_ARGUMENT),
               40: (t.dev, t.index, 1, t.ns, 2, 500, None, INVALID_ARGUMENT),                      # a range beyond the stream
               41: good + (1, None, OK)}
    sc.many_windows(RELATE, ctx, [streams[(2, 5)], streams[(3, 0)], mixed], t, lambda i: ((0, 3, 7, 64, 255, 256, 257, 441, 1000, 5000)[(i * 3 + i // 16) % 10],),
                    special, crc, rice)


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(mixed, streams):
    sc.launch_counts(RELATE, mixed, streams[(3, 0)], ((441,), {}), lambda t, w, r: check(t, [w], [441], [r]))


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_agreement_with_the_siblings(ctx, streams, mixed):
    """on the same windows: dot(i, i) is measure_windows' 128-bit sum of squares, num_equal(i, i) the bucket lengths, and
    num_opposite(i, i) bin 0 of histogram_windows (linear, shift 0)"""
    for t in (streams[(3, 5)], mixed):
        wins = [(t.dev, t.index, 0, t.ns), (t.dev, t.index, 517, 1500), (t.dev, t.index, S - 1, 2)]
        for b in (0, 100, 256):
            rel = ctx.relate_windows(wins, b)
            mea = ctx.measure_windows(wins, b)
            his = ctx.histogram_windows(wins, 2, 0, False, b)
            for (_, _, _, n), r, m, h in zip(wins, rel, mea, his):
                rc, mc, hc = r.cpu(), m.cpu(), h.cpu()
                for i in range(t.nch):
                    p = linne_amd.pair_index(t.nch, i, i)
                    assert np.array_equal(rc["dot_lo"][p], mc["sumsq_lo"][i]) and np.array_equal(rc["dot_hi"][p].astype(np.uint64), mc["sumsq_hi"][i])
                    assert rc["num_equal"][p].tolist() == bucket_lengths(n, b)
                    assert np.array_equal(rc["num_opposite"][p].astype(np.int64), hc[i, :, 0])


# 10 -----------------------------------------------------------------------------------------------------------------------------
def test_dual_mono_and_inverted_stereo(ctx, oracle):
    m = music(1, 2 * S + TAIL, 16, seed=5)
    m[0, 100:110] = 0                                            # (zeros are equal and opposite at once: they do not blur either finding)
    dual = encoded(ctx, oracle, np.concatenate([m, m]), 16, 2, True, "dual mono")
    inv = encoded(ctx, oracle, np.concatenate([m, -m]), 16, 2, False, "inverted")
    plain = encoded(ctx, oracle, music(2, 2 * S + TAIL, 16, seed=6), 16, 2, True, "stereo")
    half = encoded(ctx, oracle, np.concatenate([m, np.zeros_like(m)]), 16, 2, False, "right channel silent")
    names = {"dual mono": "identical", "inverted": "inverted", "stereo": None, "right channel silent": None}
    ts = [dual, inv, plain, half]
    for b in (0, 441):
        got = ctx.relate_streams([t.dev for t in ts], bucket_samples=b)
        check_whole = [np.array_equal(r.cpu(), expected_relate(t.full, 0, t.ns, b)) for t, r in zip(ts, got)]
        assert all(check_whole), check_whole
        for t, r in zip(ts, got):
            f = linne_amd.channel_findings(r)
            assert len(f) == len(bucket_lengths(t.ns, b)) and all(x["pairs"] == {(0, 1): names[t.name]} for x in f), t.name
            assert all(x["channels"] == {0: None, 1: "silent" if t.name == "right channel silent" else None} for x in f), t.name
        c = [linne_amd.correlation(r) for r in got]
        assert (c[0][0, 1] == 1.0).all() and (c[1][0, 1] == -1.0).all() and (np.abs(c[2][0, 1]) < 1.0).all() and np.isnan(c[3][0, 1]).all() and (c[3][0, 0] == 1.0).all()
    windowed = ctx.relate_windows([(dual.dev, dual.index, 50, 1000), (inv.dev, inv.index, 50, 1000)], 300)
    assert [x["pairs"][(0, 1)] for r in windowed for x in linne_amd.channel_findings(r)] == ["identical"] * 4 + ["inverted"] * 4
    assert ctx.relate_streams([]) == []
    many = ctx.relate_streams([dual.dev, inv.stream], bucket_samples=[441, 0], group_frames=1)      # bytes are taken too
    assert np.array_equal(many[0].cpu(), expected_relate(dual.full, 0, dual.ns, 441)) and np.array_equal(many[1].cpu(), expected_relate(inv.full, 0, inv.ns))
    for t in ts:
        t.index.close()


# 11 -----------------------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^(?:bucket (\d+) )?pair (\d+) (\d+): samples (\d+) dot (-?\d+) equal (\d+) opposite (\d+) correlation (-?\d+\.\d{6}|nan)( identical| inverted)? $")
SILENT_LINE = re.compile(r"^(?:bucket (\d+) )?channel (\d+): silent $")


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_command_line_tool(ctx, oracle, tmp_path, streams, mixed):
    path = tmp_path / "a.lnn"
    m = music(1, 2 * S + TAIL, 16, seed=5)
    inv = encoded(ctx, oracle, np.concatenate([m, -m]), 16, 2, False, "inverted")
    # a quiet inverted stream: small negative sums, whose high word is -1 and whose low word lies just below 2^64
    q = np.random.default_rng(8).integers(-10, 11, size=(1, 2 * S + TAIL)).astype(np.int32)
    q[0, :7] = (1, -1, 0, 0, 1, 0, -1)
    quiet = encoded(ctx, oracle, np.concatenate([q, -q]), 16, 2, False, "quiet, inverted")
    for t, b in ((mixed, 0), (mixed, 1024), (streams[(3, 0)], 441), (streams[(1, 5)], 0), (inv, 1000), (quiet, 441), (quiet, 7), (quiet, 0)):
        path.write_bytes(t.stream)
        r = subprocess.run([CLI, "-R", *([str(b)] if b else []), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        rel, = ctx.relate_windows([(t.dev, t.index, 0, t.ns)], b)
        assert np.array_equal(rel.cpu(), expected_relate(t.full, 0, t.ns, b))
        table, corr, found, lens = rel.cpu(), linne_amd.correlation(rel), linne_amd.channel_findings(rel), bucket_lengths(t.ns, b)
        want = []
        for k in range(len(lens)):
            for p, (i, j) in enumerate(pairs(t.nch)):
                want.append(("pair", k if b else None, i, j, lens[k], dots(table)[p][k], int(table[p, k]["num_equal"]), int(table[p, k]["num_opposite"]),
                             found[k]["pairs"].get((i, j))))
            want += [("silent", k if b else None, i) for i in range(t.nch) if found[k]["channels"][i]]
        got = []
        for line in r.stdout.splitlines():
            g, s = LINE.match(line), SILENT_LINE.match(line)
            assert g or s, line
            if s:
                got.append(("silent", None if s.group(1) is None else int(s.group(1)), int(s.group(2))))
                continue
            k, i, j = None if g.group(1) is None else int(g.group(1)), int(g.group(2)), int(g.group(3))
            got.append(("pair", k, i, j, int(g.group(4)), int(g.group(5)), int(g.group(6)), int(g.group(7)), g.group(9).strip() if g.group(9) else None))
            c = corr[i, j, k or 0]
            assert (g.group(8) == "nan") == bool(np.isnan(c)) and (np.isnan(c) or abs(float(g.group(8)) - c) <= 1e-6), line
            if t is quiet and i < j:                             # exactly inverted: -1 to the last printed digit, however small the sums
                assert g.group(8) == "-1.000000" and g.group(9) == " inverted" and -(1 << 20) < int(g.group(5)) < 0, line
        assert got == want, (t.name, b)
    inv.index.close()
    quiet.index.close()
    bad, k = crc_damaged(mixed)
    path.write_bytes(bad)
    r = subprocess.run([CLI, "-R", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and not r.stdout and f"block {k} " in r.stderr, r.stderr
