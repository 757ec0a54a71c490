"""GPU tests of the resident-stream calls at sample positions up to 2^32 - 1, all that a .lnn header's 32-bit sample count allows
(include/linne_amd.h: the windows calls, LINNEAmd_StreamIndexesCreate, LINNEAmd_SpliceStreamsDevice).  Two streams of N = 2^32 - 1
samples (tests/far_streams.py: SILENT blocks of 65535 samples, an island of oracle-encoded blocks across 2^31 and one 70000 samples
before the end, then the header's tail) are held to references that never allocate such a stream: for windows of a few thousand samples
the sibling tests' references on a dense slice of the virtual decode, for windows of billions of samples the walks over its runs of zeros
and PCM.  No expected value comes from the library under test, and everything is equal or the test fails: bytes and integers, no
tolerance.  tests/test_far_streams_cpu.py holds the builder and those references to the oracle and to zlib."""
import numpy as np
import pytest

import far_streams as fs
import linne_amd
import splice_cases
import stream_consumers as sc
from far_streams import A_START, B_START, ISLAND_SAMPLES, N32, SHAPES
from mix_refs import expected_mix, random_matrix
from overlay_refs import fade_ref
from resample_refs import random_coef, resampled_length
from signals import music
from stream_consumers import CONSUMERS, encoded, last_error, to_device
from stream_refs import expected_compare
from synth_records import silent_block
import test_gpu_stream_mix as tmix
import test_gpu_stream_overlay as tov
import test_gpu_stream_quiet as tq
import test_gpu_stream_resample as trs

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT = 0, 1
NAMES = tuple(SHAPES)
LAYS = trs.LAYS
HALF = 1 << 31
MASK64 = (1 << 64) - 1
LONG_WINDOWS = [(0, N32), (1, N32 - 2), (HALF - 70000, 70000 + (1 << 30))]
LONG_BUCKETS = [0, (1 << 30) + 1, HALF, 65535 * 1024]


class FarTrack:
    """a far stream on the device: its description (far_streams.Far), its virtual decode and its index"""

    def __init__(self, name, d, dev, index):
        self.name, self.d, self.pcm, self.dev, self.index = name, d, d.pcm, dev, index
        self.nch, self.bits, self.ns = d.nch, d.bits, d.total


class View:
    """a dense piece of a far stream's decode, as the sibling tests' references read a track"""

    def __init__(self, t, full):
        self.full, self.nch, self.bits, self.dev, self.index, self.name = full, t.nch, t.bits, t.dev, t.index, t.name


@pytest.fixture(scope="module")
def far(ctx, oracle):
    made = {name: fs.full_scale(oracle, name) for name in NAMES}
    devs = [to_device(made[name][0]) for name in NAMES]
    indexes = ctx.index_streams(devs)                           # both in one call
    out = {name: FarTrack(name, made[name][1], dev, x) for name, dev, x in zip(NAMES, devs, indexes)}
    yield out
    for t in out.values():
        t.index.close()


def places(d):
    """the windows of modest length at far positions: (first, n)"""
    la = ISLAND_SAMPLES
    k = max(i for i, f in enumerate(d.tables[1][:-1]) if f <= 3 << 30)          # the SILENT block that holds sample 3 * 2^30
    assert d.tables[3][k] == 1 and d.tables[4][k] == 65535
    spans = [(HALF - 7, 40), (HALF, 33), (HALF + 1, 500),                     # around 2^31
             (A_START - 100, 300), (A_START + la - 200, 450), (B_START - 50, 1200), (B_START + la - 100, 300),      # across the islands' edges
             (N32 - 40, 40), (N32 - 3001, 3001), (d.covered + 1000, 777), (d.covered - 100, 300),                   # the end, the tail, into the tail
             (d.tables[1][k] + 100, 1000), (A_START, la), (0, 50)]
    assert spans[-3][0] + 1000 <= d.tables[1][k + 1] and all(a + n <= N32 for a, n in spans)
    return spans


def held(raw, want, ctx, call_items, ref_items):
    """a sibling test's scaffold on windows at far positions: call_items name the far stream, ref_items the same windows on dense views;
    at group_frames 0 and 2 the codes, every byte of the sentinel-filled buffer and the saturated words are the reference's"""
    first = None
    for gf in (0, 2):
        ret, codes, buf, offs, sats = raw(ctx, call_items, gf)
        assert ret == OK and codes == [OK] * len(call_items), (gf, codes, last_error(ctx))
        wbuf, wsats = want(ref_items, codes, offs, len(buf))
        if buf != wbuf:
            bad = next(i for i in range(len(buf)) if buf[i] != wbuf[i])
            j = max(k for k in range(len(offs)) if offs[k] <= bad) if bad >= offs[0] else -1
            raise AssertionError(f"group_frames {gf}: byte {bad} (window {j} begins at {offs[j] if j >= 0 else 0}) is {buf[bad]:#x}, not {wbuf[bad]:#x}")
        assert sats == wsats, (gf, sats, wsats)
        assert first is None or buf == first
        first = buf


# 1 ------------------------------------------------------------------------------------------------------------------------------
def test_index_in_one_call_and_alone(ctx, far):
    for t in far.values():
        alone = ctx.index_stream(t.dev)
        off, first, size, typ, nsmp = t.d.tables
        for x in (t.index, alone):
            assert x.header["num_samples"] == N32 and x.header["num_samples_per_block"] == 65535 and x.num_blocks == len(off) and x.failure() == (-1, OK, 0)
            got = x.blocks()
            for g, w in zip(got, (off, first, size, typ, nsmp)):
                assert g.dtype in (np.uint64, np.uint32) and np.array_equal(g.astype(np.uint64), np.array(w, dtype=np.uint64))
        assert int(t.index.blocks()[1][-1]) == t.d.covered > 3 << 30
        alone.close()


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_decode_windows_at_far_positions(ctx, far, name):
    """decode_windows in every sample format and the single range call; the reference's conversions are the mix reference's under the
    identity matrix"""
    import torch
    t = far[name]
    spans = places(t.d)
    wins = [(t.dev, t.index, a, n) for a, n in spans]
    eye = np.eye(t.nch, dtype=np.int16)
    dense = [t.pcm.slice(a, n) for a, n in spans]
    assert sum(1 for x in dense if x.any()) >= 8 and sum(1 for x in dense if not x.any()) >= 4
    for kw, fmt, last in (({}, "s32", False), ({"dtype": torch.int16, "channels_last": True}, "s16", True), ({"s24": True}, "s24", False),
                          ({"dtype": torch.float32, "channels_last": True}, "f32", True), ({"dtype": torch.int16}, "s16", False), ({"dtype": torch.float32}, "f32", False)):
        for gf in (0, 2):
            got, sats = ctx.decode_windows(wins, group_frames=gf, return_saturated=True, **kw)
            for (a, n), x, g, s in zip(spans, dense, got, sats):
                want, wsat = expected_mix(x, 0, n, eye, 0, 0, fmt, t.bits)
                have = g.cpu().numpy()
                have = np.moveaxis(have, 0, 1) if last else have
                assert have.shape == want.shape and have.dtype == want.dtype and have.tobytes() == np.ascontiguousarray(want).tobytes() and s == wsat, (a, n, fmt, gf)
    for (a, n), x in zip(spans, dense):
        assert np.array_equal(ctx.decode_stream(t.dev, a, n, index=t.index).cpu().numpy(), x), (a, n)
    assert np.array_equal(ctx.decode_stream(t.dev, N32 - 40, None, index=t.index).cpu().numpy(), np.zeros((t.nch, 40), dtype=np.int32))
    for a, n in ((N32, 1), (N32 - 5, 6)):            # beyond the stream: refused, as anywhere
        with pytest.raises(linne_amd.LinneAmdError) as e:
            ctx.decode_stream(t.dev, a, n, index=t.index)
        assert e.value.code == INVALID_ARGUMENT


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_mix_windows_at_far_positions(ctx, far, name):
    t = far[name]
    rng = np.random.default_rng(31)
    call, ref = [], []
    for k, (a, n) in enumerate(places(t.d)):
        Co = (1, 2, 3, 8)[k % 4]
        fmt, lay, pad = LAYS[k % len(LAYS)]
        kw = dict(matrix=random_matrix(rng, Co, t.nch), Co=Co, shift=15, clip_bits=(0, 24, 16)[k % 3], fmt=fmt, lay=lay, pad=pad)
        call.append(tmix.item(t, a, n, **kw))
        ref.append(tmix.item(View(t, t.pcm.slice(a, n)), 0, n, **kw))
    held(tmix.raw_mix, tmix.want_mix, ctx, call, ref)


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_compare_windows_reports_64_bit_positions(ctx, far, name):
    """held PCM that differs in a few elements: first_sample is the position in the stream, whatever it takes to write it"""
    import torch
    t = far[name]
    rng = np.random.default_rng(32)
    wins, want = [], []
    for k, (a, n) in enumerate(places(t.d)):
        x = t.pcm.slice(a, n)
        heldpcm = x.copy()
        for _ in range(k % 4):                                      # none, one, two or three elements
            heldpcm[int(rng.integers(0, t.nch)), int(rng.integers(n // 2, n))] += int(rng.integers(1, 9))
        cnt, s, ch = expected_compare(x, 0, n, heldpcm)
        want.append((cnt, a + s if cnt else 0, ch))
        wins.append((t.dev, t.index, a, n, torch.from_numpy(heldpcm).cuda()))
    assert sum(1 for w in want if w[1] >= HALF) >= 6 and sum(1 for w in want if w[1] >= 3 << 30) >= 3 and any(w[0] == 0 for w in want)
    for gf in (0, 2):
        assert ctx.compare_windows(wins, group_frames=gf) == want, gf


# 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [(1, 1), (147, 160), (160, 147), (1, 2)], ids=lambda r: "%d/%d" % r)
def test_resample_windows_at_far_positions(ctx, far, ratio):
    """windows of output samples where the islands' edges land, 64 taps, so that the halo reaches across an edge into zeros; 160/147:
    output positions above 2^32, the last output of the resampled stream, and a halo that reaches behind sample N"""
    up, down = ratio
    taps, before = 64, 31
    call, ref, k = [], [], 0
    for t in far.values():
        rng = np.random.default_rng(1000 * up + down + t.nch)
        coef = random_coef(rng, up, taps)
        L = resampled_length(N32, up, down)
        assert (L > 1 << 32) == (up > down)
        edges = [A_START, A_START + ISLAND_SAMPLES, B_START, B_START + ISLAND_SAMPLES, HALF]
        spans = [(e * up // down - 50, 100) for e in edges] + [(L - 60, 60), (L - 1, 1), (A_START * up // down + 300, 700), (0, 20)]
        for m0, n in spans:
            fmt, lay, pad = LAYS[k % len(LAYS)]
            k += 1
            full, local = fs.resample_view(t.pcm, m0, n, up, down, before, taps)
            kw = dict(coef=coef, up=up, down=down, before=before, shift=15, clip_bits=(0, 24)[k % 2], fmt=fmt, lay=lay, pad=pad)
            call.append(trs.item(t, m0, n, **kw))
            ref.append(trs.item(View(t, full), local, n, **kw))
        last = (L - 1) * down // up                                 # the last output's input sample: its halo reaches behind N
        assert last - before + taps > N32 and (up <= down or spans[2][0] > 1 << 32)
    held(trs.raw_resample, trs.want_resample, ctx, call, ref)


# 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_overlay_windows_at_far_positions(ctx, far, name):
    """sources from island A and island B laid over each other; a source of 65537 samples across 2^31 under the full ramp 32767 .. -32768;
    every `at` is ordinary while every first_sample is far"""
    t = far[name]

    def both(n_out, sources, **kw):
        call = tov.item(n_out, [tov.src(t, a, n, at, gain) for a, n, at, gain in sources], **kw)
        ref = tov.item(n_out, [tov.src(View(t, t.pcm.slice(a, n)), 0, n, at, gain) for a, n, at, gain in sources], **kw)
        return call, ref
    ramp = fade_ref(32767, -32768, 65536)
    pairs = [both(3500, [(A_START - 100, 3400, 0, 3), (B_START - 50, 3300, 60, -2)], shift=1, fmt="s32", lay="planar", pad=5),
             both(3300, [(B_START - 7, 3300, 0, 16384), (A_START + 5, 3000, 300, 16384), (N32 - 1000, 1000, 2300, 7)], shift=15, clip_bits=16, fmt="s16", lay="interleaved"),
             both(65537, [(HALF - 40000, 65537, 0, ramp)], shift=15, fmt="s24", lay="planar", pad=1),
             both(65600, [(HALF - 40000, 65537, 63, ramp), (N32 - 65537, 65537, 0, fade_ref(-32768, 32767, 65536))], shift=14, clip_bits=24, fmt="f32", lay="interleaved"),
             both(1200, [(HALF - 600, 1200, 0, -32768)], fmt="s32", lay="strided", pad=2)]
    held(tov.raw_overlay, tov.want_overlay, ctx, [c for c, _ in pairs], [r for _, r in pairs])


# 7 ------------------------------------------------------------------------------------------------------------------------------
def far_table(name, pcm, bits, first, n, *fields):
    """consumer `name`'s table of a window of any length, as stream_consumers.want_buffer takes it: int64 (rows, buckets, words)"""
    if name == "measure":
        return sc.measure_words(fs.far_measure(pcm, first, n, *fields))
    if name == "digest":
        return sc.digest_words([[(crc, 0, size) for crc, size in fs.far_digest(pcm, bits, first, n, *fields)]])
    if name == "histogram":
        bins, shift, scale, b = fields
        return np.array(fs.far_histogram(pcm, first, n, bins, shift, bool(scale), b), dtype=np.int64)
    return sc.relate_words([[tuple(r) for r in row] for row in fs.far_relate(pcm, first, n, *fields)])


def long_call(ctx, name, t, windows, group_frames=(0, 2)):
    """windows: (first, n, the spec's own fields ...) -> the tables as Python integers [window] (rows, buckets, words), held byte for
    byte to the reference between sentinels"""
    c = CONSUMERS[name]._replace(table=lambda tr, first, n, *f: far_table(name, tr.pcm, tr.bits, first, n, *f))
    items = [(t.dev, t.index, a, n, t.nch, *f, None) for a, n, *f in windows]
    want = None
    for gf in group_frames:
        ret, codes, buf, offs, nbs = sc.raw_call(c, ctx, items, group_frames=gf)
        assert ret == OK and codes == [OK] * len(items), (gf, codes, last_error(ctx))
        assert all(nb == sc.num_buckets(it[3], it[4 + c.fields]) <= 4096 for nb, it in zip(nbs, items))
        want = sc.want_buffer(c, len(buf), items, [t] * len(items), codes, offs, nbs) if want is None else want
        bad = np.flatnonzero(buf != want)
        if bad.size:
            j = max(k for k in range(len(offs)) if offs[k] <= bad[0]) if bad[0] >= offs[0] else -1
            raise AssertionError(f"{name}, group_frames {gf}: word {int(bad[0])} (window {j}: {windows[j] if j >= 0 else None}, its table begins at {offs[j] if j >= 0 else 0}) is "
                                 f"{int(buf[bad[0]]) & MASK64:#x}, not {int(want[bad[0]]) & MASK64:#x}")
    return [c.table(t, it[2], it[3], *it[5:5 + c.fields]) for it in items]


def long_windows(extra=()):
    return [(a, n, *e, b) for a, n in LONG_WINDOWS for b in LONG_BUCKETS for e in (extra or [()])]


@pytest.mark.parametrize("name", NAMES)
def test_measure_long_windows(ctx, far, name):
    """the sums come from the islands, min and max are pulled to 0 by the zeros, the last bucket is ragged"""
    t = far[name]
    tables = long_call(ctx, "measure", t, long_windows())
    whole = tables[0].view(linne_amd.MEASURE_DTYPE).reshape(t.nch)      # [0, N), one bucket
    loud = np.concatenate([p for _, _, _, p in t.d.islands], axis=1).astype(np.int64)
    assert [int(v) for v in whole["sum"]] == [int(v) for v in loud.sum(axis=1)] and (whole["min"] < 0).all() and (whole["max"] > 0).all()
    split = tables[2].view(linne_amd.MEASURE_DTYPE).reshape(t.nch, 2)   # bucket 2^31: island A lies in both buckets
    assert (split["min"] < 0).all() and (split["max"] > 0).all() and N32 % HALF == HALF - 1


@pytest.mark.parametrize("name", NAMES)
def test_histogram_long_windows(ctx, far, name):
    """bin 0 of the whole stream is N less the islands' non-zero samples: within a few thousand of 2^32 - 1, where the 32-bit slots' sum
    must not wrap; with buckets of 2^31 the two bin-0 counts lie on either side of 2^31"""
    t = far[name]
    tables = long_call(ctx, "histogram", t, long_windows([(64, t.bits - 6, 0), (33, 0, 1)]))
    loud = np.concatenate([p for _, _, _, p in t.d.islands], axis=1)
    for ch in range(t.nch):
        for k in (0, 1):                                        # [0, N), one bucket, linear and log2
            assert int(tables[k][ch, 0, 0]) >= N32 - int((loud[ch] != 0).sum()) > N32 - 7000 and int(tables[k][ch, 0].sum()) == N32
        assert int(tables[1][ch, 0, 0]) == N32 - int((loud[ch] != 0).sum())
        two = tables[5][ch]                                     # [0, N), buckets of 2^31, log2
        assert two.shape == (2, 33) and int(two[0, 0]) > HALF - 2000 and int(two[0].sum()) == HALF and int(two[1, 0]) < HALF and int(two[1].sum()) == HALF - 1


@pytest.mark.parametrize("name", NAMES)
def test_relate_long_windows(ctx, far, name):
    """num_equal and num_opposite near 2^32"""
    t = far[name]
    tables = long_call(ctx, "relate", t, long_windows())
    whole = tables[0].view(linne_amd.RELATION_DTYPE).reshape(-1)
    assert (whole["num_equal"] > N32 - 7000).all() and (whole["num_opposite"] > N32 - 7000).all() and int(whole["num_equal"][0]) == N32


@pytest.mark.parametrize("name", NAMES)
def test_digest_long_windows(ctx, far, name):
    """num_bytes of 2^34 and more; the islands' terms carried over 2^33 bytes and more; the length term at bytes >= 2^32; and windows
    whose distance R from island A's end to the bucket's end is v * 256^k bytes, one non-zero byte at k = 0 .. 4 where the frame's
    bytes allow it (4 at 16 bits stereo: 4 * 256^k, 256^4; 9 at 24 bits and three channels: 9 * 256^k, and no R of one non-zero byte
    at k = 4 fits the stream, so that shape takes 2^32 + 5 bytes there)"""
    t = far[name]
    F = t.nch * ((t.bits + 7) // 8)
    end = A_START + ISLAND_SAMPLES
    if F == 4:
        dist = [1, 256, 65536, 1 << 24, 1 << 30, (1 << 30) + 1 + 65536]
        assert [d * F for d in dist[:5]] == [4, 4 << 8, 4 << 16, 4 << 24, 1 << 32]
    else:
        dist = [1, 256, 65536, 1 << 24, 477218589, 5 << 28]               # (477218589 * 9 = 2^32 + 5)
        assert [d * F for d in dist[:4]] == [9, 9 << 8, 9 << 16, 9 << 24] and dist[4] * F >= 1 << 32
    windows = long_windows() + [(A_START + 10, ISLAND_SAMPLES - 10 + d, 0) for d in dist] + [(end - 1, 1 + d, 0) for d in dist]
    assert all(a + n <= N32 for a, n, _ in windows)
    tables = long_call(ctx, "digest", t, windows)
    assert int(tables[0][0, 0, 1]) == N32 * F >= (1 << 34) - 4 and (N32 - end) * F >= (1 << 33) - (1 << 13)      # (2^34 - 4 bytes at four bytes a frame)


# 8 ------------------------------------------------------------------------------------------------------------------------------
QUIET_FROM_ZERO = N32
"""the quiet window from sample 0: the whole stream"""


@pytest.mark.parametrize("name", NAMES)
def test_quiet_over_the_whole_stream(ctx, far, name):
    """threshold 0 over [0, N): a run from 0 to island A, one between the islands and one from the last loud sample to N, each longer
    than 2^31 or nearly, with lead_samples, trail_samples and quiet_samples to match; threshold 2^31: one run of N; and a capacity
    the runs overflow.  The window is the whole stream: its mask of one bit per frame is 512 MiB of the context's scratch."""
    t = far[name]
    n = QUIET_FROM_ZERO
    assert n > HALF + (1 << 30)
    want = fs.far_quiet(t.pcm, 0, n, 0, 1)
    runs = want[0]
    assert runs[0] == (0, A_START) and runs[-1][0] + runs[-1][1] == n and runs[-1][1] > 60000 and want[3] == A_START and want[2] > N32 - 7000
    between = max(r[1] for r in runs[1:-1])
    assert between > HALF - 80000
    three = fs.far_quiet(t.pcm, 0, n, 0, 3000)
    ahead = fs.far_quiet(t.pcm, 0, B_START, 0, 1)               # ends in front of island B: trail_samples is the run between the islands
    assert ahead[4] == between and ahead[3] == A_START
    for m, thr, mn, cap, wanted in ((n, 0, 1, 64, want), (n, 0, 3000, 2, three), (n, 1 << 31, 1, 4, ([(0, n)], 1, n, n, n)), (n, 0, 1, 1, want), (B_START, 0, 1, 64, ahead)):
        ret, codes, answers, buf, offs = tq.raw_call(ctx, [(t.dev, t.index, 0, m, thr, mn, cap, None)])
        assert (ret, codes) == (OK, [OK]), last_error(ctx)
        assert answers == [tuple(wanted[1:])], (m, thr, mn, cap)
        assert np.array_equal(buf, tq.want_buffer(len(buf), offs, [wanted[0][:cap]])), (m, thr, mn, cap)
    assert len(three[0]) == 3 > 2 and all(r[1] > HALF - 80000 or r[0] > B_START for r in three[0])


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_splice_at_the_limit(ctx, oracle):
    """a stream of 65536 SILENT blocks of 65535 samples, cut whole and once more for one block: exactly 2^32 - 1 samples; one sample
    more is refused"""
    K = 65536
    src = fs.header(1, K * 65535, 16, 65535, 0, False) + silent_block(65535) * K
    assert K * 65535 + 65535 == N32
    dev = to_device(src)
    index = ctx.index_stream(dev)
    assert index.num_blocks == K and index.header["num_samples"] == K * 65535
    tables = splice_cases.blocks_of(src)
    plan = lambda last: splice_cases.numpy_plan([splice_cases.PlanStream(tables, K * 65535, channels=1, block=65535, ms=0)], [([(0, 0, K * 65535), (0, 0, last)], 1 << 30, 0)], [])[0][0]
    assert plan(65535)["result"] == OK and plan(65535)["total_samples"] == N32
    refused = plan(65536)
    assert (refused["result"], refused["why"]) == (INVALID_ARGUMENT, splice_cases.WHY["total"])
    out, codes = ctx.splice_streams([[(dev, index, 0, K * 65535), (dev, index, 0, 65535)], [(dev, index, 0, K * 65535), (dev, index, 0, 65536)]], return_codes=True)
    assert codes == [OK, refused["result"]] and out[1] is None and "2^32" in last_error(ctx)
    assert ctx.last_splice_blocks[0] == (K + 1, 0)
    joined = bytes(out[0].cpu().numpy())
    assert joined == fs.header(1, N32, 16, 65535, 0, False) + silent_block(65535) * (K + 1)
    x = ctx.index_stream(out[0])
    assert x.header["num_samples"] == N32 and x.num_blocks == K + 1 and int(x.blocks()[1][-1]) == N32 and x.failure() == (-1, OK, 0)
    for b in (0, HALF):
        m = ctx.measure_windows([(out[0], x, 0, None)], bucket_samples=b)[0].cpu()
        assert m.shape == (1, 2 if b else 1) and not m["min"].any() and not m["max"].any() and not m["sum"].any() and not m["sumsq_lo"].any() and not m["sumsq_hi"].any()
    x.close()
    index.close()


# 10 -----------------------------------------------------------------------------------------------------------------------------
def test_history_on_a_fresh_context(oracle, far):
    """a long-window measure, the far places, a long-window histogram, an ordinary short stream's places, the far places again: one
    context, and no answer depends on what it did before"""
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        t = far["far16"]
        index = c.index_stream(t.dev)
        spans = places(t.d)
        wins = [(t.dev, index, a, n) for a, n in spans]
        dense = [t.pcm.slice(a, n) for a, n in spans]
        m = c.measure_windows([(t.dev, index, a, n) for a, n in LONG_WINDOWS], bucket_samples=HALF)
        for (a, n), got in zip(LONG_WINDOWS, m):
            assert sc.measure_words(fs.far_measure(t.pcm, a, n, HALF)).tobytes() == np.ascontiguousarray(got.records.cpu().numpy()).tobytes()
        first = c.decode_windows(wins)
        h = c.histogram_windows([(t.dev, index, a, n) for a, n in LONG_WINDOWS], 64, shift=10, bucket_samples=65535 * 1024)
        for (a, n), got in zip(LONG_WINDOWS, h):
            assert np.array_equal(got.cpu(), np.array(fs.far_histogram(t.pcm, a, n, 64, 10, False, 65535 * 1024), dtype=np.int64))
        short = encoded(c, oracle, music(2, 3 * 1024 + 300, 16, seed=92), 16, 5, True, "short")
        got = c.decode_windows([(short.dev, short.index, 517, 1500), (short.dev, short.index, 0, short.ns)])
        assert np.array_equal(got[0].cpu().numpy(), short.full[:, 517:2017]) and np.array_equal(got[1].cpu().numpy(), short.full)
        again = c.decode_windows(wins, group_frames=2)
        for x, f, g in zip(dense, first, again):
            assert np.array_equal(f.cpu().numpy(), x) and np.array_equal(g.cpu().numpy(), x)
        short.index.close()
        index.close()
    finally:
        c.close()
