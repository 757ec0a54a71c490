"""GPU tests of LINNEAmd_LagWindowsDevice at sample positions up to 2^32 - 1, at its documented bounds -- 65536 lags, 8 pairs, 2^38
products a probe -- and with images that lie more than 4 GiB and more than 2^32 words behind the accumulators' base.  The streams are
tests/far_streams.py's two of 2^32 - 1 samples (an island of sound across 2^31, one 70000 samples before the end); every table is
far_streams.far_lag_table's, which walks the needle's runs of PCM and never allocates such a stream and which
tests/test_far_streams_cpu.py holds to lag_refs.expected_lags at reduced scale.  No expected value comes from the library under test;
every word of the sentinel-filled buffer must equal the reference's, at group_frames 0 and 2 alike."""
import numpy as np
import pytest

import far_streams as fs
import linne_amd
from far_streams import A_START as A, B_START as B, ISLAND_SAMPLES as LA, N32, SHAPES
from stream_consumers import KIND, last_error, to_device
from test_gpu_stream_far import FarTrack
from test_gpu_stream_lags import SENTINEL, probe, raw_lags

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, NG = 0, 1, 7
HALF = 1 << 31
NAMES = tuple(SHAPES)
MAX_LAGS, MAX_PRODUCTS = 65536, 1 << 38


@pytest.fixture(scope="module")
def made(oracle):
    return {name: fs.full_scale(oracle, name) for name in NAMES}


def tracks(c, made):
    devs = [to_device(made[name][0]) for name in NAMES]
    return {name: FarTrack(name, made[name][1], dev, x) for name, dev, x in zip(NAMES, devs, c.index_streams(devs))}


@pytest.fixture(scope="module")
def far(ctx, made):
    out = tracks(ctx, made)
    yield out
    for t in out.values():
        t.index.close()


def reference(q):
    return fs.far_lag_table(q["a"].pcm, q["first_a"], q["n"], q["b"].pcm, q["first_b"], q["lag_first"], q["num_lags"], q["pairs"])


def want_buffer(words, probes, codes, places, refs):
    """sentinels but the OK probes' tables and a_sq, as test_gpu_stream_lags.want_buffer lays them out"""
    buf = np.full(words, SENTINEL, dtype=np.int64)
    for q, code, (off, stride, sq), ref in zip(probes, codes, places, refs):
        if code != OK:
            continue
        table, e = ref
        w = np.ascontiguousarray(table).view(np.int64).reshape(len(q["pairs"]), q["num_lags"], 4)
        for p in range(len(q["pairs"])):
            buf[off + 4 * p * stride:off + 4 * (p * stride + q["num_lags"])] = w[p].reshape(-1)
        if sq is not None:
            buf[sq:sq + 2 * len(q["pairs"])] = e.view(np.int64).reshape(-1)
    return buf


def held(c, probes, codes=None, refs=None):
    """the call at group_frames 0 and 2: the codes, and every word of the buffer, are the reference's both times -> the references"""
    codes = [OK] * len(probes) if codes is None else codes
    refs = [reference(q) if code == OK else None for q, code in zip(probes, codes)] if refs is None else refs
    first = None
    for gf in (0, 2):
        ret, got, buf, places = raw_lags(c, probes, gf)
        assert got == codes and ret == next((x for x in codes if x != OK), OK), (gf, got, last_error(c))
        want = want_buffer(buf.shape[0], probes, codes, places, refs)
        bad = np.flatnonzero(buf != want)
        assert bad.size == 0, (gf, bad.size, bad[:4], buf[bad[:4]], want[bad[:4]], places)
        assert first is None or np.array_equal(buf, first)
        first = buf
    return refs


def dots_of(ref):
    """[pair][lag] Python integers of a reference table"""
    return [[(int(h) << 64) + int(l) for l, h in zip(row["dot_lo"], row["dot_hi"])] for row in ref[0]]


def test_lags_at_far_positions(ctx, far):
    """needles and haystacks on both sides of 2^31 and at the stream's end, in two stream shapes in one call; haystack ranges that run off
    the end at 2^32 - 1, that start before sample 0, that lie inside the stream although first_b alone is beyond it, and that miss it"""
    t16, t24 = far["far16"], far["far24"]
    ps = [probe(t16, A, LA, t16, A, -300, 601, [(0, 0), (1, 1), (0, 1)]),                                # island A against itself, across 2^31
          probe(t24, A, LA, t24, A, -300, 601, [(0, 0), (1, 1), (2, 2), (0, 1)]),
          probe(t16, A, LA, t24, B, -100, 400, [(0, 2), (1, 0)]),                                        # ... over the other stream's island B
          probe(t16, B - 50, 5000, t24, B, 0, MAX_LAGS, [(1, 2)]),                                       # 65536 lags, 535 samples off the end
          probe(t16, A, LA, t24, (1 << 32) + 5, -((1 << 32) + 5 - A) + 17, 300, [(0, 1)]),               # first_b beyond the stream, the range inside
          probe(t16, A, LA, t24, A, -A - 100, 300, [(0, 0)]),                                            # the range starts at -100
          probe(t16, A, LA, t24, (1 << 64) - 1, 5, 9, [(1, 2)]),                                         # the range misses the stream
          probe(t24, N32 - 40, 40, t16, B + LA - 10, -20, 50, [(0, 0)]), probe(t24, N32 - 1, 1, t16, A, 0, 100, [(2, 1)]),      # the tail
          probe(t16, B + LA - 5, 5, t24, N32 - 3, -2, 8, [(0, 0)], a_sq=False)]
    assert ps[3]["first_b"] + ps[3]["num_lags"] - 1 + ps[3]["n"] == N32 + 535
    refs = held(ctx, ps)
    loud = [any(any(row) for row in dots_of(r)) for r in refs]
    assert sum(loud) >= 4 and loud[:5] == [True] * 5 and not any(loud[5:8])
    assert sum(1 for q, l in zip(ps, loud) if l and q["first_b"] + q["lag_first"] + q["num_lags"] - 1 + q["n"] > HALF) >= 3
    assert all(int(e[0]) or int(e[1]) for r in refs[:7] for e in r[1])                                  # (a_sq is written whatever the haystack)


def bound_probes(far):
    t16, t24 = far["far16"], far["far24"]
    n = 1 << 22
    a = probe(t16, A - n // 2, n, t24, A - n // 2, -32768, MAX_LAGS, [(0, 0)])
    m = 1 << 19
    b = probe(t16, A - m // 2, m, t24, A - m // 2, -32768, MAX_LAGS, [(0, 0), (1, 1), (0, 2), (1, 2), (0, 1), (1, 0), (0, 0), (1, 1)])
    assert n * MAX_LAGS == m * MAX_LAGS * 8 == MAX_PRODUCTS == linne_amd.LAG_MAX_PRODUCTS and MAX_LAGS == linne_amd.LAG_MAX_LAGS
    return a, b


def test_lags_at_the_product_bound(ctx, far):
    """exactly 2^38 products a probe: 2^22 needle samples (64 chunks) under 65536 lags (256 lag tiles), and 2^19 under 65536 lags and 8
    pairs; one needle sample more is refused, and its table stays sentinels beside a right one"""
    a, b = bound_probes(far)
    over = probe(a["a"], a["first_a"], a["n"] + 1, a["b"], a["first_b"], a["lag_first"], a["num_lags"], a["pairs"])
    refs = held(ctx, [a, b])
    held(ctx, [over, a], codes=[INVALID_ARGUMENT, OK], refs=[None, refs[0]])
    assert "> 2^38 products" in last_error(ctx)
    # far16's island A slides over far24's, both at A: the dots are non-zero exactly at the lags where the two overlap, and their
    # peak lies among those (the two islands hold different music, so not at lag 0 of need)
    d = dots_of(refs[0])[0]
    lags = [l - 32768 for l, v in enumerate(d) if v]
    peak = max(range(MAX_LAGS), key=lambda l: abs(d[l])) - 32768
    assert d[peak + 32768] != 0 and -LA < min(lags) and max(lags) < LA and len(lags) > LA and abs(peak) < LA


def test_lags_with_images_beyond_4_GiB(made):
    """needles of 2^29 samples of the three-channel stream, 256 lags, 2 pairs: 2^38 products and 8192 chunks a probe.  The images lie in
    window order, a channel's words n rounded up to 4 apart: the first probe's haystack image begins 6 GiB behind the accumulators'
    base and its second channel behind word 2^31; the second probe's haystack image begins behind word 2^32, where a word offset no
    longer fits 32 bits.  On a context of its own, closed at the end, so that the suite's context does not keep the scratch: the first
    probe takes about 10 GiB of the device's memory for the length of this test, both take about 20 GiB.  With less than 16 GiB free
    the test is skipped; with less than 28 GiB the first probe runs alone."""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 16 << 30:
        pytest.skip("%.1f GiB of device memory free: the images take about 10 GiB" % (free / 2 ** 30))
    c = linne_amd.Context(0, use_torch_stream=False)
    far = tracks(c, made)
    try:
        t16, t24 = far["far16"], far["far24"]
        n, L = 1 << 29, 256
        ps = [probe(t24, A - n // 2, n, t16, A - n // 2, -128, L, [(2, 1), (0, 0)]), probe(t24, A - n // 2, n, t16, A - n // 2 + 100, -200, L, [(1, 0), (2, 1)])]
        assert n * L * 2 == MAX_PRODUCTS and n // 65536 == 8192
        # the plan's arithmetic (lnn_windows_plan.h wx_lag_image): the images of a call's windows follow each other, needle, haystack, ...
        img, at = [], 0
        for q in ps:
            for nch, m in ((3, n), (2, n + L - 1)):
                istride = (m + 3) // 4 * 4
                img.append((at, istride))
                at += nch * istride
        assert 4 * img[1][0] == 6 << 30 and img[1][0] < HALF < img[1][0] + img[1][1] and img[1][0] + img[1][1] > HALF and 4 * (img[0][0] + 2 * img[0][1]) == 1 << 32
        assert img[3][0] > 1 << 32 and 4 * at < 21 << 30
        if free < 28 << 30:
            ps = ps[:1]
        refs = held(c, ps)
        assert all(any(row) for r in refs for row in dots_of(r))
    finally:
        for t in far.values():
            t.index.close()
        c.close()


def test_too_many_tiles_are_refused(ctx, far):
    """32 probes of the whole stream, 1 lag, 8 pairs -- 2^35 products each -- are 2^24 tiles: a launch of 2^24 workgroups of 256 threads
    would have 2^32 threads, of which the device runs a part without a word.  The call is refused before any launch, and no table is
    touched.  (31 such probes are allowed; they would be minutes of work and are planned on the CPU alone, in
    tests/test_stream_lags_cpu.py.)"""
    t = far["far16"]
    ps = [probe(t, 0, N32, t, 0, 0, 1, [(k % 2, (k // 2) % 2) for k in range(8)], a_sq=False) for _ in range(32)]
    ctx.enable_timing(True)
    try:
        ctx.measure_windows([(t.dev, t.index, A, 100)])              # (the launches of the call before are another kind's)
        ret, codes, buf, places = raw_lags(ctx, ps)
        assert ret == NG and codes == [NG] * 32, (ret, codes, last_error(ctx))
        assert last_error(ctx) == "LagWindowsDevice: %d tiles of lags in one call: too many" % (1 << 24)
        assert (buf == SENTINEL).all() and buf.shape[0] > 32 * 8 * 4
        assert all(ctx.last_launches(KIND[k]) <= 0 for k in ("LAGS_T_LAGS", "LAGS_T_COMMIT", "T_WX_PLACE"))
    finally:
        ctx.enable_timing(False)
