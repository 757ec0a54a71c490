"""GPU tests of mixing the channels of windows of resident .lnn streams (Context.mix_windows, remix_streams, the command line tool's -X;
include/linne_amd.h LINNEAmd_MixWindowsDevice).  Every expected element is computed with numpy int64 (mix_refs.expected_mix) from the
oracle's decode of the same bytes, never from the library under test, and everything must be equal: bytes and integers, no tolerance --
the float32 path is a conversion and a multiplication by a power of two.  Streams hold 3 to 6 blocks of 1024 samples."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import linne_amd
import synth_records as sr
from mix_refs import ELEMENT_BYTES, expected_mix, random_matrix
from signals import music
import stream_consumers as sc
from stream_consumers import DECODE_KINDS, KIND, Stream, encoded, last_error, to_device
from stream_refs import mixed_signal
from test_cli_cpu import CLI
from test_stream_relate_cpu import WIDE_SHAPE, wide_cases

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CORRUPTION, NG = 0, 1, 6, 7
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300
SENTINEL = 0x5A
FMT = {"s32": linne_amd.PCM_S32, "s16": linne_amd.PCM_S16, "s24": linne_amd.PCM_S24, "f32": linne_amd.PCM_F32}
MIX_KIND, PLACE_KIND = KIND["MIX_T_MIX"], KIND["T_WX_PLACE"]
IDENTITY = np.eye(8, dtype=np.int16)


@pytest.fixture(scope="module")
def streams(ctx, oracle):
    """1, 2 (MS), 3 and 8 channels: 3 blocks and a tail of 300"""
    out = {nch: encoded(ctx, oracle, music(nch, 3 * S + TAIL, 16, seed=90 + nch), 16, 5 if nch == 2 else 0, nch == 2, f"{nch}ch") for nch in (1, 2, 3, 8)}
    yield out
    for t in out.values():
        t.index.close()


@pytest.fixture(scope="module")
def cut(ctx, oracle):
    """stereo: music, two SILENT, music, two RAW blocks -- and a header that names 1324 samples more than the six blocks hold"""
    x = mixed_signal(2, 16, 7 * S + TAIL, seed=11, block=S)
    whole = bytes(oracle.encode_whole(x, 16, 44100, S, 5, True))
    t = Stream(ctx, oracle, whole[:sc.blocks(whole)[6][0]], "mixed, cut")
    assert [b[2] for b in t.bl] == [COMPRESS, SILENT, SILENT, COMPRESS, RAW, RAW] and t.ns == 7 * S + TAIL and not t.full[:, 6 * S:].any()
    yield t
    t.index.close()


@pytest.fixture(scope="module")
def wide(ctx, oracle):
    """a 16-bit stereo stream whose crafted blocks decode to values over all of int32"""
    t = Stream(ctx, oracle, sr.case_stream(WIDE_SHAPE, wide_cases()), "wide values")
    assert t.nch == 2 and np.abs(t.full.astype(np.int64)).max() > 1 << 30
    yield t
    t.index.close()


# ---- the C entry point on outputs that lie in one buffer of sentinels ----
def spec_of(matrix, Co, shift=0, clip_bits=0, reserved=0):
    """a MixSpec with all 64 entries of `matrix` (8, 8) as they are: garbage outside (Co, C) stays garbage"""
    sp = linne_amd.MixSpec()
    sp.out_channels, sp.shift, sp.clip_bits, sp.reserved = Co, shift, clip_bits, reserved
    m = np.asarray(matrix)
    for o in range(8):
        for c in range(8):
            sp.coef[o][c] = int(m[o, c]) if o < m.shape[0] and c < m.shape[1] else 0
    return sp


def item(t, first, n, matrix, Co, shift=0, clip_bits=0, fmt="s32", lay="planar", pad=0, reserved=0, nco=None):
    """a window of raw_mix: lay "planar" (rows n + pad elements apart), "interleaved" (packed frames), "strided" (frames Co + pad
    elements apart, channels one apart), or (channel stride, sample stride) as they are; nco: the channels the strides are laid out for"""
    return dict(t=t, first=first, n=n, matrix=np.asarray(matrix), Co=Co, shift=shift, clip=clip_bits, fmt=fmt, lay=lay, pad=pad, reserved=reserved, nco=nco or Co)


def strides(it):
    n, k = it["n"], it["nco"]
    if isinstance(it["lay"], tuple):
        return it["lay"]
    return {"planar": (n + it["pad"], 1), "interleaved": (1, k), "strided": (1, k + it["pad"])}[it["lay"]]


def extent(it):
    """elements from the window's first to behind its last, for the Co channels the reference has"""
    cs, ss = strides(it)
    k = max(min(it["Co"], 8), 1)
    return (k - 1) * cs + max(it["n"] - 1, 0) * ss + 1 if it["n"] else 0


def raw_mix(ctx, items, group_frames=0, layouts=True):
    """LINNEAmd_MixWindowsDevice itself -> (ret, codes, the buffer's bytes, the windows' byte offsets, their saturated words (7: left
    as it was))"""
    import torch
    offs, at = [], 16
    for it in items:
        es = ELEMENT_BYTES[it["fmt"]]
        at = (at + 3) & ~3
        at += 1 if it["fmt"] == "s24" else 0                    # (packed 24-bit samples lie anywhere)
        offs.append(at)
        at += max(extent(it), 1) * es + 16
    buf = torch.full((at,), SENTINEL, dtype=torch.uint8, device="cuda")
    W = len(items)
    w, sp, ly = (linne_amd.Window * W)(), (linne_amd.MixSpec * W)(), (linne_amd.PcmLayout * W)()
    for j, it in enumerate(items):
        t = it["t"]
        dev, index = it.get("dev", t.dev), it.get("index", t.index)
        w[j].index, w[j].d_stream, w[j].first_sample, w[j].num_samples, w[j].result = index.h, dev.data_ptr(), it["first"], it["n"], -1
        cs, ss = strides(it)
        w[j].d_pcm, w[j].pcm_stride = buf.data_ptr() + offs[j], cs
        C.memmove(C.byref(sp[j]), C.byref(spec_of(it["matrix"], it["Co"], it["shift"], it["clip"], it["reserved"])), C.sizeof(linne_amd.MixSpec))
        ly[j].format, ly[j].saturated, ly[j].channel_stride, ly[j].sample_stride = FMT[it["fmt"]], 7, cs, ss
    torch.cuda.synchronize()
    ret = linne_amd.lib.LINNEAmd_MixWindowsDevice(ctx.h, w, sp, ly if layouts else None, W, group_frames)
    return ret, [w[j].result for j in range(W)], buf.cpu().numpy().tobytes(), offs, [int(ly[j].saturated) for j in range(W)]


def want_mix(items, codes, offs, size):
    """sentinels but the OK windows' elements -> (the bytes, the saturated words)"""
    buf = np.full(size, SENTINEL, dtype=np.uint8)
    sats = []
    for it, code, off in zip(items, codes, offs):
        if code != OK:
            sats.append(7)
            continue
        t, n, es = it["t"], it["n"], ELEMENT_BYTES[it["fmt"]]
        want, sat = expected_mix(t.full, it["first"], n, it["matrix"][:it["Co"]], it["shift"], it["clip"], it["fmt"], t.bits)
        sats.append(int(sat))
        cs, ss = strides(it)
        raw = np.ascontiguousarray(want).view(np.uint8).reshape(it["Co"], n, es)
        for o in range(it["Co"]):
            at = off + (o * cs + np.arange(n) * ss) * es
            for b in range(es):
                buf[at + b] = raw[o, :, b]
    return buf.tobytes(), sats


def held(ctx, items, want_codes=None, group_frames=(0, 2)):
    """the call on the items, at every group_frames: codes, every byte of the buffer and the saturated words are the reference's"""
    want_codes = want_codes or [OK] * len(items)
    for gf in group_frames:
        ret, codes, buf, offs, sats = raw_mix(ctx, items, gf)
        assert codes == want_codes and ret == next((c for c in want_codes if c != OK), OK), (gf, codes, last_error(ctx))
        want, want_sats = want_mix(items, want_codes, offs, len(buf))
        if buf != want:
            bad = next(i for i in range(len(buf)) if buf[i] != want[i])
            j = max(k for k in range(len(offs)) if offs[k] <= bad) if bad >= offs[0] else -1
            raise AssertionError(f"group_frames {gf}: byte {bad} (window {j} begins at {offs[j] if j >= 0 else 0}) is {buf[bad]:#x}, not {want[bad]:#x}")
        assert sats == want_sats, (gf, sats, want_sats)
    return ret


def tensor_bytes(x):
    return np.ascontiguousarray(x.cpu().numpy()).tobytes()


# 1 ------------------------------------------------------------------------------------------------------------------------------
def test_identity_is_the_decode(ctx, streams, cut, wide):
    """the identity matrix, shift 0, clip_bits 0: the bytes and `saturated` of decode_windows on the same windows, in every layout"""
    import torch
    for t in (streams[1], streams[2], streams[3], streams[8], cut, wide):
        spans = [(0, t.ns), (517, 1500), (S - 1, 2), (S - 130, 257), (t.ns - 1, 1)]
        wins = [(t.dev, t.index, a, n) for a, n in spans]
        eye = IDENTITY[:t.nch, :t.nch]
        for kw in ({}, {"dtype": torch.int16, "channels_last": True}, {"s24": True}, {"dtype": torch.float32, "channels_last": True}, {"dtype": torch.int16}):
            want, wsat = ctx.decode_windows(wins, return_saturated=True, **kw)
            for gf in (0, 2):
                got, gsat = ctx.mix_windows(wins, eye, return_saturated=True, group_frames=gf, **kw)
                assert [tensor_bytes(g) for g in got] == [tensor_bytes(x) for x in want] and gsat == wsat, (t.name, kw, gf)
                assert [tuple(g.shape) for g in got] == [tuple(x.shape) for x in want] and [g.dtype for g in got] == [x.dtype for x in want]
        assert t is not wide or (wsat[0] and any(ctx.decode_windows(wins, return_saturated=True, s24=True)[1]))
        # int32 with a padded stride: `out` (W, C, n) cut out of a wider allocation
        same = [(t.dev, t.index, a, 700) for a in (0, 517, S - 130)]
        big_d = torch.full((3, t.nch, 700 + 9), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        big_m = big_d.clone()
        ctx.decode_windows(same, out=big_d[:, :, :700])
        ctx.mix_windows(same, eye, out=big_m[:, :, :700])
        assert tensor_bytes(big_m) == tensor_bytes(big_d) and (big_m[:, :, 700:] == 0x5A5A5A5A).all()


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2, 3, 8])
def test_the_matrix_against_the_reference(ctx, streams, nch):
    """random int16 coefficients with the extremes among them and garbage in the unused entries; windows off the 256-frame grid of
    the pieces and across a block's edge; every output channel count, shift and layout"""
    t = streams[nch]
    rng = np.random.default_rng(300 + nch)
    spans = [(S - 1, 1), (S, 1), (S - 130, 255), (S - 130, 256), (S - 130, 257), (3, 2 * S + 5), (0, t.ns)]
    lays = [("s32", "planar", 0), ("s32", "planar", 5), ("s16", "interleaved", 0), ("s24", "interleaved", 0), ("f32", "interleaved", 0),
            ("s24", "planar", 1), ("s16", "planar", 3), ("f32", "planar", 0), ("s32", "strided", 2), ("s16", "strided", 1)]
    items, k = [], 0
    for Co in (1, 2, 8):
        for shift in (0, 1, 15, 31):
            for first, n in spans:
                fmt, lay, pad = lays[k % len(lays)]
                clip = (0, 16, 24, 32, 2)[k % 5]
                items.append(item(t, first, n, random_matrix(rng, Co, nch), Co, shift, clip, fmt, lay, pad))
                k += 1
    assert {(it["fmt"], it["lay"]) for it in items} == {(f, l) for f, l, _ in lays}
    held(ctx, items)


def test_block_types_and_the_tail(ctx, cut):
    """one window over COMPRESS, SILENT and RAW blocks that reaches behind the last block: a WX_TAIL record beside the others"""
    rng = np.random.default_rng(9)
    t = cut
    items = []
    for k, (fmt, lay, pad) in enumerate([("s32", "planar", 0), ("s16", "interleaved", 0), ("s24", "planar", 2), ("f32", "interleaved", 0), ("s32", "strided", 1)]):
        for Co, shift in ((1, 1), (2, 0), (8, 15)):
            items.append(item(t, 0, t.ns, random_matrix(rng, Co, 2), Co, shift, (0, 16)[k % 2], fmt, lay, pad))
            items.append(item(t, 6 * S - 100, 400, random_matrix(rng, Co, 2), Co, shift, 0, fmt, lay, pad))       # RAW, then the tail
            items.append(item(t, 6 * S + 7, 300, random_matrix(rng, Co, 2), Co, shift, 0, fmt, lay, pad))         # the tail alone
            items.append(item(t, S + 10, 2 * S - 20, random_matrix(rng, Co, 2), Co, shift, 0, fmt, lay, pad))     # SILENT blocks alone
    held(ctx, items)
    # one window per pass, and a window that spans passes
    held(ctx, [items[0]], group_frames=(2,))


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_extremes(ctx, wide):
    """values over all of int32 against rows of eight coefficients of +-32767: clipped at int32, clipped at 16 bits, and not clipped
    behind a shift of 31"""
    t = wide
    rows = np.array([[32767 * (-1) ** ((o >> c) & 1) for c in range(8)] for o in range(8)], dtype=np.int16)
    cases = [(0, 0, True), (0, 16, True), (31, 0, False), (15, 32, True), (31, 16, True)]
    items = []
    for shift, clip, sat in cases:
        assert expected_mix(t.full, 0, t.ns, rows, shift, clip)[1] == sat, (shift, clip)
        for fmt, lay in (("s32", "planar"), ("f32", "interleaved"), ("s16", "planar"), ("s24", "interleaved")):
            items.append(item(t, 0, t.ns, rows, 8, shift, clip, fmt, lay))
    ret, codes, buf, offs, sats = raw_mix(ctx, items)
    want, want_sats = want_mix(items, [OK] * len(items), offs, len(buf))
    assert (ret, codes) == (OK, [OK] * len(items)) and buf == want and sats == want_sats
    assert [sats[4 * k] for k in range(len(cases))] == [int(c[2]) for c in cases]
    assert sats[8:12] == [0, 0, 1, 0]                            # shift 31: sums of up to 2^17 fit everything but int16
    full32 = expected_mix(t.full, 0, t.ns, rows, 0, 0)[0]
    assert full32.max() == (1 << 31) - 1 and full32.min() == -(1 << 31)


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(ctx, streams):
    two, three = streams[2], streams[3]
    eye = IDENTITY
    bad = [dict(Co=0), dict(Co=9), dict(shift=32), dict(clip_bits=1), dict(clip_bits=33), dict(reserved=1)]
    for kw in bad:
        args = dict(Co=2, shift=0, clip_bits=0, reserved=0)
        args.update(kw)
        it = item(two, 100, 500, eye, args["Co"], args["shift"], args["clip_bits"], "s32", "planar", 0, args["reserved"], nco=2)
        good = item(two, 7, 300, eye, 2)
        ret, codes, buf, offs, sats = raw_mix(ctx, [good, it, good])
        assert (ret, codes) == (INVALID_ARGUMENT, [OK, INVALID_ARGUMENT, OK]) and last_error(ctx).startswith("window 1: MixWindowsDevice: "), (kw, last_error(ctx))
        want, want_sats = want_mix([good, it, good], codes, offs, len(buf))
        assert buf == want and sats == want_sats == [0, 7, 0], kw
    # frames two elements apart, channels one: injective for two output channels, not for three -- whatever the stream has
    refused = item(two, 0, 400, eye, 3, lay=(1, 2), nco=3)
    taken = item(three, 0, 400, eye, 2, lay=(1, 2))
    ret, codes, buf, offs, sats = raw_mix(ctx, [refused, taken])
    assert (ret, codes) == (INVALID_ARGUMENT, [INVALID_ARGUMENT, OK]) and "share an element" in last_error(ctx)
    assert buf == want_mix([refused, taken], codes, offs, len(buf))[0]
    w = [(three.dev, three.index, 0, 400)]
    with pytest.raises(linne_amd.LinneAmdError):                 # the decode call refuses these strides for the stream's three channels
        import torch
        o = torch.empty(400 * 2 + 1, dtype=torch.int32, device="cuda")
        ctx.decode_windows(w, out=torch.as_strided(o, (1, 3, 400), (0, 1, 2)), channels_last=False)
    # without layouts: pcm_stride >= num_samples is asked of Co > 1, not of the stream's channels
    for t, Co, stride, code in ((two, 1, 0, OK), (streams[1], 2, 399, INVALID_ARGUMENT), (streams[1], 2, 400, OK)):
        it = item(t, 0, 400, eye, Co, lay=(stride, 1))
        ret, codes, buf, offs, sats = raw_mix(ctx, [it], layouts=False)
        assert (ret, codes) == (code, [code]), (Co, stride, last_error(ctx))
        assert buf == want_mix([it], codes, offs, len(buf))[0]
    # the Python form refuses what is not int16 before any call
    wins = [(two.dev, two.index, 0, 100)]
    for m in ([[1, 32768]], [[-32769, 0]], [[1.5, 0.0]], [[1, 1, 1]], np.zeros((9, 2), dtype=np.int64)):
        with pytest.raises(ValueError):
            ctx.mix_windows(wins, m)
    assert ctx.mix_windows([], [[1, 1]]) == [] and ctx.mix_windows([], [[1, 1]], return_codes=True) == ([], [])
    f = linne_amd.lib.LINNEAmd_MixWindowsDevice
    assert f(ctx.h, None, None, None, 0, 0) == OK and f(ctx.h, None, (linne_amd.MixSpec * 1)(), None, 1, 0) == INVALID_ARGUMENT
    assert "MixWindowsDevice: null argument" in last_error(ctx)


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_many_windows_and_failures_stay_in_their_window(ctx, product, streams, cut):
    """64 windows of mixed C, Co, layouts and matrices in one buffer of sentinels, the damaged copies' among them"""
    t = streams[2]
    crc, rice = sc.damaged(ctx, product, t)
    k, kr = crc[2], rice[2]
    rng = np.random.default_rng(4)
    ts = [streams[2], streams[3], cut, streams[8], streams[1]]
    lays = [("s32", "planar", 0), ("s16", "interleaved", 0), ("s24", "planar", 1), ("f32", "interleaved", 0), ("s32", "planar", 3), ("f32", "planar", 2), ("s24", "interleaved", 0)]
    items, want_codes = [], [OK] * 64
    for i in range(64):
        u = ts[i % len(ts)]
        first = int(rng.integers(0, u.ns))
        n = int(rng.integers(1, min(u.ns - first, 1500) + 1)) if i % 7 else 0
        Co = (1, 2, 8, 3)[i % 4]
        fmt, lay, pad = lays[i % len(lays)]
        items.append(item(u, first, n, random_matrix(rng, Co, u.nch), Co, (0, 1, 15, 31)[(i // 4) % 4], (0, 16, 24)[i % 3], fmt, lay, pad))

    def on(damaged, first, n, code, i):
        items[i] = dict(item(t, first, n, random_matrix(rng, 2, 2), 2, 1, 16, *lays[i % len(lays)]), dev=damaged[0], index=damaged[1])
        want_codes[i] = code
    on(rice, t.bl[kr][4] + 10, 600, NG, 5)                       # over the Rice-damaged block: the fail word is set on the device
    on(rice, t.bl[kr - 1][4] + 10, 600, OK, 6)
    on(rice, 0, t.ns, NG, 7)
    on(crc, t.bl[k][4] + 3, 600, CORRUPTION, 9)                  # CRC damage: refused on the host
    on(crc, 0, t.bl[k][4] - 24, OK, 10)
    on(crc, t.bl[k + 1][4], 200, CORRUPTION, 11)
    items[20] = item(t, 0, 1000, IDENTITY, 2, shift=32)
    items[40] = item(t, 1, t.ns, IDENTITY, 2)                    # a range beyond the stream
    want_codes[20] = want_codes[40] = INVALID_ARGUMENT
    assert held(ctx, items, want_codes) == NG                    # the lowest failing window's
    ret, codes, *_ = raw_mix(ctx, items)
    text = last_error(ctx)
    assert text.startswith(f"window 5: block {kr} ")
    # codes and text are the decode call's
    wins = lambda lo, hi: [(it.get("dev", it["t"].dev), it.get("index", it["t"].index), it["first"], it["n"]) for it in items[lo:hi]]
    _, dcodes = ctx.decode_windows(wins(4, 12), return_codes=True)
    assert dcodes == want_codes[4:12] and last_error(ctx) == text.replace("window 5:", "window 1:")
    # the Python form: codes with return_codes, an error without
    mats = [it["matrix"][:it["Co"], :it["t"].nch] for it in items[8:12]]
    got, pcodes = ctx.mix_windows(wins(8, 12), mats, shift=[it["shift"] for it in items[8:12]],
                                  clip_bits=[it["clip"] for it in items[8:12]], return_codes=True)
    assert pcodes == want_codes[8:12] == [OK, CORRUPTION, OK, CORRUPTION]
    for it, g in zip(items[8:12:2], got[0::2]):
        assert np.array_equal(g.cpu().numpy(), expected_mix(it["t"].full, it["first"], it["n"], it["matrix"][:it["Co"]], it["shift"], it["clip"])[0])
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.mix_windows(wins(8, 12), mats, shift=1)               # one shift for every window
    assert e.value.code == CORRUPTION and e.value.codes == pcodes and "window 1:" in str(e.value)
    for _, index, _ in (crc, rice):
        index.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(streams):
    """the decode call's launches with kind 98 in place of kind 59, none of any other consumer's, the same for one window and for 64"""
    others = sorted(k for c in sc.CONSUMERS.values() for k in c.kinds)           # kind 59 among them
    assert PLACE_KIND in others and MIX_KIND == 98 and MIX_KIND not in others
    ctx = linne_amd.Context(0, use_torch_stream=False)
    try:
        ctx.enable_timing(True)
        for t in (streams[2], streams[3]):                       # four COMPRESS blocks each: two placing passes at group_frames 2
            index = ctx.index_stream(t.dev)
            counts = {}
            m = random_matrix(np.random.default_rng(1), 2, t.nch, garbage=False)[:2, :t.nch]
            for nw in (1, 64):
                spans = [(0, t.ns)] + [(37 * i, t.ns - 53 * i) for i in range(1, nw)]
                wins = [(t.dev, index, a, n) for a, n in spans]
                for gf in (0, 2):
                    ctx.decode_windows(wins, group_frames=gf)
                    dec = {k: ctx.last_launches(k) for k in DECODE_KINDS + [PLACE_KIND]}
                    got = ctx.mix_windows(wins, m, shift=15, clip_bits=16, group_frames=gf)
                    mine = {k: ctx.last_launches(k) for k in DECODE_KINDS + [MIX_KIND] + others}
                    a, n = spans[-1]
                    assert np.array_equal(got[-1].cpu().numpy(), expected_mix(t.full, a, n, m, 15, 16)[0])
                    assert all(mine[k] == 0 for k in others), (t.name, nw, gf, mine)
                    assert mine[MIX_KIND] == dec[PLACE_KIND] >= 1 and all(mine[k] == dec[k] for k in DECODE_KINDS), (t.name, nw, gf, dec, mine)
                    assert ctx.last_ms(MIX_KIND) > 0
                    counts[(nw, gf)] = mine
                assert counts[(nw, 0)][MIX_KIND] == 1
            assert counts[(1, 0)] == counts[(64, 0)]
            assert counts[(1, 2)][MIX_KIND] > 1                  # the window spans passes
            index.close()
    finally:
        ctx.close()


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_history(streams, cut):
    """a mix call directly behind a compare call and behind a quiet call, which keep words behind the fail words; large then small and
    small then large; every call held to its own reference"""
    import torch
    ctx = linne_amd.Context(0, use_torch_stream=False)
    try:
        rng = np.random.default_rng(21)
        t, u = streams[2], streams[8]
        ti, ui = ctx.index_stream(t.dev), ctx.index_stream(u.dev)
        small = [dict(item(t, S - 130, 257, random_matrix(rng, 8, 2), 8, 1, 16, "s16", "interleaved"), index=ti)]
        large = [dict(item(u, 0, u.ns, random_matrix(rng, Co, 8), Co, 15, 0, fmt, lay), index=ui) for Co, fmt, lay in ((1, "f32", "planar"), (8, "s32", "planar"), (2, "s24", "interleaved"))] * 4
        pcm = torch.from_numpy(np.ascontiguousarray(t.full)).cuda()
        for first, second in ((large, small), (small, large)):
            for before in ("compare", "quiet"):
                held(ctx, first, group_frames=(0,))
                if before == "compare":
                    assert ctx.compare_windows([(t.dev, ti, 0, t.ns, pcm)] * 5) == [(0, 0, 0)] * 5
                else:
                    runs = ctx.quiet_windows([(t.dev, ti, 0, t.ns)] * 3, 3, 2)
                    assert [r.cpu() for r in runs] == [sc.expected_quiet(t.full, 0, t.ns, 3, 2)[0]] * 3
                held(ctx, second, group_frames=(0, 2))
        ti.close()
        ui.close()
    finally:
        ctx.close()


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_remix_streams(ctx, oracle, streams):
    t = streams[2]
    m = music(1, 2 * S + TAIL, 16, seed=5)
    m[0, 100:110] = 0
    inv = encoded(ctx, oracle, np.concatenate([m, -m]), 16, 2, False, "inverted")
    findings, = linne_amd.channel_findings(ctx.relate_streams([inv.dev])[0])
    assert findings["pairs"] == {(0, 1): "inverted"}
    fix = linne_amd.fix_matrix(findings)
    assert fix == ((1, 0), (0, -1))
    mean, shift = linne_amd.downmix_matrix(2)
    cases = [(t, mean, shift), (t, linne_amd.select_matrix(2, [1, 0]), 0), (inv, fix, 0), (streams[3], *linne_amd.downmix_matrix(3)), (streams[8], linne_amd.select_matrix(8, [7, 0, 3]), 0)]
    for u, matrix, sh in cases:
        bits, rate, block, preset, ms = (u.index.header[k] for k in ("bits_per_sample", "sampling_rate", "num_samples_per_block", "preset", "ch_process_method"))
        ms = ms if len(matrix) > 1 else 0                        # (one channel has no mid and side)
        out, = ctx.remix_streams([u.dev], matrix, shift=sh)
        got = bytes(out.cpu().numpy().tobytes())
        want = expected_mix(u.full, 0, u.ns, matrix, sh, bits)[0]
        ret, full, _ = oracle.decode_whole(got)
        assert ret == OK and np.array_equal(full, want), u.name
        assert got == bytes(ctx.encode_streams([(want, bits, rate, block, preset, ms)])[0].cpu().numpy().tobytes()), u.name
        assert got == bytes(oracle.encode_whole(want, bits, rate, block, preset, ms)), u.name
    fixed, = ctx.remix_streams([inv.dev], fix)
    again, = linne_amd.channel_findings(ctx.relate_streams([fixed])[0])
    assert again["pairs"] == {(0, 1): "identical"}
    # many streams in one call, a matrix per stream, and the header fields a caller gives
    outs = ctx.remix_streams([t.dev, inv.stream], [mean, fix], shift=[shift, 0], group_frames=2)
    assert oracle.decode_whole(bytes(outs[0].cpu().numpy().tobytes()))[1].shape == (1, t.ns) and bytes(outs[1].cpu().numpy().tobytes()) == bytes(fixed.cpu().numpy().tobytes())
    other, = ctx.remix_streams([t.dev], mean, shift=shift, bits=24, preset=0, block=512, ms=0)
    assert bytes(other.cpu().numpy().tobytes()) == bytes(oracle.encode_whole(expected_mix(t.full, 0, t.ns, mean, shift, 24)[0], 24, 44100, 512, 0, False))
    assert ctx.remix_streams([], mean) == []
    inv.index.close()


# 9 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_command_line_tool(ctx, tmp_path, streams):
    src, dst = tmp_path / "a.lnn", tmp_path / "b.lnn"
    for t, spec, matrix, shift in ((streams[2], "1,1>>1", [[1, 1]], 1), (streams[2], "0,1/1,0", [[0, 1], [1, 0]], 0), (streams[3], "-32768,32767,1/0,0,-1>>15", [[-32768, 32767, 1], [0, 0, -1]], 15)):
        src.write_bytes(t.stream)
        r = subprocess.run([CLI, "-X", spec, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        want, = ctx.remix_streams([t.dev], matrix, shift=shift)
        assert dst.read_bytes() == bytes(want.cpu().numpy().tobytes()), spec
