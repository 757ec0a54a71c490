"""GPU tests of resampling windows of resident .lnn streams (Context.resample_windows, resample_streams; include/linne_amd.h
LINNEAmd_ResampleWindowsDevice).  Every expected element is computed with numpy int64 (resample_refs.expected_resample) from the oracle's
decode of the same bytes, never from the library under test, and everything must be equal: bytes and integers, no tolerance -- the
float32 path is a conversion and a multiplication by a power of two.  Streams hold 3 to 6 blocks of 1024 samples, or 21 blocks of 33."""
import ctypes as C

import numpy as np
import pytest

import linne_amd
import synth_records as sr
from resample_refs import ELEMENT_BYTES, expected_resample, random_coef, resampled_length
from signals import music
import stream_consumers as sc
from stream_consumers import DECODE_KINDS, KIND, Stream, encoded, last_error
from stream_refs import mixed_signal
from test_stream_relate_cpu import WIDE_SHAPE, wide_cases

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CORRUPTION, NG = 0, 1, 6, 7
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300
SENTINEL = 0x5A
FMT = {"s32": linne_amd.PCM_S32, "s16": linne_amd.PCM_S16, "s24": linne_amd.PCM_S24, "f32": linne_amd.PCM_F32}
PRESET_KIND, RESAMPLE_KIND, PLACE_KIND = KIND["RESAMPLE_T_PRESET"], KIND["RESAMPLE_T_RESAMPLE"], KIND["T_WX_PLACE"]
ONE = np.array([[1]], dtype=np.int16)
RATIOS = [(1, 1), (1, 2), (2, 1), (3, 2), (2, 3), (160, 147), (147, 160), (160, 441), (441, 80), (4, 2)]
LAYS = [("s32", "planar", 0), ("s32", "planar", 5), ("s16", "interleaved", 0), ("s24", "interleaved", 0), ("f32", "interleaved", 0),
        ("s24", "planar", 1), ("s16", "planar", 3), ("f32", "planar", 0), ("s32", "strided", 2), ("s16", "strided", 1)]


@pytest.fixture(scope="module")
def streams(ctx, oracle):
    """1, 2 (MS), 3 and 8 channels of 16 bits: 3 blocks and a tail of 300; "8bit" and "24bit": stereo streams of those widths"""
    out = {nch: encoded(ctx, oracle, music(nch, 3 * S + TAIL, 16, seed=90 + nch), 16, 5 if nch == 2 else 0, nch == 2, f"{nch}ch") for nch in (1, 2, 3, 8)}
    out["8bit"] = encoded(ctx, oracle, music(2, 2 * S + 77, 8, seed=61), 8, 0, False, "8 bits")
    out["24bit"] = encoded(ctx, oracle, music(2, 2 * S + 77, 24, seed=62), 24, 2, True, "24 bits")
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


@pytest.fixture(scope="module")
def small(ctx, oracle):
    """stereo in blocks of 33 samples, the last of 5: a filter of 64 taps crosses two block boundaries, and the last block is shorter
    than it.  (33 is the shortest block the format has: a block is longer than the 32 parameters of preset 0's first layer, and
    the encoder refuses 16)"""
    x = music(2, 20 * 33 + 5, 16, seed=17)
    t = Stream(ctx, oracle, oracle.encode_whole(x, 16, 44100, 33, 0, False), "blocks of 33")
    assert np.array_equal(t.full, x) and len(t.bl) == 21 and t.bl[-1][3] == 5
    yield t
    t.index.close()


# ---- the C entry point on outputs that lie in one buffer of sentinels ----
def item(t, first, n, coef, up, down, before=0, shift=0, clip_bits=0, fmt="s32", lay="planar", pad=0, wrong=None):
    """a window of raw_resample: lay "planar" (rows n + pad elements apart), "interleaved" (packed frames), "strided" (frames C + pad
    elements apart, channels one apart); wrong: spec fields as they are given to the call, whatever the reference would say"""
    return dict(t=t, first=first, n=n, coef=np.ascontiguousarray(coef, dtype=np.int16), up=up, down=down, before=before, shift=shift, clip=clip_bits, fmt=fmt, lay=lay, pad=pad, wrong=wrong or {})


def strides(it):
    n, k = it["n"], it["t"].nch
    return {"planar": (n + it["pad"], 1), "interleaved": (1, k), "strided": (1, k + it["pad"])}[it["lay"]]


def extent(it):
    cs, ss = strides(it)
    return (it["t"].nch - 1) * cs + max(it["n"] - 1, 0) * ss + 1 if it["n"] else 0


def raw_resample(ctx, items, group_frames=0, layouts=True):
    """LINNEAmd_ResampleWindowsDevice itself -> (ret, codes, the buffer's bytes, the windows' byte offsets, their saturated words (7:
    left as it was))"""
    import torch
    offs, at = [], 16
    for it in items:
        at = (at + 3) & ~3
        at += 1 if it["fmt"] == "s24" else 0                    # (packed 24-bit samples lie anywhere)
        offs.append(at)
        at += max(extent(it), 1) * ELEMENT_BYTES[it["fmt"]] + 16
    buf = torch.full((at,), SENTINEL, dtype=torch.uint8, device="cuda")
    W = len(items)
    w, sp, ly = (linne_amd.Window * W)(), (linne_amd.ResampleSpec * W)(), (linne_amd.PcmLayout * W)()
    for j, it in enumerate(items):
        t = it["t"]
        dev, index = it.get("dev", t.dev), it.get("index", t.index)
        w[j].index, w[j].d_stream, w[j].first_sample, w[j].num_samples, w[j].result = index.h, dev.data_ptr(), it["first"], it["n"], -1
        cs, ss = strides(it)
        w[j].d_pcm, w[j].pcm_stride = buf.data_ptr() + offs[j], cs
        f = dict(up=it["up"], down=it["down"], taps=it["coef"].shape[1], before=it["before"], shift=it["shift"], clip_bits=it["clip"], reserved=0)
        f.update({k: v for k, v in it["wrong"].items() if k != "null_coef"})
        for k, v in f.items():
            setattr(sp[j], k, v)
        if not it["wrong"].get("null_coef"):
            sp[j].coef = it["coef"].ctypes.data_as(C.POINTER(C.c_int16))
        ly[j].format, ly[j].saturated, ly[j].channel_stride, ly[j].sample_stride = FMT[it["fmt"]], 7, cs, ss
    torch.cuda.synchronize()
    ret = linne_amd.lib.LINNEAmd_ResampleWindowsDevice(ctx.h, w, sp, ly if layouts else None, W, group_frames)
    return ret, [w[j].result for j in range(W)], buf.cpu().numpy().tobytes(), offs, [int(ly[j].saturated) for j in range(W)]


def want_resample(items, codes, offs, size):
    """sentinels but the OK windows' elements -> (the bytes, the saturated words)"""
    buf = np.full(size, SENTINEL, dtype=np.uint8)
    sats = []
    for it, code, off in zip(items, codes, offs):
        if code != OK:
            sats.append(7)
            continue
        t, n, es = it["t"], it["n"], ELEMENT_BYTES[it["fmt"]]
        want, sat = expected_resample(t.full, it["first"], n, it["coef"], it["up"], it["down"], it["before"], it["shift"], it["clip"], it["fmt"], t.bits)
        sats.append(int(sat))
        cs, ss = strides(it)
        raw = np.ascontiguousarray(want).view(np.uint8).reshape(t.nch, n, es)
        for o in range(t.nch):
            at = off + (o * cs + np.arange(n) * ss) * es
            for b in range(es):
                buf[at + b] = raw[o, :, b]
    return buf.tobytes(), sats


def held(ctx, items, want_codes=None, group_frames=(0, 2)):
    """the call on the items, at every group_frames: codes, every byte of the buffer and the saturated words are the reference's"""
    want_codes = want_codes or [OK] * len(items)
    for gf in group_frames:
        ret, codes, buf, offs, sats = raw_resample(ctx, items, gf)
        assert codes == want_codes and ret == next((c for c in want_codes if c != OK), OK), (gf, codes, last_error(ctx))
        want, want_sats = want_resample(items, want_codes, offs, len(buf))
        if buf != want:
            bad = next(i for i in range(len(buf)) if buf[i] != want[i])
            j = max(k for k in range(len(offs)) if offs[k] <= bad) if bad >= offs[0] else -1
            raise AssertionError(f"group_frames {gf}: byte {bad} (window {j} begins at {offs[j] if j >= 0 else 0}) is {buf[bad]:#x}, not {want[bad]:#x}")
        assert sats == want_sats, (gf, sats, want_sats)
    return ret


def tensor_bytes(x):
    return np.ascontiguousarray(x.cpu().numpy()).tobytes()


def length(t, up, down):
    return resampled_length(t.ns, up, down)


# 1 ------------------------------------------------------------------------------------------------------------------------------
def test_identity_is_the_decode(ctx, streams, cut, wide):
    """1/1, one tap of 1, shift 0, clip_bits 0: the bytes and `saturated` of decode_windows on the same windows, in every layout"""
    import torch
    for t in (streams[1], streams[2], streams[3], streams[8], cut, wide):
        spans = [(0, t.ns), (517, 1500), (S - 1, 2), (S - 130, 257), (t.ns - 1, 1)]
        wins = [(t.dev, t.index, a, n) for a, n in spans]
        for kw in ({}, {"dtype": torch.int16, "channels_last": True}, {"s24": True}, {"dtype": torch.float32, "channels_last": True}, {"dtype": torch.int16}):
            want, wsat = ctx.decode_windows(wins, return_saturated=True, **kw)
            for gf in (0, 2):
                got, gsat = ctx.resample_windows(wins, 1, 1, coef=ONE, return_saturated=True, group_frames=gf, **kw)
                assert [tensor_bytes(g) for g in got] == [tensor_bytes(x) for x in want] and gsat == wsat, (t.name, kw, gf)
                assert [tuple(g.shape) for g in got] == [tuple(x.shape) for x in want] and [g.dtype for g in got] == [x.dtype for x in want]
        assert t is not wide or (wsat[0] and any(ctx.decode_windows(wins, return_saturated=True, s24=True)[1]))
        same = [(t.dev, t.index, a, 700) for a in (0, 517, S - 130)]         # int32 with a padded stride
        big_d = torch.full((3, t.nch, 700 + 9), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        big_r = big_d.clone()
        ctx.decode_windows(same, out=big_d[:, :, :700])
        ctx.resample_windows(same, 1, 1, coef=ONE, out=big_r[:, :, :700])
        assert tensor_bytes(big_r) == tensor_bytes(big_d)


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: "%d/%d" % r)
def test_values_against_the_reference(ctx, streams, ratio):
    """random int16 coefficients with the extremes among them; every tap count, shift, channel count and sample width; windows at
    output 0, at the last output, of 1, 255, 256 and 257 outputs, across tiles, and whole streams; every layout in turn"""
    up, down = ratio
    rng = np.random.default_rng(1000 * up + down)
    items, k = [], 0
    for P in (1, 2, 16, 33, 64):
        if up * P > 16384:
            continue
        coef = random_coef(rng, up, P)
        for key in (1, 2, 3, 8, "8bit", "24bit"):
            t = streams[key]
            n_out = length(t, up, down)
            spans = [(0, n_out), (0, 1), (n_out - 1, 1), (n_out - 257, 257), (min(250, n_out - 256), 256), (7, 255), (n_out // 2, 1)]
            for first, n in (spans if key == 2 else spans[k % len(spans)::3]):
                fmt, lay, pad = LAYS[k % len(LAYS)]
                items.append(item(t, first, n, coef, up, down, before=(0, P - 1, P // 2)[k % 3], shift=(0, 15, 31)[(k // 3) % 3], clip_bits=(0, 16, 24, 32, 2)[k % 5], fmt=fmt, lay=lay, pad=pad))
                k += 1
    held(ctx, items)


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_edges(ctx, streams, cut, small):
    t = streams[2]
    rng = np.random.default_rng(5)
    items = []
    for up, down in ((3, 2), (5, 1), (4, 6)):                    # windows that start at every phase of a small L, and end at every one
        coef = random_coef(rng, up, 7)
        for m0 in range(2 * up + 1):
            items.append(item(t, 1000 + m0, 300 + m0, coef, up, down, before=3, shift=15, fmt=LAYS[m0 % len(LAYS)][0], lay=LAYS[m0 % len(LAYS)][1], pad=LAYS[m0 % len(LAYS)][2]))
    c64, c5 = random_coef(rng, 2, 64), random_coef(rng, 1, 5)
    for first, n in ((0, 1), (0, 255), (0, 256), (0, 257), (255, 2), (256, 1), (511, 514), (100, 1300)):         # on and across the tiles of 256
        items.append(item(t, first, n, c64, 2, 1, before=63, shift=20, clip_bits=16))
        items.append(item(t, first, n, c5, 1, 1, before=4, shift=3, fmt="s16", lay="interleaved"))
    n_out = length(t, 2, 1)
    items += [item(t, 0, 40, c64, 2, 1, before=b, shift=17) for b in (0, 31, 63)]            # the halo reaches before the stream
    items += [item(t, n_out - 40, 40, c64, 2, 1, before=b, shift=17) for b in (0, 31, 63)]   # ... and behind it
    # blocks of 33 under 64 taps: the halo crosses two block boundaries, the last block is shorter than the filter
    for up, down in ((1, 1), (3, 2), (1, 3)):
        c = random_coef(rng, up, 64)
        n_s = length(small, up, down)
        items += [item(small, 0, n_s, c, up, down, before=31, shift=18), item(small, n_s - 3, 3, c, up, down, before=63, shift=18, fmt="s24", lay="planar", pad=1),
                  item(small, 40, 50, c, up, down, before=0, shift=18, fmt="f32", lay="interleaved")]
    # COMPRESS, SILENT and RAW neighbours under one filter, and the truncated stream's tail of zeros
    for up, down in ((1, 1), (160, 147), (1, 2)):
        c = random_coef(rng, up, 33)
        n_c = length(cut, up, down)
        b = lambda s: s * up // down
        items += [item(cut, 0, n_c, c, up, down, before=16, shift=16), item(cut, b(S) - 20, 60, c, up, down, before=16, shift=16, fmt="s16", lay="planar", pad=3),
                  item(cut, b(4 * S) - 9, 30, c, up, down, before=32, shift=16, fmt="f32", lay="planar"), item(cut, b(6 * S) - 40, 90, c, up, down, before=0, shift=16),
                  item(cut, n_c - 5, 5, c, up, down, before=7, shift=16, fmt="s24", lay="interleaved")]
    held(ctx, items, group_frames=(0, 1, 2))
    # a decimation whose tile spans more input than a workgroup stages
    c = random_coef(rng, 1, 64)
    assert 7 * 1024 + 64 > 4096 and length(cut, 1, 1024) == 8 and 74 * 100 + 64 > 4096 and length(cut, 1, 100) == 75
    held(ctx, [item(streams[8], 0, length(streams[8], 1, 64), c, 1, 64, before=32, shift=15), item(cut, 0, 8, c, 1, 1024, before=5, shift=12, fmt="s16", lay="interleaved"),
               item(cut, 0, 75, c, 1, 100, before=63, shift=15), item(t, 1, length(t, 1, 1024) - 1, c, 1, 1024, before=5, shift=12, fmt="s24", lay="planar")])


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_saturation_from_the_clip_and_from_the_format(ctx, wide, streams):
    t = wide
    two = np.array([[32767, 32767]], dtype=np.int16)
    items = [item(t, 0, t.ns, two, 1, 1, fmt=fmt, lay=lay, shift=sh, clip_bits=cb) for fmt, lay in (("s32", "planar"), ("s16", "interleaved"), ("s24", "planar"), ("f32", "interleaved"))
             for sh, cb in ((0, 0), (16, 0), (16, 16), (31, 2))]
    u = streams[2]
    items += [item(u, 0, u.ns, ONE, 1, 1, fmt="s16"), item(u, 0, u.ns, ONE * 2, 1, 1, fmt="s16"), item(u, 0, u.ns, ONE, 1, 1, clip_bits=12)]
    ret, codes, buf, offs, sats = raw_resample(ctx, items)
    want, want_sats = want_resample(items, codes, offs, len(buf))
    assert ret == OK and buf == want and sats == want_sats
    assert sats[0] == 1 and sats[-3] == 0 and 0 in sats[:16] and 1 in sats[-2:]                     # a clip is among them, and none


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_many_windows_and_failures_stay_in_their_window(ctx, product, streams, cut, small):
    """64 windows of mixed specs and shapes in one buffer of sentinels, CRC- and Rice-damaged neighbours and argument errors among them:
    a failing window's memory is untouched, the lowest failing window's code and text are returned"""
    t = streams[2]
    crc, rice = sc.damaged(ctx, product, t)
    k, kr = crc[2], rice[2]
    rng = np.random.default_rng(4)
    ts = [streams[2], streams[3], cut, streams[8], streams[1], small, streams["24bit"]]
    tables = {r: random_coef(rng, r[0], P) for r, P in zip(RATIOS, (1, 2, 16, 33, 64, 8, 5, 32, 3, 64))}
    items, want_codes = [], [OK] * 64
    for i in range(64):
        u = ts[i % len(ts)]
        up, down = RATIOS[i % len(RATIOS)]
        coef = tables[(up, down)]
        n_out = length(u, up, down)
        first = int(rng.integers(0, n_out))
        n = int(rng.integers(1, min(n_out - first, 900) + 1)) if i % 7 else 0
        fmt, lay, pad = LAYS[i % len(LAYS)]
        items.append(item(u, first, n, coef, up, down, before=int(rng.integers(0, coef.shape[1])), shift=(0, 15, 31, 20)[(i // 4) % 4], clip_bits=(0, 16, 24)[i % 3], fmt=fmt, lay=lay, pad=pad))
    c3 = random_coef(rng, 3, 9)

    def on(damaged, first, n, code, i, **wrong):
        fmt, lay, pad = LAYS[i % len(LAYS)]
        items[i] = dict(item(t, first, n, c3, 3, 2, before=4, shift=17, clip_bits=16, fmt=fmt, lay=lay, pad=pad, wrong=wrong), dev=damaged[0], index=damaged[1])
        want_codes[i] = code
    o = lambda s: -(-s * 3 // 2)                                 # the first output that reads from input sample s on (before 4 <= its reach back)
    on(rice, o(t.bl[kr][4]) + 10, 600, NG, 5)                    # over the Rice-damaged block: the fail word is set on the device
    on(rice, o(t.bl[kr - 1][4]) + 10, 600, OK, 6)
    on(rice, 0, length(t, 3, 2), NG, 7)
    on(crc, o(t.bl[k][4]) + 3, 600, CORRUPTION, 9)               # CRC damage: refused on the host
    on(crc, 0, (t.bl[k][4] - 8) * 3 // 2, OK, 10)                # its last output's last input sample is in front of the damaged block
    on(crc, 0, (t.bl[k][4] - 8) * 3 // 2 + 12, CORRUPTION, 11)   # ... and here the halo alone reaches into it
    on((t.dev, t.index), 0, 1000, INVALID_ARGUMENT, 20, shift=32)
    on((t.dev, t.index), 1, length(t, 3, 2), INVALID_ARGUMENT, 40)       # a range beyond the resampled stream
    on((t.dev, t.index), 0, 100, INVALID_ARGUMENT, 41, null_coef=True)
    on((t.dev, t.index), 0, 100, INVALID_ARGUMENT, 42, reserved=1)
    on((t.dev, t.index), 0, 100, INVALID_ARGUMENT, 43, before=9)
    on((t.dev, t.index), 0, 100, INVALID_ARGUMENT, 44, down=1025)
    assert (items[10]["first"] + items[10]["n"] - 1) * 2 // 3 - 4 + 8 < t.bl[k][4] <= (items[11]["first"] + items[11]["n"] - 1) * 2 // 3 - 4 + 8
    assert held(ctx, items, want_codes) == NG                    # the lowest failing window's
    ret, codes, *_ = raw_resample(ctx, items)
    text = last_error(ctx)
    assert text.startswith(f"window 5: block {kr} ")
    for i, word in ((20, "shift 32"), (41, "null coef"), (42, "reserved"), (43, "before 9"), (44, "down 1025")):
        ret1, codes1, buf1, *_ = raw_resample(ctx, [items[i]])
        assert (ret1, codes1) == (INVALID_ARGUMENT, [INVALID_ARGUMENT]) and set(buf1) == {SENTINEL}
        assert last_error(ctx).startswith("window 0: ResampleWindowsDevice: ") and word in last_error(ctx), i
    ret1, codes1, buf1, *_ = raw_resample(ctx, [items[11]])
    assert (ret1, codes1) == (CORRUPTION, [CORRUPTION]) and set(buf1) == {SENTINEL} and last_error(ctx).startswith(f"window 0: block {k} ")
    # the Python form: codes with return_codes, an error without
    wins = [(it.get("dev", t.dev), it.get("index", t.index), it["first"], it["n"]) for it in items[9:12]]
    got, pcodes = ctx.resample_windows(wins, 3, 2, coef=c3, before=4, shift=17, clip_bits=16, return_codes=True)
    assert pcodes == [CORRUPTION, OK, CORRUPTION]
    assert np.array_equal(got[1].cpu().numpy(), expected_resample(t.full, 0, items[10]["n"], c3, 3, 2, 4, 17, 16)[0])
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.resample_windows(wins, 3, 2, coef=c3, before=4, shift=17)
    assert e.value.code == CORRUPTION and e.value.codes == pcodes and "window 0:" in str(e.value)
    assert ctx.resample_windows([], 3, 2) == [] and ctx.resample_windows([], 3, 2, return_codes=True) == ([], [])
    for _, index, _ in (crc, rice):
        index.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(streams):
    """the decode call's launches, kind 59 among them, and kinds 99 and 100 once each, none of any other consumer's; the same for one
    window and for 64, whatever the ratio and the taps"""
    others = sorted(k for c in sc.CONSUMERS.values() for k in c.kinds if k != PLACE_KIND) + [KIND["MIX_T_MIX"]]
    assert (PRESET_KIND, RESAMPLE_KIND) == (99, 100) and not {99, 100} & set(others)
    ctx = linne_amd.Context(0, use_torch_stream=False)
    try:
        ctx.enable_timing(True)
        rng = np.random.default_rng(1)
        for t in (streams[2], streams[3]):                       # four COMPRESS blocks each: two placing passes at group_frames 2
            index = ctx.index_stream(t.dev)
            counts = {}
            for (up, down), P in (((1, 1), 1), ((160, 441), 32), ((3, 2), 64)):
                coef = random_coef(rng, up, P)
                n_out = length(t, up, down)
                for nw in (1, 64):
                    spans = [(0, n_out)] + [(11 * i, n_out - 17 * i) for i in range(1, nw)]
                    lows = [max(a * down // up - P // 2, 0) for a, n in spans]      # the decode call of the windows' input ranges
                    dspans = [(lo, min((a + n - 1) * down // up - P // 2 + P, t.ns) - lo) for lo, (a, n) in zip(lows, spans)]
                    for gf in (0, 2):
                        ctx.decode_windows([(t.dev, index, a, n) for a, n in dspans], group_frames=gf)
                        dec = {k: ctx.last_launches(k) for k in DECODE_KINDS + [PLACE_KIND]}
                        got = ctx.resample_windows([(t.dev, index, a, n) for a, n in spans], up, down, coef=coef, before=P // 2, shift=15, clip_bits=16, group_frames=gf)
                        mine = {k: ctx.last_launches(k) for k in DECODE_KINDS + [PLACE_KIND, PRESET_KIND, RESAMPLE_KIND] + others}
                        a, n = spans[-1]
                        assert np.array_equal(got[-1].cpu().numpy(), expected_resample(t.full, a, n, coef, up, down, P // 2, 15, 16)[0])
                        assert all(mine[k] == 0 for k in others), (t.name, nw, gf, mine)
                        assert all(mine[k] == dec[k] for k in DECODE_KINDS + [PLACE_KIND]) and mine[PLACE_KIND] >= 1, (t.name, nw, gf, dec, mine)
                        assert mine[PRESET_KIND] == 1 and mine[RESAMPLE_KIND] == 1, (t.name, nw, gf, mine)
                        assert ctx.last_ms(RESAMPLE_KIND) > 0 and ctx.last_ms(PRESET_KIND) > 0
                        counts[(up, P, nw, gf)] = mine
                assert counts[(up, P, 1, 0)] == counts[(up, P, 64, 0)] and counts[(up, P, 1, 2)][PLACE_KIND] > 1
            assert counts[(1, 1, 64, 0)] == counts[(160, 32, 64, 0)] == counts[(3, 64, 64, 0)]
            index.close()
    finally:
        ctx.close()


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_history(streams):
    """the call behind and in front of measure, quiet and mix calls on one context, large then small and small then large"""
    ctx = linne_amd.Context(0, use_torch_stream=False)
    try:
        rng = np.random.default_rng(21)
        t, u = streams[2], streams[8]
        ti, ui = ctx.index_stream(t.dev), ctx.index_stream(u.dev)
        c3, c160 = random_coef(rng, 3, 16), random_coef(rng, 160, 33)
        small_ = [dict(item(t, 130, 257, c3, 3, 2, before=8, shift=16, clip_bits=16, fmt="s16", lay="interleaved"), index=ti)]
        large = [dict(item(u, 0, length(u, 160, 147), c160, 160, 147, before=16, shift=15, fmt=fmt, lay=lay), index=ui) for fmt, lay in (("f32", "planar"), ("s32", "planar"), ("s24", "interleaved"))] * 3
        eye = np.eye(2, dtype=np.int16)
        for first, second in ((large, small_), (small_, large)):
            for between in ("measure", "quiet", "mix"):
                held(ctx, first, group_frames=(0,))
                if between == "measure":
                    m = ctx.measure_windows([(t.dev, ti, 0, t.ns)] * 3, bucket_samples=0)
                    assert all(x.min.cpu().numpy().reshape(-1).tolist() == t.full.min(axis=1).tolist() for x in m) and len(m) == 3
                elif between == "quiet":
                    runs = ctx.quiet_windows([(t.dev, ti, 0, t.ns)] * 3, 3, 2)
                    assert [r.cpu() for r in runs] == [sc.expected_quiet(t.full, 0, t.ns, 3, 2)[0]] * 3
                else:
                    got = ctx.mix_windows([(t.dev, ti, 5, 2000)] * 2, eye)
                    assert all(np.array_equal(g.cpu().numpy(), t.full[:, 5:2005]) for g in got)
                held(ctx, second, group_frames=(0, 2))
        ti.close()
        ui.close()
    finally:
        ctx.close()


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_resample_streams(ctx, oracle, streams):
    t = streams[2]
    for u, rate in ((t, 16000), (t, 48000), (streams[3], 22050), (streams["24bit"], 44100), (streams[1], 16000)):
        up, down = linne_amd.resample_ratio(44100, rate)
        coef, shift, before = linne_amd.resample_design(up, down, 32)
        bits, block, preset, ms = (u.index.header[k] for k in ("bits_per_sample", "num_samples_per_block", "preset", "ch_process_method"))
        out, = ctx.resample_streams([u.dev], rate)
        got = bytes(out.cpu().numpy().tobytes())
        want = expected_resample(u.full, 0, length(u, up, down), coef, up, down, before, shift, bits)[0]
        ret, full, _ = oracle.decode_whole(got)
        assert ret == OK and np.array_equal(full, want), (u.name, rate)
        assert int.from_bytes(got[18:22], "big") == rate and got == bytes(oracle.encode_whole(want, bits, rate, block, preset, ms)), (u.name, rate)
    # many streams in one call, of different ratios; the header fields a caller gives; the designed filter in a window call
    outs = ctx.resample_streams([t.dev, streams[3].stream], 24000, taps=16, group_frames=2)
    for u, out in zip((t, streams[3]), outs):
        coef, shift, before = linne_amd.resample_design(80, 147, 16)
        want = expected_resample(u.full, 0, length(u, 80, 147), coef, 80, 147, before, shift, 16)[0]
        assert np.array_equal(oracle.decode_whole(bytes(out.cpu().numpy().tobytes()))[1], want)
    other, = ctx.resample_streams([t.dev], 16000, bits=24, preset=0, block=512, ms=0)
    coef, shift, before = linne_amd.resample_design(160, 441, 32)
    want = expected_resample(t.full, 0, length(t, 160, 441), coef, 160, 441, before, shift, 24)[0]
    assert bytes(other.cpu().numpy().tobytes()) == bytes(oracle.encode_whole(want, 24, 16000, 512, 0, False))
    got = ctx.resample_windows([(t.dev, t.index, 10, None), (t.dev, t.index, 0, 50)], [160, 1], [441, 2])
    assert np.array_equal(got[0].cpu().numpy(), expected_resample(t.full, 10, length(t, 160, 441) - 10, coef, 160, 441, before, shift)[0])
    c2, s2, b2 = linne_amd.resample_design(1, 2, 32)
    assert np.array_equal(got[1].cpu().numpy(), expected_resample(t.full, 0, 50, c2, 1, 2, b2, s2)[0])
    assert ctx.resample_streams([], 16000) == []
    with pytest.raises(ValueError):
        ctx.resample_streams([t.dev], 44101)
