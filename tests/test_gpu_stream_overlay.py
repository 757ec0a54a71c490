"""GPU tests of overlaying windows of several resident .lnn streams (Context.overlay_windows, overlay_streams, crossfade_streams;
include/linne_amd.h LINNEAmd_OverlayWindowsDevice).  Every expected element is computed with numpy int64 and Python integers
(overlay_refs.expected_overlay) from the oracle's decode of the same bytes, never from the library under test, and everything must be
equal: bytes and integers, no tolerance -- the float32 path is a conversion and a multiplication by a power of two.  Streams hold 2 to 6
blocks of 1024 samples, or 21 blocks of 33; one mono stream holds 65537 samples for the longest ramp."""
import numpy as np
import pytest

import linne_amd
import synth_records as sr
from overlay_refs import ELEMENT_BYTES, UNIT, expected_overlay
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
OVERLAY_KIND, PLACE_KIND = KIND["OVERLAY_T_OVERLAY"], KIND["T_WX_PLACE"]
LAYS = [("s32", "planar", 0), ("s32", "planar", 5), ("s16", "interleaved", 0), ("s24", "interleaved", 0), ("f32", "interleaved", 0),
        ("s24", "planar", 1), ("s16", "planar", 3), ("f32", "planar", 0), ("s32", "strided", 2), ("s16", "strided", 1)]


@pytest.fixture(scope="module")
def streams(ctx, oracle):
    """1, 2 (MS), 3 and 8 channels of 16 bits: 3 blocks and a tail of 300; "8bit" and "24bit": stereo streams of those widths and other
    presets; "small": stereo in blocks of 33 samples, the last of 5"""
    out = {nch: encoded(ctx, oracle, music(nch, 3 * S + TAIL, 16, seed=90 + nch), 16, 5 if nch == 2 else 0, nch == 2, f"{nch}ch") for nch in (1, 2, 3, 8)}
    out["8bit"] = encoded(ctx, oracle, music(2, 2 * S + 77, 8, seed=61), 8, 0, False, "8 bits")
    out["24bit"] = encoded(ctx, oracle, music(2, 2 * S + 77, 24, seed=62), 24, 2, True, "24 bits")
    x = music(2, 20 * 33 + 5, 16, seed=17)
    out["small"] = Stream(ctx, oracle, oracle.encode_whole(x, 16, 44100, 33, 0, False), "blocks of 33")
    assert np.array_equal(out["small"].full, x) and len(out["small"].bl) == 21 and out["small"].bl[-1][3] == 5
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
def long_mono(ctx, oracle):
    """mono, 65537 samples: a ramp from 32767 to -32768 takes a step of one at every sample of it"""
    t = encoded(ctx, oracle, music(1, 65537, 16, seed=33), 16, 0, False, "65537 samples")
    yield t
    t.index.close()


# ---- the C entry point on outputs that lie in one buffer of sentinels ----
def src(t, first, n, at, gain=1, **over):
    """a source: n samples of t from `first` on, laid at output sample `at`; gain: an int or a (gain_q32, step_q32) pair; over: dev and
    index of a damaged copy, or fields as they are given to the call whatever the reference would say"""
    return dict(t=t, first=first, n=n, at=at, gain=gain, over=over)


def item(n, srcs, shift=0, clip_bits=0, fmt="s32", lay="planar", pad=0, wrong=None):
    """an output of raw_overlay: lay "planar" (rows n + pad elements apart), "interleaved" (packed frames), "strided" (frames C + pad
    elements apart, channels one apart); wrong: the output's fields as they are given to the call"""
    return dict(n=n, srcs=srcs, shift=shift, clip=clip_bits, fmt=fmt, lay=lay, pad=pad, wrong=wrong or {}, nch=srcs[0]["t"].nch)


def strides(it):
    n, k = it["n"], it["nch"]
    return {"planar": (n + it["pad"], 1), "interleaved": (1, k), "strided": (1, k + it["pad"])}[it["lay"]]


def extent(it):
    cs, ss = strides(it)
    return (it["nch"] - 1) * cs + max(it["n"] - 1, 0) * ss + 1 if it["n"] else 0


def pair(gain):
    return (int(gain) * UNIT, 0) if isinstance(gain, (int, np.integer)) else (int(gain[0]), int(gain[1]))


def raw_overlay(ctx, items, group_frames=0, layouts=True):
    """LINNEAmd_OverlayWindowsDevice itself -> (ret, codes, the buffer's bytes, the outputs' byte offsets, their saturated words (7:
    left as it was))"""
    import torch
    offs, at = [], 16
    for it in items:
        at = (at + 3) & ~3
        at += 1 if it["fmt"] == "s24" else 0                    # (packed 24-bit samples lie anywhere)
        offs.append(at)
        at += max(extent(it), 1) * ELEMENT_BYTES[it["fmt"]] + 16
    buf = torch.full((at,), SENTINEL, dtype=torch.uint8, device="cuda")
    O = len(items)
    o, ly, keep = (linne_amd.Overlay * O)(), (linne_amd.PcmLayout * O)(), []
    for k, it in enumerate(items):
        srcs = (linne_amd.OverlaySource * max(len(it["srcs"]), 1))()
        keep.append(srcs)
        for j, s in enumerate(it["srcs"]):
            t = s["t"]
            dev, index = s["over"].get("dev", t.dev), s["over"].get("index", t.index)
            q, step = pair(s["gain"])
            f = dict(index=index.h if index is not None else None, d_stream=dev.data_ptr(), first_sample=s["first"], num_samples=s["n"], at=s["at"], gain_q32=q, step_q32=step, reserved=0)
            f.update({a: b for a, b in s["over"].items() if a not in ("dev", "index")})
            for a, b in f.items():
                setattr(srcs[j], a, b)
        cs, ss = strides(it)
        f = dict(sources=srcs, num_sources=len(it["srcs"]), shift=it["shift"], clip_bits=it["clip"], reserved=0, num_samples=it["n"], d_pcm=buf.data_ptr() + offs[k], pcm_stride=cs, result=-1)
        f.update({a: b for a, b in it["wrong"].items() if a not in ("channel_stride",)})
        for a, b in f.items():
            setattr(o[k], a, b)
        ly[k].format, ly[k].saturated, ly[k].channel_stride, ly[k].sample_stride = FMT[it["fmt"]], 7, it["wrong"].get("channel_stride", cs), ss
    torch.cuda.synchronize()
    ret = linne_amd.lib.LINNEAmd_OverlayWindowsDevice(ctx.h, o, ly if layouts else None, O, group_frames)
    return ret, [o[k].result for k in range(O)], buf.cpu().numpy().tobytes(), offs, [int(ly[k].saturated) for k in range(O)]


def reference(it):
    t0 = it["srcs"][0]["t"]
    return expected_overlay(it["n"], [(s["t"].full, s["first"], s["n"], s["at"], s["gain"]) for s in it["srcs"]], it["shift"], it["clip"], it["fmt"], t0.bits)


def want_overlay(items, codes, offs, size):
    """sentinels but the OK outputs' elements -> (the bytes, the saturated words)"""
    buf = np.full(size, SENTINEL, dtype=np.uint8)
    sats = []
    for it, code, off in zip(items, codes, offs):
        if code != OK:
            sats.append(7)
            continue
        n, es = it["n"], ELEMENT_BYTES[it["fmt"]]
        want, sat = reference(it)
        sats.append(int(sat))
        cs, ss = strides(it)
        raw = np.ascontiguousarray(want).view(np.uint8).reshape(it["nch"], n, es)
        for c in range(it["nch"]):
            at = off + (c * cs + np.arange(n) * ss) * es
            for b in range(es):
                buf[at + b] = raw[c, :, b]
    return buf.tobytes(), sats


def held(ctx, items, want_codes=None, group_frames=(0, 2)):
    """the call on the items, at every group_frames: codes, every byte of the buffer and the saturated words are the reference's"""
    want_codes = want_codes or [OK] * len(items)
    first = None
    for gf in group_frames:
        ret, codes, buf, offs, sats = raw_overlay(ctx, items, gf)
        assert codes == want_codes and ret == next((c for c in want_codes if c != OK), OK), (gf, codes, last_error(ctx))
        want, want_sats = want_overlay(items, want_codes, offs, len(buf))
        if buf != want:
            bad = next(i for i in range(len(buf)) if buf[i] != want[i])
            j = max(k for k in range(len(offs)) if offs[k] <= bad) if bad >= offs[0] else -1
            raise AssertionError(f"group_frames {gf}: byte {bad} (output {j} begins at {offs[j] if j >= 0 else 0}) is {buf[bad]:#x}, not {want[bad]:#x}")
        assert sats == want_sats, (gf, sats, want_sats)
        assert first is None or buf == first                    # group_frames never changes a byte
        first = buf
    return ret


def tensor_bytes(x):
    return np.ascontiguousarray(x.cpu().numpy()).tobytes()


# 1 ------------------------------------------------------------------------------------------------------------------------------
def test_identity_is_the_decode(ctx, streams, cut, wide):
    """one source at 0 with the gain 1, shift 0, clip_bits 0: the bytes and `saturated` of decode_windows on the same windows, in
    every layout"""
    import torch
    for t in (streams[1], streams[2], streams[3], streams[8], streams["small"], cut, wide):
        spans = [(0, t.ns), (517 % t.ns, min(1500, t.ns - 517 % t.ns)), (S - 1, 2), (S - 130, 257), (t.ns - 1, 1)] if t.ns > S + 200 else [(0, t.ns), (32, 2), (100, 257), (t.ns - 1, 1)]
        wins = [(t.dev, t.index, a, n) for a, n in spans]
        outs = [(n, [(t.dev, t.index, a, n, 0, 1)]) for a, n in spans]
        for kw in ({}, {"dtype": torch.int16, "channels_last": True}, {"s24": True}, {"dtype": torch.float32, "channels_last": True}, {"dtype": torch.int16}, {"dtype": torch.float32}):
            want, wsat = ctx.decode_windows(wins, return_saturated=True, **kw)
            for gf in (0, 2):
                got, gsat = ctx.overlay_windows(outs, return_saturated=True, group_frames=gf, **kw)
                assert [tensor_bytes(g) for g in got] == [tensor_bytes(x) for x in want] and gsat == wsat, (t.name, kw, gf)
                assert [tuple(g.shape) for g in got] == [tuple(x.shape) for x in want] and [g.dtype for g in got] == [x.dtype for x in want]
        assert t is not wide or any(ctx.decode_windows(wins, return_saturated=True, s24=True)[1])
        n = min(700, t.ns - 130)
        same = [(t.dev, t.index, a, n) for a in (0, 17, 130)]   # int32 with a padded stride
        big_d = torch.full((3, t.nch, n + 9), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        big_o = big_d.clone()
        ctx.decode_windows(same, out=big_d[:, :, :n])
        ctx.overlay_windows([(n, [w + (0, (UNIT, 0))]) for w in same], out=big_o[:, :, :n])
        assert tensor_bytes(big_o) == tensor_bytes(big_d)


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_source_counts_placement_and_gaps(ctx, streams):
    """1, 2, 3 and 64 sources; sources that begin and end on, one before and one after a multiple of 256 outputs; a source of one sample;
    gaps that no source covers; two sources of one stream that overlap; every channel count; every layout in turn"""
    rng = np.random.default_rng(8)
    items, k = [], 0
    for key in (1, 2, 3, 8):
        t = streams[key]
        for K in (1, 2, 3, 64):
            n_out = 1100
            srcs = []
            for j in range(K):
                n = int(rng.integers(1, 700))
                srcs.append(src(t, int(rng.integers(0, t.ns - n + 1)), n, int(rng.integers(0, n_out - n + 1)), int(rng.integers(-32768, 32768))))
            fmt, lay, pad = LAYS[k % len(LAYS)]
            items.append(item(n_out, srcs, shift=(0, 1, 14, 31)[k % 4], clip_bits=(0, 16, 24, 32, 2)[k % 5], fmt=fmt, lay=lay, pad=pad))
            k += 1
    t = streams[2]
    for b in (255, 256, 257):                                   # begins and ends around the tiles' edges, against a background
        for e in (511, 512, 513):
            fmt, lay, pad = LAYS[k % len(LAYS)]
            items.append(item(900, [src(t, 10, 900, 0, 3), src(t, 1000 + b, e - b, b, -5)], fmt=fmt, lay=lay, pad=pad))
            items.append(item(900, [src(t, S - 7, e - b, b, 16384)], shift=14, fmt=fmt, lay=lay, pad=pad))        # zeros in front and behind
            k += 1
    items.append(item(1, [src(t, 77, 1, 0, -32768)]))                                                               # one sample of one output
    items.append(item(600, [src(t, 5, 1, 0, 7), src(t, 5, 1, 255, 7), src(t, 6, 1, 256, 7), src(t, 7, 1, 599, 7)], fmt="s16", lay="interleaved"))     # single samples, and gaps
    items.append(item(3000, [src(t, 0, 2000, 0, 2), src(t, 500, 2500, 500, 3), src(t, 1000, 10, 1005, -1)], fmt="f32", lay="planar"))      # one stream, overlapping itself
    items.append(item(5000, [src(t, 0, t.ns, 1000, 1)], fmt="s24", lay="planar", pad=1))                            # a whole stream inside a longer output
    held(ctx, items, group_frames=(0, 1, 3))


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_mixed_streams_in_one_output(ctx, streams, cut):
    """sources of 8, 16 and 24 bits, of blocks of 33 and of 1024 samples, of different presets and MS, in one output; SILENT and RAW
    blocks and the tail behind the last block among them; the float scale is that of the FIRST source's width"""
    a, b, c, d, e = streams["8bit"], streams[2], streams["24bit"], streams["small"], cut
    items = []
    for k, order in enumerate(((a, b, c, d, e), (c, e, d, a, b), (d, c, b, e, a), (e, a, b, c, d))):
        fmt, lay, pad = [("f32", "planar", 0), ("f32", "interleaved", 0), ("s32", "planar", 2), ("s24", "interleaved", 0)][k]
        srcs = [src(t, 11 * j, min(t.ns - 11 * j, 1900), 40 * j, (3, -2, 1, 500, -1)[j]) for j, t in enumerate(order)]
        items.append(item(2100, srcs, shift=k, fmt=fmt, lay=lay, pad=pad))
    # the SILENT blocks, the RAW blocks and the tail of zeros, each under a moving gain and beside a sounding neighbour
    ramp = linne_amd.fade(300, -300, 1400)
    items.append(item(e.ns, [src(e, 0, e.ns, 0, 2), src(b, 0, b.ns, 100, 1)]))
    items.append(item(1500, [src(e, S - 50, 1400, 100, ramp), src(b, 0, 1500, 0, 1)], fmt="s16", lay="planar", pad=3))
    items.append(item(1400, [src(e, 4 * S - 9, 1400, 0, ramp)], fmt="f32", lay="interleaved"))
    items.append(item(2000, [src(e, 6 * S - 40, 1364, 636, ramp), src(e, 5 * S, 2000, 0, -1)], fmt="s24", lay="planar"))
    items.append(item(300, [src(e, e.ns - 300, 300, 0, 5)]))                                                        # the tail alone: zeros
    held(ctx, items, group_frames=(0, 1, 3))


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_ramps(ctx, streams, long_mono):
    """a ramp from 32767 to -32768 over 65537 samples, across 257 tiles; ramps over 2 samples; ramps with negative Q32 fractions; the
    two ramps of a crossfade"""
    t, m = streams[2], long_mono
    full = linne_amd.fade(32767, -32768, 65537)
    items = [item(65537, [src(m, 0, 65537, 0, full)], shift=15, clip_bits=16), item(65537, [src(m, 0, 65537, 0, linne_amd.fade(-32768, 32767, 65537)), src(m, 1, 65536, 0, full)], shift=16, fmt="s16")]
    items.append(item(2, [src(t, 500, 2, 0, linne_amd.fade(32767, -32768, 2))]))
    items.append(item(258, [src(t, 500, 2, 255, linne_amd.fade(0, 100, 2)), src(t, 0, 258, 0, 1)], fmt="s16", lay="interleaved"))
    for q, step in ((-1, 0), (-UNIT // 4, 0), (-UNIT - 1, 0), (UNIT - 1, -1), (0, -1), (-(5 << 32) - 123456789, -(1 << 20) - 3), (7 << 32, -(1 << 30) + 1), (-(32768 << 32), (1 << 28) + 5)):
        items.append(item(3000, [src(t, 100, 3000, 0, (q, step))], fmt=LAYS[len(items) % len(LAYS)][0], lay=LAYS[len(items) % len(LAYS)][1], pad=LAYS[len(items) % len(LAYS)][2]))
    for n, unity in ((1, 1), (2, 16384), (257, 32767), (2000, 16384)):
        down, up = linne_amd.crossfade(n, unity)
        items.append(item(n, [src(t, 0, n, 0, down), src(streams["24bit"], 50, n, 0, up)], shift=14))
    held(ctx, items, group_frames=(0, 3))
    # a constant under a crossfade with itself stays that constant
    down, up = linne_amd.crossfade(1000, 16384)
    ret, codes, buf, offs, _ = raw_overlay(ctx, [item(1000, [src(t, 0, 1000, 0, down), src(t, 0, 1000, 0, up)], shift=14)])
    got = np.frombuffer(buf, dtype=np.uint8)[offs[0]:offs[0] + 4 * 2000].view(np.int32).reshape(2, 1000)
    assert ret == OK and np.array_equal(got, t.full[:, :1000])


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_shift_clip_saturation_and_extremes(ctx, wide, streams):
    """shifts 0, 1, 14 and 31; saturation from the clip and from the format, and none; 64 sources of values over all of int32 under gains
    of +-32767 and -32768: sums of 2^52, which nothing wraps"""
    t, u = wide, streams[2]
    items = [item(t.ns, [src(t, 0, t.ns, 0, 32767), src(t, 0, t.ns, 0, 32767)], fmt=fmt, lay=lay, shift=sh, clip_bits=cb)
             for fmt, lay in (("s32", "planar"), ("s16", "interleaved"), ("s24", "planar"), ("f32", "interleaved")) for sh, cb in ((0, 0), (1, 0), (14, 0), (16, 16), (31, 2), (31, 0))]
    for g in (32767, -32767, -32768):
        items.append(item(t.ns, [src(t, 0, t.ns, 0, g)] * 64, shift=31))
        items.append(item(t.ns, [src(t, 0, t.ns, 0, g)] * 64, shift=22, clip_bits=32, fmt="f32"))
        items.append(item(t.ns, [src(t, j % 7, t.ns - 7, j % 5, g if j % 2 else -g - (g < 0)) for j in range(64)], shift=0, fmt="s24", lay="interleaved"))
    items += [item(u.ns, [src(u, 0, u.ns, 0, 1)], fmt="s16"), item(u.ns, [src(u, 0, u.ns, 0, 2)], fmt="s16"), item(u.ns, [src(u, 0, u.ns, 0, 1)], clip_bits=12)]
    ret, codes, buf, offs, sats = raw_overlay(ctx, items)
    want, want_sats = want_overlay(items, codes, offs, len(buf))
    assert ret == OK and codes == [OK] * len(items) and buf == want and sats == want_sats
    assert sats[0] == 1 and sats[-3] == 0 and 0 in sats[:24] and 1 in sats[-2:]                     # a clip is among them, and none
    acc = 64 * 32768 * np.abs(t.full.astype(np.int64)).max()
    assert acc > 1 << 51                                        # (the premise: the sums are as large as the call allows)


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_many_outputs_and_failures_stay_in_their_output(ctx, product, streams, cut):
    """64 outputs of mixed shapes in one buffer of sentinels, outputs with a CRC-damaged and a Rice-damaged source and with each
    argument error among them: a failing output's memory is untouched, its neighbours are exact, the lowest failing output's code and
    text are returned"""
    t = streams[2]
    crc, rice = sc.damaged(ctx, product, t)
    k, kr = crc[2], rice[2]
    rng = np.random.default_rng(4)
    twos = [streams[2], cut, streams["small"], streams["24bit"], streams["8bit"]]
    items, want_codes = [], [OK] * 64
    for i in range(64):
        pool = twos if i % 3 else [streams[(1, 3, 8)[(i // 3) % 3]]]
        n_out = int(rng.integers(1, 1200))
        srcs = []
        for j in range(int(rng.integers(1, 6))):
            u = pool[int(rng.integers(0, len(pool)))]
            n = int(rng.integers(1, min(n_out, u.ns) + 1))
            g0, g1 = (int(v) for v in rng.integers(-32768, 32768, size=2))
            srcs.append(src(u, int(rng.integers(0, u.ns - n + 1)), n, int(rng.integers(0, n_out - n + 1)), linne_amd.fade(g0, g1, n) if j % 2 else g0))
        fmt, lay, pad = LAYS[i % len(LAYS)]
        items.append(item(n_out, srcs, shift=(0, 15, 31, 20)[(i // 4) % 4], clip_bits=(0, 16, 24)[i % 3], fmt=fmt, lay=lay, pad=pad))
    good = lambda: src(t, 100, 600, 0, 3)

    def on(i, code, srcs, n=600, **wrong):
        fmt, lay, pad = LAYS[i % len(LAYS)]
        items[i] = item(n, srcs, shift=3, clip_bits=16, fmt=fmt, lay=lay, pad=pad, wrong=wrong)
        want_codes[i] = code
    on(5, NG, [good(), src(t, t.bl[kr][4] + 10, 600, 0, 2, dev=rice[0], index=rice[1])])        # over the Rice-damaged block: the fail word is set on the device
    on(6, OK, [src(t, t.bl[kr - 1][4] + 10, 600, 0, 2, dev=rice[0], index=rice[1]), good()])
    on(7, NG, [src(t, 0, t.ns, 0, 2, dev=rice[0], index=rice[1])], n=t.ns)
    on(9, CORRUPTION, [good(), good(), src(t, t.bl[k][4] + 3, 600, 0, 2, dev=crc[0], index=crc[1])])              # CRC damage: refused on the host
    on(10, OK, [src(t, 0, t.bl[k][4], 0, 2, dev=crc[0], index=crc[1]), good()], n=t.bl[k][4] + 700)               # in front of the damaged block
    on(11, CORRUPTION, [src(t, 0, t.bl[k][4] + 1, 0, 2, dev=crc[0], index=crc[1])], n=t.bl[k][4] + 1)
    on(12, NG, [src(t, t.bl[kr][4] + 10, 600, 0, 2, dev=rice[0], index=rice[1]), src(t, t.bl[k][4] + 3, 600, 0, 2, dev=crc[0], index=crc[1])])     # both: the lowest-numbered failing source's code,
    on(13, NG, [src(t, t.bl[kr][4] + 10, 600, 0, 2, dev=rice[0], index=rice[1]), src(t, 0, 10, 0, 2, first_sample=t.ns)])                           # ... though the device alone finds it and the host refuses source 1
    on(14, INVALID_ARGUMENT, [good(), src(t, t.ns - 599, 600, 0, 1), src(t, t.bl[kr][4] + 10, 600, 0, 2, dev=rice[0], index=rice[1])])                     # behind a source the host refuses nothing is looked at
    on(15, CORRUPTION, [good(), src(t, t.bl[k][4] + 3, 600, 0, 2, dev=crc[0], index=crc[1]), src(t, t.ns - 599, 600, 0, 1)])
    words = {}

    def bad(i, word, srcs=None, **wrong):
        on(i, INVALID_ARGUMENT, srcs or [good(), good()], **wrong)
        words[i] = word
    bad(20, "OverlayWindowsDevice: shift 32", shift=32)
    bad(21, "OverlayWindowsDevice: num_sources 0", num_sources=0)
    bad(22, "OverlayWindowsDevice: num_sources 65", num_sources=65)
    bad(23, "OverlayWindowsDevice: null sources", sources=None)
    bad(24, "OverlayWindowsDevice: clip_bits 1 ", clip_bits=1)
    bad(25, "OverlayWindowsDevice: clip_bits 33", clip_bits=33)
    bad(26, "OverlayWindowsDevice: reserved", reserved=5)
    bad(27, "OverlayWindowsDevice: source 1: num_samples 0", [good(), src(t, 0, 600, 0, 1, num_samples=0)])
    bad(28, "OverlayWindowsDevice: source 1: at 1 + 600", [good(), src(t, 0, 600, 1, 1)])
    bad(29, "OverlayWindowsDevice: source 0: at", [src(t, 0, 600, (1 << 64) - 1, 1), good()])
    bad(30, "OverlayWindowsDevice: source 1: a gain outside", [good(), src(t, 0, 600, 0, 1, gain_q32=32768 << 32)])
    bad(31, "OverlayWindowsDevice: source 0: a gain outside", [src(t, 0, 600, 0, 1, gain_q32=-(32768 << 32), step_q32=-1), good()])
    bad(32, "OverlayWindowsDevice: source 1: a gain outside", [good(), src(t, 0, 600, 0, (32767 << 32, 1 << 23))])      # 599 steps of 2^-9: past 32768 at the last sample alone
    bad(33, "OverlayWindowsDevice: source 2: 3 channels, source 0 has 2", [good(), good(), src(streams[3], 0, 600, 0, 1)])
    bad(34, "OverlayWindowsDevice: source 1: null argument", [good(), src(t, 0, 600, 0, 1, index=None)])
    bad(35, "OverlayWindowsDevice: source 1: reserved", [good(), src(t, 0, 600, 0, 1, reserved=1)])
    bad(36, "OverlayWindowsDevice: null d_pcm", d_pcm=None)
    items[37] = item(600, [good()], shift=3, fmt="s16", lay="planar", wrong=dict(channel_stride=599))                 # the layout's own check: the channels' rows overlap
    want_codes[37], words[37] = INVALID_ARGUMENT, "OverlayWindowsDevice: "
    bad(38, "source 1: DecodeStreamDevice: samples [", [good(), src(t, t.ns - 599, 600, 0, 1)])                      # a source's range beyond its stream: the window's check
    assert want_codes[:5] == [OK] * 5 and want_codes[8] == OK
    assert held(ctx, items, want_codes, group_frames=(0, 2)) == NG                                                      # the lowest failing output's
    text = last_error(ctx)
    assert text.startswith(f"output 5: source 1: block {kr} "), text
    for i, word in sorted(words.items()):
        ret1, codes1, buf1, *_ = raw_overlay(ctx, [items[i]])
        assert (ret1, codes1) == (INVALID_ARGUMENT, [INVALID_ARGUMENT]) and set(buf1) == {SENTINEL}, i
        assert last_error(ctx).startswith("output 0: ") and word in last_error(ctx), (i, last_error(ctx))
    for i, head in ((9, f"output 0: source 2: block {k} "), (11, f"output 0: source 0: block {k} "), (12, f"output 0: source 0: block {kr} "), (13, f"output 0: source 0: block {kr} "), (7, f"output 0: source 0: block {kr} "),
                    (14, "output 0: source 1: DecodeStreamDevice: samples ["), (15, f"output 0: source 1: block {k} ")):
        ret1, codes1, buf1, *_ = raw_overlay(ctx, [items[i]])
        assert (ret1, codes1) == (want_codes[i], [want_codes[i]]) and set(buf1) == {SENTINEL} and last_error(ctx).startswith(head), (i, last_error(ctx))
    # int32 planar without layouts: pcm_stride is the rows' distance, and is checked
    plain = [item(600, [good(), src(t, 0, 300, 300, -2)], pad=4), item(600, [good()], wrong=dict(pcm_stride=599)), item(600, [src(streams[1], 0, 600, 0, 1)], wrong=dict(pcm_stride=0))]
    ret, codes, buf, offs, sats = raw_overlay(ctx, plain, layouts=False)
    assert (ret, codes, sats) == (INVALID_ARGUMENT, [OK, INVALID_ARGUMENT, OK], [7, 7, 7]) and "output 1: OverlayWindowsDevice: pcm_stride 599 < 600 samples" == last_error(ctx)
    assert buf == want_overlay(plain, codes, offs, len(buf))[0]
    # the Python form: codes with return_codes, an error without; values outside the bounds before any call
    py = lambda it: (it["n"], [(s["over"].get("dev", s["t"].dev), s["over"].get("index", s["t"].index), s["first"], s["n"], s["at"], s["gain"]) for s in it["srcs"]])
    three = [py(items[i]) for i in (9, 10, 11)]
    got, pcodes = ctx.overlay_windows(three, shift=3, clip_bits=16, return_codes=True)
    assert pcodes == [CORRUPTION, OK, CORRUPTION] and np.array_equal(got[1].cpu().numpy(), expected_overlay(items[10]["n"], [(t.full, s["first"], s["n"], s["at"], s["gain"]) for s in items[10]["srcs"]], 3, 16)[0])
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.overlay_windows(three, shift=3)
    assert e.value.code == CORRUPTION and e.value.codes == pcodes and "output 0: source 2:" in str(e.value)
    assert ctx.overlay_windows([]) == [] and ctx.overlay_windows([], return_codes=True) == ([], [])
    w = (t.dev, t.index, 0, 100)
    for outputs, kw in (([(100, [])], {}), ([(100, [w + (0, 1)] * 65)], {}), ([(100, [w + (1, 1)])], {}), ([(100, [w + (0, 32768)])], {}), ([(100, [w + (0, (32767 << 32, 1 << 30))])], {}),
                        ([(100, [w + (0, 1)])], {"shift": 32}), ([(100, [w + (0, 1)])], {"clip_bits": 1}), ([(100, [w + (0, 1), (streams[3].dev, streams[3].index, 0, 100, 0, 1)])], {}),
                        ([(100, [(t.dev, t.index, 5, 0, 0, 1)])], {})):
        with pytest.raises(ValueError):
            ctx.overlay_windows(outputs, **kw)
    for _, index, _ in (crc, rice):
        index.close()


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(streams):
    """the decode call's launches over the sources, kind 59 among them, and kind 101 once, none of any other consumer's; the same for
    one output and for 64, for one source and for 64"""
    others = sorted(k for c in sc.CONSUMERS.values() for k in c.kinds if k != PLACE_KIND) + [KIND["MIX_T_MIX"], KIND["RESAMPLE_T_PRESET"], KIND["RESAMPLE_T_RESAMPLE"]]
    assert OVERLAY_KIND == 101 and 101 not in others
    ctx = linne_amd.Context(0, use_torch_stream=False)
    try:
        ctx.enable_timing(True)
        for t in (streams[2], streams[3]):                       # four COMPRESS blocks each: two placing passes at group_frames 2
            index = ctx.index_stream(t.dev)
            counts = {}
            for no, K in ((1, 1), (64, 1), (1, 64), (64, 3)):
                spans = [(0, t.ns)] + [(11 * i, t.ns - 17 * i) for i in range(1, no * K)]
                outputs = [(t.ns, [(t.dev, index, a, n, i % 5, 2 + i) for i, (a, n) in enumerate(spans[o * K:(o + 1) * K])]) for o in range(no)]
                for gf in (0, 2):
                    ctx.decode_windows([(t.dev, index, a, n) for a, n in spans], group_frames=gf)
                    dec = {k: ctx.last_launches(k) for k in DECODE_KINDS + [PLACE_KIND]}
                    got = ctx.overlay_windows(outputs, shift=4, clip_bits=16, group_frames=gf)
                    mine = {k: ctx.last_launches(k) for k in DECODE_KINDS + [PLACE_KIND, OVERLAY_KIND] + others}
                    want = expected_overlay(t.ns, [(t.full, a, n, i % 5, 2 + i) for i, (a, n) in enumerate(spans[(no - 1) * K:])], 4, 16)[0]
                    assert np.array_equal(got[-1].cpu().numpy(), want)
                    assert all(mine[k] == 0 for k in others), (t.name, no, K, gf, mine)
                    assert all(mine[k] == dec[k] for k in DECODE_KINDS + [PLACE_KIND]) and mine[PLACE_KIND] >= 1, (t.name, no, K, gf, dec, mine)
                    assert mine[OVERLAY_KIND] == 1 and ctx.last_ms(OVERLAY_KIND) > 0, (t.name, no, K, gf, mine)
                    counts[(no, K, gf)] = mine
                assert counts[(no, K, 2)][PLACE_KIND] > 1
            assert counts[(1, 1, 0)] == counts[(64, 1, 0)] == counts[(1, 64, 0)] == counts[(64, 3, 0)]
            index.close()
    finally:
        ctx.close()


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_history(streams, long_mono):
    """the call behind and in front of measure, quiet, mix and resample calls on one context, large then small then large"""
    ctx = linne_amd.Context(0, use_torch_stream=False)
    try:
        t, u, m = streams[2], streams[8], long_mono
        ti, ui, mi = ctx.index_stream(t.dev), ctx.index_stream(u.dev), ctx.index_stream(m.dev)
        ramp = linne_amd.fade(-300, 700, 257)
        small_ = [item(300, [src(t, 130, 257, 43, ramp, index=ti), src(t, 0, 300, 0, 2, index=ti)], shift=2, clip_bits=16, fmt="s16", lay="interleaved")]
        large = [item(u.ns, [src(u, 0, u.ns, 0, 3, index=ui), src(u, 500, 2000, 100, -2, index=ui)], fmt=fmt, lay=lay) for fmt, lay in (("f32", "planar"), ("s32", "planar"), ("s24", "interleaved"))] * 2
        large.append(item(65537, [src(m, 0, 65537, 0, linne_amd.fade(32767, -32768, 65537), index=mi)], shift=15))
        eye = np.eye(2, dtype=np.int16)
        for between in ("measure", "quiet", "mix", "resample"):
            held(ctx, large, group_frames=(0,))
            held(ctx, small_, group_frames=(0,))
            if between == "measure":
                got = ctx.measure_windows([(t.dev, ti, 0, t.ns)] * 3, bucket_samples=0)
                assert all(x.min.cpu().numpy().reshape(-1).tolist() == t.full.min(axis=1).tolist() for x in got) and len(got) == 3
            elif between == "quiet":
                runs = ctx.quiet_windows([(t.dev, ti, 0, t.ns)] * 3, 3, 2)
                assert [r.cpu() for r in runs] == [sc.expected_quiet(t.full, 0, t.ns, 3, 2)[0]] * 3
            elif between == "mix":
                got = ctx.mix_windows([(t.dev, ti, 5, 2000)] * 2, eye)
                assert all(np.array_equal(g.cpu().numpy(), t.full[:, 5:2005]) for g in got)
            else:
                got = ctx.resample_windows([(t.dev, ti, 5, 2000)] * 2, 1, 1, coef=np.array([[1]], dtype=np.int16))
                assert all(np.array_equal(g.cpu().numpy(), t.full[:, 5:2005]) for g in got)
            held(ctx, small_, group_frames=(0, 2))
            held(ctx, large, group_frames=(0, 2))
        for x in (ti, ui, mi):
            x.close()
    finally:
        ctx.close()


# 9 ------------------------------------------------------------------------------------------------------------------------------
def stream_bytes(x):
    return bytes(x.cpu().numpy().tobytes())


def test_overlay_streams(ctx, oracle, streams):
    t, u, w = streams[2], streams["24bit"], streams["small"]
    head = lambda x: tuple(x.index.header[k] for k in ("bits_per_sample", "num_samples_per_block", "preset", "ch_process_method"))
    ramp = linne_amd.fade(16384, 0, u.ns)
    jobs = [(t.ns, [(t.dev, 0, None, 0, 12000), (u.dev, 0, None, 500, ramp), (w.dev, 5, 600, 2000, -9000)]), (1000, [(u.dev, 77, 900, 50, 16384)]), (t.ns + 10, [(t.dev, 0, None, 10, 16384)])]
    outs = ctx.overlay_streams(jobs, 14)
    wants = [expected_overlay(t.ns, [(t.full, 0, t.ns, 0, 12000), (u.full, 0, u.ns, 500, ramp), (w.full, 5, 600, 2000, -9000)], 14, 16)[0],
             expected_overlay(1000, [(u.full, 77, 900, 50, 16384)], 14, 24)[0], expected_overlay(t.ns + 10, [(t.full, 0, t.ns, 10, 16384)], 14, 16)[0]]
    for out, want, first in zip(outs, wants, (t, u, t)):
        bits, block, preset, ms = head(first)
        got = stream_bytes(out)
        ret, full, _ = oracle.decode_whole(got)
        assert ret == OK and np.array_equal(full, want), first.name
        assert got == bytes(oracle.encode_whole(want, bits, 44100, block, preset, ms)), first.name
    other, = ctx.overlay_streams([(1000, [(u.dev, 77, 900, 50, 16384)])], [14], bits=16, preset=0, block=512, ms=0, group_frames=2)
    assert stream_bytes(other) == bytes(oracle.encode_whole(expected_overlay(1000, [(u.full, 77, 900, 50, 16384)], 14, 16)[0], 16, 44100, 512, 0, False))
    assert ctx.overlay_streams([], 14) == []
    rate = bytearray(t.stream)
    rate[18:22] = (48000).to_bytes(4, "big")
    with pytest.raises(ValueError):
        ctx.overlay_streams([(t.ns, [(t.dev, 0, None, 0, 1), (sc.to_device(bytes(rate)), 0, None, 0, 1)])], 0)
    with pytest.raises(ValueError):
        ctx.overlay_streams([(t.ns, [])], 0)


def test_crossfade_streams(ctx, oracle, streams):
    t, u = streams[2], streams["24bit"]
    decode = lambda out: oracle.decode_whole(stream_bytes(out))[1]
    # overlap 0: what the splice_streams join decodes to
    v = encoded(ctx, oracle, music(2, 2 * S + 77, 16, seed=5), 16, 5, True, "a second stream of the first's shape")
    cuts = [[(t.dev, t.index, 0, t.ns), (v.dev, v.index, 0, v.ns), (t.dev, t.index, 0, t.ns)]]
    spliced = ctx.splice_streams(cuts)[0]
    joined = ctx.crossfade_streams([t.dev, v.dev, t.dev], 0)
    assert np.array_equal(decode(joined), decode(spliced)) and np.array_equal(decode(joined), np.concatenate([t.full, v.full, t.full], axis=1))
    v.index.close()
    # an overlap: the reference's sum of the two ramps, re-encoded with the first stream's header
    for ov in (1, 2, 257, 1000, u.ns):
        down, up = linne_amd.crossfade(ov, 16384)
        parts = [(t.full, 0, t.ns - ov, 0, 16384), (t.full, t.ns - ov, ov, t.ns - ov, down), (u.full, 0, ov, t.ns - ov, up)] + ([(u.full, ov, u.ns - ov, t.ns, 16384)] if u.ns > ov else [])
        want = expected_overlay(t.ns + u.ns - ov, parts, 14, 16)[0]
        got = stream_bytes(ctx.crossfade_streams([t.dev, u.dev], ov))
        assert got == bytes(oracle.encode_whole(want, 16, 44100, S, 5, True)), ov
    # a stream named twice with other streams between and behind it, all of different lengths: every stream keeps its own index
    w, e = streams["small"], streams["8bit"]
    assert len({t.ns, u.ns, w.ns}) == 3 and e.ns != w.ns and e.ns != t.ns
    for order, ov in (((t, u, t, w), 300), ((w, t, u, t, e), 200), ((t, u, t, w), 0), ((u, w, w, t, w), 332)):
        down, up = linne_amd.crossfade(ov, 16384) if ov else (None, None)
        parts, at = [], 0
        for i, x in enumerate(order):
            head, tail = ov if i else 0, ov if i + 1 < len(order) else 0
            parts += ([(x.full, 0, head, at, up)] if head else []) + ([(x.full, head, x.ns - head - tail, at + head, 16384)] if x.ns - head - tail else [])
            parts += [(x.full, x.ns - tail, tail, at + x.ns - tail, down)] if tail else []
            at += x.ns - tail
        bits, block, preset, ms = (order[0].index.header[k] for k in ("bits_per_sample", "num_samples_per_block", "preset", "ch_process_method"))
        want = expected_overlay(at, parts, 14, bits)[0]
        got = stream_bytes(ctx.crossfade_streams([x.dev for x in order], ov))
        assert np.array_equal(oracle.decode_whole(got)[1], want), ([x.name for x in order], ov)
        assert got == bytes(oracle.encode_whole(want, bits, 44100, block, preset, ms)), ([x.name for x in order], ov)
    # ... and in overlay_streams, where a stream named twice is indexed once
    got, = ctx.overlay_streams([(t.ns, [(t.dev, 0, 1000, 0, 16384), (u.dev, 0, 500, 100, 16384), (t.dev, 1000, 1000, 1000, 8192), (w.dev, 0, 600, 50, -16384)])], 14)
    want = expected_overlay(t.ns, [(t.full, 0, 1000, 0, 16384), (u.full, 0, 500, 100, 16384), (t.full, 1000, 1000, 1000, 8192), (w.full, 0, 600, 50, -16384)], 14, 16)[0]
    assert np.array_equal(decode(got), want)
    # a constant track crossfaded with itself stays constant
    const = sc.to_device(oracle.encode_whole(np.full((2, 3000), -12345, dtype=np.int32), 16, 44100, S, 0, False))
    for ov in (1, 255, 3000):
        assert set(decode(ctx.crossfade_streams([const, const], ov)).reshape(-1).tolist()) == {-12345}
    assert set(decode(ctx.crossfade_streams([const, const, const], 1500)).reshape(-1).tolist()) == {-12345}
    assert np.array_equal(decode(ctx.crossfade_streams([t.dev], 0)), t.full)
    for bad in (([t.dev, u.dev], u.ns + 1), ([t.dev, u.dev, t.dev], u.ns // 2 + 1), ([], 0), ([t.dev], -1)):
        with pytest.raises(ValueError):
            ctx.crossfade_streams(*bad)
