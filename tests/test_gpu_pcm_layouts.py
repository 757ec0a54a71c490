"""GPU tests of the resident stream path on PCM that is not int32 planar (include/linne_amd.h struct LINNEAmdPcmLayout;
LINNEAmd_EncodeStreamDeviceLayout, LINNEAmd_EncodeStreamsDeviceLayout, LINNEAmd_DecodeWindowsDeviceLayout): int16, packed 24-bit
and float samples, planar or interleaved, padded or not.  Encoding is held to the reference's recorded bytes and to the int32 planar
call's bytes and quirk-Q2 state; decoding to numpy's conversion of decode_stream's int32 samples, with sentinels in every gap of the
outputs; both to the launch counts of the int32 planar call."""
import ctypes as C
import hashlib
import json
import os
import wave

import numpy as np
import pytest

import linne_amd
from linne_amd import PCM_F32, PCM_S16, PCM_S24, PCM_S32
from signals import music
from test_gpu_stream_encode import alternating
from stream_consumers import crc_damaged, to_device
from stream_refs import blocks, mixed_signal

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OK, INVALID_ARGUMENT, CORRUPTION = 0, 1, 6
COMPRESS, SILENT, RAW = 0, 1, 2
ESIZE = {PCM_S32: 4, PCM_S16: 2, PCM_S24: 3, PCM_F32: 4}
RANGE = {PCM_S16: (-32768, 32767), PCM_S24: (-(1 << 23), (1 << 23) - 1)}


def as_bytes(t):
    return bytes(t.cpu().numpy())


def elements(x, fmt):
    """int (..., ) -> the numpy array of the format's elements: int32, int16, or uint8 (..., 3) little-endian"""
    x = np.asarray(x)
    if fmt == PCM_S32:
        return x.astype(np.int32)
    if fmt == PCM_S16:
        return x.astype(np.int16)
    u = x.astype(np.int64) & 0xFFFFFF
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, u >> 16], axis=-1).astype(np.uint8)


def from_elements(a, fmt):
    """the inverse: the format's elements -> int32 (S24 sign-extended) or float32"""
    if fmt == PCM_S24:
        a = a.astype(np.int32)
        return ((a[..., 0] | (a[..., 1] << 8) | (a[..., 2] << 16)) << 8) >> 8
    return a


def device_pcm(x, fmt, interleaved, byte_offset=0, pad_channel=0, pad_sample=0, sentinel=0x5A):
    """x int32 (C, N) in device memory as `fmt`: a (C, N[, 3]) view, planar or interleaved, of an allocation that ends with the last
    element the layout names (and starts byte_offset bytes before the first); pad_channel / pad_sample widen the strides, and the
    gaps hold sentinel bytes"""
    import torch
    e = elements(x, fmt)
    C_, N = x.shape
    k = 1 + pad_sample
    if interleaved:                                             # [N][C + pad_channel][k]
        box = np.full((N, C_ + pad_channel, k) + e.shape[2:], sentinel, dtype=e.dtype)
        box[:, :C_, 0] = np.moveaxis(e, 0, 1)
        cs, ss = k, (C_ + pad_channel) * k
    else:                                                       # [C][N + pad_channel][k]
        box = np.full((C_, N + pad_channel, k) + e.shape[2:], sentinel, dtype=e.dtype)
        box[:, :N, 0] = e
        cs, ss = (N + pad_channel) * k, k
    last = (C_ - 1) * cs + (N - 1) * ss + 1                     # the elements the layout spans
    flat = box.reshape(-1).view(np.uint8)[:last * ESIZE[fmt]]
    raw = torch.from_numpy(np.concatenate([np.full(byte_offset, sentinel, dtype=np.uint8), flat])).cuda()
    body = raw[byte_offset:]
    if fmt == PCM_S24:
        return torch.as_strided(body, (C_, N, 3), (3 * cs, 3 * ss, 1))
    return torch.as_strided(body.view(torch.int16 if fmt == PCM_S16 else torch.int32), (C_, N), (cs, ss))


def int32_planar(ctx, x, bits, rate, block, preset, ms, **kw):
    import torch
    return ctx.encode_stream(torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda(), bits, rate, block, preset, ms, **kw)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "golden_streams.npz"))


# 1 ------------------------------------------------------------------------------------------------------------------------------
def test_reference_bytes_from_raw_wav_data(ctx):
    import torch
    path = os.path.join(HERE, "golden", "ref_16bit_2ch.wav")
    with wave.open(path, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getnframes(), w.getframerate()) == (2, 2, 44100, 44100)
        data = w.readframes(w.getnframes())
    raw = open(path, "rb").read()
    at = raw.index(data)                                         # the data chunk as it lies in the file
    chunk = torch.from_numpy(np.frombuffer(raw[at:at + len(data)], dtype=np.uint8).copy()).cuda()
    pcm = chunk.view(torch.int16).view(44100, 2).T               # interleaved: channel stride 1, sample stride 2
    assert pcm.stride() == (1, 2)
    hashes = json.load(open(os.path.join(HERE, "golden", "golden_hashes.json")))
    for preset in (4, 7):
        want = hashes[f"wav/ref_16bit_2ch.wav_m{preset}"]
        got = as_bytes(ctx.encode_stream(pcm, 16, 44100, 10240, preset, True))
        assert len(got) == want["bytes"] and hashlib.sha256(got).hexdigest() == want["sha256"], preset


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_golden_streams_mixed_layouts_in_one_call(ctx, golden):
    tracks, want, shapes = [], [], set()
    for i in range(12):
        bits, rate, block, preset, ms = (int(v) for v in golden[f"s{i}_meta"])
        x = golden[f"s{i}_x"]
        shapes.add((x.shape[0], bits, block, preset, ms))
        for fmt in [f for f, wide in ((PCM_S16, 16), (PCM_S24, 24), (PCM_S32, 32)) if bits <= wide]:
            for inter in (False, True):
                tracks.append((device_pcm(x, fmt, inter), bits, rate, block, preset, bool(ms)))
                want.append((i, fmt, inter))
    assert len(tracks) >= 48
    got = ctx.encode_streams(tracks)
    assert ctx.last_stream_batch_count(0) == len(shapes) > 1     # layouts do not split shape groups
    for g, (i, fmt, inter) in zip(got, want):
        assert as_bytes(g) == golden[f"s{i}_lnn"].tobytes(), (i, fmt, inter)


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_edges_on_encode(ctx):
    block, preset = 1024, 2
    cases = []          # (x, bits, fmt, interleaved, keywords of device_pcm)
    for k, C_ in enumerate((1, 2, 3, 8)):
        for j, n in enumerate((1, block - 1, 2 * block + 1, 3 * block + 517)):
            x16 = music(C_, n, 16, seed=300 + 10 * k + j)
            x24 = music(C_, n, 24, seed=400 + 10 * k + j)
            cases.append((x24, 24, PCM_S24, bool(j & 1), dict(byte_offset=1 + (k + j) % 3)))            # S24 bases at byte offsets 1, 2, 3
            cases.append((x16, 16, PCM_S16, not (j & 1), dict(byte_offset=2 * (1 + 2 * (j & 1)))))      # S16 at an odd element offset
            cases.append((x16, 16, PCM_S24, bool(j & 1), dict(byte_offset=0)))
            cases.append((x24, 24, PCM_S32, True, dict()))
    x16, x24 = music(2, 2 * block + 77, 16, seed=500), music(3, block + 300, 24, seed=501)
    for fmt, x, bits in ((PCM_S16, x16, 16), (PCM_S24, x24, 24), (PCM_S32, x24, 24), (PCM_S24, x16, 16)):
        cases.append((x, bits, fmt, False, dict(pad_channel=5)))                    # padded channel stride, planar
        cases.append((x, bits, fmt, False, dict(pad_channel=3, pad_sample=1)))      # and a sample stride of 2
        cases.append((x, bits, fmt, True, dict(pad_channel=2)))                     # interleaved frames wider than C
        cases.append((x, bits, fmt, True, dict(pad_channel=1, pad_sample=2)))       # and a channel stride of 3
    assert {c[4].get("byte_offset") for c in cases if c[2] == PCM_S24} >= {1, 2, 3}
    tracks = [(device_pcm(x, fmt, inter, **kw), bits, 44100, block, preset, x.shape[0] > 1) for x, bits, fmt, inter, kw in cases]
    for t, (x, bits, fmt, inter, kw) in zip(tracks, cases):
        assert t[0].shape[:2] == x.shape and np.array_equal(from_elements(t[0].cpu().numpy(), fmt), x), (fmt, inter, kw)
    want = {}
    for x, bits, fmt, inter, kw in cases:
        key = id(x)
        if key not in want:
            want[key] = as_bytes(int32_planar(ctx, x, bits, 44100, block, preset, x.shape[0] > 1))
    for gf in (0, 3):                                            # 3: tracks span passes
        got = ctx.encode_streams(tracks, group_frames=gf)
        for g, (x, bits, fmt, inter, kw) in zip(got, cases):
            assert as_bytes(g) == want[id(x)], (gf, x.shape, bits, fmt, inter, kw)
    # and the single call
    for idx in (0, 1, len(cases) - 1, len(cases) - 6):
        x, bits, fmt, inter, kw = cases[idx]
        for gf in (0, 2):
            assert as_bytes(ctx.encode_stream(tracks[idx][0], bits, 44100, block, preset, x.shape[0] > 1, group_frames=gf)) \
                == want[id(x)], (idx, gf)


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_block_types(ctx):
    a16 = alternating(nblocks=5, seed=21)                        # COMPRESS and RAW at 16 bits
    m24 = mixed_signal(2, 24, 7 * 1024, seed=22, block=1024)     # COMPRESS, SILENT and RAW at 24 bits
    for x, bits, block, preset, fmt, inter, want_types in ((a16, 16, 4096, 7, PCM_S16, True, {COMPRESS, RAW}),
                                                           (m24, 24, 1024, 4, PCM_S24, True, {COMPRESS, SILENT, RAW}),
                                                           (m24, 24, 1024, 4, PCM_S24, False, {COMPRESS, SILENT, RAW})):
        ref, ref_state = int32_planar(ctx, x, bits, 44100, block, preset, True, parcor_state=0.0)
        ref = as_bytes(ref)
        assert want_types <= {b[2] for b in blocks(ref)}
        pcm = device_pcm(x, fmt, inter)
        for gf in (0, 2):
            got, state = ctx.encode_stream(pcm, bits, 44100, block, preset, True, group_frames=gf, parcor_state=0.0)
            assert (as_bytes(got), state) == (ref, ref_state), (bits, fmt, inter, gf)
        streams, states = ctx.encode_streams([(pcm, bits, 44100, block, preset, True)] * 2, group_frames=3, parcor_states=[0.0, 0.0])
        assert [(as_bytes(s), st) for s, st in zip(streams, states)] == [(ref, ref_state)] * 2


# 5 .. 9: decoding ---------------------------------------------------------------------------------------------------------------
class Stream:
    """a stream with all three block types whose header names `extra` samples more than its blocks hold"""
    def __init__(self, ctx, product, nch, bits, block, preset, seed, extra=0, scale=None):
        x = mixed_signal(nch, bits, 7 * block + 300, seed=seed, block=block)
        if scale is not None:
            x = (x.astype(np.int64) * scale[0] // scale[1]).astype(np.int32)
        s = bytearray(product.encode_whole(x, bits, 44100, block, preset, nch > 1))
        self.bl = blocks(bytes(s))
        s[14:18] = (x.shape[1] + extra).to_bytes(4, "big")
        self.stream, self.bits, self.nch, self.ns = bytes(s), bits, nch, x.shape[1] + extra
        self.dev = to_device(self.stream)
        self.index = ctx.index_stream(self.dev)
        self.full = ctx.decode_stream(self.dev, index=self.index).cpu().numpy()
        assert self.full.shape == (nch, self.ns) and np.array_equal(self.full[:, :x.shape[1]], x) and not self.full[:, x.shape[1]:].any()
        assert {COMPRESS, SILENT, RAW} <= {b[2] for b in self.bl}


@pytest.fixture(scope="module")
def s16(ctx, product):
    s = Stream(ctx, product, 2, 16, 1024, 4, seed=31, extra=700)
    yield s
    s.index.close()


@pytest.fixture(scope="module")
def s24(ctx, product):
    s = Stream(ctx, product, 3, 24, 1024, 3, seed=32, extra=300)
    assert s.full.max() > 32767 and s.full.min() < -32768
    yield s
    s.index.close()


def converted(v, fmt, bits):
    """numpy's conversion of int32 samples -> (the format's values, saturated)"""
    if fmt == PCM_F32:
        return v.astype(np.float32) * np.float32(2.0 ** -(bits - 1)), False
    if fmt == PCM_S32:
        return v, False
    lo, hi = RANGE[fmt]
    c = np.clip(v, lo, hi)
    return c.astype(np.int16) if fmt == PCM_S16 else c.astype(np.int32), bool((c != v).any())


def windows_of(s):
    bl = s.bl
    raw, silent = (next(b for b in bl if b[2] == t) for t in (RAW, SILENT))
    return [(5, 0), (bl[1][4] - 1, 1), (bl[2][4] + 7, 1), (17, 3 * 1024 + 5), (raw[4] - 300, raw[3] + 611), (silent[4] + 3, 1500),
            (s.ns - 1000, 1000), (s.ns - 200, 200), (bl[-1][4] + 10, s.ns - bl[-1][4] - 10), (1, s.ns - 2)]


def padded_out(fmt, W, C_, n, channels_last, sentinel):
    """a sentinel-filled (W, C + 1, n + 3) or (W, n + 3, C + 1) tensor and its (W, C, n) / (W, n, C) middle"""
    import torch
    dt = {PCM_S32: torch.int32, PCM_S16: torch.int16, PCM_S24: torch.uint8, PCM_F32: torch.float32}[fmt]
    shape = (W, n + 3, C_ + 1) if channels_last else (W, C_ + 1, n + 3)
    box = torch.full(shape + ((3,) if fmt == PCM_S24 else ()), sentinel, dtype=dt, device="cuda")
    mid = box[:, 1:n + 1, :C_] if channels_last else box[:, :C_, 2:n + 2]
    return box, mid


@pytest.mark.parametrize("fmt", [PCM_S32, PCM_S16, PCM_S24, PCM_F32])
@pytest.mark.parametrize("channels_last", [False, True])
def test_decode_formats(ctx, s16, s24, fmt, channels_last):
    import torch
    kw = dict(s24=True) if fmt == PCM_S24 else dict(dtype={PCM_S32: torch.int32, PCM_S16: torch.int16, PCM_F32: torch.float32}[fmt])
    for s in (s16, s24):
        wins = windows_of(s)
        got, sat = ctx.decode_windows([(s.dev, s.index, a, n) for a, n in wins], channels_last=channels_last, return_saturated=True, **kw)
        for (a, n), g, flag in zip(wins, got, sat):
            want, want_sat = converted(s.full[:, a:a + n], fmt, s.bits)
            g = from_elements(g.cpu().numpy(), fmt)
            g = g.T if channels_last else g
            assert g.shape == want.shape and g.dtype == want.dtype and np.array_equal(g, want), (s.bits, a, n)
            assert flag == want_sat, (s.bits, a, n)
        # into sentinel-filled, padded outputs, one window shape at a time; group_frames 2: windows in several passes
        n = 2 * 1024 + 301
        starts = [3, s.bl[1][4] - 150, s.ns - n - 77, s.ns - n]
        box, mid = padded_out(fmt, len(starts), s.nch, n, channels_last, 77)
        back = ctx.decode_windows([(s.dev, s.index, a, n) for a in starts], out=mid, channels_last=channels_last, group_frames=2, **kw)
        assert back is mid
        h = box.cpu().numpy()
        for i, a in enumerate(starts):
            want, _ = converted(s.full[:, a:a + n], fmt, s.bits)
            g = from_elements(mid[i].cpu().numpy(), fmt)
            assert np.array_equal(g.T if channels_last else g, want), (s.bits, a)
        hole = np.ones(h.shape, dtype=bool)
        if channels_last:
            hole[:, 1:n + 1, :s.nch] = False
        else:
            hole[:, :s.nch, 2:n + 2] = False
        assert (h[hole] == 77).all(), "a byte outside the windows' elements was written"


def test_saturation(ctx, s16, s24):
    import torch
    a, n = s24.bl[0][4] + 11, 2500
    v = s24.full[:, a:a + n]
    assert v.max() > 32767 and v.min() < -32768
    got, sat = ctx.decode_stream(s24.dev, a, n, index=s24.index, dtype=torch.int16, return_saturated=True)
    assert sat is True and np.array_equal(got.cpu().numpy(), np.clip(v, -32768, 32767).astype(np.int16))
    got, sat = ctx.decode_stream(s16.dev, a, n, index=s16.index, dtype=torch.int16, return_saturated=True)
    assert sat is False and np.array_equal(got.cpu().numpy(), s16.full[:, a:a + n].astype(np.int16))
    got, sat = ctx.decode_stream(s24.dev, a, n, index=s24.index, s24=True, return_saturated=True)
    assert sat is False and np.array_equal(from_elements(got.cpu().numpy(), PCM_S24), v)
    f = ctx.decode_stream(s24.dev, a, n, index=s24.index, dtype=torch.float32).cpu().numpy()
    assert f.dtype == np.float32 and np.array_equal(f.astype(np.float64) * 2.0 ** 23, v.astype(np.float64))     # exact
    # a window that saturates beside one that does not
    quiet = next(b for b in s24.bl if b[2] == SILENT)
    _, sats = ctx.decode_windows([(s24.dev, s24.index, quiet[4], 100), (s24.dev, s24.index, a, n)], dtype=torch.int16, return_saturated=True)
    assert sats == [False, True]


def test_a_failing_window_among_good_ones(ctx, s16):
    import torch

    class T:
        stream, bl = s16.stream, s16.bl
    bad, k = crc_damaged(T)
    d_bad = to_device(bad)
    index = ctx.index_stream(d_bad)
    n = 900
    wins = [(d_bad, index, s16.bl[k - 2][4] + 1, n), (d_bad, index, s16.bl[k][4] + 3, n), (s16.dev, s16.index, 4321, n)]
    arr = (linne_amd.Window * 3)()
    lays = (linne_amd.PcmLayout * 3)()
    out = torch.full((3, n, 2), -7777, dtype=torch.int16, device="cuda")
    for i, (dev, ix, a, m) in enumerate(wins):
        arr[i].index, arr[i].d_stream, arr[i].first_sample, arr[i].num_samples = ix.h, dev.data_ptr(), a, m
        arr[i].d_pcm = out[i].data_ptr()
        lays[i].format, lays[i].saturated, lays[i].channel_stride, lays[i].sample_stride = PCM_S16, 55, 1, 2
    ctx._fence()
    ret = linne_amd.lib.LINNEAmd_DecodeWindowsDeviceLayout(ctx.h, arr, lays, 3, 0)
    assert ret == CORRUPTION and [arr[i].result for i in range(3)] == [OK, CORRUPTION, OK]
    text = linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode()
    assert text.startswith("window 1: ") and f"block {k} " in text
    assert [lays[i].saturated for i in range(3)] == [0, 55, 0]
    h = out.cpu().numpy()
    assert (h[1] == -7777).all()
    for i in (0, 2):
        a = wins[i][2]
        assert np.array_equal(h[i].T, s16.full[:, a:a + n].astype(np.int16)), i
    # the Python call: the same codes, the text behind the window's number
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.decode_windows(wins, dtype=torch.int16, channels_last=True)
    assert e.value.code == CORRUPTION and e.value.codes == [OK, CORRUPTION, OK] and "window 1: " in str(e.value)
    index.close()


def test_the_training_batch(ctx, s16):
    import torch
    n, W = 3000, 6
    starts = [int(a) for a in np.random.default_rng(5).integers(0, s16.ns - n, size=W)]
    wins = [(s16.dev, s16.index, a, n) for a in starts]
    batch = torch.full((W, n, 2), 9.0, dtype=torch.float32, device="cuda")
    assert ctx.decode_windows(wins, out=batch, dtype=torch.float32, channels_last=True) is batch
    ints = torch.full((W, 2, n), 9, dtype=torch.int16, device="cuda")
    assert ctx.decode_windows(wins, out=ints, dtype=torch.int16) is ints
    for i, a in enumerate(starts):
        v = s16.full[:, a:a + n]
        assert np.array_equal(batch[i].cpu().numpy(), (v.astype(np.float32) * np.float32(2.0 ** -15)).T), i
        assert np.array_equal(ints[i].cpu().numpy(), v.astype(np.int16)), i


def test_round_trip(ctx, product):
    import torch
    x = mixed_signal(2, 16, 7 * 1024 + 300, seed=41, block=1024)
    stream = product.encode_whole(x, 16, 44100, 1024, 4, True)
    dev = to_device(stream)
    index = ctx.index_stream(dev)
    cuts = [0, 1000, 1001, 5000, x.shape[1]]
    pieces = ctx.decode_windows([(dev, index, a, b - a) for a, b in zip(cuts, cuts[1:])], dtype=torch.int16, channels_last=True)
    inter = torch.cat(pieces, dim=0)                             # (N, 2) int16, interleaved
    assert inter.shape == (x.shape[1], 2) and inter.is_contiguous()
    again = ctx.encode_streams([(inter.T, 16, 44100, 1024, 4, True)])[0]
    assert as_bytes(again) == stream
    index.close()


# 10 -----------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(s16):
    import torch
    block = 1024
    xs = [music(2, 3 * block + 100, 16, seed=600 + i) for i in range(24)]
    mixes = [(PCM_S16, True), (PCM_S16, False), (PCM_S24, True), (PCM_S24, False), (PCM_S32, True), (PCM_S32, False)]
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        c.enable_timing(True)
        enc_kinds, dec_kinds = list(range(48, 56)) + list(range(60, 69)), (56, 57, 58, 59, 28)
        census = []
        for tracks in ([torch.from_numpy(xs[0]).cuda()], [device_pcm(xs[0], PCM_S16, True)],
                       [device_pcm(x, *mixes[i % 6]) for i, x in enumerate(xs)]):
            c.encode_streams([(t, 16, 44100, block, 4, True) for t in tracks])
            census.append({k: c.last_launches(k) for k in enc_kinds})
        assert census[0] == census[1] == census[2] and census[0][60] >= 1, census
        c.encode_stream(torch.from_numpy(xs[0]).cuda(), 16, 44100, block, 4, True)
        one = {k: c.last_launches(k) for k in enc_kinds}
        c.encode_stream(device_pcm(xs[0], PCM_S24, True), 16, 44100, block, 4, True)
        assert one == {k: c.last_launches(k) for k in enc_kinds} and one == census[0] and one[60] >= 1          # the one-track batch's
        index = c.index_stream(s16.dev)
        starts = [int(a) for a in np.random.default_rng(8).integers(0, s16.ns - 2500, size=24)]
        starts[0] = 10                                           # music: COMPRESS blocks
        census = []
        c.decode_windows([(s16.dev, index, starts[0], 2500)])
        census.append({k: c.last_launches(k) for k in dec_kinds})
        c.decode_windows([(s16.dev, index, starts[0], 2500)], dtype=torch.int16, channels_last=True)
        census.append({k: c.last_launches(k) for k in dec_kinds})
        arr = (linne_amd.Window * 24)()
        lays = (linne_amd.PcmLayout * 24)()
        keep = []
        for i, a in enumerate(starts):
            fmt, inter = ((PCM_F32, True), (PCM_F32, False)) [i % 2] if i % 8 >= 6 else mixes[i % 6]
            buf = torch.empty(2 * 2500 * ESIZE[fmt], dtype=torch.uint8, device="cuda")
            keep.append(buf)
            arr[i].index, arr[i].d_stream, arr[i].first_sample, arr[i].num_samples, arr[i].d_pcm = index.h, s16.dev.data_ptr(), a, 2500, buf.data_ptr()
            lays[i].format = fmt
            lays[i].channel_stride, lays[i].sample_stride = (1, 2) if inter else (2500, 1)
        c._fence()
        assert linne_amd.lib.LINNEAmd_DecodeWindowsDeviceLayout(c.h, arr, lays, 24, 0) == OK
        census.append({k: c.last_launches(k) for k in dec_kinds})
        assert census[0] == census[1] == census[2] and census[0][59] >= 1, census
        for i, a in enumerate(starts):
            fmt = lays[i].format
            inter = lays[i].sample_stride == 2
            dt = {PCM_S32: np.int32, PCM_S16: np.int16, PCM_S24: np.uint8, PCM_F32: np.float32}[fmt]
            g = keep[i].cpu().numpy().view(dt).reshape(((2500, 2) if inter else (2, 2500)) + ((3,) if fmt == PCM_S24 else ()))
            g = from_elements(g, fmt)
            assert np.array_equal(g.T if inter else g, converted(s16.full[:, a:a + 2500], fmt, 16)[0]), i
        index.close()
    finally:
        c.close()


# 11 -----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_per_track_and_window(ctx, s16):
    import torch
    block, n = 1024, 2 * 1024 + 5
    x = music(2, n, 16, seed=70)
    want = as_bytes(int32_planar(ctx, x, 16, 44100, block, 4, True))
    good16, good24 = device_pcm(x, PCM_S16, True), device_pcm(x, PCM_S24, False)
    odd = torch.zeros(4 * n + 8, dtype=torch.uint8, device="cuda")
    # (format, channel stride, sample stride, base, expected code)
    plan = [
        (PCM_S16, 1, 2, good16.data_ptr(), OK),
        (PCM_F32, n, 1, odd.data_ptr(), INVALID_ARGUMENT),              # float input on encode
        (7, n, 1, odd.data_ptr(), INVALID_ARGUMENT),                    # an unknown format
        (PCM_S24, n, 1, good24.data_ptr(), OK),
        (PCM_S16, 1, 2, odd.data_ptr() + 1, INVALID_ARGUMENT),          # a misaligned base
        (PCM_S32, 1, 2, odd.data_ptr() + 2, INVALID_ARGUMENT),
        (PCM_S16, n - 1, 1, odd.data_ptr(), INVALID_ARGUMENT),          # channels overlap
        (PCM_S16, 1, 1, odd.data_ptr(), INVALID_ARGUMENT),              # interleaved frames narrower than C
        (PCM_S16, 0, 2, odd.data_ptr(), INVALID_ARGUMENT),
        (PCM_S16, n, 0, odd.data_ptr(), INVALID_ARGUMENT),
        (PCM_S16, 1, 2, good16.data_ptr(), OK),
    ]
    T = len(plan)
    arr = (linne_amd.Track * T)()
    lays = (linne_amd.PcmLayout * T)()
    outs = torch.zeros((T, 4 * 2 * n + 64), dtype=torch.uint8, device="cuda")
    for i, (fmt, cs, ss, base, _) in enumerate(plan):
        arr[i].header = linne_amd.Header(1, 2, 2, n, 44100, 16, block, 4, 1)
        arr[i].d_pcm, arr[i].pcm_stride, arr[i].d_out, arr[i].capacity = base, 0, outs[i].data_ptr(), outs.shape[1]
        arr[i].out_bytes, arr[i].result = 4242, -1
        lays[i].format, lays[i].channel_stride, lays[i].sample_stride = fmt, cs, ss
    ctx._fence()
    ret = linne_amd.lib.LINNEAmd_EncodeStreamsDeviceLayout(ctx.h, arr, lays, T, 0)
    assert ret == INVALID_ARGUMENT and linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode().startswith("track 1: ")
    assert [arr[i].result for i in range(T)] == [p[4] for p in plan]
    h = outs.cpu().numpy()
    for i, p in enumerate(plan):
        if p[4] == OK:
            assert bytes(h[i, :arr[i].out_bytes]) == want, i
        else:
            assert arr[i].out_bytes == 4242 and not h[i].any(), i
    # the single call: the same refusals, out_bytes untouched
    hd = linne_amd.Header(1, 2, 2, n, 44100, 16, block, 4, 1)
    for fmt, cs, ss, base, code in plan:
        nbytes = C.c_uint64(4242)
        lay = linne_amd.PcmLayout(fmt, 0, cs, ss)
        ctx._fence()
        ret = linne_amd.lib.LINNEAmd_EncodeStreamDeviceLayout(ctx.h, C.byref(hd), C.c_void_p(base), C.byref(lay), 0, C.c_void_p(outs[0].data_ptr()),
                                                              outs.shape[1], C.byref(nbytes), None)
        assert ret == code and (nbytes.value == len(want) if code == OK else nbytes.value == 4242), (fmt, cs, ss)
    # windows
    m = 500
    w_plan = [
        (PCM_F32, 1, 2, 0, OK),
        (9, m, 1, 0, INVALID_ARGUMENT),
        (PCM_S16, 1, 2, 1, INVALID_ARGUMENT),
        (PCM_F32, m, 1, 2, INVALID_ARGUMENT),
        (PCM_S24, m, 1, 1, OK),                                  # S24 at any byte
        (PCM_S16, m - 1, 1, 0, INVALID_ARGUMENT),
        (PCM_S16, 1, 1, 0, INVALID_ARGUMENT),
        (PCM_S16, m, 1, 0, OK),
    ]
    W = len(w_plan)
    warr = (linne_amd.Window * W)()
    wl = (linne_amd.PcmLayout * W)()
    wout = torch.full((W, 4 * 2 * m + 8), 77, dtype=torch.uint8, device="cuda")
    for i, (fmt, cs, ss, off, _) in enumerate(w_plan):
        warr[i].index, warr[i].d_stream, warr[i].first_sample, warr[i].num_samples = s16.index.h, s16.dev.data_ptr(), 100 + i, m
        warr[i].d_pcm, warr[i].result = wout[i].data_ptr() + off, -1
        wl[i].format, wl[i].saturated, wl[i].channel_stride, wl[i].sample_stride = fmt, 55, cs, ss
    ctx._fence()
    ret = linne_amd.lib.LINNEAmd_DecodeWindowsDeviceLayout(ctx.h, warr, wl, W, 0)
    assert ret == INVALID_ARGUMENT and linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode().startswith("window 1: ")
    assert [warr[i].result for i in range(W)] == [p[4] for p in w_plan]
    assert [wl[i].saturated for i in range(W)] == [0 if p[4] == OK else 55 for p in w_plan]
    h = wout.cpu().numpy()
    for i, (fmt, cs, ss, off, code) in enumerate(w_plan):
        v = s16.full[:, 100 + i:100 + i + m]
        if code != OK:
            assert (h[i] == 77).all(), i
            continue
        body = h[i, off:off + 2 * m * ESIZE[fmt]]
        assert (h[i, :off] == 77).all() and (h[i, off + body.size:] == 77).all(), i
        dt = {PCM_S16: np.int16, PCM_S24: np.uint8, PCM_F32: np.float32}[fmt]
        g = body.copy().view(dt).reshape(((m, 2) if ss == 2 else (2, m)) + ((3,) if fmt == PCM_S24 else ()))
        g = from_elements(g, fmt)
        assert np.array_equal(g.T if ss == 2 else g, converted(v, fmt, 16)[0]), i
