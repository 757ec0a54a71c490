"""GPU tests of comparing sample windows of resident .lnn streams with resident PCM (Context.compare_windows, verify_streams, the
verify setting of encode_stream / encode_streams (Context.set_verify), the command line tool's -V and -C; include/linne_amd.h LINNEAmd_CompareWindowsDevice).
Every expected (count, first sample, first channel) is computed with numpy from the oracle's decode of the same bytes, never from the
library under test.  Streams hold at most 8 blocks of 1024 samples."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import linne_amd
from linne_amd import PCM_F32, PCM_S16, PCM_S24, PCM_S32
from signals import music
from test_cli_cpu import CLI, wav_bytes
from test_gpu_pcm_layouts import device_pcm
from stream_consumers import Stream, crc_damaged, encoded, to_device
from stream_refs import blocks, crc16, expected_compare as expected, mixed_signal

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, CORRUPTION, NG = 0, 1, 6, 7
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300                                                       # (longer than 128 samples: presets 5-7 analyse it like any block)


def storage_bytes(t):
    """every byte of the allocation a PCM view lies in: its elements, the padding between them, the sentinels around them"""
    import torch
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).cpu().numpy().copy()


LAYOUTS = [  # format, interleaved, keywords of device_pcm
    (PCM_S32, False, {}), (PCM_S16, True, {}),
    (PCM_S24, False, dict(byte_offset=0)), (PCM_S24, False, dict(byte_offset=1)), (PCM_S24, False, dict(byte_offset=2)), (PCM_S24, False, dict(byte_offset=3)),
    (PCM_S24, True, dict(byte_offset=0)), (PCM_S24, True, dict(byte_offset=1)), (PCM_S24, True, dict(byte_offset=2)), (PCM_S24, True, dict(byte_offset=3)),
    (PCM_S16, False, dict(pad_channel=3, pad_sample=1)),         # neither planar nor packed: sample stride 2
    (PCM_S24, True, dict(pad_channel=2, byte_offset=1)),         # interleaved with a padded frame
    (PCM_S32, True, dict(pad_sample=1)),
    (PCM_S16, False, dict(pad_channel=5, byte_offset=2)),        # planar with a padded channel stride
]
FEW = [LAYOUTS[0], LAYOUTS[1], LAYOUTS[3], LAYOUTS[8], LAYOUTS[10], LAYOUTS[11]]


@pytest.fixture(scope="module")
def mixed(ctx, oracle):
    """stereo, 8 blocks: music, two SILENT, music, two RAW, music, a tail of 300"""
    x = mixed_signal(2, 16, 7 * S + TAIL, seed=11, block=S)
    t = encoded(ctx, oracle, x, 16, 5, True, "mixed")
    assert [b[2] for b in t.bl] == [COMPRESS, SILENT, SILENT, COMPRESS, RAW, RAW, COMPRESS, COMPRESS] and t.bl[-1][3] == TAIL
    yield t
    t.index.close()


@pytest.fixture(scope="module")
def three(ctx, oracle):
    """three channels, 5 blocks and a tail, all COMPRESS"""
    t = encoded(ctx, oracle, music(3, 5 * S + TAIL, 16, seed=12), 16, 0, False, "three")
    assert len(t.bl) == 6 and all(b[2] == COMPRESS for b in t.bl)
    yield t
    t.index.close()


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2, 3])
@pytest.mark.parametrize("preset", [0, 5])
def test_equality_over_layouts(ctx, oracle, nch, preset):
    t = encoded(ctx, oracle, music(nch, 3 * S + TAIL, 16, seed=20 + 8 * nch + preset), 16, preset, nch == 2)
    wins, pcms = [], []
    for first, n in ((0, t.ns), (517, 1500), (S - 1, 2), (t.ns - 1, 1)):
        for fmt, inter, kw in LAYOUTS:
            pcm = device_pcm(t.full[:, first:first + n], fmt, inter, **kw)
            wins.append((t.dev, t.index, first, n, pcm))
            pcms.append(pcm)
    before = [storage_bytes(p) for p in pcms]
    got = ctx.compare_windows(wins)
    assert got == [(0, 0, 0)] * len(wins)
    assert ctx.compare_windows(wins, group_frames=1) == got
    for b, p in zip(before, pcms):
        assert np.array_equal(b, storage_bytes(p))               # the PCM, its padding and the sentinels around it: only read
    # the call without layouts: int32 planar by pcm_stride
    import torch
    x = torch.from_numpy(t.full).cuda()
    w, d = (linne_amd.Window * 1)(), (linne_amd.Diff * 1)()
    w[0].index, w[0].d_stream, w[0].first_sample, w[0].num_samples, w[0].d_pcm, w[0].pcm_stride = t.index.h, t.dev.data_ptr(), 0, t.ns, x.data_ptr(), t.ns
    d[0].num_differing = 99
    torch.cuda.synchronize()
    assert linne_amd.lib.LINNEAmd_CompareWindowsDevice(ctx.h, w, None, d, 1, 0) == OK and w[0].result == OK
    assert (d[0].num_differing, d[0].first_sample, d[0].first_channel) == (0, 0, 0)
    t.index.close()


# 2 ------------------------------------------------------------------------------------------------------------------------------
def one_flipped(t, lo, hi):
    """[(stream sample, channel)] to flip, one at a time, for the window [lo, hi) of t"""
    raw = next(b for b in t.bl if b[2] == RAW)
    silent = next(b for b in t.bl if b[2] == SILENT)
    c = t.bl[3]                                                  # a COMPRESS block inside every window used here
    last = t.nch - 1
    return [(lo, 0), (hi - 1, last), (c[4], 0), (c[4] + S - 1, 1), (c[4] + 255, 0), (c[4] + 256, 1), (c[4] + 257, 0), (lo + 255, last), (lo + 256, 0), (lo + 257, last),
            (c[4] + 600, last), (raw[4] + 100, 0), (raw[4] + S - 1, last), (silent[4] + 100, last), (silent[4], 0)]


def test_one_differing_element_is_found_exactly(ctx, mixed):
    t = mixed
    wins, want = [], []
    for lo, hi in ((0, t.ns), (700, t.ns - 50)):
        for s, ch in one_flipped(t, lo, hi):
            assert lo <= s < hi
            held = t.full[:, lo:hi].copy()
            held[ch, s - lo] ^= 1
            for fmt, inter, kw in FEW:
                wins.append((t.dev, t.index, lo, hi - lo, device_pcm(held, fmt, inter, **kw)))
                want.append(expected(t.full, lo, hi - lo, held))
                assert want[-1] == (1, s, ch)
    assert len(wins) == 2 * 15 * len(FEW)
    assert ctx.compare_windows(wins) == want
    assert ctx.compare_windows(wins, group_frames=2) == want


def test_the_tail_region_behind_the_covered_samples(ctx, oracle):
    """a stream cut behind its third block: the header names 3 * S + TAIL samples, the blocks hold 3 * S; the rest decodes to zeros"""
    x = music(2, 3 * S + TAIL, 16, seed=31)
    whole = oracle.encode_whole(x, 16, 44100, S, 5, True)
    bl = blocks(whole)
    t = Stream(ctx, oracle, whole[:bl[3][0]], "cut")
    assert t.ns == 3 * S + TAIL and len(t.bl) == 3 and not t.full[:, 3 * S:].any() and np.array_equal(t.full[:, :3 * S], x[:, :3 * S])
    wins, want = [], []
    for lo, hi in ((0, t.ns), (3 * S - 10, t.ns), (3 * S + 7, t.ns - 5)):
        for s, ch in ((None, None), (max(lo, 3 * S), 1), (hi - 1, 0), (3 * S + 256, 1)):
            held = t.full[:, lo:hi].copy()
            if s is not None:
                held[ch, s - lo] = -3
            for fmt, inter, kw in FEW:
                wins.append((t.dev, t.index, lo, hi - lo, device_pcm(held, fmt, inter, **kw)))
                want.append(expected(t.full, lo, hi - lo, held))
                assert want[-1] == ((0, 0, 0) if s is None else (1, s, ch))
    assert ctx.compare_windows(wins) == want
    t.index.close()


def test_padding_and_neighbours_of_the_window_are_not_compared(ctx, mixed):
    import torch
    t = mixed
    lo, n = 700, 3000
    wins = []
    # padded layouts: every sentinel byte between and around the elements changed
    for fmt, inter, kw in (LAYOUTS[10], LAYOUTS[11], LAYOUTS[12], LAYOUTS[13]):
        good = device_pcm(t.full[:, lo:lo + n], fmt, inter, **kw)
        pcm = device_pcm(t.full[:, lo:lo + n], fmt, inter, sentinel=0xA5, **kw)
        assert not np.array_equal(storage_bytes(good), storage_bytes(pcm))
        wins.append((t.dev, t.index, lo, n, pcm))
    # windows that are views of the whole track's PCM, the elements just outside them changed
    for fmt, inter in ((PCM_S32, False), (PCM_S16, True), (PCM_S24, False), (PCM_S24, True)):
        held = t.full.copy()
        held[:, lo - 1] ^= 1
        held[:, lo + n] ^= 1
        big = device_pcm(held, fmt, inter)
        wins.append((t.dev, t.index, lo, n, big[:, lo:lo + n]))
    assert ctx.compare_windows(wins) == [(0, 0, 0)] * len(wins)
    # (and the same views one sample wider see them)
    wide = [(dev, index, lo - 1, n + 2, torch.as_strided(p, (p.shape[0], n + 2) + tuple(p.shape[2:]), p.stride(), p.storage_offset() - p.stride(1))) for dev, index, _, _, p in wins[4:]]
    assert ctx.compare_windows(wide) == [(4, lo - 1, 0)] * 4


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group_frames", [0, 1])
def test_counts_and_the_minimum(ctx, mixed, three, group_frames):
    rng = np.random.default_rng(7)
    wins, want = [], []
    for t in (three, mixed):
        for lo, hi in ((0, t.ns), (517, t.ns - 33), (2 * S + 300, 4 * S + 5)):
            n = hi - lo
            for k in (2, 17, "all"):
                held = t.full[:, lo:hi].copy()
                if k == "all":
                    held ^= 1
                else:
                    # spread over the window (several blocks, several workgroups); the two lowest at one sample in two channels
                    at = np.sort(rng.choice(np.arange(1, n), size=k - 1, replace=False))
                    held[t.nch - 1, at[0]] ^= 1
                    held[t.nch - 2, at[0]] ^= 2
                    for s in at[1:]:
                        held[int(rng.integers(0, t.nch)), s] ^= 4
                    assert at[-1] - at[0] > S or k == 2
                for fmt, inter, kw in FEW:
                    wins.append((t.dev, t.index, lo, n, device_pcm(held, fmt, inter, **kw)))
                    want.append(expected(t.full, lo, n, held))
                    assert want[-1] == ((t.nch * n, lo, 0) if k == "all" else (k, lo + int(at[0]), t.nch - 2))
    assert ctx.compare_windows(wins, group_frames=group_frames) == want


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_independence_of_the_windows_of_a_call(ctx, mixed, three):
    import torch
    t, u = mixed, three
    bad, k = crc_damaged(t)
    d_bad = to_device(bad)
    bad_index = ctx.index_stream(d_bad)
    held = t.full.copy()
    held[1, 2000] ^= 1
    held[0, 2500] ^= 1
    big = device_pcm(held, PCM_S16, True)                        # one PCM, overlapping windows on it
    uheld = u.full.copy()
    uheld[2, 4000] ^= 1
    ubig = device_pcm(uheld, PCM_S24, False, byte_offset=1)
    f32 = torch.zeros((2, 1000), dtype=torch.float32, device="cuda")
    n_bad = t.ns - t.bl[k][4]
    # (stream, index, first, n, pcm, format or None: the pcm's own, expected code)
    cases = [(t.dev, t.index, 1500, 2000, big[:, 1500:3500], None, OK),
             (t.dev, t.index, 1990, 20, big[:, 1990:2010], None, OK),
             (d_bad, bad_index, t.bl[k][4], n_bad, big[:, t.bl[k][4]:], None, CORRUPTION),
             (u.dev, u.index, 3000, 2000, ubig[:, 3000:5000], None, OK),
             (t.dev, t.index, 0, 1000, f32, PCM_F32, INVALID_ARGUMENT),
             (t.dev, t.index, 2001, 1000, big[:, 2001:3001], None, OK),
             (d_bad, bad_index, 0, 500, big[:, 0:500], None, OK),  # before the damaged block
             (t.dev, t.index, 0, t.ns + 1, big, None, INVALID_ARGUMENT)]
    W = len(cases)

    def call(which):
        w, ly, d = (linne_amd.Window * len(which))(), (linne_amd.PcmLayout * len(which))(), (linne_amd.Diff * len(which))()
        for j, i in enumerate(which):
            dev, index, first, n, pcm, fmt, _ = cases[i]
            if fmt is None:
                fmt, cs, ss, _, _, _ = ctx._pcm_layout(pcm)
            else:
                cs, ss = pcm.stride(0), pcm.stride(1)
            w[j].index, w[j].d_stream, w[j].first_sample, w[j].num_samples, w[j].d_pcm, w[j].result = index.h, dev.data_ptr(), first, n, pcm.data_ptr(), -1
            ly[j].format, ly[j].saturated, ly[j].channel_stride, ly[j].sample_stride = fmt, 55, cs, ss
            d[j].num_differing, d[j].first_sample, d[j].first_channel, d[j].reserved = 1234, 5678, 3, 9
        torch.cuda.synchronize()
        ret = linne_amd.lib.LINNEAmd_CompareWindowsDevice(ctx.h, w, ly, d, len(which), 0)
        assert all(ly[j].saturated == 55 for j in range(len(which)))           # not written
        return ret, [w[j].result for j in range(len(which))], [(d[j].num_differing, d[j].first_sample, d[j].first_channel, d[j].reserved) for j in range(len(which))]

    ret, codes, diffs = call(range(W))
    assert codes == [c[6] for c in cases]
    assert ret == CORRUPTION                                     # the lowest failing window's
    assert linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode().startswith(f"window 2: block {k} ")
    want = {0: (2, 2000, 1), 1: (1, 2000, 1), 3: (1, 4000, 2), 5: (1, 2500, 0), 6: (0, 0, 0)}
    for i in range(W):
        if cases[i][6] != OK:
            assert diffs[i] == (1234, 5678, 3, 9), i             # untouched
            continue
        first, n = cases[i][2], cases[i][3]
        full, h = (u.full, uheld) if i == 3 else (t.full, held)
        assert diffs[i] == expected(full, first, n, h[:, first:first + n]) + (0,) == want[i] + (0,), i
        ret1, codes1, diffs1 = call([i])                         # as it answers alone
        assert (ret1, codes1, diffs1) == (OK, [OK], [diffs[i]]), i
    for i in (2, 4, 7):                                          # and the failing ones fail alone with the same code
        ret1, codes1, diffs1 = call([i])
        assert (ret1, codes1, diffs1) == (cases[i][6], [cases[i][6]], [(1234, 5678, 3, 9)]), i
    # the Python form: codes, None for a failing window
    got, pcodes = ctx.compare_windows([c[:5] for c in cases[:4]], return_codes=True)
    assert pcodes == [OK, OK, CORRUPTION, OK] and got == [want[0], want[1], None, want[3]]
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.compare_windows([c[:5] for c in cases[:4]])
    assert e.value.code == CORRUPTION and e.value.codes == pcodes and "window 2:" in str(e.value)
    assert ctx.compare_windows([]) == [] and ctx.compare_windows([], return_codes=True) == ([], [])
    bad_index.close()


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_values_outside_the_format_differ(ctx, oracle):
    import torch
    x = music(2, 2 * S + TAIL, 24, seed=41)
    x[:, 100:900] //= 400                                        # a stretch inside int16's range
    t = encoded(ctx, oracle, x, 24, 5, True, "24 bits")
    clipped = np.clip(t.full, -32768, 32767)
    outside = t.full != clipped
    assert outside.any() and not outside[:, 100:900].any()
    for first, n in ((0, t.ns), (50, 1000)):
        pcm16, sat = ctx.decode_windows([(t.dev, t.index, first, n)], dtype=torch.int16, return_saturated=True)
        assert sat == [True] and np.array_equal(pcm16[0].cpu().numpy(), clipped[:, first:first + n])
        for pcm in (pcm16[0], device_pcm(clipped[:, first:first + n], PCM_S16, True)):
            want = expected(t.full, first, n, clipped[:, first:first + n])
            assert want[0] == int(outside[:, first:first + n].sum()) > 0
            assert ctx.compare_windows([(t.dev, t.index, first, n, pcm)]) == [want]
    # 24-bit values against S24 and S32 elements: equal
    got = ctx.compare_windows([(t.dev, t.index, 0, t.ns, device_pcm(t.full, PCM_S24, True, byte_offset=3)), (t.dev, t.index, 0, t.ns, device_pcm(t.full, PCM_S32, False))])
    assert got == [(0, 0, 0)] * 2
    t.index.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(mixed, three):
    import torch
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        c.enable_timing(True)
        counts = {}
        for t in (mixed, three):
            index = c.index_stream(t.dev)
            pcm = torch.from_numpy(t.full).cuda()
            for nw in (1, 32):
                spans = [(0, t.ns)] + [(37 * i, t.ns - 61 * i) for i in range(1, nw)]
                for gf in (0, 2):
                    c.decode_windows([(t.dev, index, a, n) for a, n in spans], group_frames=gf)
                    dec = {k: c.last_launches(k) for k in (28, 56, 57, 58, 59)}
                    got = c.compare_windows([(t.dev, index, a, n, pcm[:, a:a + n]) for a, n in spans], group_frames=gf)
                    assert got == [(0, 0, 0)] * nw
                    cmp_ = {k: c.last_launches(k) for k in (28, 56, 57, 58, 59, 79)}
                    assert cmp_[59] == 0 and cmp_[79] == dec[59] >= 1, (t.name, nw, gf, dec, cmp_)       # a launch per placing pass
                    assert all(cmp_[k] == dec[k] for k in (28, 56, 57, 58)), (t.name, nw, gf, dec, cmp_)
                    assert c.last_ms(79) > 0
                    counts[(t.name, nw, gf)] = cmp_
                assert counts[(t.name, nw, 0)][79] == 1
            assert counts[(t.name, 1, 0)] == counts[(t.name, 32, 0)]          # not a launch more for 32 windows than for one
            assert counts[(t.name, 1, 2)][79] > 1                             # the window spans passes
            index.close()
    finally:
        c.close()


# 7 ------------------------------------------------------------------------------------------------------------------------------
def rice_changed(oracle, t):
    """t's stream with one bit of a COMPRESS block's Rice payload changed and the CRC16 made right again, such that it still decodes:
    (bytes, the oracle's decode of them)"""
    k = max(i for i, b in enumerate(t.bl) if b[2] == COMPRESS and b[3] == S)
    off, size = t.bl[k][:2]
    rng = np.random.default_rng(5)
    for _ in range(256):
        bad = bytearray(t.stream)
        p = off + 11 + (size - 11) // 2 + int(rng.integers(0, (size - 11) // 2))
        bad[p] ^= 1 << int(rng.integers(0, 8))
        bad[off + 6:off + 8] = crc16(bad[off + 8:off + size]).to_bytes(2, "big")
        ret, full, _ = oracle.decode_whole(bytes(bad))
        if ret == OK and not np.array_equal(full, t.full):
            return bytes(bad), np.ascontiguousarray(full, dtype=np.int32)
    raise AssertionError("no changed bit in 256 left a stream that decodes to other samples")


def test_verify_streams(ctx, oracle, mixed, three):
    import torch
    other = encoded(ctx, oracle, music(2, mixed.ns, 16, seed=77), 16, 5, True, "other")
    bad, bad_full = rice_changed(oracle, mixed)
    m_pcm, t_pcm = device_pcm(mixed.full, PCM_S16, True), device_pcm(three.full, PCM_S24, False, byte_offset=1)
    o_pcm = torch.from_numpy(other.full).cuda()
    pairs = [(mixed.dev, m_pcm), (three.dev, t_pcm), (other.dev, o_pcm),          # good tracks of mixed shapes and formats
             (to_device(bad), m_pcm),                                               # a changed Rice payload under a right CRC16
             (other.dev, m_pcm),                                                    # another track's PCM
             (mixed.dev, m_pcm[:, :-1]),                                            # a sample fewer than the header names
             (three.dev, o_pcm[:, :three.ns]),                                      # other channels
             (to_device(mixed.stream[:10]), m_pcm)]                                 # no stream at all
    got = ctx.verify_streams(pairs)
    assert got[:3] == [(0, 0, 0, None)] * 3
    want = expected(bad_full, 0, mixed.ns, mixed.full)
    assert want[0] > 0 and got[3] == want + (None,)
    want = expected(other.full, 0, mixed.ns, mixed.full)
    assert want[0] > 1000 and got[4] == want + (None,)
    assert got[5][0] is None and f"{mixed.ns} samples" in got[5][3] and f"{mixed.ns - 1}" in got[5][3]
    assert got[6][0] is None and "3 channels" in got[6][3]
    assert got[7][0] is None and "does not index" in got[7][3]
    assert ctx.verify_streams(pairs, group_frames=3) == got
    assert ctx.verify_streams([]) == []
    other.index.close()


def test_verified_encode(ctx, mixed, three):
    import torch
    tracks = [(device_pcm(mixed.full, PCM_S16, True), 16, 44100, S, 5, True), (torch.from_numpy(three.full).cuda(), 16, 44100, S, 0, False),
              (device_pcm(three.full, PCM_S24, False, byte_offset=3), 16, 44100, S, 3, False)]
    plain = ctx.encode_streams(tracks)
    c = linne_amd.Context(0, use_torch_stream=False)             # (the setting stays off on the session's context)
    try:
        c.set_verify(True)
        checked = c.encode_streams(tracks)
        assert [bytes(s.cpu().numpy()) for s in checked] == [bytes(s.cpu().numpy()) for s in plain]
        assert bytes(plain[0].cpu().numpy()) == mixed.stream
        one = c.encode_stream(*tracks[0])
        assert bytes(one.cpu().numpy()) == mixed.stream
        streams, states, codes = c.encode_streams(tracks, parcor_states=[0.0] * 3, return_codes=True)
        assert codes == [OK] * 3 and [bytes(s.cpu().numpy()) for s in streams] == [bytes(s.cpu().numpy()) for s in plain]
        assert c.last_launches(79) == 0                          # (timing is off: nothing counted)
        c.enable_timing(True)
        c.encode_stream(*tracks[0])
        assert c.last_launches(79) == 1                          # the verified encode ends in a compare pass
        c.set_verify(False)
        c.encode_stream(*tracks[0])
        assert c.last_launches(79) == 0
    finally:
        c.close()
    # what the flag raises when a track differs: the streams against PCM with two elements changed
    held = three.full.copy()
    held[2, 777] ^= 1
    held[1, 4000] ^= 1
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx._verified(plain, [tracks[0][0], torch.from_numpy(held).cuda(), tracks[2][0]], "EncodeStreamsDevice")
    assert e.value.code == NG and e.value.codes == [OK, NG, OK]
    assert "track 1: verification failed at sample 777, channel 2 (2 elements differ)" in str(e.value)


# 8 ------------------------------------------------------------------------------------------------------------------------------
def cli(*args):
    return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_command_line_tool(tmp_path):
    x = music(2, 3000, 16, seed=91)
    wav, changed, short = tmp_path / "a.wav", tmp_path / "changed.wav", tmp_path / "short.wav"
    wav.write_bytes(wav_bytes(x, 16, 44100))
    y = x.copy()
    y[1, 2345] ^= 1
    changed.write_bytes(wav_bytes(y, 16, 44100))
    short.write_bytes(wav_bytes(x[:, :2999], 16, 44100))
    plain, checked = tmp_path / "plain.lnn", tmp_path / "checked.lnn"
    r = cli("-e", "-m", "2", str(wav), str(plain))
    assert r.returncode == 0 and "verified" not in r.stdout, r.stderr
    r = cli("-e", "-m", "2", "-V", str(wav), str(checked))
    assert r.returncode == 0 and ", verified" in r.stdout, r.stderr
    assert checked.read_bytes() == plain.read_bytes()
    r = cli("-C", str(plain), str(wav))
    assert r.returncode == 0 and "identical" in r.stdout, r.stderr
    r = cli("-C", str(plain), str(changed))
    assert r.returncode == 1 and "verification failed: sample 2345 channel 1 (1 elements differ)" in r.stderr and "identical" not in r.stdout
    r = cli("-C", str(plain), str(short))
    assert r.returncode == 1 and "3000 samples" in r.stderr and "2999 samples" in r.stderr
