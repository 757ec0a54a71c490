"""GPU tests of projecting frames of resident .lnn streams on int16 basis rows (Context.project_windows, stft_windows, spectrum_streams;
include/linne_amd.h LINNEAmd_ProjectWindowsDevice).  Every expected element is computed with numpy int64 (project_refs.expected_project)
from the oracle's decode of the same bytes, never from the library under test, and everything must be equal: words between sentinels, no
tolerance -- the float32 path is a conversion and a multiplication by a power of two.  Streams hold 3 to 6 blocks of 1024 samples, or 21
blocks of 33; the tests from 7 on build streams whose decode is chosen: planted values at the edges of the kernel's 2, 3 and 4 sample
planes, constant full scale under 4096-sample rows of full scale, and a sparse mono stream long enough for 17 frames at hop 65536."""
import ctypes as C

import numpy as np
import pytest

import linne_amd
import synth_records as sr
import far_streams as fs
import project_edges as pe
from project_refs import basis_digits, expected_project, project_length, projected_values, sample_digits, sample_planes
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
SENTINEL = 0x5A5A5A5A
PRESET_KIND, PROJECT_KIND, PLACE_KIND = KIND["PROJECT_T_PRESET"], KIND["PROJECT_T_PROJECT"], KIND["T_WX_PLACE"]
HOPS = lambda N: [1, 3, 16, 64, N, N + 5, 65536]


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
    """a 16-bit stereo stream whose crafted blocks decode to values over all of int32 (the relate and mix tests' fixture)"""
    t = Stream(ctx, oracle, sr.case_stream(WIDE_SHAPE, wide_cases()), "wide values")
    assert t.nch == 2 and np.abs(t.full.astype(np.int64)).max() > 1 << 30
    yield t
    t.index.close()


@pytest.fixture(scope="module")
def small(ctx, oracle):
    """stereo in blocks of 33 samples, the last of 5: a frame of 64 samples crosses two block boundaries"""
    x = music(2, 20 * 33 + 5, 16, seed=17)
    t = Stream(ctx, oracle, oracle.encode_whole(x, 16, 44100, 33, 0, False), "blocks of 33")
    assert np.array_equal(t.full, x) and len(t.bl) == 21 and t.bl[-1][3] == 5
    yield t
    t.index.close()


def random_basis(rng, K, N):
    """random int16 with the extremes among them; where there is room, a row of 32767 and a row of -32768"""
    b = rng.integers(-32768, 32768, (K, N)).astype(np.int16)
    b.reshape(-1)[rng.integers(0, K * N, max(K * N // 16, 1))] = rng.choice(np.array([32767, -32768, 127, 128, -128, -129, 255, 256, 0], dtype=np.int16), max(K * N // 16, 1))
    if K >= 3:
        b[K // 2], b[K - 1] = 32767, -32768
    return b


# ---- the C entry point on tables that lie in one buffer of sentinels ----
def item(t, first, n, basis, hop, before=0, shift=0, clip_bits=0, f32=False, float_exp=0, order="fk", pad=0, wrong=None, **more):
    """a window of raw_project: order "fk" (rows contiguous: (C, frames, K)) or "kf" (frames contiguous: (C, K, frames)), every stride
    padded by `pad` elements; wrong: spec fields as they are given to the call, whatever the reference would say"""
    return dict(t=t, first=first, n=n, basis=np.ascontiguousarray(basis, dtype=np.int16), hop=hop, before=before, shift=shift, clip=clip_bits, f32=f32, fexp=float_exp,
                order=order, pad=pad, wrong=wrong or {}, **more)


def strides(it):
    """(channel, frame, row) strides in elements"""
    n, K, pad = max(it["n"], 1), it["basis"].shape[0], it["pad"]
    if it["order"] == "fk":
        return (n * (K + pad) + pad, K + pad, 1)
    return (K * (n + pad) + pad, 1, n + pad)


def extent(it):
    cs, fs, rs = strides(it)
    return (it["t"].nch - 1) * cs + (it["n"] - 1) * fs + (it["basis"].shape[0] - 1) * rs + 1 if it["n"] > 0 else 0


def raw_project(ctx, items, group_frames=0):
    """LINNEAmd_ProjectWindowsDevice itself -> (ret, codes, the buffer as uint32 words, the tables' first words, the saturated words (7:
    left as it was))"""
    import torch
    offs, at = [], 4
    for it in items:
        offs.append(at)
        at += max(extent(it), 1) + 4
    buf = torch.full((at,), SENTINEL, dtype=torch.int32, device="cuda")
    W = len(items)
    w, sp = (linne_amd.Window * W)(), (linne_amd.ProjectSpec * W)()
    for j, it in enumerate(items):
        t = it["t"]
        dev, index = it.get("dev", t.dev), it.get("index", t.index)
        w[j].index, w[j].d_stream, w[j].first_sample, w[j].num_samples, w[j].result = index.h, dev.data_ptr(), it["first"], it["n"] % (1 << 64), -1
        w[j].d_pcm, w[j].pcm_stride = buf.data_ptr() + 4 * offs[j], 0
        cs, fs, rs = strides(it)
        f = dict(frame_len=it["basis"].shape[1], hop=it["hop"], num_rows=it["basis"].shape[0], before=it["before"], shift=it["shift"], clip_bits=it["clip"],
                 format=linne_amd.PCM_F32 if it["f32"] else linne_amd.PCM_S32, float_exp=it["fexp"], channel_stride=cs, frame_stride=fs, row_stride=rs, saturated=7, reserved=0)
        f.update({k: v for k, v in it["wrong"].items() if k not in ("null_basis", "d_pcm_plus")})
        for k, v in f.items():
            setattr(sp[j], k, v)
        if not it["wrong"].get("null_basis"):
            sp[j].basis = it["basis"].ctypes.data_as(C.POINTER(C.c_int16))
        w[j].d_pcm += it["wrong"].get("d_pcm_plus", 0)
    torch.cuda.synchronize()
    ret = linne_amd.lib.LINNEAmd_ProjectWindowsDevice(ctx.h, w, sp, W, group_frames)
    return ret, [w[j].result for j in range(W)], buf.cpu().numpy().view(np.uint32), offs, [int(sp[j].saturated) for j in range(W)]


REFS = {}


def reference(it):
    """the reference of an item, computed once"""
    key = (id(it["t"]), it["first"], it["n"], id(it["basis"]), it["hop"], it["before"], it["shift"], it["clip"], it["f32"], it["fexp"])
    if key not in REFS:
        REFS[key] = (it["basis"], expected_project(it["t"].full, it["first"], it["n"], it["basis"], it["hop"], it["before"], it["shift"], it["clip"], it["f32"], it["fexp"]))
    return REFS[key][1]


def want_project(items, codes, offs, size):
    """sentinels but the OK windows' elements -> (the words, the saturated words)"""
    buf = np.full(size, SENTINEL, dtype=np.uint32)
    sats = []
    for it, code, off in zip(items, codes, offs):
        if code != OK:
            sats.append(7)
            continue
        want, sat = reference(it)
        sats.append(int(sat))
        if it["n"] == 0:
            continue
        cs, fs, rs = strides(it)
        c, f, k = np.meshgrid(np.arange(it["t"].nch), np.arange(it["n"]), np.arange(it["basis"].shape[0]), indexing="ij")
        buf[off + c * cs + f * fs + k * rs] = np.ascontiguousarray(want).view(np.uint32)
    return buf, sats


def held(ctx, items, want_codes=None, group_frames=(0, 1, 3)):
    """the call on the items, at every group_frames: codes, every word of the buffer and the saturated words are the reference's"""
    want_codes = want_codes or [OK] * len(items)
    for gf in group_frames:
        ret, codes, buf, offs, sats = raw_project(ctx, items, gf)
        assert codes == want_codes and ret == next((c for c in want_codes if c != OK), OK), (gf, codes, last_error(ctx))
        want, want_sats = want_project(items, want_codes, offs, len(buf))
        if not np.array_equal(buf, want):
            bad = int(np.flatnonzero(buf != want)[0])
            j = max(k for k in range(len(offs)) if offs[k] <= bad) if bad >= offs[0] else -1
            it = items[j]
            raise AssertionError(f"group_frames {gf}: word {bad} (window {j} begins at {offs[j] if j >= 0 else 0}: N {it['basis'].shape[1]} K {it['basis'].shape[0]} H {it['hop']} "
                                 f"first {it['first']} n {it['n']} {it['order']} pad {it['pad']}) is {int(buf[bad]):#x}, not {int(want[bad]):#x}; {int((buf != want).sum())} words differ")
        assert sats == want_sats, (gf, sats, want_sats)
    return ret


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(1, 1), (63, 15), (64, 16), (65, 17), (512, 257), (4096, 16), (64, 2048)], ids=lambda v: str(v))
def test_values_against_the_reference(ctx, streams, N, K):
    """random int16 bases with the extremes among them; every hop, before at 0 and N - 1, 1, 15, 16 and 17 frames, the stream's first
    and last frames, every channel count and sample width, shifts, both formats and both stride orders in turn"""
    rng = np.random.default_rng(1000 * N + K)
    basis = random_basis(rng, K, N)
    items, k = [], 0
    keys = (1, 2, 3, 8, "8bit", "24bit")
    for H in HOPS(N):
        for key in (keys if H in (3, N) else (keys[k % 6], keys[(k + 3) % 6])):
            t = streams[key]
            F = project_length(t.ns, H)
            most = 17 if N * K * t.nch > 1 << 17 else 70                  # (the reference's frames: a few megabytes at the most)
            spans = [(0, min(F, most)), (F - 1, 1), (max(F - 15, 0), min(F, 15)), (F // 2, min(16, F - F // 2)), (max(F - most, 0), min(F, most)), (F // 3, min(65, most, F - F // 3))]
            for first, n in spans[k % 2::2]:
                items.append(item(t, first, n, basis, H, before=(0, N - 1, N // 2)[k % 3], shift=(0, 15, 31, 7)[(k // 3) % 4], clip_bits=(0, 16, 24, 32, 2)[k % 5],
                                  f32=k % 4 == 1, float_exp=(0, 31)[(k // 4) % 2] if k % 4 == 1 else 0, order=("fk", "kf")[(k // 2) % 2], pad=(0, 3, 0, 1)[k % 4]))
                k += 1
    held(ctx, items, group_frames=(0, 2))


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_edges(ctx, streams, cut, small):
    rng = np.random.default_rng(5)
    t = streams[2]
    items = []
    b64, b20 = random_basis(rng, 20, 64), random_basis(rng, 5, 20)
    for first, n in ((0, 1), (0, 15), (0, 16), (0, 17), (0, 63), (0, 64), (0, 65), (63, 2), (64, 1), (60, 140)):     # on and across the tiles of 64 frames, the waves of 16
        items.append(item(t, first, n, b64, 7, before=30, shift=12, clip_bits=24, order=("fk", "kf")[first % 2]))
        items.append(item(t, first, n, b20, 1, before=19, shift=3))
    F = project_length(t.ns, 16)
    items += [item(t, 0, 9, b64, 16, before=b, shift=10) for b in (0, 31, 63)]               # the halo reaches before the stream
    items += [item(t, F - 9, 9, b64, 16, before=b, shift=10) for b in (0, 31, 63)]           # ... and behind it
    # blocks of 33 under frames of 64: a frame crosses two block boundaries, the last block is shorter than the frame
    for H in (1, 5, 33, 70):
        Fs = project_length(small.ns, H)
        items += [item(small, 0, Fs, b64, H, before=31, shift=9), item(small, Fs - min(3, Fs), min(3, Fs), b64, H, before=63, shift=9, order="kf", pad=1),
                  item(small, Fs // 2, 1, b64, H, before=0, f32=True, float_exp=31)]
    # COMPRESS, SILENT and RAW neighbours under one frame, and the truncated stream's tail of zeros
    for H in (13, 64, 100):
        Fc = project_length(cut.ns, H)
        items += [item(cut, 0, Fc, b64, H, before=16, shift=8), item(cut, S // H - 2, 6, b64, H, before=63, shift=8, order="kf", pad=3),
                  item(cut, 4 * S // H - 1, 4, b64, H, before=32, f32=True), item(cut, 6 * S // H - 3, 8, b64, H, before=0, shift=8), item(cut, Fc - 5, 5, b64, H, before=7, shift=8)]
    held(ctx, items)


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_wide_values_every_plane_count_every_shift_and_both_saturations(ctx, wide, streams):
    """the crafted stream decodes to all of int32: tiles of 2, 3 and 4 sample planes against rows of 32767 and -32768; shifts 0 to 31;
    the clip at clip_bits and the clip at 32 bits"""
    rng = np.random.default_rng(9)
    t = wide
    basis = random_basis(rng, 19, 70)
    basis[0], basis[1] = 32767, -32768
    one = np.array([[1], [-1], [32767], [-32768]], dtype=np.int16)
    items = [item(t, 0, project_length(t.ns, H), basis, H, before=b, shift=sh, clip_bits=cb, f32=f32, float_exp=31 if f32 else 0, order=order)
             for H, b, sh, cb, f32, order in ((1, 0, 0, 0, False, "fk"), (3, 69, 31, 0, False, "kf"), (70, 35, 27, 0, True, "fk"), (75, 0, 30, 16, False, "kf"), (16, 5, 31, 2, True, "fk"))]
    items += [item(t, 0, t.ns, one, 1, shift=sh, clip_bits=(0, 16)[sh % 2]) for sh in range(32)]      # the samples themselves, shifted: every plane count, every shift
    u = streams[2]
    items += [item(u, 0, u.ns, one[:2], 1), item(u, 0, u.ns, one[:2], 1, clip_bits=12), item(u, 0, 40, basis, 64, shift=20)]
    ret, codes, buf, offs, sats = raw_project(ctx, items)
    want, want_sats = want_project(items, codes, offs, len(buf))
    assert ret == OK and codes == [OK] * len(items), last_error(ctx)
    assert np.array_equal(buf, want) and sats == want_sats
    assert sats[0] == 1 and sats[-3] == 0 and sats[-2] == 1 and sats[5] == 1 and sats[6] == 1       # both clips are among them, and none
    m = np.abs(t.full.astype(np.int64))
    assert (m < 1 << 15).any() and (m >= 1 << 23).any() and ((m >= 1 << 15) & (m < 1 << 23)).any()       # (the premise: narrow, middle and wide values)


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_many_windows_and_failures_stay_in_their_window(ctx, product, streams, cut, small):
    """64 windows of mixed specs and shapes in one buffer of sentinels, CRC- and Rice-damaged neighbours and argument errors among them:
    a failing window's memory is untouched, the lowest failing window's code and text are returned; windows share bases"""
    t = streams[2]
    crc, rice = sc.damaged(ctx, product, t)
    k, kr = crc[2], rice[2]
    rng = np.random.default_rng(4)
    ts = [streams[2], streams[3], cut, streams[8], streams[1], small, streams["24bit"]]
    shapes = [(1, 1), (63, 15), (64, 16), (65, 17), (128, 70), (20, 5), (300, 3)]
    bases = [random_basis(rng, K, N) for N, K in shapes]
    items, want_codes = [], [OK] * 64
    for i in range(64):
        u = ts[i % len(ts)]
        basis = bases[i % 5 if i % 2 else i % len(bases)]
        N = basis.shape[1]
        H = (1, 3, 16, 64, N, N + 5, 65536)[i % 7] if i % 3 else 1 + int(rng.integers(0, 2 * N))
        F = project_length(u.ns, H)
        first = int(rng.integers(0, F))
        n = int(rng.integers(1, min(F - first, 40) + 1)) if i % 9 else 0
        items.append(item(u, first, n, basis, H, before=int(rng.integers(0, N)), shift=(0, 15, 31, 20)[(i // 4) % 4], clip_bits=(0, 16, 24)[i % 3], f32=i % 5 == 2,
                          float_exp=(0, 31, 63)[i % 3] if i % 5 == 2 else 0, order=("fk", "kf")[(i // 2) % 2], pad=(0, 2)[(i // 3) % 2]))
    b3 = random_basis(rng, 6, 40)

    def on(damaged, first, n, code, i, **wrong):
        items[i] = dict(item(t, first, n, b3, 10, before=4, shift=17, clip_bits=16, order=("fk", "kf")[i % 2], pad=i % 3, wrong=wrong), dev=damaged[0], index=damaged[1])
        want_codes[i] = code
    fr = lambda s: -(-(s + 4) // 10)                            # the first frame that reads from input sample s on (it reaches 4 back)
    last = lambda s: (s + 4 - 40) // 10                         # the last frame whose samples all lie in front of sample s
    on(rice, fr(t.bl[kr][4]) + 1, 20, NG, 5)                    # over the Rice-damaged block: the fail word is set on the device
    on(rice, fr(t.bl[kr - 1][4]) + 1, 20, OK, 6)
    on(rice, 0, project_length(t.ns, 10), NG, 7)
    on(crc, fr(t.bl[k][4]) + 1, 20, CORRUPTION, 9)              # CRC damage: refused on the host
    on(crc, 0, last(t.bl[k][4]) + 1, OK, 10)                    # its last frame's last input sample is in front of the damaged block
    on(crc, 0, last(t.bl[k][4]) + 2, CORRUPTION, 11)            # ... and here the last frame alone reaches into it
    me = (t.dev, t.index)
    on(me, 0, 100, INVALID_ARGUMENT, 20, shift=32)
    on(me, 1, project_length(t.ns, 10), INVALID_ARGUMENT, 40)   # a range beyond the stream's frames
    on(me, 0, 100, INVALID_ARGUMENT, 41, null_basis=True)
    on(me, 0, 100, INVALID_ARGUMENT, 42, reserved=1)
    on(me, 0, 100, INVALID_ARGUMENT, 43, before=40)
    on(me, 0, 100, INVALID_ARGUMENT, 44, hop=65537)
    on(me, 0, 100, INVALID_ARGUMENT, 45, format=linne_amd.PCM_S16)
    on(me, 0, 100, INVALID_ARGUMENT, 46, float_exp=1)
    on(me, 0, 100, INVALID_ARGUMENT, 47, d_pcm_plus=2)
    on(me, 0, 100, INVALID_ARGUMENT, 48, frame_stride=5, row_stride=1)              # rows of 6 elements five apart
    on(me, 0, 100, INVALID_ARGUMENT, 49, channel_stride=599, frame_stride=6, row_stride=1)   # channels of 600 elements 599 apart
    on(me, 0, 100, INVALID_ARGUMENT, 50, row_stride=0)
    on(me, 0, 100, INVALID_ARGUMENT, 51, frame_stride=1, row_stride=99, channel_stride=6 * 99)       # frames contiguous, rows one short
    assert 10 * last(t.bl[k][4]) - 4 + 39 < t.bl[k][4] <= 10 * (last(t.bl[k][4]) + 1) - 4 + 39
    assert held(ctx, items, want_codes) == NG                    # the lowest failing window's
    ret, codes, *_ = raw_project(ctx, items)
    assert last_error(ctx).startswith(f"window 5: block {kr} ")
    for i, word in ((20, "shift 32"), (41, "null basis"), (42, "reserved"), (43, "before 40"), (44, "hop 65537"), (45, "format 1"), (46, "float_exp 1"), (47, "4-byte aligned"),
                    (48, "apart"), (49, "apart"), (50, "apart"), (51, "apart")):
        ret1, codes1, buf1, *_ = raw_project(ctx, [items[i]])
        assert (ret1, codes1) == (INVALID_ARGUMENT, [INVALID_ARGUMENT]) and set(buf1.tolist()) == {SENTINEL}
        assert last_error(ctx).startswith("window 0: ProjectWindowsDevice: ") and word in last_error(ctx), (i, last_error(ctx))
    ret1, codes1, buf1, *_ = raw_project(ctx, [items[40]])
    assert (ret1, codes1) == (INVALID_ARGUMENT, [INVALID_ARGUMENT]) and "beyond the stream's" in last_error(ctx)
    ret1, codes1, buf1, *_ = raw_project(ctx, [items[11]])
    assert (ret1, codes1) == (CORRUPTION, [CORRUPTION]) and set(buf1.tolist()) == {SENTINEL} and last_error(ctx).startswith(f"window 0: block {k} ")
    # the products' cap, formed in 128 bits: 2^61 frames wrap 64 bits with 2048 * 4096 * 2 products each
    huge = item(t, 0, 1 << 61, np.zeros((2048, 4096), dtype=np.int16), 1)
    assert (1 << 61) * 2048 * 4096 * 2 >= 1 << 64 and extent(huge) < 1 << 80
    w, sp = (linne_amd.Window * 1)(), (linne_amd.ProjectSpec * 1)()
    w[0].index, w[0].d_stream, w[0].first_sample, w[0].num_samples, w[0].d_pcm, w[0].result = t.index.h, t.dev.data_ptr(), 0, 1 << 61, t.dev.data_ptr() & ~3, -1
    sp[0].frame_len, sp[0].hop, sp[0].num_rows, sp[0].channel_stride, sp[0].frame_stride, sp[0].row_stride = 4096, 1, 2048, 1 << 62, 2048, 1
    sp[0].basis = huge["basis"].ctypes.data_as(C.POINTER(C.c_int16))
    assert linne_amd.lib.LINNEAmd_ProjectWindowsDevice(ctx.h, w, sp, 1, 0) == INVALID_ARGUMENT and w[0].result == INVALID_ARGUMENT and "2^40 products" in last_error(ctx)
    # the Python form: codes with return_codes, an error without
    wins = [(it.get("dev", t.dev), it.get("index", t.index), it["first"], 20) for it in (items[9], items[10], items[9])]
    got, pcodes = ctx.project_windows(wins, b3, 10, before=4, shift=17, clip_bits=16, return_codes=True)
    assert pcodes == [CORRUPTION, OK, CORRUPTION]
    assert np.array_equal(got[1].cpu().numpy(), expected_project(t.full, 0, 20, b3, 10, 4, 17, 16)[0])
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.project_windows(wins, b3, 10, before=4, shift=17)
    assert e.value.code == CORRUPTION and e.value.codes == pcodes and "window 0:" in str(e.value)
    for _, index, _ in (crc, rice):
        index.close()


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(streams):
    """the decode call's launches, kind 59 among them, and kinds 104 and 105 once each, none of any other consumer's; the same for one
    window and for 64, whatever the frame, the hop and the rows"""
    others = sorted(k for c in sc.CONSUMERS.values() for k in c.kinds if k != PLACE_KIND) + [KIND[n] for n in ("MIX_T_MIX", "RESAMPLE_T_PRESET", "RESAMPLE_T_RESAMPLE", "OVERLAY_T_OVERLAY", "LAGS_T_LAGS", "LAGS_T_COMMIT")]
    assert (PRESET_KIND, PROJECT_KIND) == (104, 105) and not {104, 105} & set(others)
    ctx = linne_amd.Context(0, use_torch_stream=False)
    try:
        ctx.enable_timing(True)
        rng = np.random.default_rng(1)
        for t in (streams[2], streams[3]):                       # four COMPRESS blocks each: two placing passes at group_frames 2
            index = ctx.index_stream(t.dev)
            for N, K, H in ((1, 1, 1), (512, 40, 128), (65, 130, 70)):
                basis = random_basis(rng, K, N)
                F = project_length(t.ns, H)
                for nw in (1, 64):
                    spans = [(0, min(F, 24))] * nw
                    lo, hi = 0, min(23 * H - N // 2 + N, t.ns)    # the decode call of the windows' input ranges
                    for gf in (0, 2):
                        ctx.decode_windows([(t.dev, index, lo, hi - lo)] * nw, group_frames=gf)
                        dec = {k: ctx.last_launches(k) for k in DECODE_KINDS + [PLACE_KIND]}
                        got = ctx.project_windows([(t.dev, index, a, n) for a, n in spans], basis, H, before=N // 2, shift=15, clip_bits=16, group_frames=gf)
                        mine = {k: ctx.last_launches(k) for k in DECODE_KINDS + [PLACE_KIND, PRESET_KIND, PROJECT_KIND] + others}
                        assert np.array_equal(got[-1].cpu().numpy(), expected_project(t.full, 0, spans[-1][1], basis, H, N // 2, 15, 16)[0])
                        assert all(mine[k] == 0 for k in others), (t.name, nw, gf, mine)
                        assert all(mine[k] == dec[k] for k in DECODE_KINDS + [PLACE_KIND]) and mine[PLACE_KIND] >= 1, (t.name, nw, gf, dec, mine)
                        assert mine[PRESET_KIND] == 1 and mine[PROJECT_KIND] == 1, (t.name, nw, gf, mine)
                        assert ctx.last_ms(PROJECT_KIND) > 0 and ctx.last_ms(PRESET_KIND) > 0
            index.close()
    finally:
        ctx.close()


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_python_forms(ctx, streams):
    """project_windows into `out` of both orders and padded strides; stft_windows against the reference with the designed basis;
    spectrum_streams against Python integers"""
    import torch
    t, u = streams[2], streams[3]
    rng = np.random.default_rng(3)
    basis = random_basis(rng, 9, 50)
    wins = [(t.dev, t.index, 5, 40), (t.dev, t.index, 0, 40)]
    want = np.stack([expected_project(t.full, a, 40, basis, 20, 7, 10, 16)[0] for a in (5, 0)])
    got, sat = ctx.project_windows(wins, basis, 20, before=7, shift=10, clip_bits=16, return_saturated=True)
    assert tuple(got.shape) == (2, 2, 40, 9) and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want) and sat == [projected_values(t.full, a, 40, basis, 20, 7, 10, 16)[1] for a in (5, 0)]
    got = ctx.project_windows(wins, basis, 20, before=7, shift=10, clip_bits=16, rows_first=True)
    assert tuple(got.shape) == (2, 2, 9, 40) and np.array_equal(got.cpu().numpy(), want.transpose(0, 1, 3, 2))
    big = torch.full((2, 2, 9 + 2, 40 + 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ctx.project_windows(wins, basis, 20, before=7, shift=10, clip_bits=16, rows_first=True, out=big[:, :, :9, :40])
    held_ = big.cpu().numpy()
    assert np.array_equal(held_[:, :, :9, :40], want.transpose(0, 1, 3, 2)) and (held_[:, :, 9:, :] == 0x5A5A5A5A).all() and (held_[:, :, :, 40:] == 0x5A5A5A5A).all()
    fl = ctx.project_windows(wins, basis, 20, before=7, dtype=torch.float32, float_exp=31)
    assert fl.dtype == torch.float32 and np.array_equal(fl.cpu().numpy(), np.stack([expected_project(t.full, a, 40, basis, 20, 7, f32=True, float_exp=31)[0] for a in (5, 0)]))
    whole = ctx.project_windows([(t.dev, t.index, 3, None)], basis, 20)
    assert whole.shape[2] == project_length(t.ns, 20) - 3
    for bad in (dict(hop=0), dict(hop=65537), dict(before=50), dict(shift=32), dict(clip_bits=1), dict(float_exp=1), dict(dtype=torch.int16)):
        with pytest.raises(ValueError):
            ctx.project_windows(wins, basis, **{"hop": 20, **bad})
    with pytest.raises(ValueError):
        ctx.project_windows(wins, basis.astype(np.int32) * 2, 20)
    # the STFT: windows in samples, centred and not
    for n_fft, hop, center, window in ((64, 16, True, "hann"), (100, 33, False, "rect"), (512, 128, True, "hann")):
        design = linne_amd.project_design(n_fft, None, window)
        first, n = 40, 2000
        f0, f1 = -(-first // hop), -(-(first + n) // hop)
        z = ctx.stft_windows([(u.dev, u.index, first, n), (u.dev, u.index, first, n)], n_fft, hop, window=window, center=center)
        assert tuple(z.shape) == (2, 3, f1 - f0, n_fft // 2 + 1, 2)
        ref = expected_project(u.full, f0, f1 - f0, design, hop, n_fft // 2 if center else 0, 15)[0]
        assert np.array_equal(z[0].cpu().numpy().reshape(3, f1 - f0, -1), ref)
        zr = ctx.stft_windows([(u.dev, u.index, first, n)], n_fft, hop, window=window, center=center, rows_first=True, dtype=torch.float32, float_exp=15, shift=0)
        ref0 = expected_project(u.full, f0, f1 - f0, design, hop, n_fft // 2 if center else 0, 0, f32=True, float_exp=15)[0]
        assert tuple(zr.shape) == (1, 3, n_fft // 2 + 1, 2, f1 - f0) and np.array_equal(zr[0].cpu().numpy().reshape(3, -1, f1 - f0), ref0.transpose(0, 2, 1))
    # the power spectrum, against Python integers
    n_fft, hop = 64, 16
    design = linne_amd.project_design(n_fft)
    got = ctx.spectrum_streams([t.dev, u.dev, t.dev], n_fft, hop)
    for x, g in zip((t, u, t), got):
        y = projected_values(x.full, 0, project_length(x.ns, hop), design, hop, n_fft // 2, 15)[0]
        want = [[sum(int(y[c, f, 2 * j]) ** 2 + int(y[c, f, 2 * j + 1]) ** 2 for f in range(y.shape[1])) for j in range(n_fft // 2 + 1)] for c in range(x.nch)]
        assert g == want and all(isinstance(v, int) for row in g for v in row)
    assert ctx.spectrum_streams([], 64, 16) == []


# 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_streams(ctx, oracle, wide):
    """the streams of tests/project_edges.py on the device: two whose chosen signal the oracle encodes -- the codec is lossless, and
    encoded() asserts that the decode is the signal --, one written block by block with synth_records, whose decode under the oracle is
    asserted to be zeros but for the four 4-plane edge values; and the "wide values" stream"""
    out = {}
    for name in pe.PLANTS:
        bits, x = pe.planted_signal(name)
        out[name] = encoded(ctx, oracle, x, bits, 5, bits == 16, name)
        assert out[name].bl[-1][2] == RAW
    data, x = pe.crafted_stream()
    out["crafted"] = Stream(ctx, oracle, data, "crafted")
    assert np.array_equal(out["crafted"].full, x) and np.count_nonzero(x) == 4
    yield dict(out, wide=wide)
    for t in out.values():
        t.index.close()


def test_plane_counts_at_their_edges(ctx, edge_streams):
    """values at the edges of the plane rule -- 32767, -32768 (2 planes), 32768, -32769, 2^23 - 1, -2^23 (3), 2^23, -2^23 - 1, INT32_MAX,
    INT32_MIN (4) --, each the only one of its width among the values its tile reads: at the tile's first frame's first sample, at its
    last frame's last sample, in a ragged last tile, and -- where the hop is beyond the frame -- in the gap between two frames, where
    it must neither widen the tile nor change an output.  The library does not report the plane count it chose: the check is that every
    element equals the reference's, which a tile cut into too few planes, or a scan that misses the value, cannot give.  The premises --
    which count each tile must choose, under which of the kernel's two scans, where its widest value lies -- are project_edges.py's,
    computed from the oracle's decode with project_refs.sample_planes, asserted here and, without a GPU, in test_stream_project_cpu.py"""
    t = edge_streams
    windows, counts = pe.edge_windows({name: x.full for name, x in t.items()}, found=[("wide", ch, p) for ch, p in pe.WIDE_AT])
    pe.assert_coverage(windows, counts)
    bases = {"one": np.array([[1], [-1], [32767], [-32768]], dtype=np.int16), "b70": random_basis(np.random.default_rng(12), 19, 70)}
    items = [item(t[w["stream"]], w["first"], w["n"], bases[w["basis"]], w["hop"], before=w["before"], shift=w["shift"], order=("fk", "kf")[k % 2], pad=k % 3) for k, w in enumerate(windows)]
    assert all(it["basis"].shape[1] == w["N"] for it, w in zip(items, windows))
    held(ctx, items, group_frames=(0, 2))


# 8 ------------------------------------------------------------------------------------------------------------------------------
FULL = {"min16": (16, -32768), "max16": (16, 32767), "min24": (24, -(1 << 23)), "max24": (24, (1 << 23) - 1)}


@pytest.fixture(scope="module")
def constant(ctx, oracle):
    """mono streams of 5 blocks whose every sample is one end of their width's range (encoded() asserts the decode)"""
    out = {name: encoded(ctx, oracle, np.full((1, 5 * S), v, dtype=np.int32), bits, 0, False, name) for name, (bits, v) in FULL.items()}
    yield out
    for t in out.values():
        t.index.close()


def test_accumulators_at_their_worst_case(ctx, constant):
    """frames of 4096 samples of constant full scale under rows of constant and alternating full scale: the largest sums a pair of
    digit planes can have.  A digit product is at most (-128) * (-128) = 2^14, and 4096 of them are 2^26 -- reached here exactly, by
    the low and by the high planes of -32768 (and of -2^23) under a row of -32768; no pair goes beyond it, so every pair's int32
    accumulator holds.  The bound is per pair of planes and the same whatever the plane count, so streams of 2 and of 3 planes
    suffice.  At shift 0 every sum leaves int32 and `saturated` is set; at shift 31 the values themselves show"""
    rows = [[-32768] * 4096, [32767] * 4096, [-129] * 4096, [127] * 4096, [128] * 4096, [32767, -32768] * 2048, [-32768, 32767] * 2048]
    basis = np.array(rows, dtype=np.int16)
    worst = 0
    for name, (bits, v) in FULL.items():
        assert (constant[name].full == v).all() and constant[name].ns >= 4096 + 63
        P = sample_planes(v)
        assert P == (2 if bits == 16 else 3)
        xd = sample_digits(v, P)
        for row in rows:
            sums = [sum(basis_digits(c)[a] for c in row) * xd[b] for a in range(2) for b in range(P)]      # (the frame is constant: the sum over n factors)
            assert all(abs(q) <= 1 << 26 for q in sums)
            worst = max(worst, max(abs(q) for q in sums))
            if v < 0 and row[0] == row[1] == -32768:
                assert sums.count(1 << 26) == 2 * P                  # every pair of planes: all digits are -128
            assert abs(sum(row) * v) > 1 << 31 or row[0] != row[1]                  # a constant row's result leaves int32 (an alternating row's is -+2048 v)
    assert worst == 1 << 26
    items = [item(constant[name], first, n, basis, H, shift=shift, order=order) for name in FULL for shift in (0, 31)
             for first, n, H, order in ((0, 65, 1, "fk"), (3, 17, 64, "kf"))]
    held(ctx, items, group_frames=(0, 2))
    assert all(reference(it)[1] == (it["shift"] == 0) for it in items)


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_tables_are_told_apart_by_pointer_rows_and_frame_length(ctx, streams):
    """windows of one call share one int16 array's pointer under three shapes -- (K, N), its first K - 3 rows, and the same words as
    rows of M -- beside an array of equal content at another address: each window's values are those of its own table"""
    rng = np.random.default_rng(21)
    K, N, M = 12, 40, 30
    base = random_basis(rng, K, N)
    views = [base, base[:K - 3], base.reshape(K * N // M, M), base.copy()]
    items = []
    for k in range(12):
        t, b = streams[(2, 3)[k % 2]], views[(k + k // 4) % 4]
        H = (1, 7, 45)[k % 3]
        items.append(item(t, 5 * k, min(70 - k, project_length(t.ns, H) - 5 * k), b, H, before=k % min(b.shape[1], 29), shift=12, clip_bits=(0, 24)[k % 2], order=("fk", "kf")[(k // 2) % 2], pad=k % 2))
    ptr = lambda it: it["basis"].ctypes.data
    assert {(ptr(it), it["basis"].shape) for it in items} == {(base.ctypes.data, (12, 40)), (base.ctypes.data, (9, 40)), (base.ctypes.data, (16, 30)), (views[3].ctypes.data, (12, 40))}
    assert views[3].ctypes.data != base.ctypes.data and np.array_equal(views[3], base)
    # the premise: a window read with the table of another shape at the same pointer has other values -- the first window of the
    # reshaped view against the whole array's first 30 columns, and the row the shorter view lacks is no row of zeros
    j = next(i for i, it in enumerate(items) if it["basis"] is views[2])
    it = items[j]
    other = expected_project(it["t"].full, it["first"], it["n"], base[:, :M], it["hop"], it["before"], it["shift"], it["clip"])[0]
    assert not np.array_equal(reference(it)[0][:, :, :K], other) and base[K - 3:].any()
    held(ctx, items, group_frames=(0, 3))


# 10 -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse(ctx, oracle):
    """a mono stream of 17 * 65536 - 100 samples -- 17 frames at hop 65536 -- as tests/far_streams.py builds them: SILENT blocks and two
    islands of sound, one under frame 3 and one under frame 9 of that hop; its decode is small enough to hold whole"""
    stream, d = fs.far_stream(oracle, 1, 16, 0, False, [(3 * 65536 - 1000, list(fs.ISLAND), 801), (9 * 65536 - 2000, list(fs.ISLAND), 802)], 17 * 65536 - 100)
    dev = sc.to_device(stream)

    class Track:
        name, nch, ns, full = "sparse mono", 1, d.total, d.pcm.dense()
    Track.dev, Track.index = dev, ctx.index_stream(dev)
    assert Track.full.shape == (1, 17 * 65536 - 100) and Track.full[0, 3 * 65536:3 * 65536 + 2000].any() and Track.full[0, 9 * 65536:9 * 65536 + 1000].any()
    yield Track
    Track.index.close()


def test_the_largest_frame_with_the_most_rows(ctx, sparse):
    """frame_len 4096 with num_rows 2048 -- each runs elsewhere with a small partner only --: 17 frames of one channel, at the largest
    hop, where every frame is an image region of its own, and at hop 1"""
    basis = random_basis(np.random.default_rng(31), 2048, 4096)
    assert basis.shape == (linne_amd.PROJECT_MAX_ROWS, linne_amd.PROJECT_MAX_FRAME) and project_length(sparse.ns, 65536) == 17
    items = [item(sparse, 0, 17, basis, 65536, before=1000, shift=14), item(sparse, 3 * 65536 - 3000, 17, basis, 1, before=4095, shift=14, order="kf", pad=1),
             item(sparse, 9 * 65536 - 2000 + fs.ISLAND_SAMPLES - 10, 17, basis, 1, before=0, shift=0, clip_bits=16)]
    held(ctx, items, group_frames=(0, 2))
    y = reference(items[0])[0]
    assert [bool(y[0, f].any()) for f in range(17)] == [f in (3, 9) for f in range(17)]       # the two islands' frames, silence between
