"""GPU tests of encoding many PCM tracks held in device memory into their .lnn streams in one call (Context.encode_streams;
include/linne_amd.h LINNEAmd_EncodeStreamsDevice): the reference's streams in one call, more frame lengths than one analysis call
takes, passes and the quirk-Q2 state per track, failing tracks among good ones, mixed shapes with -a / -l and host-settled plans,
launch counts that do not grow with the tracks, short tracks at the large-batch forms, and the plumbing of views and torch streams.
Every track's answer is held to the single call's (Context.encode_stream) and to LINNEEncoder_EncodeWhole's."""
import ctypes as C

import numpy as np
import pytest

import linne_amd
from refs import _planar_ptrs
from signals import music
from stream_refs import blocks, mixed_signal
from test_gpu_stream_encode import alternating

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, INVALID_FORMAT, INSUFFICIENT_BUFFER = 0, 1, 2, 3
COMPRESS, SILENT, RAW = 0, 1, 2
SE_KINDS = list(range(48, 56)) + list(range(60, 69))      # include/linne_amd.h: the stream encoder's kernels, single call and many tracks
MAXLEN = 16                                                # distinct frame lengths LINNEAmd_EncodeFramesDevice takes per call


def as_bytes(t):
    return bytes(t.cpu().numpy())


def analysis_calls(lengths, block):
    """the rule of include/linne_amd.h for a pass holding tracks of these lengths"""
    distinct = set()
    for n in lengths:
        if n >= block:
            distinct.add(block)
        if n % block:
            distinct.add(n % block)
    d = len(distinct)
    return 1 if d <= MAXLEN else 1 + -(-(d - MAXLEN) // MAXLEN)


@pytest.fixture(scope="module")
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_streams.npz"))


def test_reference_streams_in_one_call(ctx, golden):
    tracks, shapes = [], set()
    for i in range(12):
        bits, rate, block, preset, ms = (int(v) for v in golden[f"s{i}_meta"])
        x = golden[f"s{i}_x"]
        tracks.append((x, bits, rate, block, preset, bool(ms)))
        shapes.add((x.shape[0], bits, block, preset, ms))
    got = ctx.encode_streams(tracks)
    assert ctx.last_stream_batch_count(0) == len(shapes) > 1
    for i in range(12):
        assert as_bytes(got[i]) == golden[f"s{i}_lnn"].tobytes(), f"stream {i}"
        assert got[i].data_ptr() % 4 == 0


def test_more_lengths_than_one_analysis_call(ctx, product):
    import torch
    block = 1024
    lengths = [2 * block + 200 + 37 * i for i in range(20)] + [3 * block, 700, block]
    assert min(200 + 37 * i for i in range(20)) > 128 and len({n % block for n in lengths[:20]}) == 20
    xs = [torch.from_numpy(music(2, n, 16, seed=100 + i)).cuda() for i, n in enumerate(lengths)]
    xs.append(xs[0])                                                    # two tracks read the same PCM
    lengths.append(lengths[0])
    assert len(xs) == 24
    got = ctx.encode_streams([(x, 16, 44100, block, 4, True) for x in xs])
    want_calls = analysis_calls(lengths, block)
    assert want_calls == 2
    assert ctx.last_stream_batch_count(2) == want_calls and ctx.last_stream_batch_count(1) == 1 and ctx.last_stream_batch_count(0) == 1
    for i, x in enumerate(xs):
        b = as_bytes(got[i])
        assert b == as_bytes(ctx.encode_stream(x, 16, 44100, block, 4, True)), f"track {i}: not the single call's bytes"
        assert b == product.encode_whole(x.cpu().numpy(), 16, 44100, block, 4, True), f"track {i}: not EncodeWhole's bytes"


def test_passes_and_q2_state_per_track(ctx, product):
    xs = [alternating(nblocks=nb, seed=seed)[:, :ns] for nb, seed, ns in
          ((4, 11, 15384), (3, 12, 9000), (5, 13, 19480), (2, 14, 7192), (4, 15, 13000), (3, 16, 11288))]
    tracks = [(x, 16, 44100, 4096, 7, True) for x in xs]
    total = sum((x.shape[1] + 4095) // 4096 for x in xs)
    single = [ctx.encode_stream(x, 16, 44100, 4096, 7, True, parcor_state=0.0) for x in xs]
    single = [(as_bytes(s), st) for s, st in single]
    assert any(st != 0.0 for _, st in single)
    assert all({COMPRESS, RAW} <= {b[2] for b in blocks(s)} for s, _ in single[:3])
    for g in (1, 7, total - 1, 0):
        streams, states = ctx.encode_streams(tracks, group_frames=g, parcor_states=[0.0] * len(xs))
        assert ctx.last_stream_batch_count(1) == (-(-total // g) if g else 1), g
        for i in range(len(xs)):
            assert (as_bytes(streams[i]), states[i]) == single[i], f"group_frames {g}, track {i}"
    # the reversed order: no state leaks from one track into the next
    streams, states = ctx.encode_streams(tracks[::-1], group_frames=5, parcor_states=[0.0] * len(xs))
    for i in range(len(xs)):
        assert (as_bytes(streams[len(xs) - 1 - i]), states[len(xs) - 1 - i]) == single[i], f"reversed, track {i}"
    # two calls that thread the states = per track, two EncodeWhole calls on one encoder
    firsts = [alternating(seed=20 + i)[:, :30000 - 1000 * i] for i in range(3)]
    seconds = [alternating(nblocks=5, seed=30 + i) for i in range(3)]
    want = []
    for x1, x2 in zip(firsts, seconds):
        enc = product.new_encoder(2, 16, 44100, 4096, 7, True)
        pair = []
        for part in (x1, x2):
            part = np.ascontiguousarray(part)
            ptrs, _keep = _planar_ptrs(part)
            cap = part.size * 8 + 65536
            out = np.zeros(cap, dtype=np.uint8)
            osz = C.c_uint32(0)
            assert product.L.LINNEEncoder_EncodeWhole(enc, ptrs, part.shape[1], out.ctypes.data, cap, C.byref(osz)) == 0
            pair.append(out[:osz.value].tobytes())
        product.L.LINNEEncoder_Destroy(enc)
        want.append(pair)
    states = [0.0] * 3
    for k, (parts, g) in enumerate(((firsts, 3), (seconds, 0))):
        streams, states = ctx.encode_streams([(np.ascontiguousarray(x), 16, 44100, 4096, 7, True) for x in parts], group_frames=g, parcor_states=states)
        for i in range(3):
            assert as_bytes(streams[i]) == want[i][k], f"call {k}, track {i}"


def test_failing_tracks_among_good_ones(ctx, product):
    import torch
    rng = np.random.default_rng(7)
    good = [mixed_signal(2, 16, 8000, seed=200 + i, block=1024)[:, :8000 - 100 * i] for i in range(4)]
    want_good = [product.encode_whole(x, 16, 44100, 1024, 4, True) for x in good]
    fit = music(2, 5000, 16, seed=210)
    n_fit = len(product.encode_whole(fit, 16, 44100, 1024, 4, True))
    mono = music(1, 5000, 16, seed=211)
    noise12 = rng.integers(-2048, 2048, size=(2, 5000)).astype(np.int32)
    # (pcm, header fields after num_samples: rate, bits, block, preset, ms; capacity or None = plenty; byte offset of d_out)
    plan = [
        (good[0], (44100, 16, 1024, 4, 1), None, 0),
        (fit, (44100, 16, 4096, 8, 1), None, 0),            # preset out of range
        (fit, (44100, 16, 0, 7, 1), None, 0),               # zero block
        (good[1], (44100, 16, 1024, 4, 1), None, 0),
        (mono, (44100, 16, 1024, 4, 1), None, 0),           # MS on one channel
        (noise12, (44100, 12, 1024, 3, 0), None, 0),        # a RAW block at 12 bits
        (good[2], (44100, 16, 1024, 4, 1), None, 0),
        (fit, (44100, 16, 1024, 4, 1), n_fit - 1, 0),       # one byte short
        (fit, (44100, 16, 1024, 4, 1), 20, 0),              # under the header's 30 bytes
        (good[3], (44100, 16, 1024, 4, 1), None, 0),
        (fit, (44100, 16, 1024, 4, 1), None, 2),            # d_out not 4-byte aligned
    ]
    T = len(plan)
    room = 65536
    pcm = [torch.from_numpy(np.ascontiguousarray(p[0])).cuda() for p in plan]

    def fill(arr, bufs):
        for i, (x, (rate, bits, block, preset, ms), cap, shift) in enumerate(plan):
            arr[i].header = linne_amd.Header(1, 2, x.shape[0], x.shape[1], rate, bits, block, preset, ms)
            arr[i].d_pcm, arr[i].pcm_stride = pcm[i].data_ptr(), pcm[i].stride(0)
            arr[i].d_out, arr[i].capacity = bufs[i].data_ptr() + shift, room if cap is None else cap
            arr[i].out_bytes, arr[i].parcor_state, arr[i].result = 12345, 0.0, -1

    # the single call, track by track, into buffers of its own
    sbufs = [torch.full((room + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(T)]
    sarr = (linne_amd.Track * T)()
    fill(sarr, sbufs)
    single = []
    ctx._fence()
    for i in range(T):
        nbytes, state = C.c_uint64(12345), C.c_double(0.0)
        ret = linne_amd.lib.LINNEAmd_EncodeStreamDevice(ctx.h, C.byref(sarr[i].header), C.c_void_p(sarr[i].d_pcm), sarr[i].pcm_stride, 0,
                                                        C.c_void_p(sarr[i].d_out), sarr[i].capacity, C.byref(nbytes), C.byref(state))
        single.append((ret, nbytes.value, linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode()))
    codes = [s[0] for s in single]
    assert [codes[i] for i in (0, 3, 6, 9)] == [OK] * 4 and all(codes[i] not in (OK, INVALID_ARGUMENT) for i in (1, 2, 4))
    assert codes[5] == INVALID_FORMAT and codes[7] == codes[8] == INSUFFICIENT_BUFFER and codes[10] == INVALID_ARGUMENT
    assert single[7][1] == single[8][1] == n_fit
    # the batch call
    bufs = [torch.full((room + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(T)]
    arr = (linne_amd.Track * T)()
    fill(arr, bufs)
    ctx._fence()
    ret = linne_amd.lib.LINNEAmd_EncodeStreamsDevice(ctx.h, arr, T, 0)
    err = linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode()
    assert [(arr[i].result, arr[i].out_bytes) for i in range(T)] == [(s[0], s[1]) for s in single]
    assert ret == single[1][0] and err == "track 1: " + single[1][2]
    for k, i in enumerate((0, 3, 6, 9)):
        assert as_bytes(bufs[i][:arr[i].out_bytes]) == want_good[k], f"track {i}"
    for i in range(T):
        cap = int(arr[i].capacity) + plan[i][3]
        assert bool((bufs[i][cap:] == 0xA5).all()), f"track {i}: written at or beyond its capacity"
        if single[i][0] != OK:
            untouched = sbufs[i] == 0xA5
            assert bool((bufs[i][untouched] == 0xA5).all()), f"track {i}: written where the single call writes nothing"
        else:
            assert bool((bufs[i][arr[i].out_bytes + 3 & ~3:] == 0xA5).all())
    # the Python entry: codes per track, the exception carries them
    tracks = [(p[0], p[1][1], p[1][0], p[1][2], p[1][3], bool(p[1][4])) for p in plan[:7]]
    streams, codes = ctx.encode_streams(tracks, return_codes=True)
    assert codes == [s[0] for s in single[:7]] and [s is None for s in streams] == [c != OK for c in codes]
    assert as_bytes(streams[3]) == want_good[1]
    with pytest.raises(linne_amd.LinneAmdError) as e:
        ctx.encode_streams(tracks)
    assert e.value.code == codes[1] and e.value.codes == codes


def test_single_call_text_is_the_track_text(ctx):
    """LINNEAmd_EncodeStreamDevice is the one-track case of LINNEAmd_EncodeStreamsDevice: for every kind of failure the batch call on
    the one track reads "track 0: " and exactly the single call's text, with the same code, out_bytes and parcor_state -- and the
    single call's texts are the ones it has always had."""
    import torch
    ns, block = 20000, 4096
    sound = torch.from_numpy(music(2, ns, 16, seed=220)).cuda()
    noise12 = torch.from_numpy(np.random.default_rng(7).integers(-2048, 2048, size=(2, ns)).astype(np.int32)).cuda()
    room = 4 * ns * 2 + 65536
    buf = torch.zeros(room + 64, dtype=torch.uint8, device="cuda")

    def both(pcm, bits, preset, ms, capacity, shift=0):
        """((code, out_bytes, state, text) of the single call, the same of the batch call on the one track)"""
        hdr = linne_amd.Header(1, 2, 2, ns, 44100, bits, block, preset, ms)
        nbytes, state = C.c_uint64(12345), C.c_double(0.25)
        ctx._fence()
        ret = linne_amd.lib.LINNEAmd_EncodeStreamDevice(ctx.h, C.byref(hdr), C.c_void_p(pcm.data_ptr()), pcm.stride(0), 0,
                                                        C.c_void_p(buf.data_ptr() + shift), capacity, C.byref(nbytes), C.byref(state))
        single = (ret, nbytes.value, state.value, linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode())
        arr = (linne_amd.Track * 1)()
        arr[0].header, arr[0].d_pcm, arr[0].pcm_stride = hdr, pcm.data_ptr(), pcm.stride(0)
        arr[0].d_out, arr[0].capacity = buf.data_ptr() + shift, capacity
        arr[0].out_bytes, arr[0].parcor_state, arr[0].result = 12345, 0.25, -1
        ret = linne_amd.lib.LINNEAmd_EncodeStreamsDevice(ctx.h, arr, 1, 0)
        assert ret == arr[0].result
        return single, (ret, arr[0].out_bytes, arr[0].parcor_state, linne_amd.lib.LINNEAmd_GetLastError(ctx.h).decode())

    single, batch = both(sound, 16, 4, 1, room)
    assert single == batch and single[0] == OK and single[3] == "" and single[2] != 0.25        # the state is replaced on OK
    n = single[1]
    cases = [
        ((sound, 16, 4, 1, room, 2), INVALID_ARGUMENT, 12345, "EncodeStreamDevice: d_out is not 4-byte aligned"),
        ((sound, 16, 8, 1, room), INVALID_FORMAT, 0, "EncodeStreamDevice: header refused by SetEncodeParameter's checks"),
        ((noise12, 12, 3, 0, room), INVALID_FORMAT, 0, "block 0: a RAW block at a width other than 8, 16 or 24 bits"),
        ((sound, 16, 4, 1, n - 1), INSUFFICIENT_BUFFER, n, f"the stream takes {n} bytes, the buffer holds {n - 1}"),
    ]
    for args, code, out_bytes, text in cases:
        single, batch = both(*args)
        assert single == (code, out_bytes, 0.25, text), text                                # a failing call leaves the state alone
        assert batch == (code, out_bytes, 0.25, "track 0: " + text), text


MATRIX = [
    (1, 16, 4096, 0, False, 50000),
    (2, 16, 4096, 1, True, 60000),
    (2, 8, 2048, 2, False, 40000),
    (3, 24, 4096, 3, False, 30000),
    (2, 24, 1023, 4, True, 30000),
    (8, 16, 2048, 5, True, 20000),
    (4, 16, 1023, 6, False, 25000),
    (2, 16, 10240, 7, True, 100000),
]


def test_mixed_shapes_in_one_call(ctx, product):
    xs, tracks = [], []
    for nch, bits, block, preset, ms, ns in MATRIX:
        ns = min(ns, 30000)
        x = np.ascontiguousarray(mixed_signal(nch, bits, ns, seed=nch * 100 + preset, block=block)[:, :ns])
        xs.append(x)
        tracks.append((x, bits, 44100, block, preset, ms))
    got = ctx.encode_streams(tracks)
    assert ctx.last_stream_batch_count(0) == 8 and ctx.last_stream_batch_count(1) == 8
    frames = sum((x.shape[1] + t[3] - 1) // t[3] for x, t in zip(xs, tracks))
    assert sum(ctx.last_stream_encode_count(k) for k in range(3)) == frames
    for x, t, g in zip(xs, tracks, got):
        assert as_bytes(g) == product.encode_whole(x, t[1], 44100, t[3], t[4], t[5]), t[1:]


@pytest.mark.parametrize("setting", ["af", "learning"])
def test_af_iterations_and_learning(ctx_env, product, setting):
    xs = [np.ascontiguousarray(mixed_signal(2, 16, 9000, seed=21 + i, block=1024)[:, :9000 - 300 * i]) for i in range(2)]
    with ctx_env({}) as c:
        if setting == "af":
            c.set_af_iterations(1)
            want = [product.encode_whole(x, 16, 44100, 1024, 4, True, af_iters=1) for x in xs]
        else:
            c.set_learning(True)
            want = [product.encode_whole(x, 16, 44100, 1024, 4, True, learning=1) for x in xs]
        got = c.encode_streams([(x, 16, 44100, 1024, 4, True) for x in xs])
        assert [as_bytes(g) for g in got] == want


def test_plans_settled_on_the_host(ctx_env, product):
    xs = [np.ascontiguousarray(mixed_signal(2, 16, 30000, seed=31 + i, block=4096)[:, :30000 - 500 * i]) for i in range(3)]
    want = [product.encode_whole(x, 16, 44100, 4096, 7, True) for x in xs]
    with ctx_env({"LINNE_AMD_RICE_GUARD": "0.5"}) as c:
        got = c.encode_streams([(x, 16, 44100, 4096, 7, True) for x in xs])
        assert [as_bytes(g) for g in got] == want
        assert c.last_stream_encode_count(3) >= c.last_stream_encode_count(COMPRESS) > 0


def test_launches_do_not_grow_with_tracks(product):
    import torch
    ns = 5 * 2048 + 900
    xs = [torch.from_numpy(music(2, ns, 16, seed=300 + i)).cuda() for i in range(32)]
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        c.enable_timing(True)
        census = []
        for n in (4, 32):
            got = c.encode_streams([(x, 16, 44100, 2048, 5, True) for x in xs[:n]])
            census.append({k: c.last_launches(k) for k in SE_KINDS})
            assert c.last_stream_batch_count(2) == 1 and c.last_stream_batch_count(1) == 1
            assert c.last_ms(0) > 0
        assert census[0] == census[1]
        assert all(census[0][k] == 0 for k in (48, 50, 52, 53, 54, 55)), "the single call's own kernels are not the batch call's"
        assert all(census[0][k] == 1 for k in (49, 51) + tuple(range(60, 69))), census[0]
        c.enable_timing(False)
        for i in (0, 31):
            assert as_bytes(got[i]) == product.encode_whole(xs[i].cpu().numpy(), 16, 44100, 2048, 5, True)
    finally:
        c.close()


def test_short_tracks_reach_the_large_batch_forms(product):
    """64 stereo tracks of 25 full frames and a tail at block 4096, -m 7: 1664 frames, 13 312 jobs -- beyond the 12 288 from which the
    analysis takes k_autocorr_hist (kind 21) by itself, which one such track (26 frames, 208 jobs) is far below.  The streams never
    leave the device: one decode_windows call gives the input tensors back."""
    import torch
    tails = (200, 1311, 2048, 4001)
    base = torch.from_numpy(music(2, 25 * 4096 + 64 * 64 + max(tails), 16, seed=400)).cuda()
    xs = [base[:, 64 * i:64 * i + 25 * 4096 + tails[i % 4]] for i in range(64)]       # 64 different windows of one long signal
    c = linne_amd.Context(0, use_torch_stream=True)
    try:
        c.enable_timing(True)
        one = c.encode_stream(xs[5], 16, 44100, 4096, 7, True)
        assert c.last_launches(21) == 0, "one track alone is analysed with the latency forms"
        streams = c.encode_streams([(x, 16, 44100, 4096, 7, True) for x in xs])
        assert c.last_launches(21) >= 1, "k_autocorr_hist: a large-batch form"
        assert c.last_stream_batch_count(1) == 1 and c.last_stream_batch_count(2) == 1
        c.enable_timing(False)
        assert torch.equal(one, streams[5])
        index = [c.index_stream(s) for s in streams]
        back = c.decode_windows([(s, ix, 0, None) for s, ix in zip(streams, index)])
        for ix in index:
            ix.close()
        for i in range(64):
            assert torch.equal(back[i], xs[i]), f"track {i}"
        for i in (0, 21, 42, 63):
            assert as_bytes(streams[i]) == product.encode_whole(np.ascontiguousarray(xs[i].cpu().numpy()), 16, 44100, 4096, 7, True), f"track {i}"
    finally:
        c.close()


def test_input_views(ctx, product):
    import torch
    x = mixed_signal(3, 16, 30000, seed=51, block=4096)
    big = torch.zeros((3, x.shape[1] + 37), dtype=torch.int32, device="cuda")
    big[:, 5:5 + x.shape[1]] = torch.from_numpy(x).cuda()
    view = big[:, 5:5 + x.shape[1]]
    assert view.stride(0) > view.shape[1] and view.storage_offset() % 2 == 1
    short = music(3, 700, 16, seed=52)                                  # shorter than one block, the same shape
    got = ctx.encode_streams([(view, 16, 44100, 4096, 3, False), (short, 16, 44100, 4096, 3, False)])
    assert as_bytes(got[0]) == product.encode_whole(x, 16, 44100, 4096, 3, False)
    assert as_bytes(got[1]) == product.encode_whole(short, 16, 44100, 4096, 3, False)
    assert ctx.last_stream_batch_count(0) == 1
    assert ctx.encode_streams([]) == [] and ctx.last_stream_batch_count(1) == 0


@pytest.mark.parametrize("use_torch_stream", [True, False])
def test_torch_stream_ordering(product, use_torch_stream):
    import torch
    xs = [mixed_signal(2, 16, 30000, seed=61 + i, block=4096)[:, :30000 - 777 * i] for i in range(2)]
    want = [np.frombuffer(product.encode_whole(np.ascontiguousarray(x), 16, 44100, 4096, 7, True), dtype=np.uint8) for x in xs]
    c = linne_amd.Context(0, use_torch_stream=use_torch_stream)
    try:
        srcs = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]
        for _ in range(3):
            inps = [torch.empty_like(s) for s in srcs]
            for inp, s in zip(inps, srcs):
                inp.copy_(s)                                 # written by torch just before the call
            streams = c.encode_streams([(inp, 16, 44100, 4096, 7, True) for inp in inps])
            sums = [int(s.to(torch.int64).sum().item()) for s in streams]                           # read by torch right after it
            assert sums == [int(w.astype(np.int64).sum()) for w in want]
            for inp in inps:
                inp.zero_()
            for s, w in zip(streams, want):
                assert np.array_equal(s.cpu().numpy(), w)
    finally:
        c.close()
