"""GPU tests of encoding planar PCM held in device memory into a .lnn stream in device memory (Context.encode_stream;
include/linne_amd.h LINNEAmd_EncodeStreamDevice): the reference's streams, equality with LINNEEncoder_EncodeWhole (its result code
and bytes) over the preset matrix, passes and the quirk-Q2 state, -a / -l, plans the host settles, errors, input views, an on-device
round trip, and the plumbing of torch tensors and streams."""
import ctypes as C

import numpy as np
import pytest

import linne_amd
from refs import _planar_ptrs
from signals import music
from stream_refs import blocks, mixed_signal

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, INVALID_FORMAT, INSUFFICIENT_BUFFER = 0, 1, 2, 3
COMPRESS, SILENT, RAW = 0, 1, 2


def encode(ctx, x, bits, rate, block, preset, ms, **kw):
    """(code, stream bytes or None)"""
    try:
        r = ctx.encode_stream(x, bits, rate, block, preset, ms, **kw)
    except linne_amd.LinneAmdError as e:
        assert e.code is not None, str(e)
        return e.code, None
    return OK, bytes(r.cpu().numpy())


def whole_code(product, x, bits, rate, block, preset, ms, capacity=None):
    """(code, bytes) of EncodeWhole on a fresh encoder with room for the header"""
    x = np.ascontiguousarray(x, dtype=np.int32)
    try:
        enc = product.new_encoder(x.shape[0], bits, rate, block, preset, ms, max_block=max(block, 1024))
    except RuntimeError as e:                                        # SetEncodeParameter's code
        return int(str(e).rsplit(" ", 1)[1]), None
    ptrs, _keep = _planar_ptrs(x)
    cap = capacity if capacity is not None else x.size * 8 + 65536
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    osz = C.c_uint32(0)
    ret = product.L.LINNEEncoder_EncodeWhole(enc, ptrs, x.shape[1], out.ctypes.data, cap, C.byref(osz))
    product.L.LINNEEncoder_Destroy(enc)
    return ret, (out[:osz.value].tobytes() if ret == OK else None)


def raw_call(ctx, pcm, hdr, buf, capacity, group_frames=0, state=None):
    """LINNEAmd_EncodeStreamDevice straight: (code, *out_bytes)"""
    nbytes = C.c_uint64(0)
    st = C.c_double(0.0) if state is None else state
    ctx._fence()
    ret = linne_amd.lib.LINNEAmd_EncodeStreamDevice(ctx.h, C.byref(hdr), C.c_void_p(pcm.data_ptr()), pcm.stride(0), group_frames,
                                                    C.c_void_p(buf), capacity, C.byref(nbytes), C.byref(st))
    return ret, nbytes.value


def alternating(nch=2, bits=16, block=4096, nblocks=12, seed=3):
    """blocks of music and of full-scale noise in turn (COMPRESS, RAW, ...), the last block -- a ragged one -- noise"""
    ns = nblocks * block - 1000
    x = music(nch, ns, bits, seed=seed).astype(np.int64)
    rng = np.random.default_rng(seed)
    lim = 1 << (bits - 1)
    for b in range(1, nblocks, 2):
        e = min((b + 1) * block, ns)
        x[:, b * block:e] = rng.integers(-lim, lim, size=(nch, e - b * block))
    return np.ascontiguousarray(x, dtype=np.int32)


@pytest.fixture(scope="module")
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_streams.npz"))


def test_reference_streams(ctx, golden):
    for i in range(12):
        bits, rate, block, preset, ms = (int(v) for v in golden[f"s{i}_meta"])
        code, got = encode(ctx, golden[f"s{i}_x"], bits, rate, block, preset, bool(ms))
        assert code == OK, f"stream {i}: {code}"
        assert got == golden[f"s{i}_lnn"].tobytes(), f"stream {i}"


@pytest.mark.parametrize("nch,bits,block,preset,ms,ns", [
    (1, 16, 4096, 0, False, 50000),
    (2, 16, 4096, 1, True, 60000),
    (2, 8, 2048, 2, False, 40000),
    (3, 24, 4096, 3, False, 30000),
    (2, 24, 1023, 4, True, 30000),
    (8, 16, 2048, 5, True, 20000),
    (4, 16, 1023, 6, False, 25000),
    (2, 16, 10240, 7, True, 100000),
])
def test_equal_to_encode_whole(ctx, product, nch, bits, block, preset, ms, ns):
    x = mixed_signal(nch, bits, ns, seed=nch * 100 + preset, block=block)
    want = product.encode_whole(x, bits, 44100, block, preset, ms)
    code, got = encode(ctx, x, bits, 44100, block, preset, ms)
    assert code == OK
    assert {COMPRESS, SILENT, RAW} <= {b[2] for b in blocks(got)}
    assert got == want
    F = (x.shape[1] + block - 1) // block
    assert sum(ctx.last_stream_encode_count(k) for k in range(3)) == F
    assert min(ctx.last_stream_encode_count(k) for k in range(3)) >= 1


def test_device_round_trip_at_large_batch_forms(product):
    """4.9 minutes of stereo at block 4096, -m 7: 3174 frames, 25 392 jobs -- beyond the 12 288 / 24 576 from which the analysis takes
    k_autocorr_hist and k_fwd_loss by itself.  The stream never leaves the device."""
    import torch
    x = mixed_signal(2, 16, 13_000_000, seed=11, block=4096)
    c = linne_amd.Context(0, use_torch_stream=True)
    try:
        c.enable_timing(True)
        d_x = torch.from_numpy(x).cuda()
        stream = c.encode_stream(d_x, 16, 44100, 4096, 7, True)
        assert c.last_launches(21) >= 1                                 # k_autocorr_hist: a large-batch form
        c.enable_timing(False)
        back = c.decode_stream(stream)
        assert torch.equal(back, d_x)
        assert bytes(stream.cpu().numpy()) == product.encode_whole(x, 16, 44100, 4096, 7, True)
    finally:
        c.close()


def test_passes_and_q2_state(ctx, product):
    x = alternating()
    F = (x.shape[1] + 4095) // 4096
    results = []
    for g in (1, 7, F - 1, 0):
        stream, state = ctx.encode_stream(x, 16, 44100, 4096, 7, True, group_frames=g, parcor_state=0.0)
        results.append((bytes(stream.cpu().numpy()), state))
        assert ctx.last_stream_encode_count(COMPRESS) >= 5 and ctx.last_stream_encode_count(RAW) >= 5
    assert all(r == results[0] for r in results), [r[1] for r in results]
    assert results[0][0] == product.encode_whole(x, 16, 44100, 4096, 7, True)
    assert results[0][1] != 0.0
    # two calls that thread the state = two EncodeWhole calls on one encoder
    x1, x2 = alternating(seed=5)[:, :30000], alternating(seed=6)
    enc = product.new_encoder(2, 16, 44100, 4096, 7, True)
    want = []
    for part in (x1, x2):
        part = np.ascontiguousarray(part)
        ptrs, _keep = _planar_ptrs(part)
        cap = part.size * 8 + 65536
        out = np.zeros(cap, dtype=np.uint8)
        osz = C.c_uint32(0)
        assert product.L.LINNEEncoder_EncodeWhole(enc, ptrs, part.shape[1], out.ctypes.data, cap, C.byref(osz)) == 0
        want.append(out[:osz.value].tobytes())
    product.L.LINNEEncoder_Destroy(enc)
    state = 0.0
    for part, w, g in zip((x1, x2), want, (3, 0)):
        stream, state = ctx.encode_stream(np.ascontiguousarray(part), 16, 44100, 4096, 7, True, group_frames=g, parcor_state=state)
        assert bytes(stream.cpu().numpy()) == w


@pytest.mark.parametrize("setting", ["af", "learning"])
def test_af_iterations_and_learning(ctx_env, product, setting):
    x = mixed_signal(2, 16, 9000, seed=21, block=1024)[:, :9000]
    with ctx_env({}) as c:
        if setting == "af":
            c.set_af_iterations(1)
            want = product.encode_whole(x, 16, 44100, 1024, 4, True, af_iters=1)
        else:
            c.set_learning(True)
            want = product.encode_whole(x, 16, 44100, 1024, 4, True, learning=1)
        code, got = encode(c, x, 16, 44100, 1024, 4, True)
        assert code == OK and got == want


def test_plans_settled_on_the_host(ctx_env, product):
    x = mixed_signal(2, 16, 60000, seed=31, block=4096)
    want = product.encode_whole(x, 16, 44100, 4096, 7, True)
    with ctx_env({"LINNE_AMD_RICE_GUARD": "0.5"}) as c:
        code, got = encode(c, x, 16, 44100, 4096, 7, True)
        assert code == OK and got == want
        assert c.last_stream_encode_count(3) >= c.last_stream_encode_count(COMPRESS) > 0


@pytest.mark.parametrize("nch,bits,rate,block,preset,ms", [
    (2, 16, 44100, 4096, 8, True),          # preset out of range
    (2, 16, 44100, 0, 7, True),             # zero block
    (2, 16, 0, 4096, 7, True),              # zero rate
    (2, 0, 44100, 4096, 7, True),           # zero width
    (1, 16, 44100, 4096, 7, True),          # MS on one channel
    (2, 16, 44100, 128, 7, True),           # a block no longer than a layer
    (9, 16, 44100, 4096, 3, False),         # too many channels
])
def test_header_errors(ctx, product, nch, bits, rate, block, preset, ms):
    x = music(nch, 5000, 16, seed=1)
    want, _ = whole_code(product, x, bits, rate, block, preset, ms)
    assert want != OK
    code, _ = encode(ctx, x, bits, rate, block, preset, ms)
    assert code == want


def test_raw_block_at_12_bits(ctx, product):
    rng = np.random.default_rng(7)
    x = rng.integers(-2048, 2048, size=(2, 20000)).astype(np.int32)
    want, _ = whole_code(product, x, 12, 44100, 4096, 3, False)
    assert want == INVALID_FORMAT
    code, _ = encode(ctx, x, 12, 44100, 4096, 3, False)
    assert code == want


def test_capacity(ctx, product):
    import torch
    x = mixed_signal(2, 16, 40000, seed=41, block=4096)
    want = product.encode_whole(x, 16, 44100, 4096, 5, True)
    n = len(want)
    pcm = torch.from_numpy(x).cuda()
    hdr = linne_amd.Header(1, 2, 2, x.shape[1], 44100, 16, 4096, 5, 1)
    buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ret, nbytes = raw_call(ctx, pcm, hdr, buf.data_ptr(), n - 1)
    assert (ret, nbytes) == (INSUFFICIENT_BUFFER, n)
    assert whole_code(product, x, 16, 44100, 4096, 5, True, capacity=n - 1)[0] == INSUFFICIENT_BUFFER
    assert bool((buf[n - 1:] == 0xA5).all())
    ret, nbytes = raw_call(ctx, pcm, hdr, buf.data_ptr(), 20)                   # under the header's 30 bytes
    assert (ret, nbytes) == (INSUFFICIENT_BUFFER, n) and bool((buf[20:] == 0xA5).all())
    ret, nbytes = raw_call(ctx, pcm, hdr, buf.data_ptr(), n)
    assert (ret, nbytes) == (OK, n)
    assert bytes(buf[:n].cpu().numpy()) == want and bool((buf[n:] == 0xA5).all())
    # passes: each one's region [first byte, first byte of the next) is cleared on its own, whole words inside it and single bytes at
    # its edges, so the passes' first bytes have to meet every place in a 32-bit word
    offs = [b[0] for b in blocks(bytes(buf[:n].cpu().numpy()))]
    assert {o % 4 for g in (1, 3) for o in offs[::g]} == {0, 1, 2, 3}, offs
    for g in (1, 3):
        buf.fill_(0xA5)
        ret, nbytes = raw_call(ctx, pcm, hdr, buf.data_ptr(), n, group_frames=g)
        assert (ret, nbytes) == (OK, n), g
        assert bytes(buf[:n].cpu().numpy()) == want and bool((buf[n:] == 0xA5).all()), g
    assert raw_call(ctx, pcm, hdr, buf.data_ptr() + 2, n)[0] == INVALID_ARGUMENT
    # full-scale noise: every block RAW
    rng = np.random.default_rng(9)
    noise = rng.integers(-32768, 32768, size=(1, 9000)).astype(np.int32)
    code, got = encode(ctx, noise, 16, 44100, 1024, 0, False)
    assert code == OK and got == product.encode_whole(noise, 16, 44100, 1024, 0, False)


def test_input_views(ctx, product):
    import torch
    x = mixed_signal(3, 16, 30000, seed=51, block=4096)
    big = torch.zeros((3, x.shape[1] + 37), dtype=torch.int32, device="cuda")
    big[:, 5:5 + x.shape[1]] = torch.from_numpy(x).cuda()
    view = big[:, 5:5 + x.shape[1]]
    assert view.stride(0) > view.shape[1] and view.storage_offset() % 2 == 1
    code, got = encode(ctx, view, 16, 44100, 4096, 3, False)
    assert code == OK and got == product.encode_whole(x, 16, 44100, 4096, 3, False)
    short = music(2, 700, 16, seed=52)                                  # shorter than one block
    code, got = encode(ctx, short, 16, 44100, 1024, 7, True)
    assert code == OK and got == product.encode_whole(short, 16, 44100, 1024, 7, True)
    one = music(1, 2048, 16, seed=53)                                   # a single frame
    code, got = encode(ctx, one, 16, 44100, 2048, 2, False)
    assert code == OK and got == product.encode_whole(one, 16, 44100, 2048, 2, False)


@pytest.mark.parametrize("use_torch_stream", [True, False])
def test_torch_stream_ordering(product, use_torch_stream):
    import torch
    x = mixed_signal(2, 16, 40000, seed=61, block=4096)
    want = np.frombuffer(product.encode_whole(x, 16, 44100, 4096, 7, True), dtype=np.uint8)
    c = linne_amd.Context(0, use_torch_stream=use_torch_stream)
    try:
        src = torch.from_numpy(x).cuda()
        for _ in range(3):
            inp = torch.empty_like(src)
            inp.copy_(src)                                   # written by torch just before the call
            stream = c.encode_stream(inp, 16, 44100, 4096, 7, True)
            assert int(stream.to(torch.int64).sum().item()) == int(want.astype(np.int64).sum())     # read by torch right after it
            inp.zero_()
            assert np.array_equal(stream.cpu().numpy(), want)
    finally:
        c.close()


def test_timing_kinds(product):
    x = mixed_signal(2, 16, 40000, seed=71, block=4096)
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        c.enable_timing(True)
        stream = c.encode_stream(x, 16, 44100, 4096, 7, True, group_frames=5)
        for k in list(range(60, 68)) + [49, 51, 17]:
            assert c.last_launches(k) >= 2, k                               # two passes
        assert c.last_launches(68) >= 1 and c.last_ms(0) > 0
        for k in (48, 50, 52, 53, 54, 55):                                  # the kinds of the single call's own launches: retired
            assert c.last_launches(k) == 0, k
        assert bytes(stream.cpu().numpy()) == product.encode_whole(x, 16, 44100, 4096, 7, True)
    finally:
        c.close()
