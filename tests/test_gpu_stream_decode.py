"""GPU tests of decoding .lnn streams held in device memory (Context.index_stream / Context.decode_stream; include/linne_amd.h
LINNEAmd_StreamIndexCreate, LINNEAmd_DecodeStreamDevice): the reference's streams, equality with LINNEDecoder_DecodeWhole (its
result code and PCM, CRC check on), sample ranges, damaged streams and the plumbing of torch tensors and streams."""
import numpy as np
import pytest

import linne_amd
from stream_refs import blocks, mixed_signal

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, NG = 0, 1, 7
COMPRESS, SILENT, RAW = 0, 1, 2


def decode(ctx, stream, first=0, n=None, index=None):
    """(code, PCM as numpy or None)"""
    try:
        return OK, ctx.decode_stream(stream, first, n, index=index).cpu().numpy()
    except linne_amd.LinneAmdError as e:
        assert e.code is not None, str(e)
        return e.code, None


@pytest.fixture(scope="module")
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_streams.npz"))


def test_reference_streams(ctx, golden):
    for i in range(12):
        lnn, x = golden[f"s{i}_lnn"].tobytes(), golden[f"s{i}_x"]
        code, got = decode(ctx, lnn)
        assert code == OK, f"stream {i}: {code}"
        assert np.array_equal(got, x), f"stream {i}"


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
def test_equal_to_decode_whole(ctx, product, nch, bits, block, preset, ms, ns):
    x = mixed_signal(nch, bits, ns, seed=nch * 100 + preset, block=block)
    stream = product.encode_whole(x, bits, 44100, block, preset, ms)
    types = {b[2] for b in blocks(stream)}
    assert {COMPRESS, SILENT, RAW} <= types, f"block types {types}"
    ret, want = product.decode_whole(stream)
    assert ret == OK
    code, got = decode(ctx, stream)
    assert code == OK and np.array_equal(got, want) and np.array_equal(got, x)


def test_long_stream_takes_the_throughput_synthesis(ctx, product):
    """8 minutes of stereo at block 10240: 2068 channel-frames, beyond the 1536 from which the synthesis takes its throughput form"""
    x = mixed_signal(2, 16, 8 * 60 * 44100, seed=8, block=10240)
    stream = product.encode_whole(x, 16, 44100, 10240, 7, True)
    assert sum(1 for b in blocks(stream) if b[2] == COMPRESS) * 2 >= 1536
    ret, want = product.decode_whole(stream)
    assert ret == OK
    code, got = decode(ctx, stream)
    assert code == OK and np.array_equal(got, want)


def test_variable_block_lengths(ctx, product, reference):
    from test_gpu_parity import many_block_lengths, stream_of_blocks
    x, lens = many_block_lengths()
    stream = stream_of_blocks(product, x, 16, 44100, 4096, 7, True, lens)
    ret, want = reference.decode_whole(stream)
    assert ret == OK
    code, got = decode(ctx, stream)
    assert code == OK and want == np.ascontiguousarray(got, dtype=np.int32)


def test_false_sync_codes(ctx, product):
    """RAW 16-bit blocks of full-scale noise holding -32768 (zig-zag 0xFFFF): FF FF at offsets that start no block"""
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, size=(2, 60000)).astype(np.int32)
    x[:, ::97] = -32768
    stream = product.encode_whole(x, 16, 44100, 4096, 3, False)
    bl = blocks(stream)
    assert {b[2] for b in bl} == {RAW}
    starts = {b[0] for b in bl}
    arr = np.frombuffer(stream, dtype=np.uint8)
    ff = np.nonzero((arr[:-1] == 0xFF) & (arr[1:] == 0xFF))[0]
    assert len([p for p in ff if p >= 30 and int(p) not in starts]) > 100
    ret, want = product.decode_whole(stream)
    code, got = decode(ctx, stream)
    assert ret == OK and code == OK and np.array_equal(got, want) and np.array_equal(got, x)


@pytest.fixture(scope="module")
def mixed(product):
    x = mixed_signal(2, 16, 123457, seed=3)
    stream = product.encode_whole(x, 16, 44100, 4096, 5, True)
    ret, want = product.decode_whole(stream)
    assert ret == OK and np.array_equal(want, x)
    return stream, want


def test_ranges(ctx, mixed):
    import torch
    stream, full = mixed
    ns = full.shape[1]
    bl = blocks(stream)
    index = ctx.index_stream(stream)
    assert index.num_blocks == len(bl) and index.header["num_samples"] == ns
    d = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    cases = [(0, 1), (ns - 1, 1), (0, ns), (ns - 100, 100), (bl[-1][4], ns - bl[-1][4])]
    for off, size, typ, n, first in bl[1:6]:
        cases.append((first - 7, 20))                       # straddling a boundary
    for typ_want in (SILENT, RAW):
        b = next(b for b in bl if b[2] == typ_want)
        cases.append((b[4] + 5, b[3] - 10))                 # inside the block
        cases.append((b[4] - 3, b[3] + 6))                  # and across both its ends
    rng = np.random.default_rng(11)
    for _ in range(20):
        a = int(rng.integers(0, ns))
        cases.append((a, int(rng.integers(1, ns - a + 1))))
    for a, n in cases:
        code, got = decode(ctx, d, a, n, index=index)
        assert code == OK, (a, n)
        assert np.array_equal(got, full[:, a:a + n]), (a, n)
        code2, got2 = decode(ctx, d, a, n)                  # a fresh index: the same answer
        assert code2 == OK and np.array_equal(got2, got), (a, n)
    for a, n in [(ns, 1), (ns - 5, 6), (0, ns + 1)]:
        assert decode(ctx, d, a, n, index=index)[0] == INVALID_ARGUMENT
    assert decode(ctx, d, ns, 0, index=index)[0] == OK
    index.close()


def test_damaged_streams(ctx, product, mixed):
    stream, full = mixed
    bl = blocks(stream)
    rng = np.random.default_rng(7)
    header_bytes = list(range(0, 12)) + list(range(18, 22)) + [28, 29]
    bads = []
    for _ in range(12):
        b = bytearray(stream); p = int(rng.choice(header_bytes)); b[p] ^= 1 << int(rng.integers(0, 8)); bads.append(bytes(b))
    for _ in range(30):
        b = bytearray(stream); off = bl[int(rng.integers(0, len(bl)))][0]; p = off + int(rng.integers(0, 11))
        b[p] ^= 1 << int(rng.integers(0, 8)); bads.append(bytes(b))
    for _ in range(20):
        b = bytearray(stream); off, size = bl[int(rng.integers(0, len(bl)))][:2]; p = off + 11 + int(rng.integers(0, max(size - 11, 1)))
        if p < len(b):
            b[p] ^= 1 << int(rng.integers(0, 8)); bads.append(bytes(b))
    for _ in range(15):
        bads.append(stream[:int(rng.integers(0, len(stream)))])
    bads += [stream[:b[0]] for b in bl[1:4]] + [stream[:30], stream[:29], stream + b"\x00" * 5]
    compared = 0
    for i, bad in enumerate(bads):
        want, wpcm = product.decode_whole(bad)
        try:
            got = ctx.decode_stream(bad).cpu().numpy(); code, msg = OK, ""
        except linne_amd.LinneAmdError as e:
            got, code, msg = None, e.code, str(e)
        if code == NG and want != NG:
            assert "no encoder writes" in msg, (i, msg)      # the contract's one exception: a CRC-valid block no encoder writes
            continue
        assert code == want, (i, code, want)
        if code == OK:
            assert np.array_equal(got, wpcm), i
            compared += 1
    assert compared >= 3


def test_damage_before_and_after_a_range(ctx, mixed):
    stream, full = mixed
    bl = blocks(stream)
    k = len(bl) // 2
    off, size = bl[k][:2]
    bad = bytearray(stream)
    bad[off + size - 2] ^= 0x10                              # a payload byte of block k: its CRC fails
    bad = bytes(bad)
    index = ctx.index_stream(bad)
    before, after = bl[k - 2], bl[k + 1]
    code, got = decode(ctx, bad, before[4] + 1, before[3] - 2, index=index)
    assert code == OK and np.array_equal(got, full[:, before[4] + 1:before[4] + before[3] - 1])
    assert decode(ctx, bad, after[4], 10, index=index)[0] == 6            # DETECT_DATA_CORRUPTION
    assert decode(ctx, bad, bl[k][4] + 3, 5, index=index)[0] == 6
    index.close()


def test_input_view_at_an_odd_offset(ctx, mixed):
    import torch
    stream, full = mixed
    assert len(blocks(stream)) == 31
    src = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    for shift in (1, 3, 8, 15):                              # the gather of a block's bytes treats its end groups by the address modulo 16
        big = torch.zeros(len(stream) + 24, dtype=torch.uint8, device="cuda")
        assert big.data_ptr() % 16 == 0
        big[shift:shift + len(stream)] = src
        view = big[shift:shift + len(stream)]
        assert view.data_ptr() % 16 == shift
        code, got = decode(ctx, view)
        assert code == OK and np.array_equal(got, full), shift
        code, got = decode(ctx, view, 1000, 5000)
        assert code == OK and np.array_equal(got, full[:, 1000:6000]), shift


@pytest.mark.parametrize("use_torch_stream", [True, False])
def test_torch_stream_ordering(mixed, use_torch_stream):
    import torch
    stream, full = mixed
    c = linne_amd.Context(0, use_torch_stream=use_torch_stream)
    try:
        src = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
        want = int(full.astype(np.int64).sum())
        for _ in range(3):
            inp = torch.empty_like(src)
            inp.copy_(src)                                   # written by torch just before the call
            out = c.decode_stream(inp)
            assert int(out.to(torch.int64).sum().item()) == want          # read by torch right after it
            inp.zero_()
            idx = c.index_stream(src.clone())
            out = c.decode_stream(src, 2000, 30000, index=idx)
            assert torch.equal(out.cpu(), torch.from_numpy(full[:, 2000:32000]))
            idx.close()
    finally:
        c.close()


def test_timing_kinds(mixed):
    stream, full = mixed
    c = linne_amd.Context(0, use_torch_stream=False)
    try:
        c.enable_timing(True)
        idx = c.index_stream(stream)
        for k in range(37, 45):
            assert c.last_launches(k) >= 1, k
        assert c.last_ms(0) > 0
        c.decode_stream(stream, 0, None, index=idx)
        for k in (56, 57, 58, 59, 28):
            assert c.last_launches(k) >= 1, k
        idx.close()
    finally:
        c.close()
