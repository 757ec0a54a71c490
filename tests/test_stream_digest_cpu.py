"""CPU tests (-m "not gpu") of digesting resident .lnn streams (include/linne_amd.h LINNEAmd_DigestWindowsDevice): the boundary -- the
symbol, the structs, the timing kinds, the Python entry points, the argument errors that need no device --, the reference the GPU tests
hold the library to (expected_digest: numpy builds the byte string, zlib.crc32 hashes it; checked here against hand-written values and
against the WAV files the real reference's decoder writes), the algebra of lnn_k_digest.h restated in Python integers and held to
zlib.crc32, and the command line tool's -D option as far as it goes without a device."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import linne_amd
from signals import music
from test_cli_cpu import CLI
from stream_refs import digest_table as table, expected_digest, mixed_signal, pcm_bytes  # noqa: F401  (the GPU tests import them from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "linne_ref")
OK, INVALID_ARGUMENT = 0, 1


def wav_data(path):
    """the `data` chunk of a RIFF/WAVE file"""
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE"
    at = 12
    while at + 8 <= len(raw):
        size = struct.unpack("<I", raw[at + 4:at + 8])[0]
        if raw[at:at + 4] == b"data":
            return raw[at + 8:at + 8 + size]
        at += 8 + size + (size & 1)
    raise AssertionError("no data chunk")


def run(*args):
    return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


# ---- the algebra of lnn_k_digest.h in Python integers (reflected representation: bit 31 is x^0) ----
POLY, ONE, X8 = 0xEDB88320, 0x80000000, 0x00800000


def gf_mul(a, b):
    p = 0
    for i in range(32):
        if (a >> (31 - i)) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def xpow8(e):
    """x^(8 e)"""
    p, s = ONE, X8
    while e:
        if e & 1:
            p = gf_mul(p, s)
        s = gf_mul(s, s)
        e >>= 1
    return p


def raw(data, c=0):
    """the CRC register behind `data` from the initial value c, no final XOR"""
    for byte in data:
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
    return c


def fold(pieces, total):
    """crc32 of a string of `total` bytes from its pieces (offset, bytes), in the order given"""
    acc = 0
    for off, data in pieces:
        acc ^= gf_mul(raw(data), xpow8(total - off - len(data)))
    return acc ^ gf_mul(0xFFFFFFFF, xpow8(total)) ^ 0xFFFFFFFF


def kernel_digest(frames, b, lead, rng, ns=1, skip_zero=False):
    """the buckets' CRC-32s as k_wx_digest, k_wx_digest_preset and k_wx_digest_commit compute them: `frames` (n sample frames of F
    bytes each) cut into pieces of at most 256 frames whose boundaries lie at multiples of 256 behind `lead`, the pieces taken in
    shuffled order; a lane's term is raw(frame) (x) x^(8 F d), a (piece, bucket)'s word is taken to the bucket's end, the words are
    XORed into slot (piece's first frame // 256) % ns, and the commit XORs the slots and applies the length terms"""
    n, F = len(frames), len(frames[0])
    b = b if 0 < b < n else n
    nb = -(-n // b)
    acc = [[0] * nb for _ in range(ns)]
    cuts = sorted({0, n} | {c for c in range(lead, n, 256)})
    pieces = list(zip(cuts[:-1], cuts[1:]))
    rng.shuffle(pieces)
    for sa, sb in pieces:
        for k in range(sa // b, (sb - 1) // b + 1):
            te = min(sb, (k + 1) * b)
            r = 0
            for t in range(max(sa, k * b), te):
                if skip_zero and not any(frames[t]):
                    continue
                r ^= gf_mul(raw(frames[t]), xpow8(F * (te - 1 - t)))
            r = gf_mul(r, xpow8(F * (min((k + 1) * b, n) - te)))
            acc[(sa // 256) % ns][k] ^= r
    out = []
    for k in range(nb):
        r, size = 0, F * (min((k + 1) * b, n) - k * b)
        for s in range(ns):
            r ^= acc[s][k]
        out.append((r ^ gf_mul(0xFFFFFFFF, xpow8(size)) ^ 0xFFFFFFFF, size))
    return out


def test_symbol_structs_and_kinds_are_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bLINNEAmd_DigestWindowsDevice\s*\(", src)
    assert re.search(r"struct\s+LINNEAmdDigest\s*\{", src) and re.search(r"struct\s+LINNEAmdDigestSpec\s*\{", src)
    assert re.search(r"LINNE_AMD_DIGEST_T_DIGEST\s*=\s*83\b", src) and re.search(r"LINNE_AMD_DIGEST_T_PRESET\s*=\s*84\b", src)
    assert re.search(r"LINNE_AMD_DIGEST_T_COMMIT\s*=\s*85\b", src)
    assert "LINNEAmd_DigestWindowsDevice" in linne_amd.AMD_SYMBOLS
    assert hasattr(linne_amd.lib, "LINNEAmd_DigestWindowsDevice")


def test_struct_layouts():
    D, P = linne_amd.Digest, linne_amd.DigestSpec
    assert [(f[0], getattr(D, f[0]).offset) for f in D._fields_] == [("crc32", 0), ("reserved", 4), ("num_bytes", 8)]
    assert C.sizeof(D) == 16
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == [("bucket_samples", 0), ("d_out", 8)]
    assert C.sizeof(P) == 16
    d = linne_amd.DIGEST_DTYPE
    assert d.itemsize == 16 and [(n, d.fields[n][1]) for n in d.names] == [("crc32", 0), ("reserved", 4), ("num_bytes", 8)]


def test_python_entry_points():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(linne_amd.Context.digest_windows)
    assert list(p) == ["self", "windows", "bucket_samples", "group_frames", "return_codes"]
    assert (p["bucket_samples"].default, p["group_frames"].default, p["return_codes"].default) == (0, 0, False)
    p = sig(linne_amd.Context.digest_streams)
    assert list(p) == ["self", "streams", "bucket_samples", "group_frames"] and (p["bucket_samples"].default, p["group_frames"].default) == (0, 0)
    p = sig(linne_amd.Context.same_audio)
    assert list(p) == ["self", "stream_a", "stream_b", "bucket_samples"] and p["bucket_samples"].default == 0


def test_null_arguments_need_no_device():
    f = linne_amd.lib.LINNEAmd_DigestWindowsDevice
    w = (linne_amd.Window * 2)()
    s = (linne_amd.DigestSpec * 2)()
    for i in range(2):
        w[i].result = -1
    assert f(None, w, s, 2, 0) == INVALID_ARGUMENT and f(None, None, None, 0, 0) == INVALID_ARGUMENT
    blank = C.create_string_buffer(1 << 20)                     # zeroed memory larger than any context stands in for one
    ctx = C.addressof(blank)
    assert f(ctx, None, s, 2, 0) == INVALID_ARGUMENT            # NULL windows
    assert f(ctx, w, None, 2, 0) == INVALID_ARGUMENT            # NULL specs
    assert b"null argument" in linne_amd.lib.LINNEAmd_GetLastError(ctx)
    assert f(ctx, None, None, 0, 0) == OK and f(ctx, w, s, 0, 0) == OK
    assert [w[i].result for i in range(2)] == [-1, -1]


def test_the_reference_against_hand_written_values():
    # the check value of CRC-32: "123456789" -> 0xCBF43926; an 8-bit sample v is the byte v + 128
    mono = (np.frombuffer(b"123456789", dtype=np.uint8).astype(np.int32) - 128)[None, :]
    assert pcm_bytes(mono, 8, 0, 9) == b"123456789"
    assert expected_digest(mono, 8, 0, 9, 0) == [(0xCBF43926, 9)]
    assert expected_digest(mono, 8, 0, 9, 9) == expected_digest(mono, 8, 0, 9, 100) == [(0xCBF43926, 9)]
    assert expected_digest(mono, 8, 2, 4, 3) == [(zlib.crc32(b"345"), 3), (zlib.crc32(b"6"), 1)]
    stereo = mono[0, :8].reshape(4, 2).T                         # the same bytes, interleaved from two channels
    assert pcm_bytes(stereo, 8, 0, 4) == b"12345678" and expected_digest(stereo, 8, 1, 2, 0) == [(zlib.crc32(b"3456"), 4)]
    # one sample, and none: crc32 of one zero byte is 0xD202EF8D; a silent 8-bit sample is the byte 0x80
    assert expected_digest(np.array([[-128]]), 8, 0, 1, 0) == [(0xD202EF8D, 1)]
    assert expected_digest(np.array([[0]]), 8, 0, 1, 0) == [(zlib.crc32(b"\x80"), 1)]
    assert expected_digest(np.array([[0]]), 16, 0, 1, 0) == [(zlib.crc32(b"\0\0"), 2)] == [(0x41D912FF, 2)]
    assert expected_digest(mono, 8, 3, 0, 0) == [] and expected_digest(mono, 8, 3, 0, 5) == []
    # widths: little-endian, two's complement, truncated and never saturated
    x = np.array([[1, -2, 0x12345, -0x812345], [0x7FFF, -0x8000, 70000, -(1 << 31)]], dtype=np.int32)
    assert pcm_bytes(x, 16, 0, 2) == bytes([1, 0, 0xFF, 0x7F, 0xFE, 0xFF, 0x00, 0x80])
    assert pcm_bytes(x, 16, 2, 1) == bytes([0x45, 0x23, 0x70, 0x11])                         # 0x12345 and 70000 = 0x11170, cut
    assert pcm_bytes(x, 24, 2, 2) == bytes([0x45, 0x23, 0x01, 0x70, 0x11, 0x01, 0xBB, 0xDC, 0x7E, 0, 0, 0])
    assert pcm_bytes(x, 32, 3, 1) == bytes([0xBB, 0xDC, 0x7E, 0xFF, 0, 0, 0, 0x80])
    assert pcm_bytes(np.array([[200, -129]]), 8, 0, 2) == bytes([72, 255])                   # (v + 128) & 0xFF
    assert expected_digest(x, 24, 0, 4, 3) == [(zlib.crc32(pcm_bytes(x, 24, 0, 3)), 18), (zlib.crc32(pcm_bytes(x, 24, 3, 1)), 6)]


def test_table_reads_a_structured_array():
    a = np.zeros(2, dtype=linne_amd.DIGEST_DTYPE)
    a[1] = (0xCBF43926, 0, 1 << 40)
    assert table(a) == [(0, 0), (0xCBF43926, 1 << 40)]


@pytest.mark.skipif(not os.path.exists(REF_CLI), reason="oracle/_ref/linne_ref not built (python -c 'import __graft_entry__ as g; g.build()' where the reference's sources are)")
@pytest.mark.parametrize("bits", [8, 16, 24])
@pytest.mark.parametrize("nch", [1, 2])
def test_the_reference_against_the_reference_decoders_wav(oracle, tmp_path, bits, nch):
    """zlib.crc32 of the `data` chunk the real reference's `linne -d` writes = expected_digest of the oracle's decode, whole stream"""
    x = mixed_signal(nch, bits, 7 * 512 + 77, seed=40 + bits + nch, block=512)
    stream = bytes(oracle.encode_whole(x, bits, 22050, 512, 4, nch == 2))
    ret, full, _ = oracle.decode_whole(stream)
    assert ret == OK and np.array_equal(full, x)
    lnn, wav = tmp_path / "a.lnn", tmp_path / "a.wav"
    lnn.write_bytes(stream)
    r = subprocess.run([REF_CLI, "-d", str(lnn), str(wav)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    data = wav_data(wav)
    assert data == pcm_bytes(full, bits, 0, x.shape[1])
    assert expected_digest(full, bits, 0, x.shape[1], 0) == [(zlib.crc32(data), len(data))]


def test_the_piecewise_identity():
    rng = np.random.default_rng(83)
    for trial in range(40):
        n = int(rng.integers(1, 400))
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        cuts = sorted({0, n} | {int(c) for c in rng.integers(0, n + 1, int(rng.integers(0, 8)))})
        pieces = [(a, data[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        rng.shuffle(pieces)
        assert fold(pieces, n) == zlib.crc32(data), trial
    # w == 1: a run of 0x80 bytes is hashed like any other; w >= 2: zero bytes have raw() == 0 and their pieces may be left out
    data = b"\x80" * 300 + b"abc" + b"\x80" * 17
    assert fold([(303, data[303:]), (0, data[:300]), (300, b"abc")], len(data)) == zlib.crc32(data)
    assert raw(bytes(64)) == 0
    data = b"xy" + bytes(500) + b"z" + bytes(40)
    assert fold([(502, b"z"), (0, b"xy")], len(data)) == zlib.crc32(data)
    assert fold([], 1000) == zlib.crc32(bytes(1000)) and fold([], 0) == zlib.crc32(b"") == 0
    # the constants: x^0 is the product's identity, x^8 one byte's shift
    assert gf_mul(ONE, 0x12345678) == 0x12345678 and xpow8(1) == X8 and xpow8(0) == ONE
    assert raw(b"\x01" + bytes(3)) == gf_mul(raw(b"\x01"), xpow8(3))


@pytest.mark.parametrize("F,n,lead", [(1, 700, 0), (2, 700, 100), (4, 1030, 255), (6, 600, 1), (32, 300, 44)])
def test_the_kernels_algebra(F, n, lead):
    """lnn_k_digest.h restated (kernel_digest): lane terms, (piece, bucket) words taken to the bucket's end, slots, the commit --
    for frames of F bytes, pieces in shuffled order, buckets that straddle the pieces, with and without skipping zero frames"""
    rng = np.random.default_rng(F * 1000 + n)
    x = rng.integers(0, 256, (n, F), dtype=np.uint8)
    x[n // 3:n // 2] = 0                                         # a silent stretch
    frames = [bytes(r) for r in x]
    for b in (0, 1, 7, 255, 256, 257, 441, n - 1, n, n + 5):
        want = [(zlib.crc32(b"".join(frames[at:at + (b if 0 < b < n else n)])), F * min(b if 0 < b < n else n, n - at)) for at in range(0, n, b if 0 < b < n else n)]
        assert kernel_digest(frames, b, lead, rng) == want, b
        assert kernel_digest(frames, b, lead, rng, ns=4, skip_zero=F > 1) == want, b


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_cli_usage_and_option_errors(oracle, tmp_path):
    text = run("-h").stdout
    assert re.search(r"-D, --digest\b", text) and "-D [BUCKET_SAMPLES] STREAM.lnn" in text
    for args in (("-D",), ("-D", "-e", "a", "b"), ("-D", "-d", "a"), ("-D", "-C", "a", "b"), ("-D", "-r", "a", "b"), ("-D", "-V", "a"), ("-D", "-M", "a"),
                 ("--digest", "1", "a", "b"), ("-D", "--batch", "d", "a"), ("-D", "x", "a.lnn"), ("-D", "0", "a.lnn"), ("-D", "12x", "a.lnn"), ("-D", "-5", "a.lnn")):
        r = run(*args)
        assert r.returncode == 1 and r.stderr.strip() and not r.stdout, args
    assert "bucket sample count is out of range" in run("-D", "x", "a.lnn").stderr
    r = run("-D", "/nonexistent/a.lnn")
    assert r.returncode == 1 and "Failed to open" in r.stderr
    r = run("--digest", "100", "/nonexistent/a.lnn")
    assert r.returncode == 1 and "Failed to open" in r.stderr
    # a file that is no stream is refused before a device is asked for; a stream either answers or fails with a message
    junk, lnn = tmp_path / "junk.lnn", tmp_path / "a.lnn"
    junk.write_bytes(b"RIFF" + bytes(100))
    r = run("-D", str(junk))
    assert r.returncode == 1 and "Failed to get header information" in r.stderr
    x = np.concatenate([np.zeros((2, 1000), dtype=np.int32), music(2, 1500, 16, seed=3)], axis=1)
    lnn.write_bytes(bytes(oracle.encode_whole(x, 16, 22050, 500, 4, True)))
    r = run("-D", "1000", str(lnn))
    assert r.returncode in (0, 1), (r.returncode, r.stderr)      # (a signal would be negative)
    if r.returncode == 1:
        assert "Failed to create a device context" in r.stderr, r.stderr
