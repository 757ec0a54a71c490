"""What the stream index tests share (tests/test_stream_index_walk_cpu.py, tests/test_gpu_stream_index_batch.py): the corpus of whole,
cut and damaged streams, and a plain-Python statement of what the index of a stream's bytes is -- the header as
LINNEDecoder_DecodeHeader and LINNEDecoder_SetHeader take it, then the blocks one after the other from byte 30 on under the checks of
the block parser (lnn_parse_block_head), as LINNEDecoder_DecodeWhole walks them.  It reads bytes serially and shares nothing with the
device code: no candidates, no chains, no tables."""
import numpy as np

from splice_cases import COMPRESS, HEADER, RAW, SILENT, header_fields
from stream_refs import blocks, crc16, mixed_signal
from test_gpu_stream_windows import SHAPES

OK, INVALID_ARGUMENT, INVALID_FORMAT, INSUFFICIENT_BUFFER, INSUFFICIENT_DATA, PARAMETER_NOT_SET, CORRUPTION, NG = range(8)
SILENT_BLOCKS = 1000


class Case:
    """one stream of the corpus: its bytes (None: a NULL pointer), whether an encoder wrote it as it is, and the yardsticks"""

    def __init__(self, name, data, well_formed=False):
        self.name, self.data, self.well_formed = name, data, well_formed


def build_corpus(product):
    from test_gpu_parity import many_block_lengths, stream_of_blocks
    cases = []
    base = []
    for k in (0, 1, 3, 4, 5):                                       # five shapes at reduced length
        nch, bits, block, preset, ms, _, seed = SHAPES[k]
        ns = max(7 * block + 1000, 20000) + 37 * k
        assert 20000 <= ns <= 60000
        x = mixed_signal(nch, bits, ns, seed=seed, block=block)
        s = product.encode_whole(x, bits, 44100, block, preset, ms)
        base.append(s)
        cases.append(Case(f"{nch}ch {bits}b {block} -m{preset}", s, True))
    x, lens = many_block_lengths()
    cases.append(Case("variable block lengths", stream_of_blocks(product, np.array(x, dtype=np.int32), 16, 44100, 4096, 7, True, lens), True))
    # 1000 SILENT blocks of 11 bytes: heads at every residue of the 4096-position waves; the stream with the most candidates
    silent = product.encode_whole(np.zeros((1, SILENT_BLOCKS * 256), dtype=np.int32), 16, 44100, 256, 0, False)
    assert len(silent) == 30 + 11 * SILENT_BLOCKS
    cases.append(Case("1000 silent blocks", silent, True))
    s = base[1]                                                     # stereo 16-bit: the stream the damaged ones derive from
    bl = blocks(s)
    assert len(s) > 30 + 2 * 4096 + 11 and len(bl) >= 7
    cases.append(Case("cut to the header", s[:30]))
    for d in range(1, 12):
        cases.append(Case(f"cut to 30 + {d}", s[:30 + d]))
    for k in (1, 2):
        for d in (-1, 0, 1, 10, 11):
            cases.append(Case(f"cut to 30 + 4096 * {k} + {d}", s[:30 + 4096 * k + d]))
    mid = len(bl) // 2
    cases.append(Case("cut inside a block", s[:bl[mid][0] + bl[mid][1] // 2]))
    cases.append(Case("trailing bytes", s + bytes(range(1, 18))))
    for name, k in (("first", 0), ("middle", mid), ("last", len(bl) - 1)):
        bad = bytearray(s)
        bad[bl[k][0] + bl[k][1] - 2] ^= 0x10
        cases.append(Case(f"CRC damage in the {name} block", bytes(bad)))
    off = bl[mid][0]
    for name, field in (("beyond the stream", (len(s)).to_bytes(4, "big")), ("below 5", (3).to_bytes(4, "big")),
                        ("one less", (bl[mid][1] - 7).to_bytes(4, "big"))):
        bad = bytearray(s)
        bad[off + 2:off + 6] = field
        cases.append(Case(f"size field {name}", bytes(bad)))
    bad = bytearray(s)
    bad[off] = 0x7F
    cases.append(Case("sync word damaged", bytes(bad)))
    # a false candidate: FF FF and a size inside a RAW payload, such that its "next block" is the real next block; CRC repaired
    k = next(i for i, b in enumerate(bl[:-1]) if b[2] == RAW)
    off, size = bl[k][:2]
    p = off + 11 + 100
    bad = bytearray(s)
    bad[p:p + 2] = b"\xff\xff"
    bad[p + 2:p + 6] = (bl[k + 1][0] - p - 6).to_bytes(4, "big")
    bad[off + 6:off + 8] = crc16(bad[off + 8:off + size]).to_bytes(2, "big")
    cases.append(Case("false candidate in a RAW payload", bytes(bad), True))
    # adjacency: a stream that ends FF FF 00 00 00, and directly behind it the bytes that would complete the block head
    sb = blocks(silent)
    cut = sb[500][0] + 5
    assert silent[cut - 5:cut] == b"\xff\xff\x00\x00\x00" and silent[cut] == 5
    cases.append(Case("silent cut inside a block head", silent[:cut]))
    cases.append(Case("the rest of that block head (no signature)", silent[cut:]))
    cases.append(Case("fewer than 30 bytes", s[:29]))
    bad = bytearray(s); bad[0] ^= 0xFF
    cases.append(Case("bad signature", bytes(bad)))
    bad = bytearray(s); bad[7] = 2
    cases.append(Case("bad format version", bytes(bad)))
    cases.append(Case("NULL pointer", None))
    cases.append(Case("the first stream again", base[0], True))
    return cases


# ---- the walk ----
_CRC = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0xA001 if _c & 1 else _c >> 1
    _CRC.append(_c)


def _crc16(data):
    """CRC-16/ARC (reflected 0xA001, initial value 0, no final XOR), by its byte table"""
    c = 0
    for b in data:
        c = (c >> 8) ^ _CRC[(c ^ b) & 0xFF]
    return c


def header_code(data):
    """what LINNEDecoder_DecodeHeader, then LINNEDecoder_SetHeader on a decoder with room for 8 channels, say of a stream's first
    bytes: the code DecodeWhole returns before it looks at a block"""
    b = bytes(data)
    if len(b) < HEADER:
        return INSUFFICIENT_DATA
    if b[:4] != b"IBRA":
        return INVALID_FORMAT
    h = header_fields(b)
    if h["format_version"] != 1 or h["codec_version"] != 2:
        return INVALID_FORMAT
    if 0 in (h["num_channels"], h["num_samples"], h["sampling_rate"], h["bits_per_sample"], h["num_samples_per_block"]):
        return INVALID_FORMAT
    if h["preset"] >= 8 or h["ch_process_method"] >= 2 or (h["ch_process_method"] == 1 and h["num_channels"] == 1):
        return INVALID_FORMAT
    if h["num_channels"] > 8:
        return INSUFFICIENT_BUFFER
    return OK


def block_code(b, at, h, first):
    """the block parser on the block at byte `at` whose first sample is `first` -> (code, in the chain, size field, type, samples):
    the four checks before the CRC decide whether there is a block at all (none: the last three are None), the CRC and the checks
    behind it, in the parser's order, whether it is a sound one"""
    left = len(b) - at
    if left < 11:
        return INSUFFICIENT_DATA, False, None, None, None
    if b[at:at + 2] != b"\xff\xff":
        return INVALID_FORMAT, False, None, None, None
    size = int.from_bytes(b[at + 2:at + 6], "big")
    if size + 6 > left:
        return INSUFFICIENT_DATA, False, None, None, None
    if size < 5:
        return INVALID_FORMAT, False, None, None, None
    typ, n = b[at + 8], int.from_bytes(b[at + 9:at + 11], "big")
    C, S, bits = h["num_channels"], h["num_samples_per_block"], h["bits_per_sample"]
    code = OK
    if _crc16(b[at + 8:at + 6 + size]) != int.from_bytes(b[at + 6:at + 8], "big"):
        code = CORRUPTION
    elif n > h["num_samples"] - first or n > S:
        code = INSUFFICIENT_BUFFER
    elif typ == RAW:
        payload = bits * n * C // 8
        if bits not in (8, 16, 24):
            code = INVALID_FORMAT
        elif left - 11 < payload:
            code = INSUFFICIENT_DATA
        elif 11 + payload != size + 6:                              # (a payload other than the size field says: no encoder writes it)
            code = NG
    elif typ == SILENT:
        if size != 5:
            code = NG
    elif typ == COMPRESS:
        if n == 0:
            code = INVALID_FORMAT
    else:
        code = INVALID_FORMAT
    return code, True, size, typ, n


def index_walk(data):
    """the index of a stream's bytes -> (code, header, num_blocks, (off, first, size, type, nsmp), (block, code, byte)).  A header
    error is the code, everything else None.  Otherwise code is OK; the blocks are those a whole decode walks (size fields trusted
    from one to the next, until the samples reach the header's count or the stream ends), `first` one entry longer; the failure is
    the lowest failing block's, or the place's behind the last block when no block head stands there and the stream goes on, or
    (-1, OK, 0)"""
    code = header_code(data)
    if code != OK:
        return code, None, None, None, None
    b = bytes(data)
    h = header_fields(b)
    off, first, size, typ, nsmp = [], [0], [], [], []
    failure = (-1, OK, 0)
    at = HEADER
    while first[-1] < h["num_samples"] and at < len(b):
        c, chained, sz, t, n = block_code(b, at, h, first[-1])
        if c != OK and failure[0] < 0:
            failure = (len(off), c, at)
        if not chained:
            break
        off.append(at); size.append(sz); typ.append(t); nsmp.append(n)
        first.append(first[-1] + n)
        at += sz + 6
    return OK, h, len(off), (off, first, size, typ, nsmp), failure


def host_corpus(product):
    """streams of SILENT and RAW blocks only, written here byte by byte (LINNEDecoder_DecodeWhole decodes them on the host alone), whole
    and damaged -> [(name, bytes)]"""
    import ctypes as C
    from refs import _RefHeader
    from repair_cases import raw_block, silent_block
    rng = np.random.default_rng(77)
    nch, bits, S = 2, 16, 300
    lens = [S, S, 17, S, 1, S, 299, S, S, 150]
    body, kinds = [], []
    for i, n in enumerate(lens):
        if i % 3 == 1:
            body.append(silent_block(n)); kinds.append(SILENT)
        else:
            body.append(raw_block(rng.integers(0, 256, size=2 * nch * n, dtype=np.uint8).tobytes(), n)); kinds.append(RAW)
    hdr = _RefHeader(1, 2, nch, sum(lens), 44100, bits, S, 0, 0)
    out = np.zeros(HEADER, dtype=np.uint8)
    assert product.L.LINNEEncoder_EncodeHeader(C.byref(hdr), out.ctypes.data, out.size) == 0
    s = out.tobytes() + b"".join(body)
    starts = [HEADER + sum(len(x) for x in body[:i]) for i in range(len(body))]
    flip = lambda at, mask=0x10: s[:at] + bytes([s[at] ^ mask]) + s[at + 1:]
    field = lambda at, v, k=4: s[:at] + int(v).to_bytes(k, "big") + s[at + k:]
    cases = [("whole", s), ("cut to the header", s[:HEADER]), ("trailing bytes", s + bytes(range(1, 18))),
             ("cut inside a block", s[:starts[5] + 40]), ("cut at a block", s[:starts[5]]), ("cut inside a head", s[:starts[4] + 7]),
             ("CRC damage in the first block", flip(starts[0] + 20)), ("CRC damage in the last block", flip(len(s) - 3)),
             ("two damaged blocks", flip(starts[6] + 30)[:starts[2] + 12] + b"\x55" + flip(starts[6] + 30)[starts[2] + 13:]),
             ("sync word damaged", flip(starts[3], 0x80)), ("size field below 5", field(starts[3] + 2, 4)),
             ("size field beyond the stream", field(starts[3] + 2, len(s))), ("size field one less", field(starts[3] + 2, len(body[3]) - 7)),
             ("fewer than 30 bytes", s[:29]), ("bad signature", flip(0, 0xFF)), ("bad format version", field(4, 2)),
             ("bad codec version", field(8, 3)), ("no channels", field(12, 0, 2)), ("nine channels", field(12, 9, 2)),
             ("preset 8", field(28, 8, 1)), ("more samples than the blocks hold", field(14, sum(lens) + 5))]
    # a block of more samples than the header's block size, and one of an unknown type, each with its CRC made right.  (Not here: a
    # CRC-valid RAW or SILENT block whose payload is not what its size field says.  No encoder writes one, the index calls it NG, and
    # DecodeWhole is documented to differ on it: include/linne_amd.h, LINNEAmd_DecodeStreamDevice.)
    for name, at, v, k in (("too many samples in a block", starts[1] + 9, S + 1, 2), ("unknown block type", starts[1] + 8, 3, 1)):
        bad = bytearray(field(at, v, k))
        p, sz = starts[1], int.from_bytes(s[starts[1] + 2:starts[1] + 6], "big")
        bad[p + 6:p + 8] = _crc16(bad[p + 8:p + 6 + sz]).to_bytes(2, "big")
        cases.append((name, bytes(bad)))
    return cases
