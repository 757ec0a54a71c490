"""What the synthesis-record tests share (tests/test_synth_records_cpu.py, tests/test_gpu_synth_records.py,
tests/golden/make_synth_records_golden.py): COMPRESS blocks whose parameter records NO encoder writes -- any power-of-two unit
count in every layer, any coefficient shift, any int8 coefficient, any pre-emphasis state -- which every decode path promises to
turn into the reference decoder's PCM (linne_decoder.c:430-526, linne_lpc_synthesize.c:8-83).

* write_stream: a block writer of its own, independent of the product's host packer: the oracle's Huffman code, Rice coder and
  CRC16, the bit layout of linne_encoder.c:698-735 and the stream header of splice_cases.header_fields
* table(): the deterministic case table, per stream shape a list of Case (a frame: records [C][PARAM_WORDS] int32 in the layout of
  include/linne_amd.h, residual [C][n]); families `units`, `shift`, `coef`, `growth`, `preem` (the module's FAMILIES)
* defined(): the rule that keeps the table inside what the reference decodes without undefined behaviour
* synth_plain(): the cascade restated in Python integers of unbounded width, wrapped to int32 where the reference's int32 wraps; it
  reports the widest value it met and whether anything wrapped
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from refs import PRESET_LAYERS, ChannelTap, Oracle
from splice_cases import HEADER, header_fields

PARAM_WORDS = 160
PRM_PREV, PRM_PCOEF, PRM_UNITS, PRM_RSHIFT, PRM_COEF = 0, 2, 4, 7, 10
PREEM_SHIFT = 5
RATE = 44100
SEED = 20260
FAMILIES = ("units", "shift", "coef", "growth", "preem")
RESIDUAL_LIMIT = 1 << 20

Shape = namedtuple("Shape", "name nch bits block preset ms families")
SHAPES = (
    Shape("2ch16b1024m7ms", 2, 16, 1024, 7, True, FAMILIES),
    Shape("1ch24b1023m0", 1, 24, 1023, 0, False, FAMILIES),
    Shape("2ch16b1023m4lr", 2, 16, 1023, 4, False, FAMILIES),
    Shape("3ch24b1024m4ms", 3, 24, 1024, 4, True, FAMILIES),
    Shape("8ch16b1024m7lr", 8, 16, 1024, 7, False, ("units",)),
    Shape("2ch24b1024m0ms", 2, 24, 1024, 0, True, FAMILIES),
)
Case = namedtuple("Case", "name family n record residual")

_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        _oracle = Oracle()
    return _oracle


# ---- the block writer ----
def _bits_of(value, nbits):
    """`nbits` bits of value, most significant first (BitWriter_PutBits)"""
    return np.array([(int(value) >> (nbits - 1 - i)) & 1 for i in range(nbits)], dtype=np.uint8)


def zigzag(v):
    """LINNEUTILITY_SINT32_TO_UINT32"""
    v = int(v)
    return (-2 * v - 1) if v < 0 else 2 * v


_huff = {}


def huffman_bits(sym):
    if sym not in _huff:
        code = C.c_uint32(0)
        n = oracle().L.oracle_huffman_code(sym, C.byref(code))
        _huff[sym] = _bits_of(code.value, n)
    return _huff[sym]


def write_block(record, residual, n, bits, preset):
    """one COMPRESS block of n samples per channel: record [C][PARAM_WORDS], residual [C][>= n] -> bytes (linne_encoder.c:698-735
    for the payload, :806-855 for the 11 bytes in front of it)"""
    record = np.asarray(record, dtype=np.int64)
    nch = record.shape[0]
    layers = PRESET_LAYERS[preset]
    out = []
    for ch in range(nch):
        for st in range(2):
            u = zigzag(record[ch, PRM_PREV + st])
            assert 0 <= u < 1 << (bits + 1), "pre-emphasis prev outside the field"
            assert 0 <= record[ch, PRM_PCOEF + st] < 1 << (PREEM_SHIFT - 1)
            out += [_bits_of(u, bits + 1), _bits_of(record[ch, PRM_PCOEF + st], PREEM_SHIFT - 1)]
    for ch in range(nch):
        at = PRM_COEF
        for l, P in enumerate(layers):
            units = int(record[ch, PRM_UNITS + l])
            log2 = units.bit_length() - 1
            assert units == 1 << log2 and log2 < 8 and 0 <= record[ch, PRM_RSHIFT + l] < 16
            out += [_bits_of(log2, 3), _bits_of(record[ch, PRM_RSHIFT + l], 4)]
            for c in record[ch, at:at + P]:
                assert -128 <= c <= 127
                out.append(huffman_bits(zigzag(c)))
            at += P
    for ch in range(nch):
        code, nbits = oracle().rice_encode(np.asarray(residual[ch][:n], dtype=np.int32))
        out.append(np.unpackbits(np.frombuffer(code, dtype=np.uint8))[:nbits])
    payload = np.packbits(np.concatenate(out)).tobytes()              # (packbits pads the last byte with zeros: BitStream_Flush)
    body = bytes([0]) + int(n).to_bytes(2, "big") + payload           # type COMPRESS, samples, payload: what the CRC covers
    arr = np.frombuffer(body, dtype=np.uint8)
    crc = int(oracle().L.oracle_crc16(arr.ctypes.data, len(arr)))
    return b"\xff\xff" + (len(payload) + 5).to_bytes(4, "big") + crc.to_bytes(2, "big") + body


CLOSING_SAMPLES = 1


def silent_block(n):
    """a SILENT block of n samples: its 11 bytes and no payload (linne_encoder.c:755-771)"""
    body = bytes([1]) + int(n).to_bytes(2, "big")
    arr = np.frombuffer(body, dtype=np.uint8)
    crc = int(oracle().L.oracle_crc16(arr.ctypes.data, len(arr)))
    return b"\xff\xff" + (5).to_bytes(4, "big") + crc.to_bytes(2, "big") + body


def write_stream(records, residuals, ns, nch, bits, block, preset, ms):
    """the .lnn stream of the frames records[f] [C][PARAM_WORDS], residuals[f] [C][>= ns[f]]: header, one COMPRESS block each, and
    a closing SILENT block of CLOSING_SAMPLES samples.  The closing block keeps the streams inside what the reference reads with
    defined behaviour: its bit reader fetches four bytes at a time (bit_stream.h BitReader_GetBits), up to three bytes beyond the
    end of a COMPRESS block's payload, which at the end of a stream is beyond the end of the data"""
    total = int(sum(int(n) for n in ns)) + CLOSING_SAMPLES
    head = (b"IBRA" + (1).to_bytes(4, "big") + (2).to_bytes(4, "big") + nch.to_bytes(2, "big") + total.to_bytes(4, "big") +
            RATE.to_bytes(4, "big") + bits.to_bytes(2, "big") + block.to_bytes(4, "big") + bytes([preset, int(bool(ms))]))
    assert len(head) == HEADER
    h = header_fields(head)
    assert (h["num_channels"], h["num_samples"], h["bits_per_sample"], h["num_samples_per_block"], h["preset"], h["ch_process_method"]) == \
        (nch, total, bits, block, preset, int(bool(ms)))
    return head + b"".join(write_block(records[f], residuals[f], int(ns[f]), bits, preset) for f in range(len(ns))) + silent_block(CLOSING_SAMPLES)


def case_stream(shape, cases):
    """the stream of some cases of one shape, a block each"""
    return write_stream([c.record for c in cases], [c.residual for c in cases], [c.n for c in cases],
                        shape.nch, shape.bits, shape.block, shape.preset, shape.ms)


# ---- the defined subset ----
def defined(record, n, preset):
    """True when the reference decodes a block of n samples with this record [C][PARAM_WORDS] without undefined behaviour: every
    shift >= 1 (linne_lpc_synthesize.c:13 computes 1 << (shift - 1)) and floor(n / units) >= floor(order / units) in every layer
    (the loop bound of :27, :44 and :68 is their unsigned difference)"""
    record = np.asarray(record)
    for ch in range(record.shape[0]):
        for l, P in enumerate(PRESET_LAYERS[preset]):
            units, shift = int(record[ch, PRM_UNITS + l]), int(record[ch, PRM_RSHIFT + l])
            if shift < 1 or units < 1 or n // units < P // units:
                return False
    return True


# ---- the case table ----
def lengths(block):
    return (block, block - 1, 1000, 130)


def _tame_record(rng, shape):
    """a record whose cascade stays small: one unit per layer, coefficients in [-3, 3] at shift 9, pre-emphasis of a few 32nds"""
    rec = np.zeros((shape.nch, PARAM_WORDS), dtype=np.int32)
    layers = PRESET_LAYERS[shape.preset]
    rec[:, PRM_PREV:PRM_PREV + 2] = rng.integers(-300, 301, size=(shape.nch, 2))
    rec[:, PRM_PCOEF:PRM_PCOEF + 2] = rng.integers(0, 16, size=(shape.nch, 2))
    rec[:, PRM_UNITS:PRM_UNITS + len(layers)] = 1
    rec[:, PRM_RSHIFT:PRM_RSHIFT + len(layers)] = 9
    rec[:, PRM_COEF:PRM_COEF + sum(layers)] = rng.integers(-3, 4, size=(shape.nch, sum(layers)))
    return rec


def _layer_slice(preset, l):
    layers = PRESET_LAYERS[preset]
    at = PRM_COEF + sum(layers[:l])
    return slice(at, at + layers[l])


def _residual(rng, shape, amp=200):
    return rng.integers(-amp, amp + 1, size=(shape.nch, shape.block)).astype(np.int32)


def _shape_cases(shape, rng):
    layers = PRESET_LAYERS[shape.preset]
    nl = len(layers)
    ln = lengths(shape.block)
    cases = []

    def add(name, family, n, rec, res):
        res = np.array(res, dtype=np.int32)
        res[:, n:] = 0
        assert np.abs(res.astype(np.int64)).max() <= RESIDUAL_LIMIT
        cases.append(Case(f"{shape.name}/{name}", family, int(n), rec, res))

    if "units" in shape.families:
        # every log2 unit count 0..7 in each layer in turn (the others at one unit), a different one per channel; the four frame
        # lengths go round so that every unit count meets lengths it divides and lengths it does not
        for l in range(nl):
            for k in range(8):
                rec = _tame_record(rng, shape)
                for ch in range(shape.nch):
                    rec[ch, PRM_UNITS + l] = 1 << ((k + 3 * ch) % 8)
                add(f"units/l{l}/k{k}", "units", ln[(k + l + k // 4) % 4], rec, _residual(rng, shape))
        rec = _tame_record(rng, shape)
        rec[:, PRM_UNITS:PRM_UNITS + nl] = 8
        add("units/all8", "units", ln[3], rec, _residual(rng, shape))
        # every layer at many units: the frame's last n - units * floor(n / units) samples are synthesised by no layer
        for k, n in ((7, 1000), (6, shape.block - 1), (7, 130)):
            rec = _tame_record(rng, shape)
            rec[:, PRM_UNITS:PRM_UNITS + nl] = 1 << k
            add(f"units/all{1 << k}/n{n}", "units", n, rec, _residual(rng, shape))
    if "shift" in shape.families:
        # every shift 1..15 in every layer: case s gives layer l the shift (s + 5 l) mod 15 + 1, coefficients as large as keeps
        # about half of the cases stable
        for s in range(15):
            rec = _tame_record(rng, shape)
            for l in range(nl):
                sh = (s + 5 * l) % 15 + 1
                rec[:, PRM_RSHIFT + l] = sh
                a = max(1, min(127, (1 << sh) // 64))
                rec[:, _layer_slice(shape.preset, l)] = rng.integers(-a, a + 1, size=(shape.nch, layers[l]))
                rec[:, PRM_UNITS + l] = 1 << int(rng.integers(0, 3))
            add(f"shift/s{s}", "shift", (shape.block, shape.block, ln[1], ln[2], shape.block, ln[3])[s % 6], rec, _residual(rng, shape))
    if "coef" in shape.families:
        total = sum(layers)
        alt = np.where(np.arange(total) % 2 == 0, 127, -128)
        for name, fill in (("max", np.full(total, 127)), ("min", np.full(total, -128)), ("alternating", alt)):
            rec = _tame_record(rng, shape)
            rec[:, PRM_COEF:PRM_COEF + total] = fill
            rec[0, PRM_RSHIFT:PRM_RSHIFT + nl] = 15                   # the first channel stays bounded, the others run away
            rec[1:, PRM_RSHIFT:PRM_RSHIFT + nl] = 12
            add(f"coef/{name}", "coef", shape.block, rec, _residual(rng, shape))
        # uniform over the int8 range; the slots of the two frames are first filled with every value once, as far as they go
        perm = rng.permutation(np.arange(-128, 128))
        at = 0
        for k in range(2):
            rec = _tame_record(rng, shape)
            vals = rng.integers(-128, 128, size=shape.nch * total)
            m = min(len(vals), 256 - at)
            vals[:m] = perm[at:at + m]
            at += m
            rec[:, PRM_COEF:PRM_COEF + total] = vals.reshape(shape.nch, total)
            rec[:, PRM_RSHIFT:PRM_RSHIFT + nl] = 15 if k == 0 else 13
            add(f"coef/uniform{k}", "coef", ln[k], rec, _residual(rng, shape))
    if "growth" in shape.families:
        # (a) one pole near 1 per layer 0, large residuals of one sign: samples beyond 2^24 without a wrap in the first channel;
        # (b) the same pole in every layer: the cascade's gain takes it past 2^31; (c) all +127 at shift 1; (d) random int8 at shift 3
        big = rng.integers(RESIDUAL_LIMIT // 2, RESIDUAL_LIMIT + 1, size=(shape.nch, shape.block))
        for name in ("pole", "poles", "max_shift1", "uniform_shift3"):
            rec = _tame_record(rng, shape)
            rec[:, PRM_COEF:PRM_COEF + sum(layers)] = 0
            if name in ("pole", "poles"):
                for l in range(nl if name == "poles" else 1):
                    sl = _layer_slice(shape.preset, l)
                    rec[:, sl.stop - 1] = -31                         # y[s] = x[s] + (31 y[s - 1] - 16 >> 5): 32 x in the end,
                    rec[:, PRM_RSHIFT + l] = 5                        # and 31 y stays inside int32 while y < 2^26
                rec[:, PRM_PCOEF:PRM_PCOEF + 2] = 3
                res = big
            elif name == "max_shift1":
                rec[:, PRM_COEF:PRM_COEF + sum(layers)] = 127
                rec[:, PRM_RSHIFT:PRM_RSHIFT + nl] = 1
                res = _residual(rng, shape, 50)
            else:
                rec[:, PRM_COEF:PRM_COEF + sum(layers)] = rng.integers(-128, 128, size=(shape.nch, sum(layers)))
                rec[:, PRM_RSHIFT:PRM_RSHIFT + nl] = 3
                rec[:, PRM_UNITS:PRM_UNITS + nl] = 4
                res = _residual(rng, shape, 50)
            add(f"growth/{name}", "growth", 1000 if name == "uniform_shift3" else shape.block, rec, res)
    if "preem" in shape.families:
        # each stage's coefficient 0..15 (over the channels of 8 cases, or the 16 cases of a mono shape), prev at both ends of the
        # (bits + 1)-bit zig-zag range
        lo, hi = -(1 << shape.bits), (1 << shape.bits) - 1
        ncase = 16 if shape.nch == 1 else 8
        for i in range(ncase):
            rec = _tame_record(rng, shape)
            for ch in range(shape.nch):
                c0 = (i + 8 * ch) % 16
                rec[ch, PRM_PCOEF], rec[ch, PRM_PCOEF + 1] = c0, (18 - c0) % 16
                rec[ch, PRM_PREV], rec[ch, PRM_PREV + 1] = ((lo, hi), (hi, lo), (hi, hi), (lo, lo))[(i + ch) % 4]
            add(f"preem/c{i}", "preem", (shape.block, ln[1], shape.block, ln[3])[i % 4], rec, _residual(rng, shape))
    for c in cases:
        assert defined(c.record, c.n, shape.preset), f"{c.name} lies outside the defined subset"
    assert len(cases) <= 64
    return cases


_table = None


def table():
    """{Shape: [Case, ...]}, the same on every call and in every process"""
    global _table
    if _table is None:
        _table = {shape: _shape_cases(shape, np.random.default_rng([SEED, i])) for i, shape in enumerate(SHAPES)}
    return _table


def case_offsets(cases):
    """the first sample of every case's block in case_stream, one longer (the closing SILENT block starts at the last entry)"""
    return np.concatenate([[0], np.cumsum([c.n for c in cases])]).astype(np.int64)


def symbols(shape, cases):
    """the set of Huffman symbols (0..255) the cases' coefficients are written with"""
    total = sum(PRESET_LAYERS[shape.preset])
    seen = set()
    for c in cases:
        seen.update(zigzag(v) for v in c.record[:, PRM_COEF:PRM_COEF + total].reshape(-1))
    return seen


# ---- the oracle's synthesis of a record ----
def taps_of(record, preset):
    """[ChannelTap] of a record [C][PARAM_WORDS]: what oracle.decode_hotpath takes"""
    taps = []
    for row in np.asarray(record):
        t = ChannelTap()
        for st in range(2):
            t.preem_prev[st], t.preem_coef[st] = int(row[PRM_PREV + st]), int(row[PRM_PCOEF + st])
        at = PRM_COEF
        for l, P in enumerate(PRESET_LAYERS[preset]):
            t.num_units[l], t.rshift[l] = int(row[PRM_UNITS + l]), int(row[PRM_RSHIFT + l])
            for i in range(P):
                t.coef[l][i] = int(row[at + i])
            at += P
        taps.append(t)
    return taps


def expected_pcm(shape, case):
    """[C][n]: the oracle's synthesis of the case's residual under its record"""
    return oracle().decode_hotpath(taps_of(case.record, shape.preset), case.residual[:, :case.n], shape.bits, shape.block, shape.preset, shape.ms)


# ---- the cascade in unbounded integers ----
def _wrap(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def synth_plain(shape, case):
    """linne_decoder.c:503-522 on the case in Python integers: every product, sum and difference is formed exactly and then wrapped
    to int32 as the reference's int32 arithmetic does -> (pcm [C][n], largest |exact value| met, True if a wrap changed a value).
    The layers' tails (the samples behind units * floor(n / units)) are left as they are, as linne_lpc_synthesize.c leaves them"""
    n = case.n
    peak, wrapped = 0, False
    out = []

    def w(v):
        nonlocal peak, wrapped
        peak = max(peak, abs(v))
        r = _wrap(v)
        wrapped = wrapped or r != v
        return r

    for ch in range(shape.nch):
        d = [int(v) for v in case.residual[ch, :n]]
        row = case.record[ch]
        for l in reversed(range(len(PRESET_LAYERS[shape.preset]))):
            P = PRESET_LAYERS[shape.preset][l]
            sl = _layer_slice(shape.preset, l)
            coef = [int(v) for v in row[sl]]
            units, shift = int(row[PRM_UNITS + l]), int(row[PRM_RSHIFT + l])
            npar, nsm = P // units, n // units
            half = 1 << (shift - 1)
            for u in range(units):
                c = coef[u * npar:(u + 1) * npar]
                base = u * nsm
                for s in range(nsm - npar):
                    pred = half
                    for k in range(npar):
                        if c[k]:
                            pred = w(pred + w(c[k] * d[base + s + k]))
                    d[base + s + npar] = w(d[base + s + npar] - (pred >> shift))
        for st in range(2):                                          # LINNEPreemphasisFilter_MultiStageDeemphasis: stage 1 first, then stage 0
            stage = 1 - st
            prev, coef = int(row[PRM_PREV + stage]), int(row[PRM_PCOEF + stage])
            for s in range(n):
                d[s] = w(d[s] + (w(prev * coef) >> PREEM_SHIFT))
                prev = d[s]
        out.append(d)
    if shape.ms:
        for s in range(n):                                           # LINNEUtility_LRConversion
            out[0][s] = w(out[0][s] - (out[1][s] >> 1))
            out[1][s] = w(out[1][s] + out[0][s])
    return np.array(out, dtype=np.int64).astype(np.int32), peak, wrapped
