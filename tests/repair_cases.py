"""What the repair tests share (tests/test_repair_cpu.py, tests/test_gpu_repair.py, tests/golden/make_repair_golden.py): the table of
damaged streams and a numpy restatement of LINNEAmd_RepairStreamsDevice's contract (include/linne_amd.h, rules 2 to 6) that walks a
stream's bytes serially, as the contract reads."""
import numpy as np

import splice_cases as sc
from signals import music

HEADER = sc.HEADER
OK, INVALID_ARGUMENT, INSUFFICIENT_BUFFER = sc.OK, sc.INVALID_ARGUMENT, sc.INSUFFICIENT_BUFFER
FILL_BYTES = 11
PRESET_LAYERS = {0: (2, 32), 1: (2, 32), 2: (4, 64, 8), 3: (4, 64, 8), 4: (4, 64, 8), 5: (4, 128, 16), 6: (4, 128, 16), 7: (4, 128, 16)}
MAGIC = None                                                    # the four bytes every stream of the table begins with (set by the first source)

# ---- CRC-16/ARC (reflected 0xA001, initial value 0), the block checksum ----
_CRC = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0xA001 if _c & 1 else _c >> 1
    _CRC.append(_c)
_crc_cache = {}


def crc16(data):
    data = bytes(data)
    if data not in _crc_cache:
        c = 0
        for b in data:
            c = (c >> 8) ^ _CRC[(c ^ b) & 0xFF]
        _crc_cache[data] = c
    return _crc_cache[data]


def silent_block(n):
    body = bytes([1]) + int(n).to_bytes(2, "big")
    return b"\xff\xff" + (5).to_bytes(4, "big") + crc16(body).to_bytes(2, "big") + body


def raw_block(payload, n):
    """a RAW block of n samples with the given payload bytes (bits * n * C / 8 of them)"""
    body = bytes([2]) + int(n).to_bytes(2, "big") + bytes(payload)
    return b"\xff\xff" + (len(payload) + 5).to_bytes(4, "big") + crc16(body).to_bytes(2, "big") + body


# ---- the restatement ----
def block_bound(C, S, bits, preset):
    """B of rule 2"""
    layers = PRESET_LAYERS[preset]
    per_channel = 2 * (bits + 5) + 7 * len(layers) + 32 * sum(layers) + 15 + 36 * S
    return 11 + (C * per_channel + 7) // 8


def sound(b, p, h, B):
    """rule 2 at byte p -> (size field, samples) or None"""
    left = len(b) - p
    if left < 11 or b[p:p + 2] != b"\xff\xff":
        return None
    size = int.from_bytes(b[p + 2:p + 6], "big")
    if size + 6 > left or size < 5 or size + 6 > B:
        return None
    if crc16(b[p + 8:p + 6 + size]) != int.from_bytes(b[p + 6:p + 8], "big"):
        return None
    typ, n = b[p + 8], int.from_bytes(b[p + 9:p + 11], "big")
    if typ > 2 or n < 1 or n > h["num_samples_per_block"]:
        return None
    if typ == sc.RAW and (h["bits_per_sample"] not in (8, 16, 24) or 11 + h["bits_per_sample"] * n * h["num_channels"] // 8 != size + 6):
        return None
    if typ == sc.SILENT and size != 5:
        return None
    return size, n


def salvage_chain(b, h):
    """rule 3 -> [(offset, size field, samples)] of the kept blocks"""
    B = block_bound(h["num_channels"], h["num_samples_per_block"], h["bits_per_sample"], h["preset"])
    kept, samples, at = [], 0, HEADER
    while True:
        p = b.find(b"\xff\xff", at)
        hit = None
        while p >= 0:
            hit = sound(b, p, h, B)
            if hit:
                break
            p = b.find(b"\xff\xff", p + 1)
        if not hit or samples + hit[1] > h["num_samples"]:
            return kept
        kept.append((p, hit[0], hit[1]))
        samples += hit[1]
        at = p + hit[0] + 6


def plan(kept, N, S, stream_bytes):
    """rules 4 and 5 from the kept blocks -> (gaps, exact, layout): gaps = dicts of first_sample, num_samples, src_offset, src_bytes,
    fill_blocks; layout = the output in order, ("src", lo, hi) bytes of the source or ("fill", samples)"""
    gaps, layout, at = [], [("src", 0, HEADER)], HEADER
    for off, size, n in kept:
        if off != at:
            gaps.append({"src_offset": at, "src_bytes": off - at})
            layout.append(("gap", len(gaps) - 1))
        layout.append(("src", off, off + size + 6))
        at = off + size + 6
    have = sum(n for _, _, n in kept)
    if have < N and (stream_bytes > at or not gaps):
        gaps.append({"src_offset": at, "src_bytes": stream_bytes - at})
        layout.append(("gap", len(gaps) - 1))
    M, total = N - have, sum(g["src_bytes"] for g in gaps)
    for g in gaps:
        g["num_samples"] = M * g["src_bytes"] // total if total and len(gaps) > 1 else 0
    if gaps:
        gaps[-1]["num_samples"] = M - sum(g["num_samples"] for g in gaps[:-1])
    F, sample, out = min(S, 65535), 0, []
    blocks = {off: n for off, _, n in kept}
    for item in layout:
        if item[0] == "gap":
            g = gaps[item[1]]
            g["first_sample"], g["fill_blocks"] = sample, -(-g["num_samples"] // F)
            sample += g["num_samples"]
            if g["num_samples"]:
                out.append(("fill", g["num_samples"]))
        else:
            out.append(item)
            sample += blocks.get(item[1], 0)
    return gaps, 1 if len(gaps) <= 1 else 0, out


def repair(data, capacity=1 << 40):
    """the contract on a stream's bytes -> None for a header this table damages (case n), else (output bytes or None, report)"""
    b = bytes(data)
    if len(b) < HEADER or b[:4] != MAGIC:
        return None
    h = sc.header_fields(b)
    kept = salvage_chain(b, h)
    gaps, exact, layout = plan(kept, h["num_samples"], h["num_samples_per_block"], len(b))
    F, out = min(h["num_samples_per_block"], 65535), []
    for item in layout:
        if item[0] == "src":
            out.append(b[item[1]:item[2]])
        else:
            g = item[1]
            out += [silent_block(min(F, g - k)) for k in range(0, g, F)]
    out = b"".join(out)
    report = {"out_bytes": len(out), "result": OK, "kept_blocks": len(kept), "fill_blocks": sum(g["fill_blocks"] for g in gaps), "num_gaps": len(gaps),
              "lost_samples": h["num_samples"] - sum(n for _, _, n in kept), "exact": exact,
              "gaps": [{k: g[k] for k in ("first_sample", "num_samples", "src_offset", "src_bytes", "fill_blocks")} for g in gaps]}
    if len(out) > capacity or len(out) > 2 ** 32 - 1:
        report.update(result=INSUFFICIENT_BUFFER, kept_blocks=0, fill_blocks=0, num_gaps=0, lost_samples=0, exact=0, gaps=[])
        return None, report
    return out, report


# ---- the sources and the damage ----
SAMPLES, BLOCK = 12000, 1024                                    # eleven full blocks and a tail of 736 samples
SOURCES = {"mono/m0": (1, 0, False), "mono/m7": (1, 7, False), "stereo/m0/ms": (2, 0, True), "stereo/m7/ms": (2, 7, True), "stereo/m7/lr": (2, 7, False)}


def source_pcm(name):
    nch, preset, ms = SOURCES[name]
    return music(nch, SAMPLES, 16, seed=300 + 10 * nch + preset + int(ms))


def _flip(b, at, mask=0x10):
    b = bytearray(b)
    b[at] ^= mask
    return bytes(b)


def damage(clean):
    """cases a to k and n of a clean stream of twelve blocks -> {case: bytes}"""
    off, first, size, typ, nsmp = sc.blocks_of(clean)
    assert len(off) == 12 and nsmp == [BLOCK] * 11 + [SAMPLES - 11 * BLOCK]
    hurt = lambda b, r: _flip(b, off[r] + 11 + (size[r] - 5) // 2)         # one payload byte of block r
    junk = bytearray(np.random.default_rng(57).integers(0, 255, size=57, dtype=np.uint8).tobytes())       # (no 0xFF among them)
    junk[20:26] = b"\xff\xff" + (20).to_bytes(4, "big")
    both = lambda b, r, s: hurt(hurt(b, r), s)
    return {
        "a": clean,
        "b": hurt(clean, 5),
        "c/huge": clean[:off[5] + 2] + (0x7FFFFFF0).to_bytes(4, "big") + clean[off[5] + 6:],
        "c/7": clean[:off[5] + 2] + (7).to_bytes(4, "big") + clean[off[5] + 6:],
        "d": clean[:off[5]] + b"\x00\x00" + clean[off[5] + 2:],
        "e": clean[:off[5] + 50] + clean[off[5] + 150:],
        "f": clean[:off[5]] + bytes(junk) + clean[off[5]:],
        "g/middle": clean[:off[9] + size[9] // 2],
        "g/boundary": clean[:off[10]],
        "h": hurt(clean, 0),
        "i": hurt(clean, 11),
        "j": both(clean, 5, 6),
        "k": both(clean, 3, 8),
        "n": _flip(clean, 0, 0xFF),
    }


def embedded(clean, broken):
    """case m: block 5 of a clean 16-bit stream replaced by a RAW block of its length whose payload holds a sound SILENT block of 100
    samples; broken: the RAW block's CRC does not match (the embedded block is then kept: the documented limit)"""
    off, first, size, typ, nsmp = sc.blocks_of(clean)
    C = sc.header_fields(clean)["num_channels"]
    payload = bytearray(np.random.default_rng(13).integers(0, 255, size=2 * nsmp[5] * C, dtype=np.uint8).tobytes())
    payload[100:111] = silent_block(100)
    block = raw_block(payload, nsmp[5])
    if broken:
        block = _flip(block, 11 + 500)
    return clean[:off[5]] + block + clean[off[6]:]


def build_cases(encoder):
    """name -> (damaged bytes, clean bytes or None): every source encoded by `encoder` (the oracle, or the reference), every damage"""
    global MAGIC
    cases = {}
    for name in SOURCES:
        nch, preset, ms = SOURCES[name]
        clean = bytes(encoder.encode_whole(source_pcm(name), 16, 44100, BLOCK, preset, ms))
        MAGIC = clean[:4]
        for case, b in damage(clean).items():
            cases[f"{name}/{case}"] = (b, clean)
    for preset in sc.PREMISE_PRESETS:                           # the trim stream of the splice tests: blocks 548 / 1024 / 1024 / 1024 / 880
        trim, _ = sc.splice_with(encoder, sc.premise_cases(preset)[f"trim/m{preset}"], preset)
        off, first, size, typ, nsmp = sc.blocks_of(trim)
        assert nsmp == [548, 1024, 1024, 1024, 880]
        cases[f"trim/m{preset}/a"] = (bytes(trim), bytes(trim))
        cases[f"trim/m{preset}/l"] = (_flip(trim, off[0] + 11 + (size[0] - 5) // 2), bytes(trim))
    clean = cases["mono/m0/a"][0]
    cases["mono/m0/m/intact"] = (embedded(clean, False), None)
    cases["mono/m0/m/broken"] = (embedded(clean, True), None)
    return cases


def expected_pcm(decoder, data, repaired):
    """the samples the repaired stream must decode to, block by block: every kept block decoded alone (a stream of its header and the
    block), zeros for every fill"""
    h = sc.header_fields(data)
    gaps, _, layout = plan(salvage_chain(bytes(data), h), h["num_samples"], h["num_samples_per_block"], len(data))
    parts = []
    for item in layout[1:]:
        if item[0] == "fill":
            parts.append(np.zeros((h["num_channels"], item[1]), np.int32))
        else:
            at = item[1]
            while at < item[2]:
                size, n = int.from_bytes(data[at + 2:at + 6], "big"), int.from_bytes(data[at + 9:at + 11], "big")
                ret, pcm = decoder.decode_whole(sc.with_num_samples(data[:HEADER], n) + bytes(data[at:at + size + 6]) + bytes(4))[:2]      # (4 bytes more: the reference's bit reader fetches words)
                assert ret == OK
                parts.append(np.stack(pcm).astype(np.int32))
                at += size + 6
    return np.concatenate(parts, axis=1) if parts else np.zeros((h["num_channels"], 0), np.int32)
