"""What the splice tests share (tests/test_splice_cpu.py, tests/test_gpu_splice.py, tests/golden/make_splice_golden.py): a numpy
restatement of LINNEAmd_SpliceStreamsDevice's stream contract (include/linne_amd.h) -- the blocks of a stream read from its bytes, the
pieces a list of cuts is made of, the spliced stream assembled from source bytes and an encoder's fragment blocks -- and the inputs
of the recorded premise cases."""
import numpy as np

from signals import music

HEADER = 30
COMPRESS, SILENT, RAW = 0, 1, 2
OK, INVALID_ARGUMENT, INVALID_FORMAT, INSUFFICIENT_BUFFER, INSUFFICIENT_DATA, PARAMETER_NOT_SET, CORRUPTION, NG = range(8)
SHAPE_FIELDS = ("num_channels", "sampling_rate", "bits_per_sample", "num_samples_per_block", "preset", "ch_process_method")


def header_fields(stream):
    """the fields of the 30-byte stream header (big-endian; linne_encoder.c LINNEEncoder_EncodeHeader)"""
    b = bytes(stream[:HEADER])
    be = lambda lo, hi: int.from_bytes(b[lo:hi], "big")
    return {"format_version": be(4, 8), "codec_version": be(8, 12), "num_channels": be(12, 14), "num_samples": be(14, 18),
            "sampling_rate": be(18, 22), "bits_per_sample": be(22, 24), "num_samples_per_block": be(24, 28), "preset": be(28, 29),
            "ch_process_method": be(29, 30)}


def with_num_samples(header_bytes, n):
    """the same header with another sample count"""
    b = bytearray(header_bytes[:HEADER])
    b[14:18] = int(n).to_bytes(4, "big")
    return bytes(b)


def blocks_of(stream):
    """the blocks a whole decode walks -> (off, first, size, type, nsmp) lists, `first` one longer (the samples the blocks reach):
    what LINNEAmd_StreamIndexBlocks reports for an undamaged stream.  A block: FF FF, size field (4 bytes: the block holds
    size + 6), CRC16, type, samples (2 bytes), payload"""
    b = bytes(stream)
    total = header_fields(b)["num_samples"]
    off, first, size, typ, nsmp = [], [0], [], [], []
    at = HEADER
    while first[-1] < total and at < len(b):
        assert b[at:at + 2] == b"\xff\xff", f"no block head at byte {at}"
        sz = int.from_bytes(b[at + 2:at + 6], "big")
        off.append(at)
        size.append(sz)
        typ.append(b[at + 8])
        nsmp.append(int.from_bytes(b[at + 9:at + 11], "big"))
        first.append(first[-1] + nsmp[-1])
        at += sz + 6
    return off, first, size, typ, nsmp


def pieces(tables, lo, n):
    """the pieces of the cut [lo, lo + n) of a stream with the block tables `tables` (blocks_of), in sample order: ("copy", r0, r1)
    for the maximal run of wholly covered blocks [r0, r1), ("frag", a, b) for the samples [a, b) a partly covered block gives"""
    off, first, size, typ, nsmp = tables
    out, hi = [], lo + n
    if n == 0:
        return out
    run = None
    for r in range(len(off)):
        a, b = max(lo, first[r]), min(hi, first[r + 1])
        if a >= b:
            continue
        if (a, b) == (first[r], first[r + 1]):
            run = (run[0], r + 1) if run else (r, r + 1)
            continue
        if run:
            out.append(("copy",) + run)
            run = None
        out.append(("frag", a, b))
    if run:
        out.append(("copy",) + run)
    return out


def assemble(cuts, fragment_block):
    """the spliced stream of cuts = [(stream bytes, first_sample, num_samples), ...] -> (bytes, copied blocks, encoded blocks, copy
    runs of source bytes).  fragment_block(cut number, a, b) gives the block of the samples [a, b) of that cut's stream: bytes
    [30, end) of a fresh encoder's stream of those samples alone"""
    total = sum(n for _, _, n in cuts)
    out = [with_num_samples(bytes(cuts[0][0][:HEADER]), total)]
    copied = encoded = runs = 0
    for k, (stream, lo, n) in enumerate(cuts):
        tables = blocks_of(stream)
        off, first, size, typ, nsmp = tables
        for p in pieces(tables, lo, n):
            if p[0] == "copy":
                _, r0, r1 = p
                out.append(bytes(stream[off[r0]:off[r1 - 1] + size[r1 - 1] + 6]))
                copied += r1 - r0
                runs += 1
            else:
                out.append(fragment_block(k, p[1], p[2]))
                encoded += 1
    return b"".join(out), copied, encoded, runs


# ---- the premise cases recorded against the real reference (tests/golden/splice_answers.json) ----
PREMISE_BLOCK, PREMISE_BLOCKS, PREMISE_CUT = 1024, 8, (1500, 4500)           # the cut [1500, 6000)
PREMISE_PRESETS = (0, 7)
FRAGMENT_LENGTHS = (1, 2, 5, 17, 33, 129, 256)


def premise_pcm(seed):
    return music(2, PREMISE_BLOCK * PREMISE_BLOCKS, 16, seed=seed)


def premise_cases(preset):
    """name -> the cuts [(pcm, first, n), ...] of a case: the trim of the issue, and a join of two different streams of one shape"""
    a, b = premise_pcm(100 + preset), premise_pcm(200 + preset)
    return {f"trim/m{preset}": [(a, PREMISE_CUT[0], PREMISE_CUT[1])],
            f"join/m{preset}": [(a, 700, 3000), (b, 2048, 2500)]}


def fragment_pcm(length, preset):
    """the fragment of `length` samples whose encodability is recorded: the head of a premise stream"""
    return premise_pcm(100 + preset)[:, 300:300 + length]


def splice_with(encoder, cuts_pcm, preset, bits=16, rate=44100, block=PREMISE_BLOCK, ms=True):
    """encoder.encode_whole's streams of the cuts' PCM, spliced by assemble with the same encoder's fragment blocks ->
    (spliced bytes, expected PCM)"""
    streams = [encoder.encode_whole(x, bits, rate, block, preset, ms) for x, _, _ in cuts_pcm]
    frag = lambda k, a, b: encoder.encode_whole(cuts_pcm[k][0][:, a:b], bits, rate, block, preset, ms)[HEADER:]
    data, _, _, _ = assemble([(s, lo, n) for s, (_, lo, n) in zip(streams, cuts_pcm)], frag)
    want = np.concatenate([x[:, lo:lo + n] for x, lo, n in cuts_pcm], axis=1)
    return data, want


# ---- the library's planner (linne_amd/csrc/lnn_splice.h through lnn_splice_plan) and its numpy restatement ----
WHY = {name: i for i, name in enumerate(["none", "null", "align", "no_cuts", "range", "unreached", "shape", "empty", "total", "short_fragment", "device"])}
MAX_ORDER = {0: 32, 1: 32, 2: 64, 3: 64, 4: 64, 5: 128, 6: 128, 7: 128}


class PlanStream:
    """a source stream as an index describes it: block tables (blocks_of) and header fields"""

    def __init__(self, tables, num_samples, channels=2, bits=16, rate=44100, block=1024, preset=0, ms=1, fail_block=-1, fail_code=0):
        self.tables, self.num_samples = tables, num_samples
        self.shape = (channels, bits, rate, block, preset, ms)
        self.fail_block, self.fail_code = fail_block, fail_code


def library_plan(lib, streams, outputs, frag_bytes):
    """lnn_splice_plan: streams = [PlanStream], outputs = [(cuts, capacity, why0)] with cuts = [(stream number or -1, first, n)],
    frag_bytes = the fragments' block sizes in plan order -> (per output dict, list of piece tuples (out, cut, frag, blocks, a, b, bytes, dst))"""
    import ctypes as C
    u64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64)
    rec = u64([[len(s.tables[0]), s.num_samples, *s.shape, s.fail_block & (2 ** 64 - 1), s.fail_code] for s in streams]).reshape(-1)
    keep = [[u64(s.tables[0]), u64(s.tables[1]), u64(s.tables[2]), u64(s.tables[4])] for s in streams]
    tabs = (C.c_void_p * max(4 * len(streams), 1))(*[a.ctypes.data for group in keep for a in group])
    cut_rec, out_in = [], []
    for cuts, capacity, why0 in outputs:
        out_in.append([len(cut_rec), len(cuts), capacity, why0])
        cut_rec += [[s & (2 ** 64 - 1), first, n] for s, first, n in cuts]
    cut_rec, out_in = u64(cut_rec).reshape(-1), u64(out_in).reshape(-1)
    fb = u64(frag_bytes)
    out_rec = np.zeros(8 * len(outputs), dtype=np.uint64)
    cap = 3 * sum(len(c) for c, _, _ in outputs) + 1
    piece_rec = np.zeros(8 * cap, dtype=np.uint64)
    f = lib.lnn_splice_plan
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]
    n = f(rec.ctypes.data, tabs, len(streams), cut_rec.ctypes.data, len(cut_rec) // 3, out_in.ctypes.data, len(outputs), fb.ctypes.data, len(fb),
          out_rec.ctypes.data, piece_rec.ctypes.data, cap)
    assert 0 <= n <= cap
    names = ("result", "why", "bytes", "total_samples", "copied_blocks", "encoded_blocks", "piece0", "npieces")
    outs = [dict(zip(names, (int(v) for v in out_rec[8 * k:8 * k + 8]))) for k in range(len(outputs))]
    for o in outs:
        o["result"] = o["result"] - (1 << 64) if o["result"] >= 1 << 63 else o["result"]
    return outs, [tuple(int(v) for v in piece_rec[8 * i:8 * i + 8]) for i in range(n)]


def numpy_plan(streams, outputs, frag_bytes):
    """the same answers from the contract's words (include/linne_amd.h), in the order it checks them"""
    outs, plist = [], []
    frag_bytes = list(frag_bytes)
    nfrag = 0
    for k, (cuts, capacity, why0) in enumerate(outputs):
        o = {"result": OK, "why": 0, "bytes": 0, "total_samples": 0, "copied_blocks": 0, "encoded_blocks": 0, "piece0": len(plist), "npieces": 0}
        outs.append(o)
        why = why0 or (WHY["no_cuts"] if not cuts else 0)
        total = 0
        for s, first, n in cuts:
            if why:
                break
            if s < 0:
                why = WHY["null"]
                continue
            x = streams[s]
            if first > x.num_samples or n > x.num_samples - first:
                why = WHY["range"]
            elif x.shape != streams[cuts[0][0]].shape:
                why = WHY["shape"]
            elif n and first + n > x.tables[1][-1] and x.fail_block < 0:
                why = WHY["unreached"]
            total += n
        if not why and total > 2 ** 32 - 1:
            why = WHY["total"]
        if not why and total == 0:
            why = WHY["empty"]
        if why:
            o.update(result=INVALID_ARGUMENT, why=why)
            continue
        for s, first, n in cuts:                                  # damage at or before the last block a cut overlaps
            x = streams[s]
            if n == 0 or x.fail_block < 0 or o["result"] != OK:
                continue
            firsts = x.tables[1]
            last = max(r for r in range(len(firsts) - 1) if firsts[r] <= first + n - 1) if first + n - 1 < firsts[-1] else len(firsts) - 1
            if x.fail_block <= last:
                o["result"] = x.fail_code
        if o["result"] != OK:
            continue
        mine, at, short = [], HEADER, False
        for i, (s, first, n) in enumerate(cuts):
            x = streams[s]
            off, _, size, _, _ = x.tables
            for p in pieces(x.tables, first, n):
                if p[0] == "copy":
                    a, b = off[p[1]], off[p[2] - 1] + size[p[2] - 1] + 6
                    mine.append([k, i, 0, p[2] - p[1], a, b, b - a])
                    o["copied_blocks"] += p[2] - p[1]
                else:
                    short = short or p[2] - p[1] <= MAX_ORDER[x.shape[4]]
                    mine.append([k, i, 1, 1, p[1], p[2], None])
                    o["encoded_blocks"] += 1
        if short:
            o.update(result=INVALID_ARGUMENT, why=WHY["short_fragment"], copied_blocks=0, encoded_blocks=0)
            continue
        for p in mine:
            if p[2]:
                p[6] = frag_bytes[nfrag] if nfrag < len(frag_bytes) else 0
                nfrag += 1
            plist.append(tuple(p) + (at,))
            at += p[6]
        o.update(total_samples=total, npieces=len(mine), bytes=at)
        if at > capacity or at > 2 ** 32 - 1:
            o["result"] = INSUFFICIENT_BUFFER
    return outs, plist
