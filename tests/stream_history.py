"""What tests/test_stream_history_cpu.py and tests/test_gpu_stream_history.py share: the scenarios that ask whether the answer of a
call on resident .lnn streams depends on the calls the context served before it, as plain data, and every step's expected answer.
Nothing here touches a GPU or the library.

The resident-stream calls work in buffers of the context that grow and are never cleared ("What the resident calls
share"): a windows call's accumulators lie behind its scratch, so a small call's accumulators land where the larger call before it
kept its samples, and each consumer has to reset its own.  A scenario is a list of steps that the GPU test runs in order on ONE
context.  A step is a dict:

    {"call": the entry point, "wins": [(stream name, first sample, samples)], "gf": group_frames, "note": the stale state the step
     is written to meet, and the call's own inputs: "buckets" (measure, digest), "thr" / "mins" / "caps" (quiet), "flips" (compare:
     window -> [(channel, sample)] whose held PCM differs from the stream), "codes" (the windows' expected results, all OK if absent),
     "raises" (the code of a call refused as a whole)}

expected(step, mat) is its answer from the references of tests/stream_refs.py on the oracle's decode of the oracle's bytes, whatever
ran before the step.  The streams are small: twelve to twenty-four blocks and a ragged tail."""
import numpy as np

import index_cases as ic
import repair_cases as rc
import splice_cases as sc
from signals import music
from stream_refs import crc16, expected_compare, expected_digest, expected_measure, expected_quiet

OK, INVALID_ARGUMENT, CORRUPTION, NG = 0, 1, 6, 7
COMPRESS, SILENT, RAW = 0, 1, 2
CONSUMERS = ["place", "measure", "digest", "quiet", "compare"]
ACCUMULATING = ("measure", "digest", "quiet")
LATER = ("histogram", "relate")             # they run before and after every consumer, themselves included, in scenarios of their own below
OTHER_CALLS = ["index_streams", "repair_streams", "splice_streams", "encode_streams", "set_verify"]
RATE = 44100

# name -> (channels, bits, block, preset, mid/side, whole blocks, tail): stereo 16-bit at 1024, mono 24-bit at 512, three channels
# 8-bit at 256; presets 0 to 4 and one stereo stream at 7
SPEC = {"mixed": (2, 16, 1024, 4, True, 12, 300), "loud": (2, 16, 1024, 7, True, 12, 555), "mono": (1, 24, 512, 2, False, 16, 100),
        "hush": (1, 24, 512, 0, False, 24, 200), "three": (3, 8, 256, 1, False, 20, 77), "faint": (3, 8, 256, 3, False, 22, 130)}
NAMES = list(SPEC)
MIXED_ORDER = "csscrrcscrcc"                # music, SILENT and RAW blocks of "mixed" (the tail is music)
MIXED_TYPES = [{"c": COMPRESS, "s": SILENT, "r": RAW}[k] for k in MIXED_ORDER] + [COMPRESS]
LOUD = 7


def num_samples(name):
    return SPEC[name][5] * SPEC[name][2] + SPEC[name][6]


def pcm_of(name):
    """the stream's samples.  mixed: music with silent and full-scale-noise blocks; loud: three times the level, clipped, every frame
    loud but the planted zeros; hush / faint: within +-3 but for planted spikes; mono / three: music.  Every stream has zeros
    planted at places of its own, so that no two streams have the same quiet runs"""
    nch, bits, block, preset, ms, nb, tail = SPEC[name]
    ns, seed = num_samples(name), 500 + NAMES.index(name)
    x = music(nch, ns, bits, seed=seed).astype(np.int64)
    lim = 1 << (bits - 1)
    rng = np.random.default_rng(seed)
    if name == "mixed":
        for i, k in enumerate(MIXED_ORDER):
            if k == "s":
                x[:, i * block:(i + 1) * block] = 0
            elif k == "r":
                x[:, i * block:(i + 1) * block] = rng.integers(-lim, lim, size=(nch, block))
    elif name == "loud":
        x = np.clip(3 * x, -lim, lim - 1)
        x[0, np.abs(x[0]) < LOUD] = LOUD
    elif name in ("hush", "faint"):
        x = x // (lim // 4)
        for at in rng.integers(0, ns, size=40):
            x[int(at) % nch, int(at)] = lim // 3
    k = NAMES.index(name)
    for j in range(30):                      # zeros of 1 to 90 frames, at places and of lengths of the stream's own
        at = (131 * j * (k + 2) + 17 * k) % (ns - 100)
        x[:, at:at + 1 + (7 * j + 13 * k) % 90] = 0
    return np.ascontiguousarray(x, dtype=np.int32)


class Material:
    """the streams: their PCM, the oracle's bytes of it and the oracle's decode of those bytes; the damaged streams of scenario (c)"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.pcm, self.data, self.full, self.bits = {}, {}, {}, {}
        for name in NAMES:
            nch, bits, block, preset, ms, _, _ = SPEC[name]
            self.add(name, bytes(oracle.encode_whole(pcm_of(name), bits, RATE, block, preset, ms)), pcm_of(name))
        # a payload byte of a COMPRESS block of "loud" flipped: the block's CRC fails, the index names it
        bl = self.tables("loud")
        self.crc_block = 5
        bad = bytearray(self.data["loud"])
        bad[bl[0][5] + bl[2][5] + 6 - 2] ^= 0x10
        self.add("loud/crc", bytes(bad), None)
        # a bit of the Rice codes of a COMPRESS block of "loud" flipped and the CRC made right again, such that the whole decode fails
        self.rice_block = 8
        off, size = bl[0][8], bl[2][8] + 6
        rng = np.random.default_rng(77)
        for _ in range(64):
            bad = bytearray(self.data["loud"])
            p = off + 11 + (size - 11) // 2 + int(rng.integers(0, (size - 11) // 2))
            bad[p] ^= 1 << int(rng.integers(0, 8))
            bad[off + 6:off + 8] = crc16(bad[off + 8:off + size]).to_bytes(2, "big")
            ret = oracle.decode_whole(bytes(bad))[0]
            if ret != OK:
                self.rice_code = ret
                self.add("loud/rice", bytes(bad), None)
                break
        assert "loud/rice" in self.data, "no flip in 64 made the whole decode fail"
        # more shapes than one call takes: mono 16-bit streams of one block each, every one of another block size
        self.tiny = [f"tiny{i}" for i in range(65)]
        for i, name in enumerate(self.tiny):
            x = music(1, 100 + i, 16, seed=900 + i)
            self.add(name, bytes(oracle.encode_whole(x, 16, RATE, 100 + i, 0, False)), x)

    def add(self, name, data, pcm):
        self.data[name] = data
        if pcm is None:                      # a damaged stream: its sound blocks are the clean stream's, byte for byte
            self.full[name] = self.full[name.split("/")[0]]
        else:
            ret, full = self.oracle.decode_whole(data)[:2]
            assert ret == OK, name
            self.full[name] = np.ascontiguousarray(full, dtype=np.int32)
        self.pcm[name] = pcm
        self.bits[name] = int.from_bytes(data[22:24], "big")

    def tables(self, name):
        """(off, first, size, type, nsmp) by the serial block walk of index_cases"""
        return ic.index_walk(self.data[name])[3]

    def failure(self, name):
        return ic.index_walk(self.data[name])[4]


_MATERIAL = {}


def material(oracle):
    if "m" not in _MATERIAL:
        _MATERIAL["m"] = Material(oracle)
    return _MATERIAL["m"]


# ---------------------------------------------------------------------------------------------------------------------------------
# steps and their expected answers

BUCKETS = (1, 7, 441, 0)
THRESHOLDS = (0, 3, 40, 1 << 15)
MINS = (1, 2, 17, 64, 5)
CAP = 512
# cycled through the windows of a step from the step's own offset: histogram (num_bins, shift, log2, bucket_samples), relate bucket_samples
SPECS = {"histogram": [(1024, 4, False, 0), (33, 0, True, 441), (64, 9, False, 7), (2, 0, True, 0), (1024, 0, False, 300), (65, 2, True, 1), (1, 0, False, 64)],
         "relate": [0, 441, 7, 1, 300, 64, 256]}


def step(call, wins, k=0, gf=0, note="", **kw):
    """a windows step; k shifts the buckets, thresholds and min_samples so that consecutive steps use other ones"""
    s = {"call": call, "wins": list(wins), "gf": gf, "note": note}
    W = len(wins)
    if call in ("measure", "digest"):
        s["buckets"] = [BUCKETS[(k + i) % 4] for i in range(W)]
    elif call == "quiet":
        s["thr"] = [THRESHOLDS[(k + i) % 4] for i in range(W)]
        s["mins"] = [MINS[(k + 2 * i) % 5] for i in range(W)]
        s["caps"] = [CAP] * W
    elif call == "compare":
        # every other window holds PCM that differs in 1 + k % 3 elements; which windows alternates from one compare step to the next
        s["flips"] = {i: [((i + j) % SPEC_OF(wins[i][0])[0], (3 * k + 11 * j) % wins[i][2]) for j in range(1 + k % 3)] for i in range(W) if (i + k) % 2 == 0}
    elif call in SPECS:
        s["specs"] = [SPECS[call][(k + i) % len(SPECS[call])] for i in range(W)]
    s.update(kw)
    return s


def SPEC_OF(name):
    return SPEC[name.split("/")[0]] if not name.startswith("tiny") else (1, 16, 0, 0, False, 1, 0)


def held_pcm(s, i, mat):
    """the PCM a compare step holds against window i"""
    name, first, n = s["wins"][i]
    held = mat.full[name][:, first:first + n].copy()
    for ch, at in s.get("flips", {}).get(i, []):
        held[ch, at] ^= 1
    return held


def expected(s, mat):
    """per window the step's answer (None for a window that fails): place the samples, compare (count, first sample, first channel),
    measure and digest their tables, quiet (the runs that fit, num_runs, quiet_samples, lead, trail)"""
    out = []
    codes = s.get("codes") or [OK] * len(s["wins"])
    for i, (name, first, n) in enumerate(s["wins"]):
        full = mat.full[name]
        if codes[i] != OK:
            out.append(None)
        elif s["call"] == "place":
            out.append(full[:, first:first + n])
        elif s["call"] == "compare":
            out.append(expected_compare(full, first, n, held_pcm(s, i, mat)))
        elif s["call"] == "measure":
            out.append(expected_measure(full, first, n, s["buckets"][i]))
        elif s["call"] == "digest":
            out.append(expected_digest(full, mat.bits[name], first, n, s["buckets"][i]))
        else:
            runs, *rest = expected_quiet(full, first, n, s["thr"][i], s["mins"][i])
            out.append((runs[:s["caps"][i]], *rest))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) every ordered pair of consumers adjacent at least once

def de_bruijn(k, n):
    """the lexicographically least de Bruijn sequence of order n over k symbols (the concatenation of the Lyndon words whose length
    divides n): read cyclically, every word of length n occurs once"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)
    db(1, 1)
    return seq


def order_a():
    seq = de_bruijn(len(CONSUMERS), 2)
    return [CONSUMERS[i] for i in seq + seq[:1]]


SPANS = [(37, 700), (250, 64), (1000, 650), (3000, 333)]        # the same few windows, call after call, on other streams each time
ANCHOR_HIGH = 9
SMALL_STREAMS = ["mixed", "mono", "hush", "three", "faint"]


def scenario_a(shift=0):
    """26 calls.  Call k has the windows SPANS on four of the five smaller streams, rotated by one from call to call, and in front of
    them an anchor window over whole blocks of "loud", the largest shape: the anchor's pass is the call's largest, so the anchor alone
    decides where the call's accumulators begin (o_acc).  The anchor shrinks by a block behind every call that leaves little behind
    its scratch (place, compare, quiet), stays behind measure and digest, and is long again in every place and compare call: every
    accumulator region then begins in bytes the call before it wrote.  shift: other streams and parameters for the second context of
    scenario (f)"""
    steps, nc, prev = [], ANCHOR_HIGH, None
    for k, call in enumerate(order_a()):
        if call in ("place", "compare") or prev is None:
            nc = ANCHOR_HIGH
        elif prev in ("place", "compare", "quiet"):
            nc -= 1
        assert nc >= 3
        wins = [("loud", 1024, nc * 1024 - 24)] + [(SMALL_STREAMS[(k + i + shift) % 5], a, n) for i, (a, n) in enumerate(SPANS)]
        steps.append(step(call, wins, k=k + shift, note=f"behind {prev or 'nothing'}: its accumulators begin where that call's "
                          f"{'accumulators' if prev in ACCUMULATING else 'scratch'} lay" if call in ACCUMULATING else f"behind {prev or 'nothing'}: the words that come back"))
        prev = call
    return steps


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) large, then small, then large again

def largest_block(mat, name):
    """the COMPRESS block of a stream whose slot in a pass's packed segment is the largest (the stream at a 16-byte aligned address)"""
    off, first, size, typ, nsmp = mat.tables(name)
    return max((r for r in range(len(off)) if typ[r] == COMPRESS and nsmp[r] >= 200), key=lambda r: (off[r] & 15) + size[r])


def scenario_b(mat):
    """name -> steps.  b/X: the whole stream through consumer X; 64 samples inside one block through another consumer, whose
    accumulators (a few hundred bytes) begin inside X's samples; the whole stream again with group_frames = 1, pass after pass in the
    same scratch; the 64 samples again.  The 64 samples lie in the block whose pass is the stream's largest, so that the one-block
    passes of the third call end where the small call's did.  b/many/X: 64 windows of every shape, then one window"""
    out = {}
    rng = np.random.default_rng(12)
    for j, (x, y, name) in enumerate((("measure", "digest", "mixed"), ("digest", "quiet", "mono"), ("quiet", "measure", "three"))):
        r = largest_block(mat, name)
        first = mat.tables(name)[1][r]
        whole, small = [(name, 0, num_samples(name))], [(name, first + 70, 64)]
        out[f"b/{x}"] = [step(x, whole, k=2, note="grows the scratch: samples of the whole stream"),
                         step(y, small, k=j + 1, note=f"its accumulators begin inside the whole-stream call's samples"),
                         step(x, whole, k=1, gf=1, note="many passes in one scratch, its accumulators where the small call's lay"),
                         step(y, small, k=j + 1, note="the same 64 samples again: the same answer")]
        wins = []
        for i in range(64):
            nm = NAMES[i % 6]
            a = int(rng.integers(0, num_samples(nm) - 900))
            wins.append((nm, a, int(rng.integers(1, 900))))
        out[f"b/many/{x}"] = [step(x, wins, k=j, note="64 windows of every shape: long lists, accumulators of every window"),
                              step(y, [(name, first + 5, 150)], k=j + 2, note="one window: its accumulators inside the 64 windows' samples")]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) after failures

def good_calls(k):
    """one good call of each consumer over windows that the failing calls' windows overlap"""
    wins = [("loud", 2000 + 100 * k, 3000), ("mixed", 500, 2000 + 10 * k), ("three", 100 * k, 1500)]
    return [step(call, wins, k=k + j, note="a good call behind a failing one") for j, call in enumerate(CONSUMERS)]


def scenario_c(mat):
    """[(the failing step, the good steps behind it)].  A failing step's good windows are held to their references too"""
    bl = mat.tables("loud")
    k, r = mat.crc_block, mat.rice_block
    ns = num_samples("loud")
    good = [("mixed", 100, 900), ("three", 300, 1000)]
    runs = expected_quiet(mat.full["hush"], 0, num_samples("hush"), 3, 2)[1]
    fails = [step("digest", [good[0], ("loud/rice", bl[1][r] + 10, 700), ("loud/rice", bl[1][r - 1] + 10, 700), good[1]], k=1, codes=[OK, NG, OK, OK],
                  note="a window over a block whose Rice codes do not end where they should: its fail word is set on the device"),
             step("measure", [("loud/crc", bl[1][k] + 3, 600), good[0], ("loud/crc", 0, bl[1][k] - 24), ("loud/crc", bl[1][k + 1], 200)], k=2,
                  codes=[CORRUPTION, OK, OK, CORRUPTION], note="windows that reach the index's fail_block: refused on the host, the others run"),
             step("compare", [good[1], ("loud", 1, ns), good[0]], k=0, codes=[OK, INVALID_ARGUMENT, OK], note="a window beyond the stream"),
             step("quiet", [("hush", 0, num_samples("hush")), good[0]], k=1, thr=[3, 0], mins=[2, 1], caps=[runs - 1, CAP],
                  note="a capacity one record too small: the runs are counted, the last one is not written"),
             step("measure", [(name, 0, 50) for name in mat.tiny], k=3, raises=NG, note="65 stream shapes: the call is refused as a whole")]
    return [(f, good_calls(i)) for i, f in enumerate(fails)]


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) the other resident calls in between

SIXTEEN = NAMES + ["loud/crc", "loud/rice"] + [f"tiny{i}" for i in range(8)]


def cut_inside(mat, name, r):
    """a cut of `name` from inside block r to inside block r + 2: both its edge blocks are decoded and encoded again"""
    first = mat.tables(name)[1]
    n = first[r + 1] - first[r]
    return (name, first[r] + n // 3, 2 * n)


def gapped(mat, name, blocks):
    """the stream with a payload byte flipped in each of `blocks`"""
    off, first, size, typ, nsmp = mat.tables(name)
    b = bytearray(mat.data[name])
    for r in blocks:
        b[off[r] + 11 + (size[r] - 5) // 2] ^= 0x10
    return bytes(b)


def scenario_d(mat):
    """the list of the issue; the steps behind the refused splice carry "count": their launches are compared with the same call's on a
    fresh context"""
    windows = [("mixed", 700, 3000), ("mono", 100, 2000), ("faint", 1000, 1500)]
    tracks = ["mono", "three", "mixed"]
    return [{"call": "index_streams", "streams": SIXTEEN, "note": "16 streams: the scan's lists, row tables and candidates"},
            {"call": "repair_streams", "streams": [gapped(mat, "mixed", [6])], "note": "the candidates of one stream where 16 streams' lay"},
            {"call": "index_streams", "streams": ["three"], "note": "one stream behind a repair"},
            {"call": "splice_streams", "cuts": [[cut_inside(mat, "loud", 2)]], "note": "the inner decode-windows and encode-streams calls"},
            {"call": "repair_streams", "streams": [gapped(mat, "loud", [3, 8]), gapped(mat, "mono", [0, 5, 6]), gapped(mat, "mixed", [0, 12])],
             "note": "three streams with gaps: the splice's buffers lie between two repairs"},
            {"call": "set_verify", "on": True, "note": ""},
            {"call": "encode_streams", "tracks": tracks, "note": "verified: an inner compare call behind the encode"},
            {"call": "set_verify", "on": False, "note": ""},
            {"call": "encode_streams", "tracks": tracks[::-1], "note": "not verified: no compare call runs"},
            {"call": "splice_streams", "cuts": [[("loud", 100, num_samples("loud"))]], "raises": INVALID_ARGUMENT,
             "note": "a cut beyond its stream: refused; outer_keep and span_keep must not stay set"},
            {"call": "splice_streams", "cuts": [[cut_inside(mat, "mixed", 8)], [cut_inside(mat, "mono", 3), ("mono", 0, 700)]], "count": True, "note": "a good splice behind the refused one"},
            *[dict(step(call, windows, k=j, note="a windows call behind the refused splice"), count=True) for j, call in enumerate(CONSUMERS)],
            {"call": "index_streams", "streams": SIXTEEN, "count": True, "note": "the 16 again: every index equal to the first one"}]


def expected_index(mat, name):
    """(code, num_blocks, the five tables, failure) by the block walk"""
    code, h, nb, tables, failure = ic.index_walk(mat.data[name])
    return code, nb, tables, failure


def expected_repair(data):
    rc.MAGIC = bytes(data[:4])
    return rc.repair(data)


def expected_splice(mat, cuts):
    """(bytes, copied blocks, re-encoded blocks, the PCM the spliced stream decodes to)"""
    name0 = cuts[0][0]

    def fragment(k, a, b):
        nch, bits, block, preset, ms, _, _ = SPEC[cuts[k][0]]
        return bytes(mat.oracle.encode_whole(mat.full[cuts[k][0]][:, a:b], bits, RATE, block, preset, ms))[sc.HEADER:]
    data, copied, encoded, _ = sc.assemble([(mat.data[name], lo, n) for name, lo, n in cuts], fragment)
    assert name0 in SPEC
    return data, copied, encoded, np.concatenate([mat.full[name][:, lo:lo + n] for name, lo, n in cuts], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# (e) the old indexes after the growth, (f) two contexts

def scenario_e():
    wins = [("mixed", 3 * 1024 - 40, 2200), ("mono", 0, num_samples("mono")), ("three", 77, 64), ("faint", 2000, 900), ("hush", 5000, 3000), ("loud", 0, 5000)]
    return [step(call, wins, k=j + 1, note="indexes built before the scratch grew beside them") for j, call in enumerate(CONSUMERS)]


def scenario_f():
    """(context A's list, context B's): (a)'s calls, B's on other streams with other parameters"""
    return scenario_a(0), scenario_a(2)


# ---------------------------------------------------------------------------------------------------------------------------------
# histogram and relate: their counters and records lie in the context's scratch where the measure, digest and quiet calls keep their
# accumulators, behind every pass's buffers.  Each runs before and after every other consumer, large, then small, then large again, and
# behind failing calls

def windows_of(k):
    """an anchor over whole blocks of the largest shape and SPANS on four of the smaller streams, rotated from call to call"""
    return [("loud", 1024, (9 - k % 3) * 1024 - 24)] + [(SMALL_STREAMS[(k + i) % 5], a, n) for i, (a, n) in enumerate(SPANS)]


def scenario_between(x):
    """x before and after every consumer that came before it"""
    steps = [step(x, windows_of(0), k=0, note="the context's first call")]
    for k, call in enumerate(CONSUMERS + list(LATER[:LATER.index(x)]), 1):
        steps.append(step(call, windows_of(2 * k), k=k, note=f"behind the {x} call: its accumulators or samples where that call's tables lay"))
        steps.append(step(x, windows_of(2 * k + 1), k=3 * k, gf=k % 2, note=f"behind {call}: its tables where that call's accumulators or scratch lay"))
    return steps


LARGE = {"histogram": ([(1024, 2, False, 0)], [(33, 0, True, 7)], [(1024, 2, False, 441)]), "relate": ([0], [7], [441])}


def scenario_large_small_large(mat, x):
    name = "mixed"
    r = largest_block(mat, name)
    first = mat.tables(name)[1][r]
    whole, small = [(name, 0, num_samples(name))], [(name, first + 70, 64)]
    big, few, passes = LARGE[x]
    steps = [step(x, whole, specs=big, note="grows the scratch: samples of the whole stream, the slots of one long bucket"),
             step(x, small, specs=few, note="its tables begin inside the whole-stream call's samples"),
             step(x, whole, specs=passes, gf=1, note="many passes in one scratch, its tables where the small call's lay"),
             step(x, small, specs=few, note="the same 64 samples again: the same answer"),
             step(x, whole, specs=big, note="and the whole stream as at first")]
    rng = np.random.default_rng(12)
    wins = []
    for i in range(64):
        nm = NAMES[i % 6]
        a = int(rng.integers(0, num_samples(nm) - 900))
        wins.append((nm, a, int(rng.integers(1, 900))))
    return steps + [step(x, wins, k=1, note="64 windows of every shape: long lists, tables of every window"),
                    step(x, [(name, first + 5, 150)], k=3, note="one window: its tables inside the 64 windows' samples"),
                    step(x, wins, k=4, note="the 64 windows with other specs")]


def scenario_behind_failures(mat, x):
    bl = mat.tables("loud")
    k, r = mat.crc_block, mat.rice_block
    good = [("mixed", 100, 900), ("three", 300, 1000)]
    after = [("loud", 2000, 3000), ("mixed", 500, 2000), ("three", 0, 1500)]
    return [step(x, [good[0], ("loud/rice", bl[1][r] + 10, 700), ("loud/rice", bl[1][r - 1] + 10, 700), good[1]], k=1, codes=[OK, NG, OK, OK],
                 note="a window over a block whose Rice codes do not end where they should: its fail word is set on the device, its table is not committed"),
            step(x, after, k=2, note="a good call behind it"),
            step(x, [("loud/crc", bl[1][k] + 3, 600), good[0], ("loud/crc", 0, bl[1][k] - 24), ("loud", 1, num_samples("loud"))], k=2,
                 codes=[CORRUPTION, OK, OK, INVALID_ARGUMENT], note="windows refused on the host, the others run"),
            step(x, after, k=5, gf=2, note="a good call behind it"),
            step(x, [(nm, 0, 50) for nm in mat.tiny], k=3, raises=NG, note="65 stream shapes: the call is refused as a whole"),
            step(x, after, k=0, note="a good call behind it"),
            step("measure", after, k=1, note="and a sibling behind that")]


def entry_points(steps):
    return {s["call"] for s in steps}
