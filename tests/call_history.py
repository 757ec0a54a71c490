"""What tests/test_call_history_cpu.py and tests/test_gpu_call_history.py share: the scenarios that ask whether a context's answer
depends on the calls before it, as plain data, and the oracle's answer for every step.  Nothing here touches a GPU.

A scenario is a list of steps that the GPU test runs in order on ONE context (or one API handle).  A step's expected output is the
oracle's answer for that step's input alone, whatever came before it.  An encode step is

    {"shape": (channels, bits, block, preset, ms), "ns": lengths, "bmap": base frame per frame, "seed", "kind": the material,
     "af", "learn": the oracle's settings, "env": knobs of the call, "set": context setters to call before it}

and its frames are the base frames bases(shape, seed, kind)[bmap], cut to their lengths.  The oracle runs once per distinct
(shape, settings, length, content) of the whole module (CACHE, filled by test_gpu_batch_forms.OracleBatch from batch_of(step));
every answer is decoded again by the oracle's own synthesis when it is computed.

replay_classes() restates the bookkeeping of build_classes (linne_amd/csrc/lnn_device.hip) -- the resident class table of a
context, what a call finds there, and whether it appends to it or starts it over -- so that the CPU test can assert that the
scenarios take the branches they are written for.
"""
import numpy as np

from signals import music, music_frames

MAXCLS = 16         # linne_amd/csrc/lnn_dev_common.h LNN_MAXCLS: length classes of the resident table
META = 8            # LNN_META: slots of the pinned metadata ring
NBASE = 4
SENTINEL = -123456
INVALID_ARGUMENT, INVALID_FORMAT = 1, 2       # include/linne.h LINNEApiResult


def shp(nch, bits, block, preset, ms):
    return (nch, bits, block, preset, bool(ms))


_BASES = {}


def bases(shape, seed, kind):
    """[NBASE][C][block]: 'music' (base 1 at a third of the level), 'loud' (three times the level, clipped) or 'quiet' (1/64)"""
    nch, bits, block = shape[:3]
    key = (nch, bits, block, seed, kind)
    if key not in _BASES:
        b = music_frames(NBASE, nch, block, bits, seed=seed).astype(np.int64)
        if kind == "loud":
            b = np.clip(3 * b, -(1 << (bits - 1)), (1 << (bits - 1)) - 1)
        elif kind == "quiet":
            b = b // 64
        else:
            assert kind == "music", kind
            b[1] = np.trunc(b[1] / 3.0)
        b = b.astype(np.int32)
        b.setflags(write=False)
        _BASES[key] = b
    return _BASES[key]


def enc(shape, ns, rot=0, seed=1, kind="music", af=0, learn=0, env=None, set=(), name=""):
    ns = np.array(list(ns), dtype=np.uint32)
    return {"shape": shape, "ns": ns, "bmap": (np.arange(len(ns)) + rot) % NBASE, "seed": seed, "kind": kind, "af": af, "learn": learn,
            "env": dict(env or {}), "set": tuple(set), "name": name or f"{len(ns)} frames of {sorted(set_of(ns), reverse=True)}"}


def set_of(ns):
    return {int(n) for n in ns}


def frames_of(step):
    """[F][C][block] int32, zero behind each frame's length"""
    x = bases(step["shape"], step["seed"], step["kind"])[step["bmap"]].copy()
    for f, n in enumerate(step["ns"]):
        x[f, :, int(n):] = 0
    return np.ascontiguousarray(x)


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle's answers: test_gpu_batch_forms.OracleBatch computes them (and decodes each with the oracle's own synthesis) from
# batch_of(step), and keeps them in CACHE by (shape, settings, length, content) over the whole module

CACHE = {}


def batch_of(step):
    """a step in the form OracleBatch and check_encode read"""
    nch, bits, block, preset, ms = step["shape"]
    return {"frames": frames_of(step), "ns": step["ns"], "bases": bases(step["shape"], step["seed"], step["kind"]), "bmap": step["bmap"],
            "nch": nch, "bits": bits, "block": block, "preset": preset}


def held(oracle, step):
    """(the oracle's answers of a step as an OracleBatch, the batch)"""
    from test_gpu_batch_forms import OracleBatch
    batch = batch_of(step)
    return OracleBatch(oracle, batch, step["shape"][4], cache=CACHE, af=step["af"], learn=step["learn"]), batch


# ---------------------------------------------------------------------------------------------------------------------------------
# build_classes' bookkeeping, restated

def distinct(ns):
    out = []
    for n in ns:
        if int(n) not in out:
            out.append(int(n))
    return out


def replay_classes(calls):
    """calls: [(shape, lengths)] in order on one context -> [(branch, resident lengths after the call)] with branch one of
    'first' (nothing resident), 'restart by shape', 'restart by overflow', 'append', 'reuse' (nothing missing).  As build_classes:
    the table is kept while the shape is the same and it has room for the missing lengths; otherwise it starts over with this call's"""
    resident, rshape, out = [], None, []
    for shape, ns in calls:
        lens = distinct(ns)
        assert len(lens) <= MAXCLS, "such a call is refused"
        same = rshape == shape
        missing = [n for n in lens if not (same and n in resident)]
        if not missing:
            branch = "reuse"
        elif not same:
            branch, resident = ("first" if rshape is None else "restart by shape"), list(lens)
        elif len(resident) + len(missing) > MAXCLS:
            branch, resident = "restart by overflow", list(lens)
        else:
            branch, resident = "append", resident + missing
        rshape = shape
        out.append((branch, list(resident)))
    return out


def calls_of(steps):
    return [(s["shape"], s["ns"]) for s in steps]


# ---------------------------------------------------------------------------------------------------------------------------------
# scenario 1: the class table grows, call after call

S1 = shp(2, 16, 2048, 7, True)


def scenario1():
    return [enc(S1, [2048] * 4, rot=0),
            enc(S1, [2048, 2048, 777, 2048, 777], rot=1),
            enc(S1, [2048, 1001, 129, 2048, 1001, 129], rot=2),        # 1001: analysis length 1008, odd units 63 (quirk Q1)
            enc(S1, [2048] * 3, rot=3),
            enc(S1, [777] * 3, rot=0),
            enc(S1, [1001, 777, 777, 1001, 777], rot=1)]                # tail first


S1_BRANCHES = ["first", "append", "append", "reuse", "reuse", "reuse"]


# ---------------------------------------------------------------------------------------------------------------------------------
# scenario 2: the table overflows and starts over

S2 = shp(1, 16, 1024, 4, False)
A2 = [1024, 1000, 900, 801, 777, 640, 513, 400, 255, 129]
B2 = [1023, 960, 850, 768, 700, 555, 512, 333, 200, 130]
C2 = [A2[1], A2[4], A2[8], B2[0], B2[5], B2[9]]
D2 = B2[:6] + [A2[1], A2[4]] + [A2[0], A2[2], A2[3]] + [1011, 911, 611, 411, 211]      # 8 resident after C, 8 not


def scenario2():
    return [enc(S2, A2, name="A"), enc(S2, B2, rot=1, name="B"), enc(S2, C2, rot=2, name="C"), enc(S2, D2, rot=3, name="D"),
            enc(S2, A2, name="E = A"), enc(S2, [A2[9], A2[0], A2[9]], rot=1, name="F")]


S2_BRANCHES = ["first", "restart by overflow", "append", "restart by overflow", "restart by overflow", "reuse"]


# ---------------------------------------------------------------------------------------------------------------------------------
# scenario 3: the shape changes, a field at a time and all at once

def scenario3():
    a = shp(2, 16, 2048, 7, True)
    shapes = [a, shp(2, 24, 2048, 7, True), shp(2, 24, 2048, 7, False), shp(2, 24, 2048, 6, False), shp(2, 24, 1024, 6, False),
              shp(1, 24, 1024, 0, False), shp(8, 8, 1024, 4, True), a]
    return [enc(s, [s[2], 777, s[2]], rot=i, seed=3) for i, s in enumerate(shapes)]


S3_BRANCHES = ["first"] + ["restart by shape"] * 7


# ---------------------------------------------------------------------------------------------------------------------------------
# scenario 4: modes switched on and off (X: the plain calls' input, Y: the input of the calls with a mode on)

S4 = shp(2, 16, 1024, 3, True)


def scenario4():
    def X(*setters):
        return enc(S4, [1024, 777], rot=0, seed=4, set=setters, name="plain")

    def Y(name, *setters, **kw):
        return enc(S4, [1024, 777], rot=2, seed=4, set=setters, name=name, **kw)

    return [X(),
            Y("-a 1", ("set_af_iterations", 1), af=1), X(("set_af_iterations", 0)),
            Y("-l", ("set_learning", True), learn=1), X(("set_learning", False)),
            Y("capture on", ("set_search_capture", True)), X(("set_search_capture", False)),
            Y("timing on", ("enable_timing", True)), X(("enable_timing", False))]


# ---------------------------------------------------------------------------------------------------------------------------------
# scenario 5: kernel forms taking turns on one context

S5 = shp(2, 24, 2048, 7, True)
SIX = [2048, 2048, 777, 2048, 1001, 2048]


def scenario5():
    return [enc(S5, [2048], seed=5, name="one frame"),
            enc(S5, [777 if f % 5 == 4 else 2048 for f in range(40)], rot=1, seed=5, name="40 frames"),
            enc(S5, [2048], rot=2, seed=5, name="one frame"),
            enc(S5, SIX, rot=3, seed=5, name="default"),
            enc(S5, SIX, seed=5, env={"LINNE_AMD_HIST": "1", "LINNE_AMD_FWD_LOSS": "1", "LINNE_AMD_STATS_ROWS": "1"}, name="hist + fwd_loss + stats_rows"),
            enc(S5, SIX, rot=1, seed=5, kind="loud", name="default, loud"),
            enc(S5, SIX, rot=2, seed=5, kind="quiet", env={"LINNE_AMD_PREP_GENERAL": "1"}, name="prep_general, quiet"),
            enc(S5, [2048, 777, 2048, 777, 2048, 1001], rot=3, seed=5, env={"LINNE_AMD_SORT": "0"}, name="unsorted, alternating"),
            enc(S5, SIX, rot=2, seed=5, name="default")]


def inexact_rows(step):
    """channel-frames of a step whose sum of squares reaches 2^53: k_prep's exact-sum test fails for them (k_prep_slow's row list)"""
    x = frames_of(step).astype(np.int64)
    assert step["shape"][4] and step["shape"][0] == 2
    side = x[:, 1] - x[:, 0]
    mid = x[:, 0] + (side >> 1)
    return sum(int(((y * y).sum(axis=1) >= (1 << 53)).sum()) for y in (mid, side))


# ---------------------------------------------------------------------------------------------------------------------------------
# scenario 6: more calls in flight than the metadata ring has slots.  All calls but the last have the same number of frames, so that a
# ring slot is laid out the same way whichever of them wrote it; the decode calls take the ring's 4th, 8th and 12th acquisition, so
# that a slot that held an encode call's class indices is next taken by an encode call, and a decode call's lengths by a decode call.
# The LAST call is larger (40 frames, its first eight full ones): d_clsidx / d_map grow through ensure_buf while fourteen calls are
# still queued in front of it.

F6 = 24
F6_LAST = 40
POOL6 = [2048, 777, 1001, 129]
ORDER6 = "eeedeeedeeedeee"


def scenario6():
    steps = []
    for i, op in enumerate(ORDER6):
        ns = [POOL6[(f // (1 + i % 3) + i) % 4] for f in range(F6)]
        if i == len(ORDER6) - 1:
            ns = [2048] * 8 + [POOL6[(f + 1) % 4] for f in range(F6_LAST - 8)]
        s = enc(S1, ns, rot=i, name=f"call {i}")
        s["op"] = "encode" if op == "e" else "decode"
        steps.append(s)
    return steps


# ---------------------------------------------------------------------------------------------------------------------------------
# scenario 7: the entry points mixed on one context

S7 = shp(2, 16, 1024, 4, True)
S7D = shp(1, 24, 2048, 0, False)


def scenario7():
    """the frame steps; the streams are stream_inputs()"""
    return {"first": enc(S7, [1024, 1024, 555], seed=7), "decode": enc(S7D, [2048, 2048, 300, 2048], rot=1, seed=7)}


def stream_inputs():
    """[(pcm, bits, rate, block, preset, ms)]: a stereo 16-bit stream (COMPRESS, a SILENT and a RAW block, a tail) and a mono 24-bit one"""
    a = music(2, 7 * 1024 + 300, 16, seed=70).copy()
    a[:, 2 * 1024:3 * 1024] = 0
    a[:, 4 * 1024:5 * 1024] = np.random.default_rng(7).integers(-32768, 32768, size=(2, 1024))
    b = music(1, 3 * 2048 + 1001, 24, seed=71)
    return [(a, 16, 44100, 1024, 4, True), (b, 24, 48000, 2048, 5, False)]


# ---------------------------------------------------------------------------------------------------------------------------------
# scenario 8: after a refused call

S8 = shp(2, 16, 1024, 4, True)
S8B = shp(1, 16, 2048, 0, False)
SEVENTEEN = [1024 - 8 * i for i in range(17)]


def scenario8():
    """[(name, shape, lengths, the LINNEApiResult documented for it)]: argument errors only"""
    return [("a length of 0", S8, [1024, 0, 777], INVALID_ARGUMENT),
            ("a length above the block", S8, [1024, 1025], INVALID_ARGUMENT),
            ("17 distinct lengths", S8, SEVENTEEN, INVALID_ARGUMENT),
            ("preset 8", shp(2, 16, 1024, 8, True), [1024, 777], INVALID_FORMAT),
            ("a block not longer than a layer's order", shp(2, 16, 64, 4, True), [64, 64], INVALID_FORMAT),
            ("MS with one channel", shp(1, 16, 1024, 4, True), [1024, 777], INVALID_FORMAT)]


def good8(i):
    return enc(S8, [1024, 777, 1024], rot=i, seed=8), enc(S8B, [2048, 1001], rot=i, seed=8)


# ---------------------------------------------------------------------------------------------------------------------------------
# scenario 9: one LINNEEncoder / LINNEDecoder handle, many streams.  handle_sequence() drives any library that exports the LINNE API
# (the reference, when tests/golden/make_reference_golden.py records it; the product, in the GPU test).

STEREO9 = (2, 16, 44100, 1024, 7, True)
MONO9 = (1, 24, 44100, 2048, 7, False)
BLOCKS9 = [1024, 1024, 1024, 1024, 555]


# Noise levels of the 'n' blocks that open streams 1..3, each between two thresholds of the reference's RAW / COMPRESS decision for
# that block: the one with nothing carried (a fresh handle: the block comes out RAW) and the one with the Q2 value the last COMPRESS
# block of the stream BEFORE it left on the handle (COMPRESS).  Found by bisection on the real reference; the recording holds the
# block's type off the used handle, and the CPU test holds it against the oracle's type of the same block off a fresh handle.
AMP9 = [None, 0.551619, 0.718602, 0.729228]


def _mixed(nch, bits, block, nblocks, tail, seed, order, amp=None):
    """blocks of music (c), silence (s), full-scale noise (r: the encoder writes it RAW) and noise at `amp` of full scale (n), then a
    tail of music (a COMPRESS block: what the next stream of the handle finds carried)"""
    x = music(nch, nblocks * block + tail, bits, seed=seed).copy()
    rng = np.random.default_rng(seed)
    for i, k in enumerate(order):
        sl = slice(i * block, (i + 1) * block)
        if k == "s":
            x[:, sl] = 0
        elif k == "r":
            x[:, sl] = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(nch, block))
        elif k == "n":
            x[:, sl] = np.rint(np.random.default_rng(seed + 1000).uniform(-1, 1, size=(nch, block)) * amp * ((1 << (bits - 1)) - 1))
    return x


def handle_inputs():
    """the PCM of the four streams: EncodeWhole stereo, EncodeWhole mono, five EncodeBlock calls stereo, EncodeWhole stereo"""
    return [_mixed(2, 16, 1024, 5, 300, 91, "crcsc"), _mixed(1, 24, 2048, 4, 777, 92, "ncsr", AMP9[1]),
            _mixed(2, 16, 1024, 4, 555, 93, "ncsr", AMP9[2]), _mixed(2, 16, 1024, 4, 129, 94, "nscr", AMP9[3])]


def handle_key(i, x):
    from refs import digest
    return f"handle_sequence/{i}/{x.shape[0]}x{x.shape[1]}/{digest(x)['sha256'][:20]}"


def handle_sequence(api):
    """the four streams of ONE encoder handle of `api` (a LinneApi): EncodeWhole at 16-bit stereo, SetEncodeParameter to 24-bit mono,
    EncodeWhole, SetEncodeParameter back, a header and five EncodeBlock calls, EncodeWhole"""
    import ctypes as C
    from refs import _planar_ptrs, _RefEncodeParameter, _RefHeader
    xs = handle_inputs()
    L = api.L
    enc_h = api.new_encoder(*STEREO9, max_block=2048)
    out = np.zeros(1 << 20, dtype=np.uint8)

    def set_parameter(nch, bits, rate, block, preset, ms):
        par = _RefEncodeParameter(nch, bits, rate, block, preset, int(ms), 0, 0)
        assert L.LINNEEncoder_SetEncodeParameter(enc_h, C.byref(par)) == 0

    def whole(x):
        ptrs, keep = _planar_ptrs(x)
        osz = C.c_uint32(0)
        ret = L.LINNEEncoder_EncodeWhole(enc_h, ptrs, x.shape[1], out.ctypes.data, out.size, C.byref(osz))
        assert ret == 0, f"EncodeWhole -> {ret}"
        return out[:osz.value].tobytes()

    streams = [whole(xs[0])]
    set_parameter(*MONO9)
    streams.append(whole(xs[1]))
    set_parameter(*STEREO9)
    x = xs[2]
    nch, bits, rate, block, preset, ms = STEREO9
    hdr = _RefHeader(1, 2, nch, x.shape[1], rate, bits, block, preset, int(ms))
    assert L.LINNEEncoder_EncodeHeader(C.byref(hdr), out.ctypes.data, out.size) == 0
    off, prog = 30, 0
    for n in BLOCKS9:
        ptrs, keep = _planar_ptrs(x[:, prog:prog + n])
        osz = C.c_uint32(0)
        ret = L.LINNEEncoder_EncodeBlock(enc_h, ptrs, n, out.ctypes.data + off, out.size - off, C.byref(osz))
        assert ret == 0, f"EncodeBlock -> {ret}"
        off += osz.value
        prog += n
    assert prog == x.shape[1]
    streams.append(out[:off].tobytes())
    streams.append(whole(xs[3]))
    L.LINNEEncoder_Destroy(enc_h)
    return streams


DECODE_ORDER9 = [0, 1, 2, 1, 3, 1, 0]      # formats alternate


def decode_through_one_handle(api, streams):
    """[(return code, pcm)] of LINNEDecoder_DecodeWhole of streams[i] for i in DECODE_ORDER9, all through one decoder handle"""
    import ctypes as C
    from refs import _planar_ptrs, _RefDecoderConfig
    cfg = _RefDecoderConfig(2, 5, 128, 1)
    dec = api.L.LINNEDecoder_Create(C.byref(cfg), None, 0)
    assert dec
    got = []
    for i in DECODE_ORDER9:
        data = streams[i]
        buf = np.frombuffer(data, dtype=np.uint8)
        nch, ns = int.from_bytes(data[12:14], "big"), int.from_bytes(data[14:18], "big")
        pcm = np.zeros((nch, ns), dtype=np.int32)
        ptrs, keep = _planar_ptrs(pcm)
        ret = api.L.LINNEDecoder_DecodeWhole(dec, buf.ctypes.data, len(data), ptrs, nch, ns)
        got.append((int(ret), keep))
    api.L.LINNEDecoder_Destroy(dec)
    return got


def block_types(stream):
    """the block type byte of every block of a .lnn stream (0 COMPRESS, 1 SILENT, 2 RAW): sync 0xFFFF, size (4 bytes, of what follows
    it), CRC16, type"""
    out, off = [], 30
    while off < len(stream):
        assert stream[off:off + 2] == b"\xff\xff", off
        size = int.from_bytes(stream[off + 2:off + 6], "big")
        out.append(stream[off + 8])
        off += 6 + size
    return out


FORMAT9 = [STEREO9, MONO9, STEREO9, STEREO9]


ENCODE_SCENARIOS = {1: scenario1, 2: scenario2, 3: scenario3, 4: scenario4, 5: scenario5, 6: scenario6}
