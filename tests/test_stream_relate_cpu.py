"""CPU tests (-m "not gpu") of relating the channels of resident .lnn streams (include/linne_amd.h LINNEAmd_RelateWindowsDevice): the
boundary -- the symbol, the structs, the kinds, the Python entry points, the argument errors that need no device --, LINNE_AMD_PAIR,
the reference the GPU tests hold the library to (relate_refs.expected_relate: numpy and Python integers on the oracle's decode,
checked here against hand-written values), the host helpers correlation and channel_findings, the premises of the GPU tests' fixtures
by the oracle's decode, the host's plan for the per-pair consumer (a stand-alone program, also built with the address and
undefined-behaviour sanitizers, which also shows the bucket records of the older consumers byte for byte) and the command line tool's
-R option as far as it goes without a device."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import linne_amd
import synth_records as sr
from relate_refs import CARRY_NS, CARRY_PEAK, bucket_lengths, carry_stereo_signal, carry_stereo_stream, dots, exact_dot, expected_relate, pairs
from signals import music
from stream_refs import blocks, mixed_signal
from test_cli_cpu import CLI
from test_stream_histogram_cpu import LONG, PLAN_WINDOWS, PROGRAM, THREE, live_in_order
from test_windows_plan_cpu import slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linne_amd", "csrc")
OK, INVALID_ARGUMENT = 0, 1
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300
LO, HI = -(1 << 31), (1 << 31) - 1
WIDE_SHAPE = next(s for s in sr.SHAPES if s.name == "2ch16b1023m4lr")


def wide_cases():
    """the two-channel growth cases whose cascades wrap int32, a tame block in front of them and one behind"""
    cases = sr.table()[WIDE_SHAPE]
    tame = [c for c in cases if c.family == "units"]
    return [tame[0]] + [c for c in cases if c.family == "growth"] + [tame[1]]


def run(*args):
    return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_symbol_structs_and_kinds_are_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bLINNEAmd_RelateWindowsDevice\s*\(", src)
    assert re.search(r"struct\s+LINNEAmdRelation\s*\{", src) and re.search(r"struct\s+LINNEAmdRelateSpec\s*\{", src)
    assert re.search(r"#define\s+LINNE_AMD_NUM_PAIRS\(C\)", src) and re.search(r"#define\s+LINNE_AMD_PAIR\(C,\s*i,\s*j\)", src)
    for name, kind in (("RELATE", 95), ("PRESET", 96), ("COMMIT", 97)):
        assert re.search(r"LINNE_AMD_RELATE_T_%s\s*=\s*%d\b" % (name, kind), src), name
    assert re.search(r"LINNE_AMD_HISTOGRAM_T_COMMIT\s*=\s*94\b", src)                            # no older kind renumbered
    assert "LINNEAmd_RelateWindowsDevice" in linne_amd.AMD_SYMBOLS
    assert hasattr(linne_amd.lib, "LINNEAmd_RelateWindowsDevice")


def test_struct_layouts(tmp_path):
    R, P = linne_amd.Relation, linne_amd.RelateSpec
    assert [(f[0], getattr(R, f[0]).offset) for f in R._fields_] == [("dot_lo", 0), ("dot_hi", 8), ("num_equal", 16), ("num_opposite", 24)]
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == [("bucket_samples", 0), ("d_out", 8), ("pair_stride", 16)]
    assert C.sizeof(R) == 32 and C.sizeof(P) == 24
    d = linne_amd.RELATION_DTYPE
    assert d.itemsize == 32 and [(n, d.fields[n][1], d.fields[n][0].str) for n in d.names] == \
        [("dot_lo", 0, "<u8"), ("dot_hi", 8, "<i8"), ("num_equal", 16, "<u8"), ("num_opposite", 24, "<u8")]
    # and the C compiler's view of the header
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
    if cc:
        src, exe = tmp_path / "size.c", tmp_path / "size"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "linne_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                       'sizeof(struct LINNEAmdRelation), sizeof(struct LINNEAmdRelateSpec), offsetof(struct LINNEAmdRelation, dot_hi), '
                       'offsetof(struct LINNEAmdRelation, num_opposite), offsetof(struct LINNEAmdRelateSpec, d_out), offsetof(struct LINNEAmdRelateSpec, pair_stride)); return 0; }\n')
        b = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["32", "24", "8", "24", "8", "16"]


def test_pair_macro_enumerates_the_upper_triangle(tmp_path):
    for n in range(1, 9):
        assert [linne_amd.pair_index(n, i, j) for i, j in pairs(n)] == list(range(n * (n + 1) // 2))
    for bad in ((2, 1, 0), (2, 0, 2), (3, -1, 0)):
        with pytest.raises(AssertionError):
            linne_amd.pair_index(*bad)
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
    if cc:
        src, exe = tmp_path / "pair.c", tmp_path / "pair"
        src.write_text('#include <stdio.h>\n#include <stdint.h>\n#include "linne_amd.h"\nint main(void) { uint32_t c, i, j; for (c = 1; c <= 8; c++) { printf("%u:", (unsigned)LINNE_AMD_NUM_PAIRS(c)); '
                       'for (i = 0; i < c; i++) for (j = i; j < c; j++) printf(" %u", (unsigned)LINNE_AMD_PAIR(c, i, j)); printf("\\n"); } return 0; }\n')
        b = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        lines = subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines()
        assert lines == ["%d: %s" % (n * (n + 1) // 2, " ".join(str(p) for p in range(n * (n + 1) // 2))) for n in range(1, 9)]
        assert lines[7].startswith("36:")


def test_python_entry_points():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(linne_amd.Context.relate_windows)
    assert list(p) == ["self", "windows", "bucket_samples", "group_frames", "return_codes"]
    assert [p[k].default for k in ("bucket_samples", "group_frames", "return_codes")] == [0, 0, False]
    p = sig(linne_amd.Context.relate_streams)
    assert list(p) == ["self", "streams", "bucket_samples", "group_frames"] and [p[k].default for k in ("bucket_samples", "group_frames")] == [0, 0]
    assert list(sig(linne_amd.pair_index)) == ["C", "i", "j"]
    assert list(sig(linne_amd.correlation)) == ["relation"] and list(sig(linne_amd.channel_findings)) == ["relation"]
    assert callable(linne_amd.Relations.dot) and callable(linne_amd.Relations.cpu)


def test_null_arguments_need_no_device():
    f = linne_amd.lib.LINNEAmd_RelateWindowsDevice
    w = (linne_amd.Window * 2)()
    s = (linne_amd.RelateSpec * 2)()
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


def row(t, p, k=0):
    r = t[p, k]
    return (int(r["dot_hi"]) << 64) + int(r["dot_lo"]), int(r["num_equal"]), int(r["num_opposite"])


def test_the_reference_against_hand_written_values():
    # INT32_MIN against itself: product 2^62, equal, not opposite (its negation is no int32); against INT32_MAX: neither
    t = expected_relate(np.array([[LO], [LO], [HI]], dtype=np.int32), 0, 1)
    assert t.shape == (6, 1) and t.dtype == linne_amd.RELATION_DTYPE
    assert row(t, 0) == (1 << 62, 1, 0) and row(t, 1) == (1 << 62, 1, 0)
    assert row(t, 2) == (-(1 << 31) * ((1 << 31) - 1), 0, 0) and row(t, 5) == (((1 << 31) - 1) ** 2, 1, 0)
    assert (int(t[2, 0]["dot_hi"]), int(t[2, 0]["dot_lo"])) == (-1, (1 << 64) - (1 << 31) * ((1 << 31) - 1))     # the two's complement, word by word
    # INT32_MAX against its negation is opposite
    t = expected_relate(np.array([[HI, HI], [-HI, HI]], dtype=np.int32), 0, 2)
    assert row(t, 1) == (0, 1, 1) and row(t, 0) == (2 * HI * HI, 2, 0)
    # a sum below -2^64: 8 products of -2^62
    t = expected_relate(np.array([[LO] * 8, [-LO - 1] * 8], dtype=np.int64).astype(np.int32), 0, 8)
    assert row(t, 1)[0] == 8 * LO * HI < -(1 << 64) and int(t[1, 0]["dot_hi"]) == -2
    t = expected_relate(np.array([[LO] * 9], dtype=np.int32), 0, 9)
    assert row(t, 0) == (9 << 62, 9, 0) and (int(t[0, 0]["dot_hi"]), int(t[0, 0]["dot_lo"])) == (2, 1 << 62)    # above 2^65
    # a frame of zeros counts as equal and as opposite in every pair, the diagonal included
    full = np.array([[3, 0, -4, 0, 7, 7, -1], [3, 0, 4, 5, -7, 7, 1], [0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    t = expected_relate(full, 0, 7)
    assert [row(t, p) for p in range(6)] == [(9 + 16 + 49 + 49 + 1, 7, 2), (9 - 16 - 49 + 49 - 1, 3, 4), (0, 2, 2),
                                             (9 + 16 + 25 + 49 + 49 + 1, 7, 1), (0, 1, 1), (0, 7, 7)]
    t = expected_relate(full, 1, 5, 2)                           # buckets [1, 3) [3, 5) [5, 6): the last one short
    assert t.shape == (6, 3) and [row(t, 1, k) for k in range(3)] == [(-16, 1, 2), (-49, 0, 1), (49, 1, 0)]
    assert [row(t, 0, k)[1] for k in range(3)] == bucket_lengths(5, 2) == [2, 2, 1]
    assert expected_relate(full, 3, 0, 4).shape == (6, 0) and expected_relate(full[:1], 6, 1, 5000).shape == (1, 1)
    assert exact_dot([LO] * 5, [LO] * 5) == 5 << 62 and exact_dot([], []) == 0 and exact_dot([-1, 2], [3, 4]) == 5
    assert dots(t)[1] == [-16, -49, 49]


def table_of(rows_):
    """a RELATION_DTYPE table (P, nb) from [P][nb] tuples (dot, equal, opposite)"""
    t = np.zeros((len(rows_), len(rows_[0])), dtype=linne_amd.RELATION_DTYPE)
    for p, r in enumerate(rows_):
        for k, (d, e, o) in enumerate(r):
            t[p, k] = (d & ((1 << 64) - 1), d >> 64, e, o)
    return t


def test_correlation_and_findings_on_hand_tables():
    # stereo, three buckets of 10 frames: identical; inverted; unrelated with a silent right channel
    t = table_of([[(400, 10, 0), (400, 10, 0), (90, 10, 1)], [(400, 10, 0), (-400, 0, 10), (0, 1, 1)], [(400, 10, 0), (400, 10, 0), (0, 10, 10)]])
    c = linne_amd.correlation(t)
    assert c.shape == (2, 2, 3) and c.dtype == np.float64
    assert c[:, :, 0].tolist() == [[1.0, 1.0], [1.0, 1.0]] and c[:, :, 1].tolist() == [[1.0, -1.0], [-1.0, 1.0]]
    assert c[0, 0, 2] == 1.0 and np.isnan(c[0, 1, 2]) and np.isnan(c[1, 0, 2]) and np.isnan(c[1, 1, 2])
    f = linne_amd.channel_findings(t)
    assert [x["pairs"][(0, 1)] for x in f] == ["identical", "inverted", None]
    assert [x["channels"] for x in f] == [{0: None, 1: None}, {0: None, 1: None}, {0: None, 1: "silent"}]
    # two silent channels are identical, not inverted; sums beyond float64's integers still divide exactly
    big = 1 << 100
    t = table_of([[(0, 5, 5)], [(0, 5, 5)], [(0, 1, 1)], [(0, 5, 5)], [(0, 1, 1)], [(big, 5, 1)]])      # (the third channel is zero in one frame)
    f, = linne_amd.channel_findings(t)
    assert f["pairs"] == {(0, 1): "identical", (0, 2): None, (1, 2): None} and f["channels"] == {0: "silent", 1: "silent", 2: None}
    assert np.isnan(linne_amd.correlation(t)[0, 1, 0]) and linne_amd.correlation(t)[2, 2, 0] == 1.0
    t = table_of([[(big + 1, 5, 0)], [(-(big // 2), 0, 0)], [(big - 1, 5, 0)]])
    assert math.isclose(linne_amd.correlation(t)[0, 1, 0], -0.5, rel_tol=1e-15)
    assert linne_amd.relation_dots(t) == [[big + 1], [-(big // 2)], [big - 1]]
    # the helpers read the reference's tables too
    x = np.array([[1, 2, 3, 4], [2, 4, 6, 8], [-1, -2, -3, -4]], dtype=np.int32)
    t = expected_relate(x, 0, 4)
    c = linne_amd.correlation(t)[:, :, 0]
    assert np.allclose(c, [[1, 1, -1], [1, 1, -1], [-1, -1, 1]], rtol=0, atol=1e-15)
    assert linne_amd.channel_findings(t)[0]["pairs"] == {(0, 1): None, (0, 2): "inverted", (1, 2): None}


def wave_widths(full, block):
    """per wave of 64 frames of the kernel's walk (blocks of `block` frames cut into pieces of 256 and waves of 64): how many of its
    values have a magnitude above 2^23, and how many it holds"""
    out = []
    for at in range(0, full.shape[1], block):
        for a in range(at, min(at + block, full.shape[1]), 64):
            w = np.abs(full[:, a:min(a + 64, at + block, full.shape[1])].astype(np.int64))
            out.append((int((w > 1 << 23).sum()), w.size))
    return out


def first_wide_frame(full):
    """the first sample frame with a value of magnitude above 2^23"""
    return int(np.flatnonzero((np.abs(np.asarray(full).astype(np.int64)) > 1 << 23).any(axis=0))[0])


def test_premises_of_the_gpu_fixtures(oracle, record_property):
    # the mixed stream's block types
    x = mixed_signal(2, 16, 7 * S + TAIL, seed=11, block=S)
    bl = blocks(bytes(oracle.encode_whole(x, 16, 44100, S, 5, True)))
    assert [b[2] for b in bl] == [COMPRESS, SILENT, SILENT, COMPRESS, RAW, RAW, COMPRESS, COMPRESS] and bl[-1][3] == TAIL
    # the carry stream: RAW blocks, R = -L, sums beyond +-2^64
    stream = carry_stereo_stream(oracle)
    ret, full, _ = oracle.decode_whole(stream)
    assert ret == OK and np.array_equal(full, carry_stereo_signal()) and full.shape == (2, CARRY_NS)
    assert len(blocks(stream)) == 257 and all(b[2] == RAW for b in blocks(stream))
    t = expected_relate(full, 0, CARRY_NS)
    assert row(t, 1) == (-CARRY_NS * CARRY_PEAK ** 2, 0, CARRY_NS) and row(t, 1)[0] < -(1 << 64)
    assert row(t, 0) == (CARRY_NS * CARRY_PEAK ** 2, CARRY_NS, 0) == row(t, 2) and row(t, 0)[0] > 1 << 64
    assert int(t[1, 0]["dot_hi"]) == -2 and int(t[0, 0]["dot_hi"]) == 1
    # the wide-value stream: a 16-bit header, values of magnitude 2^24 or more in both channels, and waves of every kind
    cases = wide_cases()
    ret, full, _ = oracle.decode_whole(sr.case_stream(WIDE_SHAPE, cases))
    assert ret == OK and full.shape[0] == 2 and WIDE_SHAPE.bits == 16
    mag = np.abs(full.astype(np.int64))
    record_property("widest_value", int(mag.max()))
    print("the wide-value stream's widest magnitude per channel:", mag.max(axis=1).tolist())
    assert (mag.max(axis=1) >= 1 << 24).all(), mag.max(axis=1)
    assert mag.max() > 1 << 30                                   # the cascades wrap: values over all of int32
    ww = wave_widths(full, WIDE_SHAPE.block)
    assert any(w == 0 for w, n in ww) and any(w == n for w, n in ww)
    assert any(0 < w < n for w, n in ww), "no wave holds wide values among narrow ones"
    # the table has no wave with a single wide value, but a window that ends behind the stream's first wide frame has one: the frames
    # in front of it are narrow, and the lanes behind a window's end hold nothing
    f = first_wide_frame(full)
    assert f > 300 and (mag[:, f - 300:f] <= 1 << 23).all() and (mag[:, f] > 1 << 23).any()
    # dual mono and inverted stereo survive the encoder
    m = music(1, 2 * S + TAIL, 16, seed=5)
    for x, ms in ((np.concatenate([m, m]), True), (np.concatenate([m, -m]), False)):
        ret, full, _ = oracle.decode_whole(bytes(oracle.encode_whole(x, 16, 44100, S, 2, ms)))
        assert ret == OK and np.array_equal(full, x)


# ---- the plan ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("relate_plan")
    src = str(d / "plan.cpp")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    exes = []
    for name, extra in (("plan", []), ("plan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        b = subprocess.run(cmd + ["-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        exes.append(exe)
    return exes


def plan(programs, gf, bucketing):
    streams = [LONG, THREE]
    text = ["%d %d %d %d" % (gf, bucketing, len(streams), len(PLAN_WINDOWS))]
    for s in streams:
        text.append("%d %d %d %d %d %d %d" % (s["C"], s["bits"], s["S"], len(s["blocks"]), s["covered"], s["bytes"], s["address"]))
        text += ["%d %d %d %d %d" % b for b in s["blocks"]]
    text += [" ".join(str(v) for v in w) for w in PLAN_WINDOWS]
    outs = []
    for exe in programs:
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = [x.split() for x in outs[0].splitlines()]
    return [int(v) for v in lines[0][1:]], [bytes.fromhex(x[1]) for x in lines[1:]]


def geometry(i):
    k, lo, n, b, cs, out, *_ = PLAN_WINDOWS[i]
    b_ = n if b == 0 or b > n else b
    return (LONG, THREE)[k], n, b_, -(-n // b_), slots(b_), cs, out


@pytest.mark.parametrize("gf", [0, 2])
def test_plan_of_the_per_pair_consumer(programs, gf):
    """bucketing kind 5: an accumulator and an output record per (pair, bucket), a window's slots P * nb apart; the pair count travels
    in the record's last word, the other fields are per channel's"""
    assert re.search(r"WX_BUCKETS_PER_PAIR\s*=\s*5\b", open(os.path.join(CSRC, "lnn_windows_plan.h")).read())
    (nacc, nout, size), recs = plan(programs, gf, 5)
    assert size == 64
    a = o = 0
    for raw, i in zip(recs, live_in_order()):
        s, n, b_, nb, ns, cs, out = geometry(i)
        P = s["C"] * (s["C"] + 1) // 2
        assert raw == struct.pack("<QQQQQQIIII", out, b_, nb, a, o, cs, ns, i, s["C"], P), i
        a += ns * P * nb
        o += P * nb
    assert (nacc, nout) == (a, o)
    assert a == 32 * 3 + 2 * 3 * 3 + 4 * 3 + 6 * 15 + 6 * 192 + 6                                   # the long buckets' slots; 3 pairs and 6


@pytest.mark.parametrize("gf", [0, 2])
def test_records_of_the_older_consumers_are_byte_for_byte_what_they_were(programs, gf):
    """kinds 1 to 4 against a restatement, written here in Python, of what the header filled before kind 5 existed -- not against the
    parent commit's header itself, which a test cannot reach.  A guard for later changes: it passes on the parent commit too"""
    order = live_in_order()
    for kind in (1, 4):                                          # per channel; per bin
        (nacc, nout, _), recs = plan(programs, gf, kind)
        a = o = 0
        for raw, i in zip(recs, order):
            s, n, b_, nb, ns, cs, out = geometry(i)
            bins, shift, scale = PLAN_WINDOWS[i][6:9]
            units, last = (1, 0) if kind == 1 else (bins, bins | shift << 16 | scale << 24)
            assert raw == struct.pack("<QQQQQQIIII", out, b_, nb, a, o, cs, ns, i, s["C"], last), (kind, i)
            a += ns * s["C"] * nb * units
            o += s["C"] * nb * units
        assert (nacc, nout) == (a, o)
    (nacc, nout, _), recs = plan(programs, gf, 2)               # per frame
    a = o = 0
    for raw, i in zip(recs, order):
        s, n, b_, nb, ns, cs, out = geometry(i)
        sstride = (nb + 15) & ~15
        assert raw == struct.pack("<QQQQQQIIII", out, b_, nb, a, o, n, ns, i, s["C"] * ((s["bits"] + 7) // 8), sstride), i
        a += ns * sstride if ns > 1 else nb
        o += nb
    assert (nacc, nout) == (a, o)
    (nacc, nout, _), recs = plan(programs, gf, 3)               # bitmask
    a = o = 0
    for raw, i in zip(recs, order):
        k, lo, n, b, cs, out, bins, shift, scale, qm, qc, qt = PLAN_WINDOWS[i]
        assert raw == struct.pack("<QQQQQQIIII", out, qm, qc, a, o, n, qt, i, (LONG, THREE)[k]["C"], 0), i
        a += -(-n // 64)
        o += -(-(-(-n // 64)) // 256)
    assert (nacc, nout) == (a + 3 * o + 1, o)


# ---- the tool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_cli_usage_and_option_errors(oracle, tmp_path):
    text = run("-h").stdout
    assert re.search(r"-R, --relate\b", text) and "-R [BUCKET_SAMPLES] STREAM.lnn" in text
    for args in (("-R",), ("-R", "-e", "a", "b"), ("-R", "-d", "a"), ("-R", "-M", "a"), ("-R", "-D", "a"), ("-R", "-V", "a"), ("-M", "-R", "a"), ("-D", "-R", "a"),
                 ("-R", "-S", "0", "a"), ("-R", "-L", "64", "a"), ("-r", "-R", "a", "b"), ("-C", "-R", "a", "b"), ("--relate", "1", "a", "b"), ("-R", "--batch", "d", "a"),
                 ("-R", "x", "a.lnn"), ("-R", "0", "a.lnn"), ("-R", "12x", "a.lnn"), ("-R", "-5", "a.lnn")):
        r = run(*args)
        assert r.returncode == 1 and r.stderr.strip() and not r.stdout, args
    assert "bucket sample count is out of range" in run("-R", "0", "a.lnn").stderr
    assert "no other mode" in run("-R", "-M", "a").stderr and "-R takes" in run("-R").stderr
    for args in (("-R", "/nonexistent/a.lnn"), ("--relate", "441", "/nonexistent/a.lnn")):
        r = run(*args)
        assert r.returncode == 1 and "Failed to open" in r.stderr, args
    # a file that is no stream is refused before a device is asked for; a stream either answers or fails with a message
    junk, lnn = tmp_path / "junk.lnn", tmp_path / "a.lnn"
    junk.write_bytes(b"RIFF" + bytes(100))
    r = run("-R", str(junk))
    assert r.returncode == 1 and "Failed to get header information" in r.stderr
    x = np.concatenate([np.zeros((2, 1000), dtype=np.int32), music(2, 1500, 16, seed=3)], axis=1)
    lnn.write_bytes(bytes(oracle.encode_whole(x, 16, 22050, 500, 4, True)))
    r = run("-R", "441", str(lnn))
    assert r.returncode in (0, 1), (r.returncode, r.stderr)      # (a signal would be negative)
    if r.returncode == 1:
        assert "Failed to create a device context" in r.stderr, r.stderr
