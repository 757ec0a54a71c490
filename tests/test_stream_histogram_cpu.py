"""CPU tests (-m "not gpu") of histogramming the sample levels of resident .lnn streams (include/linne_amd.h
LINNEAmd_HistogramWindowsDevice): the boundary -- the symbol, the struct, the kinds, the Python entry points, the argument errors that
need no device --, the reference the GPU tests hold the library to (expected_histogram: numpy.bincount on the oracle's decode, checked
here against hand-written values), level_threshold, the premises of the GPU tests' fixtures by the oracle's decode, the host's plan for
the per-bin consumer (a stand-alone program, also built with the address and undefined-behaviour sanitizers, which also shows the
bucket records of the older consumers byte for byte) and the command line tool's -L option as far as it goes without a device."""
import ctypes as C
import inspect
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import linne_amd
from signals import music
from stream_refs import bins_of, blocks, expected_histogram, mixed_signal  # noqa: F401
from test_cli_cpu import CLI
from test_windows_plan_cpu import slots, stream as plan_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linne_amd", "csrc")
OK, INVALID_ARGUMENT = 0, 1
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300
CONSTANT = 1000                             # the constant track's value
LO, HI = -(1 << 31), (1 << 31) - 1


def constant_signal(nch, ns, value=CONSTANT):
    return np.full((nch, ns), value, dtype=np.int32)


def run(*args):
    return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_symbol_struct_and_kinds_are_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bLINNEAmd_HistogramWindowsDevice\s*\(", src)
    assert re.search(r"struct\s+LINNEAmdHistogramSpec\s*\{", src)
    for name, kind in (("HISTOGRAM", 92), ("PRESET", 93), ("COMMIT", 94)):
        assert re.search(r"LINNE_AMD_HISTOGRAM_T_%s\s*=\s*%d\b" % (name, kind), src), name
    assert re.search(r"LINNE_AMD_HIST_LINEAR\s*=\s*0\b", src) and re.search(r"LINNE_AMD_HIST_LOG2\s*=\s*1\b", src)
    assert re.search(r"#define\s+LINNE_AMD_HIST_MAX_BINS\s+1024\b", src)
    assert re.search(r"LINNE_AMD_QUIET_T_ENDS\s*=\s*91\b", src)                                  # no older kind renumbered
    assert "LINNEAmd_HistogramWindowsDevice" in linne_amd.AMD_SYMBOLS
    assert hasattr(linne_amd.lib, "LINNEAmd_HistogramWindowsDevice")
    assert (linne_amd.HIST_LINEAR, linne_amd.HIST_LOG2, linne_amd.HIST_MAX_BINS) == (0, 1, 1024)


def test_struct_layout(tmp_path):
    P = linne_amd.HistogramSpec
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == [("bucket_samples", 0), ("num_bins", 8), ("shift", 12), ("scale", 16), ("reserved", 20),
                                                                    ("d_out", 24), ("channel_stride", 32)]
    assert C.sizeof(P) == 40
    # and the C compiler's view of the header
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
    if cc:
        src, exe = tmp_path / "size.c", tmp_path / "size"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "linne_amd.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(struct LINNEAmdHistogramSpec), '
                       'offsetof(struct LINNEAmdHistogramSpec, d_out), offsetof(struct LINNEAmdHistogramSpec, reserved)); return 0; }\n')
        b = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["40", "24", "20"]


def test_python_entry_points():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(linne_amd.Context.histogram_windows)
    assert list(p) == ["self", "windows", "num_bins", "shift", "log2", "bucket_samples", "group_frames", "return_codes"]
    assert [p[k].default for k in ("shift", "log2", "bucket_samples", "group_frames", "return_codes")] == [0, False, 0, 0, False]
    assert p["num_bins"].default is inspect.Parameter.empty
    p = sig(linne_amd.Context.histogram_streams)
    assert list(p) == ["self", "streams", "num_bins", "shift", "log2", "bucket_samples", "group_frames"]
    p = sig(linne_amd.level_threshold)
    assert list(p) == ["counts", "fraction", "shift"] and p["shift"].default == 0
    h = linne_amd.Histogram("counts", 33, 4, True, 441)
    assert (h.counts, h.num_bins, h.shift, h.log2, h.bucket_samples) == ("counts", 33, 4, True, 441) and callable(h.cpu)


def test_null_arguments_need_no_device():
    f = linne_amd.lib.LINNEAmd_HistogramWindowsDevice
    w = (linne_amd.Window * 2)()
    s = (linne_amd.HistogramSpec * 2)()
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
    ext = np.array([LO, HI, 0, 1, -1], dtype=np.int32)
    # shift 0, linear: |INT32_MIN| = 2^31 is taken in 64 bits, one above |INT32_MAX|
    assert list(bins_of(ext, 1 << 40, 0, False)) == [1 << 31, (1 << 31) - 1, 0, 1, 1]
    assert list(bins_of(ext, 1024, 0, False)) == [1023, 1023, 0, 1, 1]                          # the catch-all bin
    # shift 31: INT32_MIN alone reaches m = 1
    assert list(bins_of(ext, 1024, 31, False)) == [1, 0, 0, 0, 0]
    assert list(bins_of(ext, 1024, 31, True)) == [1, 0, 0, 0, 0]
    # log2 at shift 0: the bit length, 32 for INT32_MIN, 31 for INT32_MAX, 0 for 0
    assert list(bins_of(ext, 64, 0, True)) == [32, 31, 0, 1, 1]
    assert list(bins_of(ext, 33, 0, True)) == [32, 31, 0, 1, 1] and list(bins_of(ext, 32, 0, True)) == [31, 31, 0, 1, 1]
    assert list(bins_of([1, 2, 3, 4, 7, 8, 255, 256, -256, 32767, -32768], 64, 0, True)) == [1, 2, 2, 3, 3, 4, 8, 9, 9, 15, 16]
    assert list(bins_of([15, 16, 31, 32, -47, -48], 64, 4, False)) == [0, 1, 1, 2, 2, 3]
    assert list(bins_of([15, 16, 31, 32, -47, -48, 64], 64, 4, True)) == [0, 1, 1, 2, 2, 2, 3]
    assert list(bins_of([15, 16, 31, 32, -47, -48, 64], 2, 4, True)) == [0, 1, 1, 1, 1, 1, 1]       # two bins: below 2^shift, and the rest
    assert list(bins_of(ext, 1, 0, False)) == [0] * 5 and list(bins_of(ext, 1, 7, True)) == [0] * 5   # one bin takes everything
    full = np.array([[3, -4, 0, 7, 7, -1, 2], [LO, HI, 5, 5, 5, 5, 5]], dtype=np.int32)
    h = expected_histogram(full, 0, 7, 8)
    assert h.shape == (2, 1, 8) and h.dtype == np.int64
    assert h[0, 0].tolist() == [1, 1, 1, 1, 1, 0, 0, 2] and h[1, 0].tolist() == [0, 0, 0, 0, 0, 5, 0, 2]
    h = expected_histogram(full, 1, 5, 4, b=2)                   # buckets [1, 3) [3, 5) [5, 6): the last one short
    assert h.shape == (2, 3, 4) and h[0].tolist() == [[1, 0, 0, 1], [0, 0, 0, 2], [0, 1, 0, 0]] and h[1].tolist() == [[0, 0, 0, 2], [0, 0, 0, 2], [0, 0, 0, 1]]
    assert expected_histogram(full, 1, 5, 4, b=2).sum(axis=2).tolist() == [[2, 2, 1]] * 2       # the bins of a bucket add up to its samples
    assert expected_histogram(full, 0, 7, 5, log2=True)[:, 0].tolist() == [[1, 1, 2, 3, 0], [0, 0, 0, 5, 2]]
    assert expected_histogram(full, 0, 7, 2, shift=2)[:, 0].tolist() == [[4, 3], [0, 7]]
    assert expected_histogram(full, 3, 0, 4, b=4).shape == (2, 0, 4)                             # no samples: no buckets
    assert expected_histogram(full, 6, 1, 3, b=5000)[:, 0].tolist() == [[0, 0, 1], [0, 0, 1]]


def test_level_threshold():
    f = linne_amd.level_threshold
    c = [16, 16, 32, 64]                                         # 128 samples; the last bin holds everything above
    assert f(c, 0.0) == 0 and f(c, 0.125) == 0 and f(c, 0.126) == 1 and f(c, 0.25) == 1 and f(c, 0.26) == 2 and f(c, 0.375) == 2 and f(c, 0.5) == 2
    assert f(c, 0.51) is None and f(c, 1.0) is None              # that bin is the catch-all
    assert f([16, 16, 32, 0], 1.0) == 2 and f([16, 16, 32, 0], 0.95) == 2                        # nothing above: the last real bin answers
    assert f(c, 0.25, shift=4) == 31 and f(c, 0.0, shift=4) == 15 and f(c, 0.5, shift=31) == (3 << 31) - 1   # T = ((j + 1) << shift) - 1
    assert f([5], 0.5) is None and f([5], 0.0) is None           # one bin is the catch-all
    assert f([0, 0, 7, 0], 0.5) == 2 and f([0, 0, 0, 0], 0.5) == 0
    assert f(np.array(c, dtype=np.int64), 0.25) == 1 and isinstance(f(np.array([1, 0]), 1.0), int)
    assert f(np.array([[16, 16], [48, 48]]).sum(axis=0), 0.5) == 0                                 # the sum over channels
    big = [(1 << 32) - 1, 1, 0]
    assert f(big, 1.0) == 1 and f(big, 0.5) == 0                 # "all of them" is exact in integers


def test_premises_of_the_gpu_fixtures(oracle):
    """the constant track decodes to its one value from COMPRESS blocks (not SILENT, not RAW); the mixed stream's block types"""
    for nch in (1, 2):
        x = constant_signal(nch, 3 * S + TAIL)
        stream = bytes(oracle.encode_whole(x, 16, 44100, S, 0, nch == 2))
        ret, full, _ = oracle.decode_whole(stream)
        assert ret == OK and np.array_equal(full, x) and set(np.unique(full)) == {CONSTANT}
        assert [b[2] for b in blocks(stream)] == [COMPRESS] * 4
        h = expected_histogram(full, 0, full.shape[1], 1024)
        assert h[:, 0, CONSTANT].tolist() == [3 * S + TAIL] * nch and h.sum() == nch * (3 * S + TAIL)
    x = mixed_signal(2, 16, 7 * S + TAIL, seed=11, block=S)
    bl = blocks(bytes(oracle.encode_whole(x, 16, 44100, S, 5, True)))
    assert [b[2] for b in bl] == [COMPRESS, SILENT, SILENT, COMPRESS, RAW, RAW, COMPRESS, COMPRESS] and bl[-1][3] == TAIL
    # log2 with two bins on music: one bin takes (nearly) everything
    h = expected_histogram(music(2, 4 * S, 16, seed=9), 0, 4 * S, 2, log2=True)
    assert (h[:, 0, 1] > 0.9 * 4 * S).all()


# ---- the plan ------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "lnn_windows_plan.h"
/* stdin: group_frames bucketing nstreams nwindows; per stream: C bits S nb covered stream_bytes address, then nb x (off first size type
 * nsmp); per window: stream lo n bucket_samples cstride out bins shift scale quiet_min quiet_capacity quiet_threshold */
struct Stream { WxIndexView x; std::vector<uint64_t> off, first; std::vector<uint32_t> size, type, nsmp; unsigned long long address; };
int main(void)
{
    unsigned gf, bucketing, ns, nw;
    if (scanf("%u %u %u %u", &gf, &bucketing, &ns, &nw) != 4) return 2;
    std::vector<Stream> st(ns);
    for (Stream &s : st) {
        unsigned long long covered, bytes;
        memset(&s.x, 0, sizeof(s.x));
        if (scanf("%u %u %u %u %llu %llu %llu", &s.x.shape.num_channels, &s.x.shape.bits_per_sample, &s.x.shape.num_samples_per_block, &s.x.nb, &covered, &bytes, &s.address) != 7) return 2;
        s.x.covered = covered; s.x.stream_bytes = bytes;
        for (uint32_t r = 0; r < s.x.nb; r++) {
            unsigned long long off, first; unsigned size, type, nsmp;
            if (scanf("%llu %llu %u %u %u", &off, &first, &size, &type, &nsmp) != 5) return 2;
            s.off.push_back(off); s.first.push_back(first); s.size.push_back(size); s.type.push_back(type); s.nsmp.push_back(nsmp);
        }
        s.x.h_off = s.off.data(); s.x.h_first = s.first.data(); s.x.h_size = s.size.data(); s.x.h_type = s.type.data(); s.x.h_nsmp = s.nsmp.data();
    }
    std::vector<WxRange> rg(nw);
    for (WxRange &r : rg) {
        unsigned k, bins, shift, scale, qt; unsigned long long lo, n, b, cs, out, qm, qc;
        if (scanf("%u %llu %llu %llu %llu %llu %u %u %u %llu %llu %u", &k, &lo, &n, &b, &cs, &out, &bins, &shift, &scale, &qm, &qc, &qt) != 12 || k >= ns) return 2;
        memset(&r, 0, sizeof(r));
        r.x = st[k].x; r.stream = (const uint8_t *)(uintptr_t)st[k].address; r.lo = lo; r.n = n; r.live = n != 0;
        r.bucket_samples = b; r.bucket_cstride = cs; r.bucket_out = (void *)(uintptr_t)out; r.hist = WXH_SPEC(bins, shift, scale);
        r.quiet_min = qm; r.quiet_capacity = qc; r.quiet_threshold = qt;
        r.fmt = LINNE_AMD_PCM_S32; r.sstride = 1; r.stride = n;
        if (n) r.r1 = (lo + n - 1u < r.x.covered) ? wx_block_of(r.x.h_first, r.x.nb, lo + n - 1u) : r.x.nb;
    }
    WxPlanned p;
    if (wx_plan_count(rg.data(), nw, gf, p) != WXP_OK) return 3;
    /* exactly the reserved sizes, from the heap: the sanitizer build sees a record written past them */
    std::vector<WxWindow> win(p.nlive); std::vector<WxBucket> side(p.nlive); std::vector<WxBlock> rec(p.total_rec); std::vector<uint32_t> crec(p.total_crec);
    wx_plan_fill(rg.data(), nw, gf, (WxBucketing)bucketing, p, win.data(), side.data(), rec.data(), crec.data());
    printf("fill %llu %llu %zu\n", (unsigned long long)p.nacc, (unsigned long long)p.nout, sizeof(WxBucket));
    for (const WxBucket &m : side) {
        printf("bucket ");
        for (size_t j = 0; j < sizeof(m); j++) printf("%02x", ((const unsigned char *)&m)[j]);
        printf(" %u %u %u\n", WXH_BINS(m.hist), WXH_SHIFT(m.hist), WXH_LOG2(m.hist));
    }
    return 0;
}
"""
LONG = plan_stream(2, 16, 4096, [SILENT] * 40, [5] * 40, 0x30000)
THREE = plan_stream(3, 8, 64, [COMPRESS, RAW, COMPRESS], [40, 198, 33], 0x40000 + 5)
# (stream, lo, n, bucket_samples, channel_stride, d_out, num_bins, shift, scale, quiet min, capacity, threshold)
PLAN_WINDOWS = [(0, 0, 40 * 4096, 0, 1, 0x1000, 1024, 0, 0, 1, 5, 7), (1, 3, 100, 7, 20, 0x2000, 1, 31, 1, 2, 6, 8), (0, 5, 0, 3, 0, 0, 9, 9, 0, 1, 1, 1),
                (1, 0, 192, 1, 192, 0x3000, 33, 4, 1, 3, 7, 9), (0, 100, 20000, 8192, 3, 0x4000, 65, 15, 0, 4, 8, 10), (1, 64, 64, 64, 1, 0x5000, 2, 0, 0, 5, 9, 1 << 31),
                (0, 0, 16384, 16384, 1, 0x6000, 64, 5, 1, 6, 10, 12)]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("histogram_plan")
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
    fill = [int(v) for v in lines[0][1:]]
    return fill, [(bytes.fromhex(x[1]), tuple(int(v) for v in x[2:])) for x in lines[1:]]


def live_in_order():
    """the live windows' numbers as the plan takes them: the groups in order of first appearance, a group's windows in the caller's"""
    live = [i for i, w in enumerate(PLAN_WINDOWS) if w[2]]
    return [i for k in dict.fromkeys(PLAN_WINDOWS[i][0] for i in live) for i in live if PLAN_WINDOWS[i][0] == k]


@pytest.mark.parametrize("gf", [0, 2])
def test_plan_of_the_per_bin_consumer(programs, gf):
    """bucketing kind 4: the accumulators as per channel with num_bins units where that has one, an output record per bin; bins, shift
    and scale travel in the record's last word, the other fields are per channel's"""
    (nacc, nout, size), recs = plan(programs, gf, 4)
    assert size == 64
    a = o = 0
    for (raw, spec), i in zip(recs, live_in_order()):
        k, lo, n, b, cs, out, bins, shift, scale, *_ = PLAN_WINDOWS[i]
        C_ = (LONG, THREE)[k]["C"]
        b_ = n if b == 0 or b > n else b
        nb, ns = -(-n // b_), slots(b_)
        assert spec == (bins, shift, scale)
        assert raw == struct.pack("<QQQQQQIIII", out, b_, nb, a, o, cs, ns, i, C_, bins | shift << 16 | scale << 24), i
        a += ns * C_ * nb * bins
        o += C_ * nb * bins
    assert (nacc, nout) == (a, o)
    assert a == 32 * 2 * 1024 + 2 * 2 * 3 * 65 + 4 * 2 * 64 + 3 * 15 + 3 * 192 * 33 + 3 * 2         # the long buckets' slots, mixed num_bins


@pytest.mark.parametrize("gf", [0, 2])
def test_records_of_the_older_consumers_are_byte_for_byte_what_they_were(programs, gf):
    """kinds 1, 2 and 3 against a restatement of what they filled before kind 4 existed; a histogram spec beside them changes nothing"""
    order = live_in_order()
    # per channel
    (nacc, nout, _), recs = plan(programs, gf, 1)
    a = o = 0
    for (raw, _), i in zip(recs, order):
        k, lo, n, b, cs, out, *_ = PLAN_WINDOWS[i]
        C_ = (LONG, THREE)[k]["C"]
        b_ = n if b == 0 or b > n else b
        nb, ns = -(-n // b_), slots(b_)
        assert raw == struct.pack("<QQQQQQIIII", out, b_, nb, a, o, cs, ns, i, C_, 0), i
        a += ns * C_ * nb
        o += C_ * nb
    assert (nacc, nout) == (a, o)
    # per frame
    (nacc, nout, _), recs = plan(programs, gf, 2)
    a = o = 0
    for (raw, _), i in zip(recs, order):
        k, lo, n, b, cs, out, *_ = PLAN_WINDOWS[i]
        s = (LONG, THREE)[k]
        b_ = n if b == 0 or b > n else b
        nb, ns = -(-n // b_), slots(b_)
        sstride = (nb + 15) & ~15
        assert raw == struct.pack("<QQQQQQIIII", out, b_, nb, a, o, n, ns, i, s["C"] * ((s["bits"] + 7) // 8), sstride), i
        a += ns * sstride if ns > 1 else nb
        o += nb
    assert (nacc, nout) == (a, o)
    # bitmask
    (nacc, nout, _), recs = plan(programs, gf, 3)
    a = o = 0
    for (raw, _), i in zip(recs, order):
        k, lo, n, b, cs, out, bins, shift, scale, qm, qc, qt = PLAN_WINDOWS[i]
        assert raw == struct.pack("<QQQQQQIIII", out, qm, qc, a, o, n, qt, i, (LONG, THREE)[k]["C"], 0), i
        a += -(-n // 64)
        o += -(-(-(-n // 64)) // 256)
    assert (nacc, nout) == (a + 3 * o + 1, o)


# ---- the tool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_cli_usage_and_option_errors(oracle, tmp_path):
    text = run("-h").stdout
    assert re.search(r"-L, --levels\b", text) and "-L BINS[,SHIFT[,log2]] STREAM.lnn" in text
    for args in (("-L",), ("-L", "64"), ("-L", "64", "-e", "a", "b"), ("-L", "64", "-d", "a"), ("-L", "64", "-C", "a", "b"), ("-L", "64", "-r", "a", "b"), ("-L", "64", "-V", "a"),
                 ("-L", "64", "-M", "a"), ("-L", "64", "-D", "a"), ("-L", "64", "-S", "0", "a"), ("-M", "-L", "64", "a"), ("-D", "-L", "64", "a"), ("-S", "0", "-L", "64", "a"),
                 ("-r", "-L", "64", "a", "b"), ("-C", "-L", "64", "a", "b"), ("--levels", "64", "a", "b"), ("-L", "64", "--batch", "d", "a"),
                 ("-L", "x", "a.lnn"), ("-L", "0", "a.lnn"), ("-L", "1025", "a.lnn"), ("-L", "12x", "a.lnn"), ("-L", "-5", "a.lnn"), ("-L", "64,", "a.lnn"), ("-L", "64,32", "a.lnn"),
                 ("-L", "64,x", "a.lnn"), ("-L", "64,4,", "a.lnn"), ("-L", "64,4,log3", "a.lnn"), ("-L", "64,4,log2,1", "a.lnn"), ("--levels=,4", "a.lnn")):
        r = run(*args)
        assert r.returncode == 1 and r.stderr.strip() and not r.stdout, args
    assert "bin count is out of range" in run("-L", "1025", "a.lnn").stderr
    assert "level shift is out of range" in run("-L", "64,32", "a.lnn").stderr
    assert "level scale is neither linear nor log2" in run("-L", "64,4,log3", "a.lnn").stderr
    assert "no other mode" in run("-L", "64", "-M", "a").stderr
    for args in (("-L", "64", "/nonexistent/a.lnn"), ("--levels", "1024,31,log2", "/nonexistent/a.lnn"), ("-L1,0,linear", "/nonexistent/a.lnn"), ("--levels=33,4", "/nonexistent/a.lnn")):
        r = run(*args)
        assert r.returncode == 1 and "Failed to open" in r.stderr, args
    # a file that is no stream is refused before a device is asked for; a stream either answers or fails with a message
    junk, lnn = tmp_path / "junk.lnn", tmp_path / "a.lnn"
    junk.write_bytes(b"RIFF" + bytes(100))
    r = run("-L", "64", str(junk))
    assert r.returncode == 1 and "Failed to get header information" in r.stderr
    x = np.concatenate([np.zeros((2, 1000), dtype=np.int32), music(2, 1500, 16, seed=3)], axis=1)
    lnn.write_bytes(bytes(oracle.encode_whole(x, 16, 22050, 500, 4, True)))
    r = run("-L", "33,0,log2", str(lnn))
    assert r.returncode in (0, 1), (r.returncode, r.stderr)      # (a signal would be negative)
    if r.returncode == 1:
        assert "Failed to create a device context" in r.stderr, r.stderr
