"""CPU tests (-m "not gpu") of mixing the channels of resident .lnn streams (include/linne_amd.h LINNEAmd_MixWindowsDevice): the
reference the GPU tests hold the library to (mix_refs.expected_mix: numpy int64 on the oracle's decode, checked here against
hand-written values), the matrix helpers, the boundary -- the symbol, the struct, the kind, the Python entry points, the argument errors
that need no device --, the host's plan with a mix record per window (a stand-alone program, also built with the address and
undefined-behaviour sanitizers, which also prints every record of the older consumers: they are byte for byte what the plan produced
before it knew of mix records, as tests/golden/windows_plan_records.json recorded them), the command line tool's -X option as far as it
goes without a device, and the premises of the GPU tests' fixtures by the oracle's decode."""
import ctypes as C
import hashlib
import inspect
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import linne_amd
import synth_records as sr
from mix_refs import expected_mix, mixed_values, random_matrix
from signals import music
from stream_refs import blocks, mixed_signal
from test_cli_cpu import CLI
from test_stream_histogram_cpu import LONG, PLAN_WINDOWS, THREE, live_in_order
from test_stream_relate_cpu import WIDE_SHAPE, wide_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linne_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "windows_plan_records.json")
OK, INVALID_ARGUMENT = 0, 1
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300
LO, HI = -(1 << 31), (1 << 31) - 1


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_the_reference_against_hand_written_values():
    v = np.array([[-3, -1, 1, 3, 5, -5], [0, 0, 0, 0, 0, 0]], dtype=np.int32)
    # halves round towards plus infinity, the negative ones too: -1.5 -> -1, -0.5 -> 0, 0.5 -> 1, 1.5 -> 2, 2.5 -> 3, -2.5 -> -2
    assert expected_mix(v, 0, 6, [[1, 1]], 1)[0].tolist() == [[-1, 0, 1, 2, 3, -2]]
    assert expected_mix(v, 0, 6, [[1, 0]], 2)[0].tolist() == [[-1, 0, 0, 1, 1, -1]]              # quarters: -0.75 -> -1, -0.25 -> 0, 1.25 -> 1
    assert expected_mix(v, 1, 3, [[1, 0], [0, 1], [-2, 7]], 0)[0].tolist() == [[-1, 1, 3], [0, 0, 0], [2, -2, -6]]
    assert expected_mix(v, 1, 3, [[-2, 7]])[0].tolist() == [[2, -2, -6]]
    # shift 0: the sum as it is, clipped at int32; shift 31: the largest sum there is comes down to 18 bits
    w = np.array([[LO, HI]] * 8, dtype=np.int32)
    rows = [[-32768] * 8, [32767] * 8, [1, 0, 0, 0, 0, 0, 0, 0]]
    y, sat = mixed_values(w, rows, 0, 0)
    assert y.tolist() == [[HI, LO], [LO, HI], [LO, HI]] and sat
    y, sat = mixed_values(w, rows, 31, 0)
    assert y.tolist() == [[8 * 32768, (-8 * 32768 * HI + (1 << 30)) >> 31], [-8 * 32767, (8 * 32767 * HI + (1 << 30)) >> 31], [-1, 1]] and not sat
    assert y[0][0] == 1 << 18 and (-(1 << 49) + (1 << 30)) >> 31 == -(1 << 18)                     # 2^49: the bound the header states
    # clip_bits 2, 16, 32
    v = np.array([[-3, -2, -1, 0, 1, 2]], dtype=np.int32)
    assert expected_mix(v, 0, 6, [[1]], 0, 2)[0].tolist() == [[-2, -2, -1, 0, 1, 1]] and expected_mix(v, 0, 6, [[1]], 0, 2)[1] is True
    assert expected_mix(v[:, 1:5], 0, 4, [[1]], 0, 2)[1] is False
    v = np.array([[-32769, -32768, 32767, 32768]], dtype=np.int32)
    got, sat = expected_mix(v, 0, 4, [[1]], 0, 16)
    assert got.tolist() == [[-32768, -32768, 32767, 32767]] and sat and expected_mix(v, 1, 2, [[1]], 0, 16)[1] is False
    got, sat = expected_mix(v, 0, 4, [[32767]], 0, 32)
    assert got.tolist() == [[-32769 * 32767, -32768 * 32767, 32767 * 32767, 32768 * 32767]] and not sat
    got, sat = expected_mix(np.array([[HI, LO, 1 << 30, -(1 << 30)]], dtype=np.int32), 0, 4, [[2]], 0, 32)
    assert got.tolist() == [[HI, LO, HI, LO]] and sat            # 2^31 is one too many, -2^31 fits: the sample that clips is the third
    assert expected_mix(np.array([[-(1 << 30)]], dtype=np.int32), 0, 1, [[2]], 0, 32)[1] is False
    assert np.array_equal(expected_mix(v, 0, 4, [[2]], 0, 32)[0], expected_mix(v, 0, 4, [[2]], 0, 0)[0])
    # the formats: S16 and S24 saturate behind the clip and say so; S24 is little-endian bytes
    got, sat = expected_mix(v, 0, 4, [[2]], 0, 0, "s16")
    assert got.dtype == np.int16 and got.tolist() == [[-32768, -32768, 32767, 32767]] and sat
    got, sat = expected_mix(v, 0, 4, [[-256]], 0, 0, "s24")
    assert got.dtype == np.uint8 and got.shape == (1, 4, 3) and sat
    assert got[0].tolist() == [[0xFF, 0xFF, 0x7F], [0xFF, 0xFF, 0x7F], [0x00, 0x01, 0x80], [0x00, 0x00, 0x80]]
    assert expected_mix(v, 1, 2, [[1]], 0, 0, "s24")[1] is False
    # the F32 scale: 2^-(clip_bits - 1), or 2^-(bits - 1) of the stream where clip_bits is 0
    got, sat = expected_mix(v, 0, 4, [[1]], 0, 16, "f32")
    assert got.dtype == np.float32 and got.tolist() == [[-1.0, -1.0, 32767 / 32768, 32767 / 32768]] and sat
    assert expected_mix(v, 0, 4, [[1]], 0, 0, "f32", bits=16)[0].tolist() == [[-32769 / 32768, -1.0, 32767 / 32768, 1.0]]
    assert expected_mix(v, 0, 4, [[1]], 0, 0, "f32", bits=24)[0].tolist() == [[x / (1 << 23) for x in (-32769, -32768, 32767, 32768)]]
    assert expected_mix(v, 0, 4, [[1]], 0, 24, "f32", bits=16)[0].tolist() == [[x / (1 << 23) for x in (-32769, -32768, 32767, 32768)]]
    big = np.array([[HI, LO, 16777217]], dtype=np.int32)         # (float)y rounds to nearest even first: 2^31, and 2^24 for 2^24 + 1
    assert expected_mix(big, 0, 3, [[1]], 0, 32, "f32")[0].tolist() == [[1.0, -1.0, 16777216 / (1 << 31)]]
    # entries behind the stream's channels and the matrix' rows are never read
    m = random_matrix(np.random.default_rng(1), 2, 3)
    x = music(3, 50, 16, seed=3)
    assert m.shape == (8, 8) and np.array_equal(expected_mix(x, 0, 50, m[:2], 3, 16)[0], expected_mix(x, 0, 50, m[:2, :3], 3, 16)[0])
    assert {32767, -32767, -32768} <= set(m[:2, :3].reshape(-1).tolist())


def test_the_matrix_helpers():
    assert linne_amd.downmix_matrix(1) == (((1,),), 0) and linne_amd.downmix_matrix(2) == (((1, 1),), 1)
    assert linne_amd.downmix_matrix(4) == (((1, 1, 1, 1),), 2) and linne_amd.downmix_matrix(8) == (((1,) * 8,), 3)
    assert linne_amd.downmix_matrix(3) == (((10923,) * 3,), 15) and linne_amd.downmix_matrix(6) == (((5461,) * 6,), 15)
    assert linne_amd.downmix_matrix(5) == (((6554,) * 5,), 15) and linne_amd.downmix_matrix(7) == (((4681,) * 7,), 15)
    v = np.array([[100, -7], [50, -8], [-30, 3]], dtype=np.int32)
    assert expected_mix(v, 0, 2, *linne_amd.downmix_matrix(3))[0].tolist() == [[40, -4]]
    assert expected_mix(v[:2], 0, 2, *linne_amd.downmix_matrix(2))[0].tolist() == [[75, -7]]       # -7.5 -> -7
    for bad in (0, 9):
        with pytest.raises(AssertionError):
            linne_amd.downmix_matrix(bad)
    assert linne_amd.select_matrix(2, [1, 0]) == ((0, 1), (1, 0)) and linne_amd.select_matrix(3, [2]) == ((0, 0, 1),)
    assert linne_amd.select_matrix(3, [0, 0, 2, 1]) == ((1, 0, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0))
    for bad in ((2, [2]), (2, []), (2, [-1]), (9, [0])):
        with pytest.raises(AssertionError):
            linne_amd.select_matrix(*bad)
    none = {"pairs": {(0, 1): None}, "channels": {0: None, 1: None}}
    assert linne_amd.fix_matrix(none) == ((1, 0), (0, 1))
    assert linne_amd.fix_matrix({"pairs": {(0, 1): "identical"}, "channels": {0: None, 1: None}}) == ((1, 0),)
    assert linne_amd.fix_matrix({"pairs": {(0, 1): "inverted"}, "channels": {0: None, 1: None}}) == ((1, 0), (0, -1))
    # a = (x, -x, x, y): 1 is negated, 2 is dropped, and the pair (1, 2) changes nothing further
    f = {"pairs": {(0, 1): "inverted", (0, 2): "identical", (0, 3): None, (1, 2): "inverted", (1, 3): None, (2, 3): None}, "channels": {i: None for i in range(4)}}
    assert linne_amd.fix_matrix(f) == ((1, 0, 0, 0), (0, -1, 0, 0), (0, 0, 0, 1))
    # channel_findings' own output goes in as it is
    x = music(1, 64, 16, seed=2)[0]
    pcm = np.stack([x, -x, x])
    rel = np.zeros((6, 1), dtype=linne_amd.RELATION_DTYPE)
    for i in range(3):
        for j in range(i, 3):
            p = linne_amd.pair_index(3, i, j)
            rel[p, 0]["num_equal"], rel[p, 0]["num_opposite"] = int((pcm[i] == pcm[j]).sum()), int((pcm[i].astype(np.int64) + pcm[j] == 0).sum())
    bucket, = linne_amd.channel_findings(rel)
    assert linne_amd.fix_matrix(bucket) == ((1, 0, 0), (0, -1, 0))
    fixed = expected_mix(pcm, 0, 64, linne_amd.fix_matrix(bucket))[0]
    assert np.array_equal(fixed[0], fixed[1]) and np.array_equal(fixed[0], x)


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_symbol_struct_and_kind_are_declared_listed_and_exported(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "linne_amd.h")).read(), flags=re.S)
    assert re.search(r"\bLINNEAmd_MixWindowsDevice\s*\(", src) and re.search(r"struct\s+LINNEAmdMixSpec\s*\{", src)
    assert re.search(r"LINNE_AMD_MIX_T_MIX\s*=\s*98\b", src)
    assert "LINNEAmd_MixWindowsDevice" in linne_amd.AMD_SYMBOLS and hasattr(linne_amd.lib, "LINNEAmd_MixWindowsDevice")
    M = linne_amd.MixSpec
    assert [(f[0], getattr(M, f[0]).offset) for f in M._fields_] == [("out_channels", 0), ("shift", 4), ("clip_bits", 8), ("reserved", 12), ("coef", 16)]
    assert C.sizeof(M) == 144
    sp = M()
    sp.coef[2][5] = -7
    assert struct.unpack_from("<h", bytes(sp), 16 + 2 * (2 * 8 + 5)) == (-7,)                       # [o][c], row by row
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
    if cc:
        code, exe = tmp_path / "size.c", tmp_path / "size"
        code.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "linne_amd.h"\nint main(void) { printf("%zu %zu %zu %d\\n", sizeof(struct LINNEAmdMixSpec), '
                        'offsetof(struct LINNEAmdMixSpec, coef), sizeof(((struct LINNEAmdMixSpec *)0)->coef[0]), (int)LINNE_AMD_MIX_T_MIX); return 0; }\n')
        b = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(code), "-o", str(exe)], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["144", "16", "16", "98"]


def test_python_entry_points():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(linne_amd.Context.mix_windows)
    assert list(p) == ["self", "windows", "matrix", "shift", "clip_bits", "out", "group_frames", "return_codes", "dtype", "channels_last", "s24", "return_saturated"]
    assert [p[k].default for k in list(p)[3:]] == [0, 0, None, 0, False, None, False, False, False]
    p = sig(linne_amd.Context.remix_streams)
    assert list(p) == ["self", "streams", "matrix", "shift", "bits", "preset", "block", "ms", "group_frames"]
    assert [p[k].default for k in list(p)[3:]] == [0, None, None, None, None, 0]
    assert list(sig(linne_amd.downmix_matrix)) == ["C"] and list(sig(linne_amd.select_matrix)) == ["C", "channels"] and list(sig(linne_amd.fix_matrix)) == ["findings"]
    # decode_windows is what it was
    p = sig(linne_amd.Context.decode_windows)
    assert list(p) == ["self", "windows", "out", "group_frames", "return_codes", "dtype", "channels_last", "s24", "return_saturated"]


def test_null_arguments_need_no_device_and_a_compute_call_fails_loudly():
    f = linne_amd.lib.LINNEAmd_MixWindowsDevice
    w, s, ly = (linne_amd.Window * 2)(), (linne_amd.MixSpec * 2)(), (linne_amd.PcmLayout * 2)()
    for i in range(2):
        w[i].result = -1
    assert f(None, w, s, ly, 2, 0) == INVALID_ARGUMENT and f(None, None, None, None, 0, 0) == INVALID_ARGUMENT
    blank = C.create_string_buffer(1 << 20)                     # zeroed memory larger than any context stands in for one
    ctx = C.addressof(blank)
    assert f(ctx, None, s, ly, 2, 0) == INVALID_ARGUMENT        # NULL windows
    assert f(ctx, w, None, ly, 2, 0) == INVALID_ARGUMENT        # NULL specs
    assert b"MixWindowsDevice: null argument" in linne_amd.lib.LINNEAmd_GetLastError(ctx)
    assert f(ctx, None, None, None, 0, 0) == OK and f(ctx, w, s, None, 0, 0) == OK
    assert [w[i].result for i in range(2)] == [-1, -1]
    if linne_amd.device_count() == 0:                           # no device: no context, and so no call -- nothing computes in its place
        with pytest.raises(Exception):
            linne_amd.Context(0).mix_windows([], [[1]])


# ---- the plan ------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "lnn_windows_plan.h"
/* stdin: group_frames bucketing mix nstreams nwindows; per stream: C bits S nb covered stream_bytes address, then nb x (off first size
 * type nsmp); per window: stream lo n bucket_samples cstride out bins shift scale quiet_min quiet_capacity quiet_threshold, and with mix
 * out_channels shift clip_bits and 64 coefficients.  Every record the plan fills comes out in hexadecimal */
struct Stream { WxIndexView x; std::vector<uint64_t> off, first; std::vector<uint32_t> size, type, nsmp; unsigned long long address; };
static void hex(const char *what, const void *p, size_t n) { printf("%s ", what); for (size_t j = 0; j < n; j++) printf("%02x", ((const unsigned char *)p)[j]); printf("\n"); }
int main(void)
{
    unsigned gf, bucketing, mix, ns, nw;
    if (scanf("%u %u %u %u %u", &gf, &bucketing, &mix, &ns, &nw) != 5) return 2;
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
#ifdef WITH_MIX
    std::vector<struct LINNEAmdMixSpec> specs(nw);
#endif
    for (unsigned i = 0; i < nw; i++) {
        WxRange &r = rg[i];
        unsigned k, bins, shift, scale, qt; unsigned long long lo, n, b, cs, out, qm, qc;
        if (scanf("%u %llu %llu %llu %llu %llu %u %u %u %llu %llu %u", &k, &lo, &n, &b, &cs, &out, &bins, &shift, &scale, &qm, &qc, &qt) != 12 || k >= ns) return 2;
        memset(&r, 0, sizeof(r));
        r.x = st[k].x; r.stream = (const uint8_t *)(uintptr_t)st[k].address; r.lo = lo; r.n = n; r.live = n != 0;
        r.bucket_samples = b; r.bucket_cstride = cs; r.bucket_out = (void *)(uintptr_t)out; r.hist = WXH_SPEC(bins, shift, scale);
        r.quiet_min = qm; r.quiet_capacity = qc; r.quiet_threshold = qt;
        r.fmt = LINNE_AMD_PCM_S32; r.sstride = 1; r.stride = n; r.out = (void *)(uintptr_t)out;
        if (n) r.r1 = (lo + n - 1u < r.x.covered) ? wx_block_of(r.x.h_first, r.x.nb, lo + n - 1u) : r.x.nb;
        if (mix) {
#ifdef WITH_MIX
            struct LINNEAmdMixSpec &m = specs[i];
            memset(&m, 0, sizeof(m));
            if (scanf("%u %u %u", &m.out_channels, &m.shift, &m.clip_bits) != 3) return 2;
            for (int o = 0; o < 8; o++) for (int c = 0; c < 8; c++) { int v; if (scanf("%d", &v) != 1) return 2; m.coef[o][c] = (int16_t)v; }
            r.mix = &m;
#else
            return 4;
#endif
        }
    }
    WxPlanned p;
    if (wx_plan_count(rg.data(), nw, gf, p) != WXP_OK) return 3;
    /* exactly the reserved sizes, from the heap: the sanitizer build sees a record written past them */
    std::vector<WxWindow> win(p.nlive); std::vector<WxBucket> side(bucketing ? p.nlive : 0); std::vector<WxBlock> rec(p.total_rec); std::vector<uint32_t> crec(p.total_crec);
#ifdef WITH_MIX
    std::vector<WxMix> mrec(mix ? p.nlive : 0);
    wx_plan_fill(rg.data(), nw, gf, (WxBucketing)bucketing, p, win.data(), bucketing ? side.data() : NULL, rec.data(), crec.data(), mix ? mrec.data() : NULL);
    const WxLists ls = wx_lists(p, nw, 0, bucketing ? sizeof(WxBucket) : mix ? sizeof(WxMix) : 0);
#else
    wx_plan_fill(rg.data(), nw, gf, (WxBucketing)bucketing, p, win.data(), bucketing ? side.data() : NULL, rec.data(), crec.data());
    const WxLists ls = wx_lists(p, nw, 0, bucketing ? sizeof(WxBucket) : 0);
#endif
    printf("fill %llu %llu %llu %llu %u %u %u %zu\n", (unsigned long long)p.nacc, (unsigned long long)p.nout, (unsigned long long)p.nmask, (unsigned long long)p.scratch_bytes, p.nwin, p.nrec, p.ncrec, p.passes.size());
    printf("lists %llu %llu %llu %llu %llu %llu\n", (unsigned long long)ls.o_back, (unsigned long long)ls.o_win, (unsigned long long)ls.o_side, (unsigned long long)ls.o_rec, (unsigned long long)ls.o_crec, (unsigned long long)ls.bytes);
    for (const WxPass &q : p.passes) printf("pass %u %u %u %u %u %llu %d\n", q.group, q.rec0, q.nrec, q.c0, q.nc, (unsigned long long)q.seg_bytes, q.check_only);
    for (const WxWindow &w : win) hex("window", &w, sizeof(w));
    for (const WxBucket &m : side) hex("bucket", &m, sizeof(m));
    for (uint32_t i = 0; i < p.nrec; i++) hex("block", &rec[i], sizeof(WxBlock));
    hex("crec", crec.data(), sizeof(uint32_t) * p.ncrec);
#ifdef WITH_MIX
    for (const WxMix &m : mrec) hex("mix", &m, sizeof(m));
    printf("sizes %zu\n", sizeof(WxMix));
#endif
    return 0;
}
"""
# a window's spec: (out_channels, shift, clip_bits), then its 64 coefficients row by row, garbage in every entry
MIX_RNG = np.random.default_rng(98)
MIX_SPECS = [((1, 2, 8, 3, 2, 1, 8)[i], (0, 1, 15, 31, 7, 0, 3)[i], (0, 16, 24, 32, 2, 8, 0)[i], MIX_RNG.integers(-32768, 32768, size=(8, 8))) for i in range(len(PLAN_WINDOWS))]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("mix_plan")
    src = str(d / "plan.cpp")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    exes = []
    for name, extra in (("plan", []), ("plan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        b = subprocess.run(cmd + ["-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-DWITH_MIX", *extra, "-I", CSRC, "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        exes.append(exe)
    return exes


def plan_input(gf, bucketing, mix):
    streams = [LONG, THREE]
    text = ["%d %d %d %d %d" % (gf, bucketing, int(mix), len(streams), len(PLAN_WINDOWS))]
    for s in streams:
        text.append("%d %d %d %d %d %d %d" % (s["C"], s["bits"], s["S"], len(s["blocks"]), s["covered"], s["bytes"], s["address"]))
        text += ["%d %d %d %d %d" % b for b in s["blocks"]]
    for w, (co, sh, cb, m) in zip(PLAN_WINDOWS, MIX_SPECS):
        text.append(" ".join(str(v) for v in w) + (" %d %d %d " % (co, sh, cb) + " ".join(str(int(v)) for v in m.reshape(-1)) if mix else ""))
    return "\n".join(text) + "\n"


def plan(programs, gf, bucketing, mix):
    outs = []
    for exe in programs:
        r = subprocess.run([exe], input=plan_input(gf, bucketing, mix), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    return outs[0]


@pytest.mark.parametrize("gf", [0, 2])
def test_plan_carries_a_mix_record_per_window(programs, gf):
    text = plan(programs, gf, 0, True)
    lines = [x.split() for x in text.splitlines()]
    recs = [bytes.fromhex(x[1]) for x in lines if x[0] == "mix"]
    order = live_in_order()
    assert len(recs) == len(order) and lines[-1] == ["sizes", "160"]
    for raw, i in zip(recs, order):
        s = (LONG, THREE)[PLAN_WINDOWS[i][0]]
        co, sh, cb, m = MIX_SPECS[i]
        B, Bf = cb or 32, cb or s["bits"]
        coef = np.zeros((8, 8), dtype="<i2")
        coef[:co, :s["C"]] = m[:co, :s["C"]]                    # nothing of the garbage behind the rows and columns in use
        want = struct.pack("<IIiiIIII", co, sh, -(1 << (B - 1)), (1 << (B - 1)) - 1, np.float32(2.0 ** -(Bf - 1)).view(np.uint32), i, 0, 0) + coef.tobytes()
        assert raw == want, i
    # the mix records lie where a bucketed consumer has its bucket records, 160 bytes each, and nothing else moves
    plain = plan(programs, gf, 0, False)
    keep = lambda t: [x for x in t.splitlines() if x.split()[0] not in ("mix", "sizes", "lists")]
    assert keep(text) == keep(plain)
    la, lb = ([int(v) for v in next(x for x in t.splitlines() if x.startswith("lists")).split()[1:]] for t in (text, plain))
    assert la[:3] == lb[:3] and la[3] >= la[2] + 160 * len(order) and lb[3] == lb[2]


@pytest.mark.parametrize("gf", [0, 2])
def test_records_of_the_older_consumers_are_byte_for_byte_what_they_were(programs, gf):
    """every line the program prints for bucketing kinds 0 to 5 -- sizes, passes, window, bucket and block records, the COMPRESS list --
    against the digest recorded from the same program built without WITH_MIX against the plan header of the commit before mix records"""
    golden = json.load(open(GOLDEN))
    for kind in range(6):
        text = "\n".join(x for x in plan(programs, gf, kind, False).splitlines() if not x.startswith("sizes")) + "\n"
        assert hashlib.sha256(text.encode()).hexdigest() == golden["gf %d kind %d" % (gf, kind)], (gf, kind)
    assert hashlib.sha256((PROGRAM + plan_input(gf, 5, False)).encode()).hexdigest() == golden["input gf %d" % gf]     # the recording is of this program and this input


# ---- the tool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_cli_usage_and_remix_spec_errors(oracle, tmp_path):
    run = lambda *a: subprocess.run([CLI, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    text = run("-h").stdout
    assert re.search(r"-X, --remix\b", text) and "-X ROW[/ROW...][>>SHIFT] IN.lnn OUT.lnn" in text
    src, dst = tmp_path / "a.lnn", tmp_path / "b.lnn"
    src.write_bytes(bytes(oracle.encode_whole(music(2, 2 * S, 16, seed=1), 16, 44100, S, 0, True)))
    for spec, word in (("1,1,1", "2 channels"), ("1/1", "2 channels"), ("1,1/1", "row 1 has 1"), ("1,32768", "outside int16"), ("-32769,1", "outside int16"),
                       ("1,1>>32", "shift 32"), ("1,,1", "coefficient is expected"), ("", "coefficient is expected"), ("1,1>>", "malformed"), ("1,1>1", "malformed"),
                       ("1,1/", "coefficient is expected"), ("1,x", "coefficient is expected"), ("1,1>>1x", "malformed"), ("/".join(["1,1"] * 9), "more than 8")):
        r = run("-X", spec, str(src), str(dst))
        assert r.returncode == 1 and word in r.stderr and not dst.exists(), (spec, r.stderr)
    assert run("-X", "1,1", str(src)).returncode == 1 and run("-X", "1,1", "-e", str(src), str(dst)).returncode == 1
    assert "-X takes" in run("-X", "1,1", str(src)).stderr
    r = run("-X", "1,1", str(tmp_path / "missing.lnn"), str(dst))
    assert r.returncode == 1 and "Failed to open" in r.stderr


# ---- the fixtures' premises ----------------------------------------------------------------------------------------------------
def test_premises_of_the_gpu_fixtures(oracle):
    # the mixed stream, cut behind its sixth block: COMPRESS, SILENT and RAW blocks, and zeros behind them
    x = mixed_signal(2, 16, 7 * S + TAIL, seed=11, block=S)
    whole = bytes(oracle.encode_whole(x, 16, 44100, S, 5, True))
    bl = blocks(whole)
    assert [b[2] for b in bl] == [COMPRESS, SILENT, SILENT, COMPRESS, RAW, RAW, COMPRESS, COMPRESS]
    ret, full, _ = oracle.decode_whole(whole[:bl[6][0]])
    assert ret == OK and full.shape == (2, 7 * S + TAIL) and np.array_equal(full[:, :6 * S], x[:, :6 * S]) and not full[:, 6 * S:].any()
    # the crafted stream decodes beyond +-2^23, to all of int32; rows of +-32767 then clip at 32 and at 16 bits but not behind shift 31
    ret, full, _ = oracle.decode_whole(sr.case_stream(WIDE_SHAPE, wide_cases()))
    mag = np.abs(full.astype(np.int64))
    assert ret == OK and full.shape[0] == 2 and (mag.max(axis=1) >= 1 << 24).all() and mag.max() > 1 << 30
    rows = np.array([[32767 * (-1) ** ((o >> c) & 1) for c in range(8)] for o in range(8)], dtype=np.int16)
    n = full.shape[1]
    assert [expected_mix(full, 0, n, rows, sh, cb)[1] for sh, cb in ((0, 0), (0, 16), (31, 0))] == [True, True, False]
    # the music streams survive the encoder, the eight-channel one in blocks of 1024 too
    for nch in (1, 2, 3, 8):
        x = music(nch, 3 * S + TAIL, 16, seed=90 + nch)
        stream = bytes(oracle.encode_whole(x, 16, 44100, S, 5 if nch == 2 else 0, nch == 2))
        ret, full, _ = oracle.decode_whole(stream)
        assert ret == OK and np.array_equal(full, x) and len(blocks(stream)) == 4
    # an inverted pair survives it as well
    m = music(1, 2 * S + TAIL, 16, seed=5)
    ret, full, _ = oracle.decode_whole(bytes(oracle.encode_whole(np.concatenate([m, -m]), 16, 44100, S, 2, False)))
    assert ret == OK and np.array_equal(full, np.concatenate([m, -m]))
