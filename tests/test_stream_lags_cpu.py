"""Sliding resident .lnn streams over each other, without a GPU (include/linne_amd.h LINNEAmd_LagWindowsDevice; linne_amd.lag_dots,
lag_correlation, best_lag): the reference of tests/lag_refs.py against hand-written values, the structs compiled against the header,
the boundary through the C entry point (a probe's own argument checks come before any device work), the plan's images, probe records,
tiles and runs from a stand-alone program, and the host helpers' rules."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import linne_amd
from lag_refs import expected_lags, haystack, lag_sums, limb_sums, table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linne_amd", "csrc")
OK, INVALID_ARGUMENT = 0, 1


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_the_reference_against_hand_written_values():
    a = np.array([1, 2, 3], dtype=np.int32)
    b = np.array([4, 5, 6, 7], dtype=np.int32)
    # a needle of 3 samples at lags -2 .. 2 of a haystack of 4: both of the haystack's ends lie inside the range
    assert haystack(b, 0, -2, 5, 3).tolist() == [0, 0, 4, 5, 6, 7, 0]
    dots, b_sq, a_sq = lag_sums(a, 0, 3, b, 0, -2, 5)
    assert dots == [3 * 4, 2 * 4 + 3 * 5, 4 + 10 + 18, 5 + 12 + 21, 6 + 14] and b_sq == [16, 16 + 25, 16 + 25 + 36, 25 + 36 + 49, 36 + 49] and a_sq == 14
    # a range of the needle's stream, first_b moves the haystack, and a range that misses the stream
    assert lag_sums(b, 1, 2, b, 1, 0, 1) == ([25 + 36], [25 + 36], 25 + 36)
    assert lag_sums(a, 0, 3, b, 2, 0, 2) == ([6 + 14, 7], [36 + 49, 49], 14)
    assert lag_sums(a, 0, 3, b, 100, 0, 2) == ([0, 0], [0, 0], 14) and lag_sums(a, 0, 3, b, 0, -9, 2) == ([0, 0], [0, 0], 14)
    # values over all of int32: Python integers, and the table's two's-complement words
    w = np.array([-(1 << 31)] * 5, dtype=np.int32)
    v = np.array([(1 << 31) - 1] * 5, dtype=np.int32)
    dots, b_sq, a_sq = lag_sums(w, 0, 5, v, 0, 0, 1)
    assert dots == [-5 * (1 << 31) * ((1 << 31) - 1)] and b_sq == [5 * ((1 << 31) - 1) ** 2] and a_sq == 5 << 62 and a_sq > 1 << 64
    t, e = expected_lags(np.stack([w]), 0, 5, np.stack([v]), 0, 0, 1, [(0, 0)])
    assert (int(t[0, 0]["dot_hi"]) << 64) + int(t[0, 0]["dot_lo"]) == dots[0] and int(t[0, 0]["dot_hi"]) == -2
    assert (int(t[0, 0]["b_sq_hi"]) << 64) + int(t[0, 0]["b_sq_lo"]) == b_sq[0] and e.tolist() == [[(5 << 62) & ((1 << 64) - 1), 1]]
    # the two forms of the reference agree
    rng = np.random.default_rng(3)
    x, y = rng.integers(-1 << 15, 1 << 15, 40), rng.integers(-1 << 15, 1 << 15, 50)
    fast = lag_sums(x, 3, 30, y, 5, -20, 60)
    xs, hs = [int(q) for q in x[3:33]], [int(q) for q in haystack(y, 5, -20, 60, 30)]
    assert fast[0] == [sum(p * q for p, q in zip(xs, hs[l:l + 30])) for l in range(60)] and fast[1] == [sum(q * q for q in hs[l:l + 30]) for l in range(60)]
    # ... and the third, on limbs, for long needles of values over all of int32: the extremes of both signs among them
    x, y = rng.integers(-1 << 31, 1 << 31, 70), rng.integers(-1 << 31, 1 << 31, 90)
    x[:4], y[5:9] = [-(1 << 31), (1 << 31) - 1, -1, 65536], [(1 << 31) - 1, -(1 << 31), -65536, -1]
    slow = lag_sums(x, 3, 60, y, 5, -20, 80)
    assert slow == limb_sums(x[3:63], haystack(y, 5, -20, 80, 60), 60, 80) and max(abs(v) for v in slow[0]) > 1 << 64


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_symbol_structs_limits_and_kinds_are_declared_listed_and_exported(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "linne_amd.h")).read(), flags=re.S)
    name = "LINNEAmd_LagWindowsDevice"
    assert re.search(r"\b%s\s*\(" % name, src) and name in linne_amd.AMD_SYMBOLS and hasattr(linne_amd.lib, name)
    assert re.search(r"LINNE_AMD_LAGS_T_LAGS\s*=\s*102\b", src) and re.search(r"LINNE_AMD_LAGS_T_COMMIT\s*=\s*103\b", src)
    assert (linne_amd.LAG_MAX_LAGS, linne_amd.LAG_MAX_PRODUCTS) == (65536, 1 << 38)
    S, P = linne_amd.LagSum, linne_amd.LagProbe
    assert [(f[0], getattr(S, f[0]).offset) for f in S._fields_] == [("dot_lo", 0), ("dot_hi", 8), ("b_sq_lo", 16), ("b_sq_hi", 24)]
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == [("index_a", 0), ("d_stream_a", 8), ("first_a", 16), ("num_samples", 24), ("index_b", 32), ("d_stream_b", 40),
                                                                    ("first_b", 48), ("lag_first", 56), ("num_lags", 64), ("num_pairs", 68), ("chan_a", 72), ("chan_b", 80),
                                                                    ("d_out", 88), ("pair_stride", 96), ("d_a_sq", 104), ("reserved", 112), ("result", 120)]
    assert (C.sizeof(S), C.sizeof(P)) == (32, 128) and linne_amd.LAG_DTYPE.itemsize == 32
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler holds the structs to the header"
    code, exe = tmp_path / "size.c", tmp_path / "size"
    fields = ["sizeof(struct LINNEAmdLagSum)", "sizeof(struct LINNEAmdLagProbe)"]
    fields += ["offsetof(struct LINNEAmdLagSum, %s)" % f[0] for f in S._fields_] + ["offsetof(struct LINNEAmdLagProbe, %s)" % f[0] for f in P._fields_]
    code.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "linne_amd.h"\nint main(void) { size_t v[] = { %s }; size_t i; for (i = 0; i < sizeof(v) / sizeof(v[0]); i++) printf("%%zu ", v[i]); '
                    'printf("%%d %%d %%llu %%llu\\n", (int)LINNE_AMD_LAGS_T_LAGS, (int)LINNE_AMD_LAGS_T_COMMIT, (unsigned long long)LINNE_AMD_LAG_MAX_LAGS, (unsigned long long)LINNE_AMD_LAG_MAX_PRODUCTS); return 0; }\n'
                    % ", ".join(fields))
    b = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(code), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    want = [32, 128] + [getattr(S, f[0]).offset for f in S._fields_] + [getattr(P, f[0]).offset for f in P._fields_] + [102, 103, 65536, 1 << 38]
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == want


def test_python_entry_points():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(linne_amd.Context.lag_windows)
    assert list(p) == ["self", "probes", "group_frames", "return_codes"] and [p[k].default for k in list(p)[2:]] == [0, False]
    p = sig(linne_amd.Context.align_streams)
    assert list(p) == ["self", "pairs_of_streams", "max_lag", "needle"] and p["needle"].default is None
    assert list(sig(linne_amd.lag_dots)) == ["table"] and list(sig(linne_amd.lag_correlation))[0] == "table" and list(sig(linne_amd.best_lag))[:2] == ["table", "lag_first"]


TOP = (1 << 64) - 1
# every INVALID_ARGUMENT case of a probe's own: (the probe's fields, a word of the text)
BAD = [(dict(index_a=None), "null argument"), (dict(d_stream_a=None), "null argument"), (dict(index_b=None), "null argument"), (dict(d_stream_b=None), "null argument"),
       (dict(d_out=None), "null d_out"), (dict(reserved=1 << 40), "reserved is not 0"), (dict(num_samples=0), "num_samples 0"),
       (dict(num_lags=0), "num_lags 0 is not 1 .. 65536"), (dict(num_lags=65537), "num_lags 65537"), (dict(num_pairs=0), "num_pairs 0 is not 1 .. 8"), (dict(num_pairs=9), "num_pairs 9"),
       (dict(num_samples=(1 << 38) // 10 + 1, num_lags=5, num_pairs=2, pair_stride=5), "> 2^38 products"), (dict(num_samples=TOP, num_lags=65536, num_pairs=8, pair_stride=65536), "> 2^38 products"),
       (dict(num_samples=(1 << 22) + 1, num_lags=65536, num_pairs=1, pair_stride=65536), "> 2^38 products"),
       (dict(chan_a=2), "pair 1: channel 2 of a needle of 2"), (dict(chan_b=3), "pair 1: channel 3 of a haystack of 3"), (dict(chan_a=255), "channel 255 of a needle"),
       (dict(d_out="four bytes on"), "d_out is not 8-byte aligned"), (dict(d_a_sq="four bytes on"), "d_a_sq is not 8-byte aligned"), (dict(pair_stride=9), "pair_stride 9 < 10 lags")]


class FakeIndex(C.Structure):
    """how struct LINNEAmdStreamIndex begins (linne_amd/csrc/lnn_device.hip); the rest is zeroed room"""
    _fields_ = [("device", C.c_int), ("header", linne_amd.Header), ("shape", linne_amd.Shape), ("rest", C.c_char * 4096)]


def test_arguments_are_checked_before_any_device_work():
    f = linne_amd.lib.LINNEAmd_LagWindowsDevice
    err = linne_amd.lib.LINNEAmd_GetLastError
    q = (linne_amd.LagProbe * 2)()
    assert f(None, q, 2, 0) == INVALID_ARGUMENT and f(None, None, 0, 0) == INVALID_ARGUMENT
    blank = C.create_string_buffer(1 << 20)                     # zeroed memory larger than any context stands in for one
    ctx = C.addressof(blank)
    assert f(ctx, None, 2, 0) == INVALID_ARGUMENT and b"LagWindowsDevice: null argument" in err(ctx)
    assert f(ctx, None, 0, 0) == OK and f(ctx, q, 0, 0) == OK
    # memory laid out as an index begins stands in for indexes of 2 and of 3 channels; their streams hold no samples, which the
    # needle's window check says
    index = [FakeIndex() for _ in range(2)]
    for x, nch in zip(index, (2, 3)):
        x.header.num_channels = x.shape.num_channels = nch
        x.shape.bits_per_sample = x.header.bits_per_sample = 16
    stream = C.create_string_buffer(64)
    out = C.create_string_buffer(4096)
    assert C.addressof(out) % 8 == 0

    def fill(fields):
        for k in range(2):
            p = q[k]
            p.index_a, p.d_stream_a, p.first_a, p.num_samples = C.addressof(index[0]), C.addressof(stream), 0, 10
            p.index_b, p.d_stream_b, p.first_b, p.lag_first, p.num_lags, p.num_pairs = C.addressof(index[1]), C.addressof(stream), 0, -5, 10, 2
            for j in range(8):
                p.chan_a[j], p.chan_b[j] = 0, 0
            p.d_out, p.pair_stride, p.d_a_sq, p.reserved, p.result = C.addressof(out), 10, C.addressof(out) + 2048, 0, -1
        for k, v in fields.items():
            if k in ("chan_a", "chan_b"):
                getattr(q[1], k)[1] = v
            else:
                setattr(q[1], k, C.addressof(out) + 4 if v == "four bytes on" else v)

    for fields, word in BAD:
        fill(fields)
        assert f(ctx, q, 2, 0) == INVALID_ARGUMENT and [q[k].result for k in range(2)] == [INVALID_ARGUMENT] * 2
        # probe 0 passes its own checks: its needle is checked as a window is, and its stream holds no samples
        assert err(ctx) == b"probe 0: needle: DecodeStreamDevice: samples [0, 10) beyond the stream's 0", fields
        q[0] = q[1]
        assert f(ctx, q, 1, 0) == INVALID_ARGUMENT and q[0].result == INVALID_ARGUMENT
        text = err(ctx).decode()
        assert text.startswith("probe 0: LagWindowsDevice: ") and word in text, (fields, text)
    assert set(out.raw) == {0}
    if linne_amd.device_count() == 0:                           # no device: no context, and so no call -- nothing computes in its place
        with pytest.raises(Exception):
            linne_amd.Context(0).lag_windows([])


# ---- the tool ------------------------------------------------------------------------------------------------------------------
def test_cli_usage_and_lag_spec_errors(oracle, tmp_path):
    from signals import music
    from test_cli_cpu import CLI
    assert os.path.exists(CLI), "linne_amd_cli is not built (python -c 'import __graft_entry__ as g; g.build()')"
    run = lambda *a: subprocess.run([CLI, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    text = run("-h").stdout
    assert re.search(r"-A, --align\b", text) and "-A OTHER.lnn[,MAX_LAG[,FIRST,N]] IN.lnn" in text
    src, other = tmp_path / "a.lnn", tmp_path / "b.lnn"
    src.write_bytes(bytes(oracle.encode_whole(music(2, 2 * 1024, 16, seed=1), 16, 44100, 1024, 0, True)))
    other.write_bytes(bytes(oracle.encode_whole(music(2, 1500, 16, seed=2), 16, 44100, 1024, 0, True)))
    for spec, word in (("", "a file name is expected"), (",5", "a file name is expected"), (f"{other},", "a largest lag in samples is expected"),
                       (f"{other},x", "a largest lag in samples is expected"), (f"{other},-1", "a largest lag in samples is expected"), (f"{other},+1", "a largest lag in samples is expected"),
                       (f"{other},5x", "malformed"), (f"{other},5.5", "malformed"), (f"{other},32768", "outside 0 .. 32767"), (f"{other},99999999999999999999999", "outside 64 bits"),
                       (f"{other},5,7", "come together"), (f"{other},5,0,0", "a needle of 0 samples"), (f"{other},5,2000,100", "a needle of 100 samples from 2000 on in a stream of 2048"),
                       (f"{other},5,1,2048", "a needle of 2048 samples from 1 on"), (str(tmp_path / "missing.lnn"), "Failed to open"), (f"{tmp_path / 'missing.lnn'},7", "Failed to open")):
        r = run("-A", spec, str(src))
        assert r.returncode == 1 and word in r.stderr and r.stdout == "", (spec, r.stderr)
    assert run("-A", str(other)).returncode == 1 and run("-A", str(other), "-e", str(src)).returncode == 1
    assert "-A takes" in run("-A", str(other)).stderr and "-A takes" in run("-A", str(other), str(src), str(src)).stderr
    r = run("-A", str(other), str(tmp_path / "missing.lnn"))
    assert r.returncode == 1 and "Failed to open" in r.stderr


# ---- the host helpers ----------------------------------------------------------------------------------------------------------
def test_lag_dots_and_correlation_against_hand_values():
    t = table_of([[6, -6, 0, 1 << 70], [-(1 << 70), 3, 3, 3]], [[9, 9, 0, 1 << 80], [1 << 80, 9, 9, 9]])
    assert linne_amd.lag_dots(t) == [[6, -6, 0, 1 << 70], [-(1 << 70), 3, 3, 3]] and linne_amd.lag_energies(t)[0] == [9, 9, 0, 1 << 80]
    r = linne_amd.lag_correlation(t, a_sq=[4, 1 << 60])
    assert r.shape == (2, 4) and r.dtype == np.float64
    assert r[0, 0] == 1.0 and r[0, 1] == -1.0 and math.isnan(r[0, 2]) and r[0, 3] == 2.0 ** 70 / math.sqrt(4 * 2.0 ** 80)
    assert r[1, 0] == -1.0 and r[1, 1] == 3 / math.sqrt(9 * 2.0 ** 60)
    assert np.isnan(linne_amd.lag_correlation(t, a_sq=[0, 0])).all()


def test_best_lag_rules():
    best = linne_amd.best_lag
    # the lag maximises dot / sqrt(b_sq): 6 / 3 against 7 / 4 against 100 / 100
    assert best(table_of([[6, 7, 100]], [[9, 16, 10000]]), -1, a_sq=[4]) == (-1, 1.0)
    # the pairs' dots and energies are added per lag: pair 0 alone says lag 0, the sums say lag 1
    t = table_of([[5, 4], [0, 4]], [[25, 16], [25, 16]])
    assert best(t[:1], 0, a_sq=[1])[0] == 0 and best(t, 0, a_sq=[1, 1])[0] == 1
    assert best(t, 0, a_sq=[1, 1])[1] == 8 / math.sqrt(2 * 32)
    # exact comparison: 2^70 / sqrt(2^80 + 1) is below 2^70 / sqrt(2^80), which float64 cannot tell
    t = table_of([[1 << 70, 1 << 70]], [[(1 << 80) + 1, 1 << 80]])
    assert best(t, 5, a_sq=[1 << 60])[0] == 6
    # ties go to the smaller |lag|, then to the negative lag
    flat = table_of([[3] * 5], [[9] * 5])
    assert best(flat, -2, a_sq=[1])[0] == 0 and best(flat, 1, a_sq=[1])[0] == 1 and best(flat, -5, a_sq=[1])[0] == -1
    two = table_of([[3, 0, 3]], [[9, 9, 9]])
    assert best(two, -1, a_sq=[1])[0] == -1
    # negative dots: the least negative wins; a lag without energy counts as 0 and beats them
    assert best(table_of([[-6, -3]], [[9, 9]]), 0, a_sq=[1]) == (1, -1.0)
    lag, r = best(table_of([[-6, 0, -3]], [[9, 0, 9]]), 0, a_sq=[1])
    assert lag == 1 and math.isnan(r)
    assert math.isnan(best(table_of([[1]], [[1]]), 0)[1])        # (no a_sq: the lag alone)


# ---- the plan ------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "lnn_windows_plan.h"
/* stdin: group_frames nblocks S N nprobes, then per probe: checked first_a n hay_lo hay_n b0 nlags npair live_a live_b (hay_n 0: the
 * range misses the stream and there is no haystack window).  One stream of two channels, nblocks SILENT blocks of S samples, N samples
 * in its header.  Out come the counts, the window records, the image records of all windows, the probe records, the tiles and the runs
 * -- and whether the same ranges planned for the placing call give the same block records, byte for byte.  With the argument `count`:
 * the counts of wx_lag_count alone, no list is written */
int main(int argc, char **argv)
{
    unsigned gf, nb, S, nq; unsigned long long N;
    if (scanf("%u %u %u %llu %u", &gf, &nb, &S, &N, &nq) != 5) return 2;
    std::vector<uint64_t> off(nb), first(nb); std::vector<uint32_t> size(nb, 5), type(nb, SX_SILENT), nsmp(nb, S);
    for (unsigned r = 0; r < nb; r++) { off[r] = 30 + 11ull * r; first[r] = (uint64_t)S * r; }
    WxIndexView x; memset(&x, 0, sizeof(x));
    x.shape.num_channels = 2; x.shape.bits_per_sample = 16; x.shape.num_samples_per_block = S; x.nb = nb; x.covered = (uint64_t)S * nb; x.stream_bytes = 30 + 11ull * nb;
    x.h_off = off.data(); x.h_first = first.data(); x.h_size = size.data(); x.h_type = type.data(); x.h_nsmp = nsmp.data();
    std::vector<WxLagIn> in(nq); std::vector<WxRange> rg;
    auto window = [&](unsigned long long lo, unsigned long long n, int live) {
        WxRange r; memset(&r, 0, sizeof(r));
        r.x = x; r.stream = (const uint8_t *)(uintptr_t)0x30000; r.live = live; r.lo = lo; r.n = n;
        r.r1 = (lo + n - 1u < x.covered) ? wx_block_of(x.h_first, x.nb, lo + n - 1u) : x.nb;
        rg.push_back(r);
    };
    for (unsigned k = 0; k < nq; k++) {
        int checked, la, lb; unsigned long long fa, n, hlo, hn; long long b0; unsigned nl, np;
        if (scanf("%d %llu %llu %llu %llu %lld %u %u %d %d", &checked, &fa, &n, &hlo, &hn, &b0, &nl, &np, &la, &lb) != 10) return 2;
        WxLagIn &q = in[k];
        memset(&q, 0, sizeof(q));
        q.wa = (uint32_t)rg.size(); q.wb = WXL_NOWIN; q.checked = checked;
        if (!checked) continue;                                 /* (a probe that failed its own checks brings no windows) */
        q.n = n; q.b0 = b0; q.nlags = nl; q.npair = np; q.out = (void *)(uintptr_t)(0x1000 * (k + 1)); q.pstride = nl + k; q.a_sq = (uint64_t *)(uintptr_t)(0x100 * (k + 1));
        for (unsigned p = 0; p < 8; p++) { q.ca[p] = (uint8_t)(p & 1u); q.cb[p] = (uint8_t)((p + k) & 1u); }
        window(fa, n, la);
        if (hn) { q.wb = (uint32_t)rg.size(); window(hlo, hn, lb); }
    }
    const uint32_t W = (uint32_t)rg.size();
    WxPlanned p;
    if (wx_plan_count(rg.data(), W, gf, p) != WXP_OK) return 3;
    wx_lag_count(in.data(), nq, p);
    if (argc > 1 && strcmp(argv[1], "count") == 0) {           /* the counts alone: what the call's guard reads, and the guard's bound */
        printf("count %llu %llu %llu %llu\n", (unsigned long long)p.rs_tiles, (unsigned long long)p.lg_runs, (unsigned long long)p.lg_probes, (unsigned long long)WX_MAX_TILES);
        return 0;
    }
    /* exactly the reserved sizes, from the heap: the sanitizer build sees a record written past them */
    std::vector<WxWindow> win(p.nlive); std::vector<WxBlock> rec(p.total_rec); std::vector<uint32_t> crec(p.total_crec);
    std::vector<WxLagTile> tile(p.rs_tiles); std::vector<uint32_t> run(p.lg_runs); std::vector<WxLagProbe> prec(p.lg_probes); std::vector<WxLagImage> img(W);
    if (W) memset(img.data(), 0, sizeof(WxLagImage) * W);
    wx_plan_fill(rg.data(), W, gf, WX_NO_BUCKETS, p, win.data(), NULL, rec.data(), crec.data(), NULL, NULL, NULL, NULL, NULL, img.data());
    const uint64_t images = p.nacc;
    wx_lag_fill(in.data(), nq, p, prec.data(), tile.data(), run.data());
    const WxLists plain = wx_lists(p, W, 0, 0), ls = wx_lists(p, W, 0, 0, false, false, true);
    printf("fill %llu %llu %llu %llu %llu %llu %llu %llu %llu %u\n", (unsigned long long)images, (unsigned long long)p.lg_part, (unsigned long long)p.nacc, (unsigned long long)p.rs_tiles, (unsigned long long)p.ntile,
            (unsigned long long)p.lg_probes, (unsigned long long)p.nlg, (unsigned long long)p.lg_runs, (unsigned long long)p.nlgrun, p.nwin);
    printf("lists %llu %llu %llu %llu %llu %llu\n", (unsigned long long)plain.bytes, (unsigned long long)ls.o_tile, (unsigned long long)ls.o_lgrun, (unsigned long long)ls.o_lgprobe, (unsigned long long)ls.o_lgimg, (unsigned long long)ls.bytes);
    for (uint32_t k = 0; k < p.nwin; k++) {
        const WxWindow &w = win[k];
        printf("window %u %llu %llu %llu %llu %u %llu\n", w.fidx, (unsigned long long)w.lo, (unsigned long long)w.hi, (unsigned long long)(uintptr_t)w.out, (unsigned long long)w.stride, w.fmt, (unsigned long long)w.sstride);
    }
    for (uint32_t i = 0; i < W; i++) printf("image %llu %llu %llu %llu\n", (unsigned long long)img[i].img, (unsigned long long)img[i].istride, (unsigned long long)img[i].lo, (unsigned long long)img[i].n);
    for (const WxLagProbe &m : prec)
        printf("probe %llu %llu %llu %llu %lld %u %d %u %u %u %u %u %u\n", (unsigned long long)(uintptr_t)m.out, (unsigned long long)m.pstride, (unsigned long long)(uintptr_t)m.a_sq, (unsigned long long)m.n, (long long)m.b0,
                m.wa, m.wb == WXL_NOWIN ? -1 : (int)m.wb, m.nlags, m.npair, m.nchunk, m.ntl, (unsigned)m.ca[1], (unsigned)m.cb[0]);
    for (const WxLagTile &t : tile) printf("tile %u %u %u %u\n", t.probe, t.pair, t.l0, t.chunk);
    for (uint32_t r : run) printf("run %u\n", r);
    /* the placing call on the same ranges: the same passes and block records, and window records that differ in their targets alone */
    WxPlanned q;
    if (wx_plan_count(rg.data(), W, gf, q) != WXP_OK) return 3;
    std::vector<WxWindow> win2(q.nlive); std::vector<WxBlock> rec2(q.total_rec); std::vector<uint32_t> crec2(q.total_crec);
    wx_plan_fill(rg.data(), W, gf, WX_NO_BUCKETS, q, win2.data(), NULL, rec2.data(), crec2.data());
    int same = q.nrec == p.nrec && q.nwin == p.nwin && q.ncrec == p.ncrec && q.passes.size() == p.passes.size() && q.scratch_bytes == p.scratch_bytes && q.nacc == 0;
    same = same && (p.nrec == 0 || memcmp(rec.data(), rec2.data(), sizeof(WxBlock) * p.nrec) == 0);
    for (uint32_t k = 0; same && k < p.nwin; k++) same = win[k].lo == win2[k].lo && win[k].hi == win2[k].hi && win[k].covered == win2[k].covered && win[k].fidx == win2[k].fidx;
    printf("same %d\n", same);
    return 0;
}
"""
PLAN_S, PLAN_BLOCKS = 8192, 10
PLAN_N = PLAN_BLOCKS * PLAN_S - 7                               # the header names a little less than the blocks hold
# (checked, first_a, n, the haystack's clipped (lo, n), b0, lags, pairs, live_a, live_b): lags of 255, 256 and 257 and needles of 65535,
# 65536 and 65537 samples; a haystack that starts in front of sample 0, one that ends behind the stream, one that misses it; a probe
# whose own checks failed, one with a refused needle, one with a refused haystack; the same range as needle and haystack
PLAN_PROBES = [(1, 0, 100, (0, 354), 0, 255, 1, 1, 1), (1, 5, 1, (0, 200), -56, 256, 2, 1, 1), (1, 7, 33, (40, 289), 0, 257, 8, 1, 1),
               (1, 0, 65535, (0, 65535 + 512), 0, 513, 1, 1, 1), (1, 1, 65536, (1, 65536), 0, 1, 2, 1, 1), (1, 100, 65537, (PLAN_N - 70000, 70000), 0, 257, 1, 1, 1),
               (1, 9, 50, (0, 0), -(1 << 40), 300, 3, 1, 1), (0, 0, 10, (0, 19), 0, 10, 1, 1, 1), (1, 0, 10, (0, 19), 0, 10, 1, 0, 1), (1, 0, 10, (0, 19), 0, 10, 1, 1, 0),
               (1, 64, 64, (64, 64), 0, 1, 2, 1, 1)]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lag_plan")
    src = str(d / "plan.cpp")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    exes = []
    for name, extra in (("plan", []), ("plan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        b = subprocess.run(cmd + ["-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, "-I", os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        exes.append(exe)
    return exes


@pytest.mark.parametrize("gf", [0, 2])
def test_plan_images_probes_tiles_and_runs(programs, gf):
    text = "%d %d %d %d %d\n" % (gf, PLAN_BLOCKS, PLAN_S, PLAN_N, len(PLAN_PROBES))
    for checked, fa, n, (hlo, hn), b0, nl, npair, la, lb in PLAN_PROBES:
        text += "%d %d %d %d %d %d %d %d %d %d\n" % (checked, fa, n, hlo, hn, b0, nl, npair, la, lb)
    outs = []
    for exe in programs:
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = [x.split() for x in outs[0].splitlines()]
    # what Python makes of the same probes
    windows, images, probes, tiles, runs, img, W = [], [], [], [], [], 0, 0
    for k, (checked, fa, n, (hlo, hn), b0, nl, npair, la, lb) in enumerate(PLAN_PROBES):
        if not checked:
            continue
        wa, wb = W, (W + 1 if hn else -1)
        for lo, m, live in [(fa, n, la)] + ([(hlo, hn, lb)] if hn else []):
            if live:
                istride = (m + 3) // 4 * 4
                windows.append([W, lo, lo + m, 4 * img, istride, 0, 1])          # the window's target is its image: int32, sample stride 1
                images.append([img, istride, lo, m])
                img += 2 * istride
            else:
                images.append([0] * 4)
            W += 1
        if la and (lb or not hn):
            nchunk, ntl = -(-n // 65536), -(-nl // 256)
            probes.append([0x1000 * (k + 1), nl + k, 0x100 * (k + 1), n, b0, wa, wb, nl, npair, nchunk, ntl, 1, k & 1])
            for p in range(npair):
                for lt in range(ntl):
                    runs.append([len(tiles)])
                    tiles += [[len(probes) - 1, p, 256 * lt, c] for c in range(nchunk)]
    take = lambda word: [[int(v) for v in x[1:]] for x in lines if x[0] == word]
    assert take("window") == windows and take("image") == images and take("probe") == probes and take("tile") == tiles and take("run") == runs
    assert len(probes) == 8 and [p[9:11] for p in probes[:6]] == [[1, 1], [1, 1], [1, 2], [1, 3], [1, 1], [2, 2]]     # (the premise: 255, 256, 257 lags; 65535, 65536, 65537 samples)
    assert probes[6][6] == -1 and probes[7][5:7] == [W - 2, W - 1]
    images_end, part, nacc, rs_tiles, ntile, lg_probes, nlg, lg_runs, nlgrun, nwin = take("fill")[0]
    assert images_end == img and part == (img + 3) // 4 * 4 and nacc == part + 2 * (2 * 256 + 4) * len(tiles)
    assert [rs_tiles, ntile, lg_probes, nlg, lg_runs, nlgrun, nwin] == [len(tiles)] * 2 + [len(probes)] * 2 + [len(runs)] * 2 + [len(windows)]
    plain, o_tile, o_run, o_probe, o_img, total = take("lists")[0]
    assert plain == o_tile and o_run >= o_tile + 16 * len(tiles) and o_probe >= o_run + 4 * len(runs) and o_img >= o_probe + 80 * len(probes) and total >= o_img + 32 * W
    assert o_run % 256 == 0 and o_probe % 256 == 0 and o_img % 256 == 0 and total % 256 == 0
    assert take("same") == [[1]]                                    # the older kinds' records: unchanged byte for byte


def test_tiles_of_whole_stream_probes_reach_the_launch_bound(programs):
    """wx_lag_count over probes of 2^32 - 1 needle samples, 1 lag and 8 pairs, 2^35 products each: 32 of them are 2^24 tiles, one more
    than WX_MAX_TILES, the most workgroups of 256 threads whose launch stays below 2^32 threads; 31 stay below"""
    n = (1 << 32) - 1
    counts = {}
    for nq in (31, 32):
        text = "0 1 8192 %d %d\n" % (n, nq) + "1 0 %d 0 %d 0 1 8 1 1\n" % (n, n) * nq
        outs = [subprocess.run([exe, "count"], input=text, capture_output=True, text=True) for exe in programs]
        assert all(r.returncode == 0 for r in outs) and outs[0].stdout == outs[1].stdout, [r.stderr for r in outs]
        word, tiles, runs, probes, most = outs[0].stdout.split()
        assert word == "count" and (int(runs), int(probes), int(most)) == (8 * nq, nq, 0xFFFFFF)
        counts[nq] = int(tiles)
    assert counts == {31: 31 * 8 * 65536, 32: 1 << 24} and counts[31] <= 0xFFFFFF < counts[32] and (0xFFFFFF + 1) * 256 == 1 << 32
