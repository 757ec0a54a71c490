"""Overlaying windows of several resident .lnn streams, without a GPU (include/linne_amd.h LINNEAmd_OverlayWindowsDevice;
linne_amd.fade, linne_amd.crossfade): the reference of tests/overlay_refs.py against hand-written values, the two ramp helpers, the
boundary through the C entry point (an output's own argument checks come before any device work), the structs compiled against the
header, the plan's source images, output records and tiles from a stand-alone program, and the command line tool's -J parsing."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import linne_amd
from overlay_refs import UNIT, expected_overlay, fade_ref, gains, overlaid_values
from signals import music
from test_cli_cpu import CLI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linne_amd", "csrc")
OK, INVALID_ARGUMENT = 0, 1
SILENT = 1


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_the_reference_against_hand_written_values():
    x = np.array([[10, -20, 30, -40, 50], [1, 2, 3, 4, 5]], dtype=np.int32)
    z = np.array([[100, 200, 300], [7, 8, 9]], dtype=np.int32)
    y, sat = overlaid_values(5, [(x, 0, 5, 0, 1)])
    assert np.array_equal(y, x) and not sat                                     # one unity source at 0: the identity
    y, _ = overlaid_values(7, [(x, 1, 3, 2, 1)])
    assert y.tolist() == [[0, 0, -20, 30, -40, 0, 0], [0, 0, 2, 3, 4, 0, 0]]     # a gap in front and behind: zeros
    y, _ = overlaid_values(5, [(x, 0, 5, 0, 2), (z, 0, 3, 1, -1)])
    assert y[0].tolist() == [20, -140, -140, -380, 100] and y[1].tolist() == [2, -3, -2, -1, 10]
    y, _ = overlaid_values(4, [(x, 0, 3, 0, 1), (x, 1, 3, 1, 1)])               # one stream twice, overlapping itself
    assert y[0].tolist() == [10, -40, 60, -40]
    # a ramp: gain 3 at sample 0, half a unit less per sample -> floors 3, 2, 2, 1, 1
    assert gains(3 * UNIT, -UNIT // 2, 5).tolist() == [3, 2, 2, 1, 1]
    y, _ = overlaid_values(5, [(x, 0, 5, 0, (3 * UNIT, -UNIT // 2))])
    assert y[0].tolist() == [30, -40, 60, -40, 50]
    # negative Q32 fractions: -0.25 is the gain -1, -1 - 2^-32 the gain -2, and 2^32 - 1 units the gain 0
    assert gains(-UNIT // 4, 0, 2).tolist() == [-1, -1] and gains(-UNIT - 1, 0, 1).tolist() == [-2] and gains(UNIT - 1, 0, 1).tolist() == [0]
    assert gains(-1, -1, 3).tolist() == [-1, -1, -1] and gains(0, -1, 3).tolist() == [0, -1, -1]
    y, _ = overlaid_values(5, [(x, 0, 5, 0, (-UNIT // 4, 0))])
    assert y[0].tolist() == [-10, 20, -30, 40, -50]
    assert gains(5 * UNIT, 3, 5000).tolist() == [(5 * UNIT + 3 * i) >> 32 for i in range(5000)]        # the long form is the short one
    # the shift rounds halves up, the clip and the formats
    y, _ = overlaid_values(5, [(x, 0, 5, 0, 1), (x, 0, 5, 0, 2)], shift=2)
    assert y[0].tolist() == [8, -15, 23, -30, 38]                                # 30/4 = 7.5 -> 8, -60/4 = -15, 90/4 = 22.5 -> 23
    big = np.array([[1 << 30, -(1 << 30), 100]], dtype=np.int32)
    y, sat = overlaid_values(3, [(big, 0, 3, 0, 4)])
    assert y[0].tolist() == [(1 << 31) - 1, -(1 << 31), 400] and sat
    y, sat = overlaid_values(3, [(big, 0, 3, 0, 4)], shift=2, clip_bits=16)
    assert y[0].tolist() == [32767, -32768, 100] and sat
    got, sat = expected_overlay(1, [(big, 2, 1, 0, 1)], fmt="s24")
    assert got.tolist() == [[[100, 0, 0]]] and not sat
    got, sat = expected_overlay(3, [(big, 0, 3, 0, 1)], fmt="s16")
    assert got.tolist() == [[32767, -32768, 100]] and sat
    got, _ = expected_overlay(1, [(big, 2, 1, 0, 1)], fmt="f32", bits=8)
    assert got.tolist() == [[100 / 128]]
    got, _ = expected_overlay(1, [(big, 2, 1, 0, 1)], clip_bits=24, fmt="f32", bits=8)
    assert got.tolist() == [[100 / (1 << 23)]]
    with pytest.raises(AssertionError):
        gains(32768 * UNIT, 0, 1)


# ---- the ramp helpers ----------------------------------------------------------------------------------------------------------
def test_fade_hits_both_ends_exactly():
    g = linne_amd.overlay_gain
    for g0, g1, n in ((0, 16384, 1), (16384, 0, 1), (0, 1, 2), (32767, -32768, 65537), (-32768, 32767, 65537), (5, 5, 9), (-3, 4, 7), (4, -3, 7), (0, 32767, 3),
                      (16384, 0, 4410), (0, 16384, 4411), (1, 0, 1 << 20), (-1, 0, 1 << 20), (32767, -32768, (1 << 31) - 1)):
        q, step = linne_amd.fade(g0, g1, n)
        assert (q, step) == fade_ref(g0, g1, n) and g(q, step, 0) == g0 and g(q, step, n) == g1, (g0, g1, n)
        lo, hi = min(g0, g1), max(g0, g1)
        assert all(lo <= g(q, step, i) <= hi for i in {1, n // 2, n - 1}), (g0, g1, n)      # and stays between them
        if n <= 65537:
            ramp = gains(q, step, n)
            assert np.all(np.diff(ramp) >= 0) if g1 >= g0 else np.all(np.diff(ramp) <= 0)
    for bad in ((0, 32768, 5), (-32769, 0, 5), (0, 1, 0), (0, 1, -1)):
        with pytest.raises(ValueError):
            linne_amd.fade(*bad)


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 65537])
@pytest.mark.parametrize("unity", [1, 16384, 32767])
def test_crossfade_sums_to_unity_at_every_sample(n, unity):
    (a, sa), (b, sb) = linne_amd.crossfade(n, unity)
    assert (a, sa) == linne_amd.fade(unity, 0, n) and (b, sb) == ((unity << 32) + (1 << 32) - 1 - a, -sa)
    down, up = gains(a, sa, n), gains(b, sb, n)
    assert np.array_equal(down + up, np.full(n, unity)) and down[0] == unity and up[0] == 0
    assert down.min() >= 0 and up.max() <= unity and np.all(np.diff(down) <= 0) and np.all(np.diff(up) >= 0)
    assert [linne_amd.overlay_gain(a, sa, i) + linne_amd.overlay_gain(b, sb, i) for i in (0, n // 2, n - 1)] == [unity] * 3


def test_crossfade_bounds():
    for bad in ((0, 16384), (-1, 16384), (5, 0), (5, 32768)):
        with pytest.raises(ValueError):
            linne_amd.crossfade(*bad)


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_symbol_structs_and_kind_are_declared_listed_and_exported(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "linne_amd.h")).read(), flags=re.S)
    name = "LINNEAmd_OverlayWindowsDevice"
    assert re.search(r"\b%s\s*\(" % name, src) and name in linne_amd.AMD_SYMBOLS and hasattr(linne_amd.lib, name)
    assert re.search(r"LINNE_AMD_OVERLAY_T_OVERLAY\s*=\s*101\b", src) and linne_amd.OVERLAY_MAX_SOURCES == 64
    S, O = linne_amd.OverlaySource, linne_amd.Overlay
    assert [(f[0], getattr(S, f[0]).offset) for f in S._fields_] == [("index", 0), ("d_stream", 8), ("first_sample", 16), ("num_samples", 24), ("at", 32), ("gain_q32", 40),
                                                                    ("step_q32", 48), ("reserved", 56)]
    assert [(f[0], getattr(O, f[0]).offset) for f in O._fields_] == [("sources", 0), ("num_sources", 8), ("shift", 12), ("clip_bits", 16), ("reserved", 20), ("num_samples", 24),
                                                                    ("d_pcm", 32), ("pcm_stride", 40), ("result", 48)]
    assert (C.sizeof(S), C.sizeof(O)) == (64, 56)
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler holds the structs to the header"
    code, exe = tmp_path / "size.c", tmp_path / "size"
    fields = ["sizeof(struct LINNEAmdOverlaySource)", "sizeof(struct LINNEAmdOverlay)"]
    fields += ["offsetof(struct LINNEAmdOverlaySource, %s)" % f[0] for f in S._fields_] + ["offsetof(struct LINNEAmdOverlay, %s)" % f[0] for f in O._fields_]
    code.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "linne_amd.h"\nint main(void) { size_t v[] = { %s }; size_t i; for (i = 0; i < sizeof(v) / sizeof(v[0]); i++) printf("%%zu ", v[i]); '
                    'printf("%%d %%d\\n", (int)LINNE_AMD_OVERLAY_T_OVERLAY, LINNE_AMD_OVERLAY_MAX_SOURCES); return 0; }\n' % ", ".join(fields))
    b = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(code), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    want = [64, 56] + [getattr(S, f[0]).offset for f in S._fields_] + [getattr(O, f[0]).offset for f in O._fields_] + [101, 64]
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == want


def test_python_entry_points():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(linne_amd.Context.overlay_windows)
    assert list(p) == ["self", "outputs", "shift", "clip_bits", "out", "group_frames", "return_codes", "dtype", "channels_last", "s24", "return_saturated"]
    assert [p[k].default for k in list(p)[2:]] == [0, 0, None, 0, False, None, False, False, False]
    p = sig(linne_amd.Context.overlay_streams)
    assert list(p)[:8] == ["self", "jobs", "shift", "bits", "preset", "block", "ms", "group_frames"] and [p[k].default for k in list(p)[3:8]] == [None, None, None, None, 0]
    assert list(sig(linne_amd.Context.crossfade_streams))[:3] == ["self", "streams", "overlap"]
    assert list(sig(linne_amd.fade)) == ["g0", "g1", "n"] and list(sig(linne_amd.crossfade)) == ["n", "unity"]
    p = sig(linne_amd.Context.decode_windows)                   # decode_windows is what it was
    assert list(p) == ["self", "windows", "out", "group_frames", "return_codes", "dtype", "channels_last", "s24", "return_saturated"]


TOP = (1 << 64) - 1
# every INVALID_ARGUMENT case that needs no index: (the output's fields, source 1's fields, a word of the text)
BAD = [(dict(num_sources=0), {}, "num_sources 0"), (dict(num_sources=65), {}, "num_sources 65"), (dict(sources=None), {}, "null sources"), (dict(shift=32), {}, "shift 32"),
       (dict(clip_bits=1), {}, "clip_bits 1"), (dict(clip_bits=33), {}, "clip_bits 33"), (dict(reserved=1), {}, "reserved"),
       ({}, dict(index=None), "source 1: null argument"), ({}, dict(d_stream=None), "source 1: null argument"), ({}, dict(reserved=1 << 40), "source 1: reserved"),
       ({}, dict(num_samples=0), "source 1: num_samples 0"), ({}, dict(at=91), "source 1: at 91 + 10 samples beyond the output's 100"),
       ({}, dict(at=101, num_samples=1), "beyond the output's 100"), ({}, dict(at=TOP, num_samples=2), "beyond the output's 100"), ({}, dict(at=5, num_samples=TOP), "beyond the output's 100"),
       ({}, dict(gain_q32=32768 << 32), "source 1: a gain outside"), ({}, dict(gain_q32=(-32768 << 32) - 1), "a gain outside"),
       ({}, dict(gain_q32=32767 << 32, step_q32=1 << 29), "a gain outside"),                                     # 9 steps of an eighth: 32768 at the last sample
       ({}, dict(gain_q32=0, step_q32=-(1 << 63)), "a gain outside"), ({}, dict(gain_q32=(1 << 63) - 1, step_q32=(1 << 63) - 1), "a gain outside"),
       ({}, dict(index="three channels"), "source 1: 3 channels, source 0 has 2"),
       (dict(d_pcm=None), {}, "null d_pcm"), (dict(pcm_stride=99), {}, "pcm_stride 99 < 100 samples")]
# the layout's checks, with the sources' 2 channels: (the output's fields, -, the layout's fields, a word of the text)
LAYOUT_BAD = [({}, {}, dict(format=4), "a PCM format this call does not take"), ({}, {}, dict(channel_stride=99), "let two samples share an element"),
              ({}, {}, dict(channel_stride=1, sample_stride=1), "let two samples share an element"), ({}, {}, dict(channel_stride=0), "let two samples share an element"),
              ({}, {}, dict(sample_stride=0), "let two samples share an element"), ({}, {}, dict(channel_stride=1 << 62), "let two samples share an element"),
              (dict(d_pcm="two bytes on"), {}, dict(format=0, channel_stride=1, sample_stride=2), "not aligned to its format's element")]


class FakeIndex(C.Structure):
    """how struct LINNEAmdStreamIndex begins (linne_amd/csrc/lnn_device.hip); the rest is zeroed room"""
    _fields_ = [("device", C.c_int), ("header", linne_amd.Header), ("shape", linne_amd.Shape), ("rest", C.c_char * 4096)]


def test_arguments_are_checked_before_any_device_work():
    f = linne_amd.lib.LINNEAmd_OverlayWindowsDevice
    err = linne_amd.lib.LINNEAmd_GetLastError
    o = (linne_amd.Overlay * 2)()
    assert f(None, o, None, 2, 0) == INVALID_ARGUMENT and f(None, None, None, 0, 0) == INVALID_ARGUMENT
    blank = C.create_string_buffer(1 << 20)                     # zeroed memory larger than any context stands in for one
    ctx = C.addressof(blank)
    assert f(ctx, None, None, 2, 0) == INVALID_ARGUMENT and b"OverlayWindowsDevice: null argument" in err(ctx)
    assert f(ctx, None, None, 0, 0) == OK and f(ctx, o, None, 0, 0) == OK
    # Memory laid out as an index begins -- its device, its header, its shape -- stands in for indexes of 2 and of 3 channels; their
    # streams hold no samples, which the sources' own check says.  LINNEAmd_StreamIndexHeader holds the stand-in to the library's layout
    index = [FakeIndex() for _ in range(3)]
    for x, nch in zip(index, (2, 2, 3)):
        x.header.num_channels = x.shape.num_channels = nch
        x.shape.bits_per_sample = x.header.bits_per_sample = 16
        back = linne_amd.Header()
        assert linne_amd.lib.LINNEAmd_StreamIndexHeader(C.c_void_p(C.addressof(x)), C.byref(back)) == OK and (back.num_channels, back.bits_per_sample, back.num_samples) == (nch, 16, 0)
    stream = C.create_string_buffer(64)
    pcm = C.create_string_buffer(1024)
    ly = (linne_amd.PcmLayout * 2)()

    def fill(out_fields, src_fields, lay_fields=None):
        srcs = [(linne_amd.OverlaySource * 64)() for _ in range(2)]
        for k in range(2):
            for j in range(2):
                s = srcs[k][j]
                s.index, s.d_stream, s.first_sample, s.num_samples, s.at, s.gain_q32, s.step_q32, s.reserved = C.addressof(index[j]), C.addressof(stream), 0, 10, 0, 1 << 32, 0, 0
            o[k].sources, o[k].num_sources, o[k].shift, o[k].clip_bits, o[k].reserved, o[k].num_samples = srcs[k], 2, 0, 0, 0, 100
            o[k].d_pcm, o[k].pcm_stride, o[k].result = C.addressof(pcm), 100, -1
            ly[k].format, ly[k].saturated, ly[k].channel_stride, ly[k].sample_stride = linne_amd.PCM_S16, 7, 100, 1
        for k, v in src_fields.items():
            setattr(srcs[1][1], k, C.addressof(index[2]) if v == "three channels" else v)
        for k, v in out_fields.items():
            setattr(o[1], k, C.addressof(pcm) + 2 if v == "two bytes on" else v)
        for k, v in (lay_fields or {}).items():
            setattr(ly[1], k, v)
        return srcs

    assert C.addressof(pcm) % 4 == 0
    for out_fields, src_fields, lay_fields, word in [b[:2] + (None, b[2]) for b in BAD] + LAYOUT_BAD:
        layouts = ly if lay_fields is not None else None
        keep = fill(out_fields, src_fields, lay_fields)
        assert f(ctx, o, layouts, 2, 0) == INVALID_ARGUMENT
        assert [o[k].result for k in range(2)] == [INVALID_ARGUMENT] * 2
        # output 0 passes its own checks: its sources are checked as windows are, and their streams hold no samples
        assert err(ctx) == b"output 0: source 0: DecodeStreamDevice: samples [0, 10) beyond the stream's 0", (out_fields, src_fields, lay_fields)
        o[0], ly[0] = o[1], ly[1]
        assert f(ctx, o, layouts, 1, 0) == INVALID_ARGUMENT and o[0].result == INVALID_ARGUMENT
        text = err(ctx).decode()
        assert text.startswith("output 0: OverlayWindowsDevice: ") and word in text, (out_fields, src_fields, lay_fields, text)
        assert [ly[k].saturated for k in range(2)] == [7, 7]       # a failing output's stays as it was
        del keep
    assert set(pcm.raw) == {0}
    if linne_amd.device_count() == 0:                           # no device: no context, and so no call -- nothing computes in its place
        with pytest.raises(Exception):
            linne_amd.Context(0).overlay_windows([])


# ---- the tool ------------------------------------------------------------------------------------------------------------------
def test_cli_usage_and_join_spec_errors(oracle, tmp_path):
    assert os.path.exists(CLI), "linne_amd_cli is not built (python -c 'import __graft_entry__ as g; g.build()')"
    run = lambda *a: subprocess.run([CLI, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    text = run("-h").stdout
    assert re.search(r"-J, --join\b", text) and "-J OTHER.lnn[,OVERLAP] IN.lnn OUT.lnn" in text
    src, other, mono, dst = tmp_path / "a.lnn", tmp_path / "b.lnn", tmp_path / "m.lnn", tmp_path / "c.lnn"
    src.write_bytes(bytes(oracle.encode_whole(music(2, 2 * 1024, 16, seed=1), 16, 44100, 1024, 0, True)))
    other.write_bytes(bytes(oracle.encode_whole(music(2, 1500, 16, seed=2), 16, 44100, 1024, 0, True)))
    mono.write_bytes(bytes(oracle.encode_whole(music(1, 1500, 16, seed=3), 16, 44100, 1024, 0, False)))
    for spec, word in (("", "a file name is expected"), (",5", "a file name is expected"), (f"{other},", "an overlap in samples is expected"),
                       (f"{other},x", "an overlap in samples is expected"), (f"{other},-1", "an overlap in samples is expected"), (f"{other},+1", "an overlap in samples is expected"),
                       (f"{other},5x", "malformed"), (f"{other},5.5", "malformed"), (f"{other},99999999999", "outside 0 .."),
                       (str(tmp_path / "missing.lnn"), "Failed to open"), (f"{tmp_path / 'missing.lnn'},7", "Failed to open"),
                       (str(mono), "cannot be joined"), (f"{other},1501", "an overlap of 1501 samples"), (f"{other},2049", "an overlap of 2049 samples")):
        r = run("-J", spec, str(src), str(dst))
        assert r.returncode == 1 and word in r.stderr and not dst.exists(), (spec, r.stderr)
    assert run("-J", str(other), str(src)).returncode == 1 and run("-J", str(other), "-e", str(src), str(dst)).returncode == 1
    assert "-J takes" in run("-J", str(other), str(src)).stderr and "-J takes" in run("-J", str(other), "-Z", "16000", str(src), str(dst)).stderr
    r = run("-J", str(other), str(tmp_path / "missing.lnn"), str(dst))
    assert r.returncode == 1 and "Failed to open" in r.stderr


# ---- the plan ------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "lnn_windows_plan.h"
/* stdin: group_frames nblocks S N noutputs, then per output: n nsrc checked, and per source: first n at gain step live.  One stream
 * of two channels, nblocks SILENT blocks of S samples, N samples in its header.  Out come the counts, per live source its window record,
 * the source records of all windows, the output records and the tiles -- and whether the same ranges planned for the placing call give
 * the same block records, byte for byte */
int main(void)
{
    unsigned gf, nb, S, no; unsigned long long N;
    if (scanf("%u %u %u %llu %u", &gf, &nb, &S, &N, &no) != 5) return 2;
    std::vector<uint64_t> off(nb), first(nb); std::vector<uint32_t> size(nb, 5), type(nb, SX_SILENT), nsmp(nb, S);
    for (unsigned r = 0; r < nb; r++) { off[r] = 30 + 11ull * r; first[r] = (uint64_t)S * r; }
    WxIndexView x; memset(&x, 0, sizeof(x));
    x.shape.num_channels = 2; x.shape.bits_per_sample = 16; x.shape.num_samples_per_block = S; x.nb = nb; x.covered = (uint64_t)S * nb; x.stream_bytes = 30 + 11ull * nb;
    x.h_off = off.data(); x.h_first = first.data(); x.h_size = size.data(); x.h_type = type.data(); x.h_nsmp = nsmp.data();
    std::vector<WxOvOut> outs(no); std::vector<WxRange> rg; std::vector<struct LINNEAmdOverlaySource> src;
    for (unsigned k = 0; k < no; k++) {
        unsigned long long n; unsigned ns; int checked;
        if (scanf("%llu %u %d", &n, &ns, &checked) != 3) return 2;
        WxOvOut &o = outs[k];
        memset(&o, 0, sizeof(o));
        o.w0 = (uint32_t)src.size(); o.nsrc = checked ? ns : 0; o.checked = checked; o.n = n; o.out = (void *)(uintptr_t)(0x1000 * (k + 1));
        o.stride = 1; o.sstride = 2; o.fmt = LINNE_AMD_PCM_F32; o.shift = k % 32; o.clip_bits = k % 2 ? 12 : 0;
        for (unsigned j = 0; j < ns; j++) {
            unsigned long long f, m, at; long long g, st; int live;
            if (scanf("%llu %llu %llu %lld %lld %d", &f, &m, &at, &g, &st, &live) != 6) return 2;
            if (!checked) continue;                             /* (an output that failed its own checks brings no windows) */
            struct LINNEAmdOverlaySource s; memset(&s, 0, sizeof(s));
            s.first_sample = f; s.num_samples = m; s.at = at; s.gain_q32 = g; s.step_q32 = st;
            src.push_back(s);
            WxRange r; memset(&r, 0, sizeof(r));
            r.x = x; r.stream = (const uint8_t *)(uintptr_t)0x30000; r.live = live; r.lo = f; r.n = m;
            r.r1 = (f + m - 1u < x.covered) ? wx_block_of(x.h_first, x.nb, f + m - 1u) : x.nb;
            rg.push_back(r);
        }
    }
    const uint32_t W = (uint32_t)rg.size();
    for (uint32_t i = 0; i < W; i++) rg[i].ov = &src[i];
    WxPlanned p;
    if (wx_plan_count(rg.data(), W, gf, p) != WXP_OK) return 3;
    wx_overlay_count(outs.data(), no, p);
    /* exactly the reserved sizes, from the heap: the sanitizer build sees a record written past them */
    std::vector<WxWindow> win(p.nlive); std::vector<WxBlock> rec(p.total_rec); std::vector<uint32_t> crec(p.total_crec);
    std::vector<WxTile> tile(p.rs_tiles); std::vector<WxOvOutput> orec(p.ov_outs); std::vector<WxOvSource> srec(W);
    if (W) memset(srec.data(), 0, sizeof(WxOvSource) * W);
    wx_plan_fill(rg.data(), W, gf, WX_NO_BUCKETS, p, win.data(), NULL, rec.data(), crec.data(), NULL, NULL, NULL, NULL, srec.data());
    wx_overlay_fill(outs.data(), no, rg.data(), p, orec.data(), tile.data());
    const WxLists plain = wx_lists(p, W, 0, 0), ls = wx_lists(p, W, 0, 0, false, true);
    printf("fill %llu %llu %llu %llu %llu %u %u\n", (unsigned long long)p.nacc, (unsigned long long)p.rs_tiles, (unsigned long long)p.ntile, (unsigned long long)p.ov_outs, (unsigned long long)p.nov, p.nwin, p.nrec);
    printf("lists %llu %llu %llu %llu %llu %llu\n", (unsigned long long)plain.bytes, (unsigned long long)plain.o_tile, (unsigned long long)ls.o_tile, (unsigned long long)ls.o_ovout, (unsigned long long)ls.o_ovsrc, (unsigned long long)ls.bytes);
    for (uint32_t k = 0; k < p.nwin; k++) {
        const WxWindow &w = win[k];
        printf("window %u %llu %llu %llu %llu %u %llu\n", w.fidx, (unsigned long long)w.lo, (unsigned long long)w.hi, (unsigned long long)(uintptr_t)w.out, (unsigned long long)w.stride, w.fmt, (unsigned long long)w.sstride);
    }
    for (uint32_t i = 0; i < W; i++) {
        const WxOvSource &m = srec[i];
        printf("source %llu %llu %llu %llu %lld %lld\n", (unsigned long long)m.img, (unsigned long long)m.istride, (unsigned long long)m.at, (unsigned long long)m.n, (long long)m.gain, (long long)m.step);
    }
    for (const WxOvOutput &m : orec)
        printf("output %llu %llu %llu %llu %u %u %u %u %d %d %u %u\n", (unsigned long long)(uintptr_t)m.out, (unsigned long long)m.stride, (unsigned long long)m.sstride, (unsigned long long)m.n, m.src0, m.nsrc, m.C, m.shift, m.lo, m.hi, m.scale_bits, m.fmt);
    for (const WxTile &t : tile) printf("tile %u %u %llu %llu\n", t.win, t.p0, (unsigned long long)t.m0, (unsigned long long)t.n0);
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
PLAN_N = 10 * 64 - 7                                            # the header names a little less than the blocks hold
# (samples, checked, sources (first, n, at, gain, step, live)): one source, a tile and one more, sources of 1 and of 4 k + 1 .. 4 k + 4
# samples, one stream twice, a source in the tail behind the blocks, an output whose own checks failed, one with a failing source
PLAN_OUTPUTS = [(257, 1, [(0, 257, 0, 1 << 32, 0, 1)]),
                (1000, 1, [(5, 1, 0, 3 << 32, -7, 1), (100, 2, 255, -(1 << 31), 1, 1), (0, 3, 256, 5, 5, 1), (60, 4, 512, 0, 0, 1), (63, 5, 995, 1, 2, 1)]),
                (300, 0, [(0, 300, 0, 1 << 32, 0, 0)]),
                (PLAN_N, 1, [(0, PLAN_N, 0, 1 << 46, -(1 << 36), 1), (PLAN_N - 10, 10, 3, 9, 9, 1)]),
                (512, 1, [(0, 100, 0, 1 << 32, 0, 1), (0, 700, 0, 1 << 32, 0, 0), (64, 64, 448, 2 << 32, 0, 1)]),
                (1, 1, [(PLAN_N - 1, 1, 0, -1, 0, 1)])]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlay_plan")
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
def test_plan_images_outputs_and_tiles(programs, gf):
    text = "%d 10 64 %d %d\n" % (gf, PLAN_N, len(PLAN_OUTPUTS))
    for n, checked, sources in PLAN_OUTPUTS:
        text += "%d %d %d\n" % (n, len(sources), checked) + "".join(" ".join(str(v) for v in s) + "\n" for s in sources)
    outs = []
    for exe in programs:
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = [x.split() for x in outs[0].splitlines()]
    # what Python makes of the same outputs
    windows, sources, records, tiles, img, w0 = [], [], [], [], 0, 0
    for k, (n, checked, srcs) in enumerate(PLAN_OUTPUTS):
        if not checked:
            continue
        for j, (first, m, at, gain, step, live) in enumerate(srcs):
            if not live:
                sources.append([0] * 6)
                continue
            istride = (m + 3) // 4 * 4
            windows.append([w0 + j, first, first + m, 4 * img, istride, 0, 1])       # the window's target is its image: int32, sample stride 1
            sources.append([img, istride, at, m, gain, step])
            img += 2 * istride
        if all(s[5] for s in srcs):
            B, Bf = (12, 12) if k % 2 else (32, 16)
            records.append([0x1000 * (k + 1), 1, 2, n, w0, len(srcs), 2, k % 32, -(1 << (B - 1)), (1 << (B - 1)) - 1, int(np.float32(2.0 ** -(Bf - 1)).view(np.uint32)), 3])
            tiles += [[len(records) - 1, 0, t0, 0] for t0 in range(0, n, 256)]
        w0 += len(srcs)
    take = lambda word: [[int(v) for v in x[1:]] for x in lines if x[0] == word]
    assert take("window") == windows and take("source") == sources and take("output") == records and take("tile") == tiles
    assert len(records) == 4 and len(tiles) == 2 + 4 + 3 + 1        # (the premise: outputs 2 and 4 have no tiles)
    fill = take("fill")[0]
    assert fill[:6] == [img, len(tiles), len(tiles), len(records), len(records), len(windows)]
    plain, plain_tile, o_tile, o_out, o_src, total = take("lists")[0]
    assert plain_tile == plain == o_tile and o_out >= o_tile + 24 * len(tiles) and o_src >= o_out + 80 * len(records) and total >= o_src + 48 * w0
    assert o_out % 256 == 0 and o_src % 256 == 0 and total % 256 == 0
    assert take("same") == [[1]]                                    # the older kinds' records: unchanged byte for byte
