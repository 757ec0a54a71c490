"""Resampling windows of resident .lnn streams, without a GPU (include/linne_amd.h LINNEAmd_ResampleWindowsDevice, LINNEAmd_ResampleLength,
LINNEAmd_ResampleDesign; linne_amd.resample_ratio): the reference of tests/resample_refs.py against hand-written values, the host
functions, the designed filters' quality against the Kaiser formula, the boundary through the C entry point (its per-window argument
checks come before any device work), and the plan's input ranges, images and tiles from a stand-alone program."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import linne_amd
from signals import music
from test_cli_cpu import CLI
from resample_refs import expected_resample, kaiser_prototype, prototype_of, resampled_length, resampled_values, stopband_db

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linne_amd", "csrc")
OK, INVALID_ARGUMENT = 0, 1
SILENT = 1


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_the_reference_against_hand_written_values():
    x = np.array([[10, -20, 30, -40, 50, 60, 70], [1, 2, 3, 4, 5, 6, 7]], dtype=np.int32)
    one = [[1]]
    y, sat = resampled_values(x, 0, 7, one, 1, 1, 0)
    assert np.array_equal(y, x) and not sat                                        # 1/1, P = 1: the identity
    y, _ = resampled_values(x, 0, 4, one, 1, 2, 0)
    assert resampled_length(7, 1, 2) == 4 and y.tolist() == [[10, 30, 50, 70], [1, 3, 5, 7]]        # 1/2: the even samples
    y, _ = resampled_values(x, 1, 2, one, 1, 2, 0)
    assert y.tolist() == [[30, 50], [3, 5]]                                         # a window counts output samples
    y, _ = resampled_values(x, 0, 14, [[1], [0]], 2, 1, 0)
    assert y[0].tolist() == [10, 0, -20, 0, 30, 0, -40, 0, 50, 0, 60, 0, 70, 0]   # 2/1 with phases {1}, {0}: zero-stuffing
    y, _ = resampled_values(x, 0, 7, [[1, 1]], 1, 1, 0, shift=1)
    assert y[0].tolist() == [-5, 5, -5, 5, 55, 65, 35]                              # a two-tap average: halves round up, 0 behind N
    y, _ = resampled_values(x, 0, 7, [[1, 1]], 1, 1, 1, shift=1)
    assert y[0].tolist() == [5, -5, 5, -5, 5, 55, 65]                               # before = 1: 0 in front of sample 0
    # an impulse through 3/2: x[4] = 1; output m reads x[n - before + k] through coef[p][k], t = 2 m, p = t % 3, n = t // 3
    imp = np.zeros((1, 9), dtype=np.int32)
    imp[0, 4] = 1
    coef = np.arange(1, 13).reshape(3, 4)                                           # coef[p][k] = 4 p + k + 1
    y, _ = resampled_values(imp, 0, resampled_length(9, 3, 2), coef, 3, 2, 1)
    want = np.zeros(14, dtype=np.int64)
    for m in range(14):
        p, n = (2 * m) % 3, (2 * m) // 3
        k = 4 - (n - 1)
        if 0 <= k < 4:
            want[m] = coef[p][k]
    assert y[0].tolist() == want.tolist() == [0, 0, 0, 4, 12, 7, 2, 10, 5, 0, 0, 0, 0, 0]      # every second point of the prototype (prototype_of)
    assert prototype_of(coef)[0::2].tolist() == [4, 12, 7, 2, 10, 5]
    # the clip and the formats
    big = np.array([[1 << 30, -(1 << 30), 100]], dtype=np.int32)
    y, sat = resampled_values(big, 0, 3, [[4]], 1, 1, 0)
    assert y[0].tolist() == [(1 << 31) - 1, -(1 << 31), 400] and sat
    y, sat = resampled_values(big, 0, 3, [[4]], 1, 1, 0, shift=2, clip_bits=16)
    assert y[0].tolist() == [32767, -32768, 100] and sat
    got, sat = expected_resample(big, 2, 1, [[1]], 1, 1, 0, fmt="s24")
    assert got.tolist() == [[[100, 0, 0]]] and not sat
    got, sat = expected_resample(big, 0, 3, [[1]], 1, 1, 0, fmt="s16")
    assert got.tolist() == [[32767, -32768, 100]] and sat
    got, _ = expected_resample(big, 2, 1, [[1]], 1, 1, 0, fmt="f32", bits=8)
    assert got.tolist() == [[100 / 128]]
    got, _ = expected_resample(big, 2, 1, [[1]], 1, 1, 0, clip_bits=24, fmt="f32", bits=8)
    assert got.tolist() == [[100 / (1 << 23)]]


# ---- the host functions --------------------------------------------------------------------------------------------------------
def test_resample_length_against_python_integers():
    f = linne_amd.lib.LINNEAmd_ResampleLength
    top = (1 << 64) - 1
    for n in (0, 1, 2, 146, 147, 148, 441, (1 << 32) - 1, 1 << 32, (1 << 53) + 1, top // 1024, top // 1024 + 1, top - 1, top):
        for up, down in ((1, 1), (1, 2), (2, 1), (3, 2), (160, 147), (160, 441), (441, 80), (1024, 1), (1, 1024), (1024, 1023), (1 << 31, 3), ((1 << 32) - 1, (1 << 32) - 1)):
            assert f(n, up, down) == min(-(-(n * up) // down), top), (n, up, down)
    assert f(5, 1, 0) == 0 and linne_amd.resample_length(7, 3, 2) == 11


def test_resample_ratio():
    r = linne_amd.resample_ratio
    assert r(44100, 16000) == (160, 441) and r(44100, 48000) == (160, 147) and r(48000, 44100) == (147, 160)
    assert r(44100, 22050) == (1, 2) and r(48000, 24000) == (1, 2) and r(16000, 16000) == (1, 1) and r(8000, 48000) == (6, 1)
    assert r(1024, 1) == (1, 1024) and r(3, 3072) == (1024, 1)
    for bad in ((44100, 44101), (1025, 1), (1, 1025), (0, 5), (5, 0), (-1, 2)):
        with pytest.raises(ValueError):
            r(*bad)


DESIGNS = [(1, 1, 1), (1, 1, 2), (1, 1, 32), (1, 1, 33), (1, 2, 32), (2, 1, 16), (3, 2, 4), (160, 441, 32), (160, 147, 32), (147, 160, 64), (1, 1024, 64), (1024, 1, 16), (256, 3, 64), (5, 5, 7)]


@pytest.mark.parametrize("up,down,taps", DESIGNS)
def test_design(up, down, taps):
    coef, shift, before = linne_amd.resample_design(up, down, taps)
    assert coef.dtype == np.int16 and coef.shape == (up, taps) and shift in (14, 15) and before == (taps - 1) // 2
    assert set(coef.astype(np.int64).sum(axis=1).tolist()) == {1 << shift}          # a constant stays that constant
    x = np.full((1, (4 * taps + 7) * -(-down // up)), -12345, dtype=np.int32)
    m0 = -(-(taps * up) // down)
    n = resampled_length(x.shape[1] - taps, up, down) - m0
    assert n > 0 and set(resampled_values(x, m0, n, coef, up, down, before, shift)[0].reshape(-1).tolist()) == {-12345}
    # the prototype is symmetric: phase p is phase L - 1 - p backwards; a phase that is its own mirror image may differ from itself
    # backwards at its largest coefficient, where its rounding remainder went
    proto = prototype_of(coef).astype(np.int64)
    diff = np.flatnonzero(proto != proto[::-1])
    own = {p + (taps - 1 - k) * up for p in range(up) if 2 * p == up - 1 for k in range(taps) if coef[p][k] == coef[p].max()}
    assert set(diff.tolist()) <= own | {proto.size - 1 - j for j in own}, (diff, own)
    # and it is the formula's, scaled phase by phase and rounded to nearest: all coefficients of a phase but one, which takes the
    # remainder of the others' rounding -- half a unit each at the most
    ideal = kaiser_prototype(up, down, taps).reshape(taps, up)[::-1].T               # [p][k]
    ideal = ideal / ideal.sum(axis=1, keepdims=True) * (1 << shift)
    off = np.sort(np.abs(coef - ideal), axis=1)
    assert (taps == 1 or off[:, :-1].max() <= 0.5 + 1e-6) and off[:, -1].max() <= 0.5 * taps + 1e-6


def test_design_bounds_are_refused():
    f = linne_amd.lib.LINNEAmd_ResampleDesign
    buf = (C.c_int16 * 16384)()
    sh, be = C.c_uint32(77), C.c_uint32(77)
    for up, down, taps in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1025, 1, 1), (1, 1025, 1), (1, 1, 65), (1024, 1, 17), (257, 1, 64), ((1 << 32) - 1, 1, 1)):
        assert f(up, down, taps, buf, C.byref(sh), C.byref(be)) == INVALID_ARGUMENT, (up, down, taps)
        with pytest.raises(ValueError):
            linne_amd.resample_design(up, down, taps)
    assert f(1, 1, 1, None, C.byref(sh), C.byref(be)) == INVALID_ARGUMENT and f(1, 1, 1, buf, None, C.byref(be)) == INVALID_ARGUMENT
    assert f(1, 1, 1, buf, C.byref(sh), None) == INVALID_ARGUMENT and (sh.value, be.value) == (77, 77) and not any(buf)
    assert f(1024, 1024, 16, buf, C.byref(sh), C.byref(be)) == OK and f(256, 1, 64, buf, C.byref(sh), C.byref(be)) == OK


@pytest.mark.parametrize("up,down", [(160, 441), (160, 147)])
def test_filter_quality(up, down):
    """The stopband attenuation of the default designs (32 taps per phase), by FFT of the quantised prototype, against the float64
    prototype from the Kaiser formula (resample_refs.kaiser_prototype, computed here: the reference is the formula).  The quantised
    design may be 6 dB worse, the allowance for rounding to 15 bits.  Measured: 160/441 79.22 dB quantised (shift 15) against 79.83 dB,
    160/147 80.34 dB (shift 14) against 81.55 dB (DESIGN.md has them too)"""
    coef, shift, _ = linne_amd.resample_design(up, down, 32)
    ideal = stopband_db(kaiser_prototype(up, down, 32), up, down, 32)
    got = stopband_db(prototype_of(coef), up, down, 32)
    print(f"stopband {up}/{down}: quantised {got:.2f} dB, float64 {ideal:.2f} dB, shift {shift}")
    assert ideal > 60.0                                            # (the premise: a Kaiser window of beta 8 has side lobes below -58 dB)
    assert got >= ideal - 6.0


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_symbols_struct_and_kinds_are_declared_listed_and_exported(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "linne_amd.h")).read(), flags=re.S)
    for name in ("LINNEAmd_ResampleWindowsDevice", "LINNEAmd_ResampleLength", "LINNEAmd_ResampleDesign"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in linne_amd.AMD_SYMBOLS and hasattr(linne_amd.lib, name), name
    assert re.search(r"LINNE_AMD_RESAMPLE_T_PRESET\s*=\s*99\b", src) and re.search(r"LINNE_AMD_RESAMPLE_T_RESAMPLE\s*=\s*100\b", src)
    R = linne_amd.ResampleSpec
    assert [(f[0], getattr(R, f[0]).offset) for f in R._fields_] == [("up", 0), ("down", 4), ("taps", 8), ("before", 12), ("shift", 16), ("clip_bits", 20), ("reserved", 24), ("coef", 32)]
    assert C.sizeof(R) == 40
    assert (linne_amd.RESAMPLE_MAX_TAPS, linne_amd.RESAMPLE_MAX_RATIO, linne_amd.RESAMPLE_MAX_COEFS) == (64, 1024, 16384)
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
    if cc:
        code, exe = tmp_path / "size.c", tmp_path / "size"
        code.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "linne_amd.h"\nint main(void) { printf("%zu %zu %zu %d %d %d %d %d\\n", sizeof(struct LINNEAmdResampleSpec), '
                        'offsetof(struct LINNEAmdResampleSpec, reserved), offsetof(struct LINNEAmdResampleSpec, coef), (int)LINNE_AMD_RESAMPLE_T_PRESET, (int)LINNE_AMD_RESAMPLE_T_RESAMPLE, '
                        'LINNE_AMD_RESAMPLE_MAX_TAPS, LINNE_AMD_RESAMPLE_MAX_RATIO, LINNE_AMD_RESAMPLE_MAX_COEFS); return 0; }\n')
        b = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(code), "-o", str(exe)], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["40", "24", "32", "99", "100", "64", "1024", "16384"]


def test_python_entry_points():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(linne_amd.Context.resample_windows)
    assert list(p) == ["self", "windows", "up", "down", "coef", "taps", "before", "shift", "clip_bits", "out", "group_frames", "return_codes", "dtype", "channels_last", "s24", "return_saturated"]
    assert [p[k].default for k in list(p)[4:]] == [None, 32, None, None, 0, None, 0, False, None, False, False, False]
    p = sig(linne_amd.Context.resample_streams)
    assert list(p) == ["self", "streams", "rate", "taps", "bits", "preset", "block", "ms", "group_frames"]
    assert [p[k].default for k in list(p)[3:]] == [32, None, None, None, None, 0]
    assert list(sig(linne_amd.resample_ratio)) == ["rate_in", "rate_out"]
    p = sig(linne_amd.Context.decode_windows)                   # decode_windows and mix_windows are what they were
    assert list(p) == ["self", "windows", "out", "group_frames", "return_codes", "dtype", "channels_last", "s24", "return_saturated"]
    assert list(sig(linne_amd.Context.mix_windows))[:5] == ["self", "windows", "matrix", "shift", "clip_bits"]


def spec_of(up=1, down=1, taps=1, before=0, shift=0, clip_bits=0, reserved=0, coef=True):
    sp = linne_amd.ResampleSpec()
    sp.up, sp.down, sp.taps, sp.before, sp.shift, sp.clip_bits, sp.reserved = up, down, taps, before, shift, clip_bits, reserved
    return sp


# every INVALID_ARGUMENT case of a window's spec, and a word of the text it gets
BAD_SPECS = [(dict(up=0), "up 0"), (dict(up=1025), "up 1025"), (dict(down=0), "down 0"), (dict(down=1025), "down 1025"), (dict(taps=0), "taps 0"),
             (dict(taps=65), "taps 65"), (dict(up=1024, taps=17), "coefficients"), (dict(up=257, taps=64), "coefficients"), (dict(taps=4, before=4), "before 4"),
             (dict(before=1), "before 1"), (dict(shift=32), "shift 32"), (dict(clip_bits=1), "clip_bits 1"), (dict(clip_bits=33), "clip_bits 33"),
             (dict(reserved=1), "reserved"), (dict(reserved=1 << 32), "reserved"), (dict(coef=False), "null coef")]


def test_arguments_are_checked_before_any_device_work():
    f = linne_amd.lib.LINNEAmd_ResampleWindowsDevice
    err = linne_amd.lib.LINNEAmd_GetLastError
    table = (C.c_int16 * 16384)()
    w, s, ly = (linne_amd.Window * 2)(), (linne_amd.ResampleSpec * 2)(), (linne_amd.PcmLayout * 2)()
    for i in range(2):
        w[i].result = -1
    assert f(None, w, s, ly, 2, 0) == INVALID_ARGUMENT and f(None, None, None, None, 0, 0) == INVALID_ARGUMENT
    blank = C.create_string_buffer(1 << 20)                     # zeroed memory larger than any context stands in for one
    ctx = C.addressof(blank)
    assert f(ctx, None, s, ly, 2, 0) == INVALID_ARGUMENT        # NULL windows
    assert f(ctx, w, None, ly, 2, 0) == INVALID_ARGUMENT        # NULL specs
    assert b"ResampleWindowsDevice: null argument" in err(ctx)
    assert f(ctx, None, None, None, 0, 0) == OK and f(ctx, w, s, None, 0, 0) == OK
    assert [w[i].result for i in range(2)] == [-1, -1]
    # a window's spec: refused with the call's name and the field, whatever else the window names (here: nothing); window 0 is sound
    # but for its stream, window 1 has the fault
    for fields, word in BAD_SPECS:
        good, bad = spec_of(), spec_of(**{k: v for k, v in fields.items() if k != "coef"})
        good.coef = C.cast(table, C.POINTER(C.c_int16))
        if fields.get("coef", True):
            bad.coef = C.cast(table, C.POINTER(C.c_int16))
        C.memmove(C.byref(s, 0), C.byref(good), C.sizeof(good))
        C.memmove(C.byref(s, C.sizeof(good)), C.byref(bad), C.sizeof(bad))
        for i in range(2):
            w[i].result = -1
        assert f(ctx, w, s, ly, 2, 0) == INVALID_ARGUMENT
        assert [w[i].result for i in range(2)] == [INVALID_ARGUMENT] * 2
        assert err(ctx) == b"window 0: DecodeStreamDevice: null argument", fields      # the lowest failing window's text
        C.memmove(C.byref(s, 0), C.byref(bad), C.sizeof(bad))
        assert f(ctx, w, s, ly, 1, 0) == INVALID_ARGUMENT
        text = err(ctx).decode()
        assert text.startswith("window 0: ResampleWindowsDevice: ") and word in text, (fields, text)
    if linne_amd.device_count() == 0:                           # no device: no context, and so no call -- nothing computes in its place
        with pytest.raises(Exception):
            linne_amd.Context(0).resample_windows([], 1, 1)


# ---- the tool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_cli_usage_and_resample_spec_errors(oracle, tmp_path):
    run = lambda *a: subprocess.run([CLI, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    text = run("-h").stdout
    assert re.search(r"-Z, --resample\b", text) and "-Z RATE[,TAPS] IN.lnn OUT.lnn" in text
    src, dst = tmp_path / "a.lnn", tmp_path / "b.lnn"
    src.write_bytes(bytes(oracle.encode_whole(music(2, 2 * 1024, 16, seed=1), 16, 44100, 1024, 0, True)))
    for spec, word in (("", "sampling rate is expected"), ("x", "sampling rate is expected"), ("+16000", "sampling rate is expected"), ("0", "outside 1 .."),
                       ("5000000000", "outside 1 .."), ("16000,", "tap count is expected"), ("16000,x", "tap count is expected"), ("16000,0", "taps are outside"),
                       ("16000,65", "taps are outside"), ("16000x", "malformed"), ("16000,32x", "malformed"), ("16000,32,1", "malformed"), ("16000.5", "malformed"),
                       ("44101", "beyond 1024/1024"), ("3", "beyond 1024/1024"), ("32000,64", "16384 coefficients")):
        r = run("-Z", spec, str(src), str(dst))
        assert r.returncode == 1 and word in r.stderr and not dst.exists(), (spec, r.stderr)
    assert linne_amd.resample_ratio(44100, 32000) == (320, 441) and 320 * 64 > linne_amd.RESAMPLE_MAX_COEFS      # (the last case's premise)
    assert run("-Z", "16000", str(src)).returncode == 1 and run("-Z", "16000", "-e", str(src), str(dst)).returncode == 1
    assert "-Z takes" in run("-Z", "16000", str(src)).stderr and "-Z takes" in run("-Z", "16000", "-X", "1,1", str(src), str(dst)).stderr
    r = run("-Z", "16000", str(tmp_path / "missing.lnn"), str(dst))
    assert r.returncode == 1 and "Failed to open" in r.stderr


# ---- the plan ------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "lnn_windows_plan.h"
/* stdin: group_frames nblocks S N nwindows, then per window: first n up down taps before table (a number: windows of one number share
 * one array).  One stream of two channels, nblocks SILENT blocks of S samples, N samples in its header.  Out come, per live window,
 * its window record's range and image and its resample record, then the tiles and the coefficient area */
int main(void)
{
    unsigned gf, nb, S, nw; unsigned long long N;
    if (scanf("%u %u %u %llu %u", &gf, &nb, &S, &N, &nw) != 5) return 2;
    std::vector<uint64_t> off(nb), first(nb); std::vector<uint32_t> size(nb, 5), type(nb, SX_SILENT), nsmp(nb, S);
    for (unsigned r = 0; r < nb; r++) { off[r] = 30 + 11ull * r; first[r] = (uint64_t)S * r; }
    WxIndexView x; memset(&x, 0, sizeof(x));
    x.shape.num_channels = 2; x.shape.bits_per_sample = 16; x.shape.num_samples_per_block = S; x.nb = nb; x.covered = (uint64_t)S * nb; x.stream_bytes = 30 + 11ull * nb;
    x.h_off = off.data(); x.h_first = first.data(); x.h_size = size.data(); x.h_type = type.data(); x.h_nsmp = nsmp.data();
    std::vector<WxRange> rg(nw); std::vector<struct LINNEAmdResampleSpec> specs(nw);
    std::vector<std::vector<int16_t> > tables(16);
    for (unsigned i = 0; i < nw; i++) {
        unsigned long long m0, n; unsigned table;
        struct LINNEAmdResampleSpec &s = specs[i];
        memset(&s, 0, sizeof(s));
        if (scanf("%llu %llu %u %u %u %u %u", &m0, &n, &s.up, &s.down, &s.taps, &s.before, &table) != 7 || table >= 16) return 2;
        if (tables[table].empty()) { tables[table].resize((size_t)s.up * s.taps); for (size_t j = 0; j < tables[table].size(); j++) tables[table][j] = (int16_t)(1000 * table + j); }
        if (tables[table].size() != (size_t)s.up * s.taps) return 2;
        s.coef = tables[table].data(); s.shift = 3; s.clip_bits = 16;
        WxRange &r = rg[i];
        memset(&r, 0, sizeof(r));
        r.x = x; r.stream = (const uint8_t *)(uintptr_t)0x30000; r.live = n != 0;
        r.fmt = LINNE_AMD_PCM_S16; r.sstride = 2; r.stride = 1; r.out = (void *)(uintptr_t)(0x1000 * (i + 1));
        r.rs = &s; r.m_lo = m0; r.m_n = n;
        if (n) {
            const WxrInput in = wxr_input(m0, n, s, N);
            r.lo = in.lo; r.n = in.hi - in.lo;
            r.r1 = (in.hi - 1u < x.covered) ? wx_block_of(x.h_first, x.nb, in.hi - 1u) : x.nb;
        }
    }
    WxPlanned p;
    if (wx_plan_count(rg.data(), nw, gf, p) != WXP_OK) return 3;
    wx_resample_count(rg.data(), nw, p);
    /* exactly the reserved sizes, from the heap: the sanitizer build sees a record written past them */
    std::vector<WxWindow> win(p.nlive); std::vector<WxResample> rs(p.nlive); std::vector<WxBlock> rec(p.total_rec); std::vector<uint32_t> crec(p.total_crec);
    std::vector<WxTile> tile(p.rs_tiles); std::vector<uint32_t> coef(p.rs_words);
    wx_plan_fill(rg.data(), nw, gf, WX_NO_BUCKETS, p, win.data(), NULL, rec.data(), crec.data(), NULL, rs.data(), tile.data(), coef.data());
    const WxLists plain = wx_lists(p, nw, 0, sizeof(WxResample)), ls = wx_lists(p, nw, 0, sizeof(WxResample), true);
    printf("fill %llu %llu %llu %llu %u %u\n", (unsigned long long)p.nacc, (unsigned long long)p.rs_tiles, (unsigned long long)p.ntile, (unsigned long long)p.rs_words, p.nwin, p.nrec);
    printf("lists %llu %llu %llu %llu\n", (unsigned long long)plain.bytes, (unsigned long long)ls.o_tile, (unsigned long long)ls.o_coef, (unsigned long long)ls.bytes);
    for (uint32_t k = 0; k < p.nwin; k++) {
        const WxWindow &w = win[k]; const WxResample &m = rs[k];
        printf("window %u %llu %llu %llu %llu %u %llu | %llu %llu %llu %u %llu %llu %llu %llu %llu %llu %u %u %u %u %d %d %u %u %u %u\n", w.fidx, (unsigned long long)w.lo, (unsigned long long)w.hi,
                (unsigned long long)(uintptr_t)w.out, (unsigned long long)w.stride, w.fmt, (unsigned long long)w.sstride,
                (unsigned long long)(uintptr_t)m.out, (unsigned long long)m.stride, (unsigned long long)m.sstride, m.fmt, (unsigned long long)m.m_lo, (unsigned long long)m.m_hi,
                (unsigned long long)m.n_first, (unsigned long long)m.img, (unsigned long long)m.istride, (unsigned long long)m.coef, m.up, m.down, m.taps, m.shift, m.lo, m.hi, m.fidx, m.C, m.prow, m.scale_bits);
    }
    for (const WxTile &t : tile) printf("tile %u %u %llu %llu\n", t.win, t.p0, (unsigned long long)t.m0, (unsigned long long)t.n0);
    printf("coef"); for (uint32_t v : coef) printf(" %u", v); printf("\n");
    for (uint32_t i = 0; i < p.nrec; i++) printf("block %u %u %llu\n", rec[i].win, rec[i].type, (unsigned long long)rec[i].first);
    return 0;
}
"""
# (first output, outputs, up, down, taps, before, table): at output 0, at the last output, a tile and one more, one output, none, shared
# tables, an odd number of taps, the longest decimation
PLAN_N = 10 * 64 - 7                                            # the header names a little less than the blocks hold
PLAN_SPECS = [(0, 257, 3, 2, 4, 1, 0), (900, 50, 3, 2, 4, 1, 0), (5, 0, 1, 1, 1, 0, 1), (0, PLAN_N, 1, 1, 1, 0, 1), (7, 1, 160, 441, 33, 16, 2),
              (100, 130, 160, 441, 33, 16, 2), (0, 1, 1, 1024, 64, 63, 3), (230, 513, 2, 1, 5, 0, 4), (3, 300, 3, 2, 4, 3, 5)]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_plan")
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
def test_plan_input_ranges_images_and_tiles(programs, gf):
    text = "%d 10 64 %d %d\n" % (gf, PLAN_N, len(PLAN_SPECS)) + "".join(" ".join(str(v) for v in s) + "\n" for s in PLAN_SPECS)
    outs = []
    for exe in programs:
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = [x.replace("|", " ").split() for x in outs[0].splitlines()]
    live = [i for i, s in enumerate(PLAN_SPECS) if s[1]]
    for i in live:
        m0, n, up, down = PLAN_SPECS[i][:4]
        assert m0 + n <= resampled_length(PLAN_N, up, down), i   # (the premise: the windows are inside their resampled streams)
    # what Python makes of the same windows
    want, tiles, img, words, offs = [], [], 0, 0, {}
    coef_area = []
    for k, i in enumerate(live):
        m0, n, up, down, taps, before, table = PLAN_SPECS[i]
        nf, nl = m0 * down // up, (m0 + n - 1) * down // up
        lo, hi = max(nf - before, 0), min(nl - before + taps, PLAN_N)
        istride = (nl - nf + taps + 3) // 4 * 4
        prow = (taps + 1) // 2
        if table not in offs:
            offs[table] = words
            words += up * prow
            vals = [(1000 * table + j) & 0xFFFF for j in range(up * taps)]
            for p in range(up):
                row = vals[p * taps:(p + 1) * taps] + [0]
                coef_area += [row[2 * j] | row[2 * j + 1] << 16 for j in range(prow)]
        want.append([i, lo, hi, 4 * (img + lo + before - nf), istride, 0, 1, 0x1000 * (i + 1), 1, 2, 1, m0, m0 + n, nf, img, istride, offs[table], up, down, taps, 3,
                     -32768, 32767, i, 2, prow, int(np.float32(2.0 ** -15).view(np.uint32))])
        tiles += [[k, a * down % up, a, a * down // up] for a in range(m0, m0 + n, 256)]
        img += 2 * istride
    got = [[int(v) for v in x[1:]] for x in lines if x[0] == "window"]
    assert got == want
    assert [[int(v) for v in x[1:]] for x in lines if x[0] == "tile"] == tiles
    assert [int(v) for v in next(x for x in lines if x[0] == "coef")[1:]] == coef_area
    fill = [int(v) for v in lines[0][1:]]
    assert fill[:5] == [img, len(tiles), len(tiles), words, len(live)]
    plain, o_tile, o_coef, total = (int(v) for v in lines[1][1:])
    assert o_tile == plain and o_coef >= o_tile + 24 * len(tiles) and total >= o_coef + 4 * words and o_coef % 256 == 0 and total % 256 == 0
    # the blocks placed are those of the input ranges: every window's first record begins at or before its lo, none begins at or behind its hi
    blocks = [[int(v) for v in x[1:]] for x in lines if x[0] == "block"]
    for k, row in enumerate(want):
        mine = [b for b in blocks if b[0] == k and b[1] == SILENT]
        assert mine and min(b[2] for b in mine) <= row[1] < min(b[2] for b in mine) + 64 and max(b[2] for b in mine) < row[2], k
