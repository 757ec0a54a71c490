"""Projecting frames of resident .lnn streams on int16 basis rows, without a GPU (include/linne_amd.h LINNEAmd_ProjectWindowsDevice,
LINNEAmd_ProjectLength, LINNEAmd_ProjectDesign): the reference of tests/project_refs.py against hand-written values, the host functions,
the boundary through the C entry point (its per-window argument checks come before any device work), the kernel's digit representation
in Python integers, and the plan's input ranges, images, tables and tiles -- with the injectivity rule and the products' cap, which
need a stream's channel count -- from a stand-alone program."""
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
from project_refs import (INT32_MAX, INT32_MIN, basis_digits, dot_by_digits, expected_project, frames_of, project_length, projected_values,
                          s8, sample_digits, sample_mask, sample_planes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linne_amd", "csrc")
OK, INVALID_ARGUMENT = 0, 1
SILENT = 1


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_the_reference_against_hand_written_values():
    x = np.array([[10, -20, 30, -40, 50, 60, 70], [1, 2, 3, 4, 5, 6, 7]], dtype=np.int32)
    assert project_length(7, 2) == 4 and project_length(7, 7) == 1 and project_length(7, 8) == 1 and project_length(0, 3) == 0 and project_length(5, 0) == 0
    assert frames_of(x, 0, 4, 3, 2, 0)[0].tolist() == [[10, -20, 30], [30, -40, 50], [50, 60, 70], [70, 0, 0]]       # zeros behind the stream
    assert frames_of(x, 0, 2, 3, 2, 1)[1].tolist() == [[0, 1, 2], [2, 3, 4]]                                         # and in front of sample 0
    assert frames_of(x, 2, 2, 2, 2, 0)[1].tolist() == [[5, 6], [7, 0]]                                               # a window counts frames
    y, sat = projected_values(x, 0, 4, [[1, 1, 1], [1, 0, -1]], 2)
    assert y[0].tolist() == [[20, -20], [40, -20], [180, -20], [70, 70]] and y[1].tolist() == [[6, -2], [12, -2], [18, -2], [7, 7]] and not sat
    y, _ = projected_values(x, 0, 7, [[1]], 1)
    assert np.array_equal(y[:, :, 0], x)                                            # N = K = H = 1: the identity
    y, _ = projected_values(x, 0, 4, [[1, 1, 1]], 2, shift=1)
    assert y[0, :, 0].tolist() == [10, 20, 90, 35] and y[1, :, 0].tolist() == [3, 6, 9, 4]     # halves round up: 7 / 2 -> 4
    y, _ = projected_values(-x, 0, 4, [[1, 1, 1]], 2, shift=1)
    assert y[1, :, 0].tolist() == [-3, -6, -9, -3]                                  # ... towards plus infinity: -7 / 2 -> -3
    big = np.array([[1 << 30, -(1 << 30), 100]], dtype=np.int32)
    y, sat = projected_values(big, 0, 3, [[4]], 1)
    assert y[0, :, 0].tolist() == [INT32_MAX, INT32_MIN, 400] and sat
    y, sat = projected_values(big, 0, 3, [[4]], 1, shift=2, clip_bits=16)
    assert y[0, :, 0].tolist() == [32767, -32768, 100] and sat
    got, sat = expected_project(big, 2, 1, [[3]], 1, f32=True, float_exp=2)
    assert got.dtype == np.float32 and got.tolist() == [[[75.0]]] and not sat
    got, _ = expected_project(big, 0, 1, [[1], [3]], 1, f32=True)
    assert got.tolist() == [[[float(1 << 30), float(1 << 31)]]]                     # 3 * 2^30 clips to 2^31 - 1, which rounds to 2^31 as a float


# ---- the host functions --------------------------------------------------------------------------------------------------------
def test_project_length_against_python_integers():
    f = linne_amd.lib.LINNEAmd_ProjectLength
    top = (1 << 64) - 1
    for n in (0, 1, 2, 127, 128, 129, (1 << 32) - 1, 1 << 32, (1 << 53) + 1, top - 65536, top - 1, top):
        for hop in (1, 2, 3, 128, 160, 65535, 65536, 65537, (1 << 32) - 1):
            assert f(n, hop) == -(-n // hop) == project_length(n, hop), (n, hop)
        assert f(n, 0) == 0
    assert linne_amd.project_length(7, 2) == 4


def ideal_basis(n_fft, bins, hann):
    n = np.arange(n_fft, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft) if hann else np.ones(n_fft)
    ang = 2 * np.pi * np.arange(bins)[:, None] * n[None, :] / n_fft
    out = np.empty((2 * bins, n_fft))
    out[0::2], out[1::2] = 32767 * w * np.cos(ang), -32767 * w * np.sin(ang)
    return out, w


@pytest.mark.parametrize("n_fft,bins,window", [(1, 1, "rect"), (2, 2, "hann"), (8, 5, "rect"), (63, 32, "hann"), (64, 33, "hann"), (400, 201, "hann"),
                                               (512, 257, "hann"), (512, 257, "rect"), (4096, 1024, "hann"), (4096, 3, "rect")])
def test_design(n_fft, bins, window):
    b = linne_amd.project_design(n_fft, bins, window)
    assert b.dtype == np.int16 and b.shape == (2 * bins, n_fft)
    ideal, w = ideal_basis(n_fft, bins, window == "hann")
    # libm's last-bit error can move a near-tie by one step, no more
    assert np.abs(b - np.rint(ideal)).max() <= 1
    assert np.abs(b[0] - np.rint(32767 * w)).max() <= 1 and not b[1].any()           # row 0 is the window times 32767; bin 0 has no sine
    if window == "rect":
        assert set(b[0].tolist()) == {32767}
    n = np.arange(1, n_fft)
    for j in range(bins):                                                           # cosines are even about n = 0 (mod N), sines odd
        assert np.array_equal(b[2 * j, n], b[2 * j, n_fft - n]) and np.array_equal(b[2 * j + 1, n], -b[2 * j + 1, n_fft - n]), j
    if n_fft % 2 == 0 and bins == n_fft // 2 + 1:                                   # the Nyquist bin: the window with alternating signs, no sine
        assert np.array_equal(b[-2], b[0] * np.where(np.arange(n_fft) % 2, -1, 1)) and not b[-1].any()


def test_design_bounds_are_refused():
    f = linne_amd.lib.LINNEAmd_ProjectDesign
    buf = (C.c_int16 * (2048 * 4096))()
    for n_fft, bins, window in ((0, 1, 0), (4097, 1, 0), (8, 0, 0), (8, 6, 0), (4096, 1025, 0), (4096, 2049, 1), (8, 1, 2), ((1 << 32) - 1, 1, 0), (1, 2, 0)):
        assert f(n_fft, bins, window, buf) == INVALID_ARGUMENT, (n_fft, bins, window)
    assert f(8, 1, 0, None) == INVALID_ARGUMENT and not any(buf[:64])
    assert f(4096, 1024, 1, buf) == OK and f(8, 5, 0, buf) == OK and f(1, 1, 1, buf) == OK
    for bad in ((0, 1), (4097, 1), (8, 6), (8, 0), (4096, 1025)):
        with pytest.raises(ValueError):
            linne_amd.project_design(*bad)
    with pytest.raises(ValueError):
        linne_amd.project_design(8, 5, "kaiser")
    assert linne_amd.project_design(8).shape == (10, 8)


# ---- the boundary --------------------------------------------------------------------------------------------------------------
FIELDS = [("frame_len", 0), ("hop", 4), ("num_rows", 8), ("before", 12), ("shift", 16), ("clip_bits", 20), ("format", 24), ("float_exp", 28),
          ("channel_stride", 32), ("frame_stride", 40), ("row_stride", 48), ("saturated", 56), ("reserved", 60), ("basis", 64)]


def test_symbols_struct_kinds_and_limits_are_declared_listed_and_exported(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "linne_amd.h")).read(), flags=re.S)
    for name in ("LINNEAmd_ProjectWindowsDevice", "LINNEAmd_ProjectLength", "LINNEAmd_ProjectDesign"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in linne_amd.AMD_SYMBOLS and hasattr(linne_amd.lib, name), name
    assert re.search(r"LINNE_AMD_PROJECT_T_PRESET\s*=\s*104\b", src) and re.search(r"LINNE_AMD_PROJECT_T_PROJECT\s*=\s*105\b", src)
    P = linne_amd.ProjectSpec
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == FIELDS and C.sizeof(P) == 72
    assert (linne_amd.PROJECT_MAX_FRAME, linne_amd.PROJECT_MAX_ROWS, linne_amd.PROJECT_MAX_HOP, linne_amd.PROJECT_MAX_PRODUCTS) == (4096, 2048, 65536, 1 << 40)
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
    if cc:
        code, exe = tmp_path / "size.c", tmp_path / "size"
        code.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "linne_amd.h"\n#define O(f) offsetof(struct LINNEAmdProjectSpec, f)\n'
                        'int main(void) { printf("%zu " , sizeof(struct LINNEAmdProjectSpec)); '
                        + "".join('printf("%%zu ", O(%s)); ' % f for f, _ in FIELDS) +
                        'printf("%d %d %llu %llu %llu %llu\\n", (int)LINNE_AMD_PROJECT_T_PRESET, (int)LINNE_AMD_PROJECT_T_PROJECT, (unsigned long long)LINNE_AMD_PROJECT_MAX_FRAME, '
                        '(unsigned long long)LINNE_AMD_PROJECT_MAX_ROWS, (unsigned long long)LINNE_AMD_PROJECT_MAX_HOP, (unsigned long long)LINNE_AMD_PROJECT_MAX_PRODUCTS); return 0; }\n')
        b = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(code), "-o", str(exe)], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
        assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["72"] + [str(o) for _, o in FIELDS] + ["104", "105", "4096", "2048", "65536", str(1 << 40)]


def test_python_entry_points():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(linne_amd.Context.project_windows)
    assert list(p) == ["self", "windows", "basis", "hop", "before", "shift", "clip_bits", "dtype", "float_exp", "rows_first", "out", "group_frames", "return_codes", "return_saturated"]
    assert [p[k].default for k in list(p)[4:]] == [0, 0, 0, None, 0, False, None, 0, False, False]
    p = sig(linne_amd.Context.stft_windows)
    assert list(p)[:6] == ["self", "windows", "n_fft", "hop", "window", "center"] and (p["window"].default, p["center"].default) == ("hann", True)
    assert list(sig(linne_amd.Context.spectrum_streams)) == ["self", "streams", "n_fft", "hop"]
    assert list(sig(linne_amd.project_design)) == ["n_fft", "bins", "window"] and list(sig(linne_amd.project_length)) == ["num_samples", "hop"]


def spec_of(frame_len=4, hop=2, num_rows=3, before=0, shift=0, clip_bits=0, format=0, float_exp=0, reserved=0, strides=(64, 3, 1)):
    sp = linne_amd.ProjectSpec()
    sp.frame_len, sp.hop, sp.num_rows, sp.before, sp.shift, sp.clip_bits, sp.format, sp.float_exp, sp.reserved = frame_len, hop, num_rows, before, shift, clip_bits, format, float_exp, reserved
    sp.channel_stride, sp.frame_stride, sp.row_stride = strides
    sp.saturated = 7
    return sp


# every INVALID_ARGUMENT case of a window's spec that needs no stream, and a word of the text it gets
BAD_SPECS = [(dict(frame_len=0), "frame_len 0"), (dict(frame_len=4097), "frame_len 4097"), (dict(hop=0), "hop 0"), (dict(hop=65537), "hop 65537"),
             (dict(num_rows=0), "num_rows 0"), (dict(num_rows=2049), "num_rows 2049"), (dict(before=4), "before 4"), (dict(frame_len=1, before=1), "before 1"),
             (dict(shift=32), "shift 32"), (dict(clip_bits=1), "clip_bits 1"), (dict(clip_bits=33), "clip_bits 33"), (dict(format=1), "format 1"),
             (dict(format=2), "format 2"), (dict(format=4), "format 4"), (dict(format=3, float_exp=64), "float_exp 64"), (dict(float_exp=1), "float_exp 1"),
             (dict(reserved=1), "reserved"), (dict(basis=False), "null basis"), (dict(d_pcm=0), "null d_pcm"), (dict(d_pcm=0x1002), "4-byte aligned")]


def test_arguments_are_checked_before_any_device_work():
    f = linne_amd.lib.LINNEAmd_ProjectWindowsDevice
    err = linne_amd.lib.LINNEAmd_GetLastError
    table = (C.c_int16 * 64)()
    w, s = (linne_amd.Window * 2)(), (linne_amd.ProjectSpec * 2)()
    for i in range(2):
        w[i].result = -1
    assert f(None, w, s, 2, 0) == INVALID_ARGUMENT and f(None, None, None, 0, 0) == INVALID_ARGUMENT
    blank = C.create_string_buffer(1 << 20)                     # zeroed memory larger than any context stands in for one
    ctx = C.addressof(blank)
    assert f(ctx, None, s, 2, 0) == INVALID_ARGUMENT            # NULL windows
    assert f(ctx, w, None, 2, 0) == INVALID_ARGUMENT            # NULL specs
    assert b"ProjectWindowsDevice: null argument" in err(ctx)
    assert f(ctx, None, None, 0, 0) == OK and f(ctx, w, s, 0, 0) == OK
    assert [w[i].result for i in range(2)] == [-1, -1]
    # a window's spec: refused with the call's name and the field, whatever else the window names (here: no stream); window 0 is sound
    # but for its stream, window 1 has the fault
    for fields, word in BAD_SPECS:
        good, bad = spec_of(), spec_of(**{k: v for k, v in fields.items() if k not in ("basis", "d_pcm")})
        good.basis = C.cast(table, C.POINTER(C.c_int16))
        if fields.get("basis", True):
            bad.basis = C.cast(table, C.POINTER(C.c_int16))
        C.memmove(C.byref(s, 0), C.byref(good), C.sizeof(good))
        C.memmove(C.byref(s, C.sizeof(good)), C.byref(bad), C.sizeof(bad))
        for i in range(2):
            w[i].result, w[i].d_pcm, w[i].num_samples = -1, 0x1000, 1
        w[1].d_pcm = fields.get("d_pcm", 0x1000)
        assert f(ctx, w, s, 2, 0) == INVALID_ARGUMENT
        assert [w[i].result for i in range(2)] == [INVALID_ARGUMENT] * 2
        assert err(ctx) == b"window 0: DecodeStreamDevice: null argument", fields      # the lowest failing window's text
        C.memmove(C.byref(s, 0), C.byref(bad), C.sizeof(bad))
        w[0].d_pcm = w[1].d_pcm
        assert f(ctx, w, s, 1, 0) == INVALID_ARGUMENT
        text = err(ctx).decode()
        assert text.startswith("window 0: ProjectWindowsDevice: ") and word in text, (fields, text)
        assert s[0].saturated == 7                              # a failing window's `saturated` stays as it was
    if linne_amd.device_count() == 0:                           # no device: no context, and so no call -- nothing computes in its place
        with pytest.raises(Exception):
            linne_amd.Context(0).project_windows([], [[1]], 1)


# ---- the tool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_cli_usage_and_spectrum_spec_errors(oracle, tmp_path):
    run = lambda *a: subprocess.run([CLI, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    text = run("-h").stdout
    assert re.search(r"-F, --spectrum\b", text) and "-F N_FFT[,HOP[,FIRST,N]] IN.lnn" in text
    src = tmp_path / "a.lnn"
    src.write_bytes(bytes(oracle.encode_whole(music(2, 2 * 1024, 16, seed=1), 16, 44100, 1024, 0, True)))
    for spec, word in (("", "frame length in samples is expected"), ("x", "frame length in samples is expected"), ("+512", "frame length in samples is expected"),
                       ("0", "outside 1 .. 2047"), ("2048", "outside 1 .. 2047"), ("5000000000", "outside 1 .. 2047"), ("512,", "hop in samples is expected"),
                       ("512,x", "hop in samples is expected"), ("512,0", "outside 1 .. 65536"), ("512,65537", "outside 1 .. 65536"), ("512,128,5", "come together"),
                       ("512,128,x,5", "sample number is expected"), ("512,128,5,", "sample number is expected"), ("512x", "malformed"), ("512,128x", "malformed"),
                       ("512,128,0,5,6", "malformed"), ("512.5", "malformed"), ("99999999999999999999999", "outside 64 bits"), ("512,128,0,99999999999999999999999", "outside 64 bits"),
                       ("512,128,2049,0", "in a stream of 2048"), ("512,128,2000,49", "in a stream of 2048")):
        r = run("-F", spec, str(src))
        assert r.returncode == 1 and word in r.stderr and not r.stdout, (spec, r.stderr)
    assert run("-F", "512").returncode == 1 and "-F takes" in run("-F", "512").stderr and "-F takes" in run("-F", "512", "-X", "1,1", str(src)).stderr
    assert "-F takes" in run("-F", "512", str(src), str(src)).stderr
    r = run("-F", "512", str(tmp_path / "missing.lnn"))
    assert r.returncode == 1 and "Failed to open" in r.stderr


# ---- the digits ----------------------------------------------------------------------------------------------------------------
def test_digits_recombine_exactly_and_fit_int8():
    for v in range(-32768, 32768):                              # all of int16
        lo, hi = basis_digits(v)
        assert -128 <= lo <= 127 and -128 <= hi <= 127 and 256 * hi + lo + 128 == v, v
    sweep = {INT32_MIN, INT32_MAX, 0x7F7F7F80, 0x7F7F7F7F, -0x7F7F7F80, 0, 1, -1, 127, 128, -128, -129, 255, 256}
    for e in (7, 8, 15, 16, 23, 24, 31):
        sweep |= {v for v in ((1 << e) - 1, 1 << e, (1 << e) + 1, -(1 << e) - 1, -(1 << e), -(1 << e) + 1) if INT32_MIN <= v <= INT32_MAX}
    rng = np.random.default_rng(5)
    sweep |= set(int(v) for v in rng.integers(INT32_MIN, INT32_MAX, 4000, endpoint=True)) | set(range(-70000, 70000, 37)) | set(range(-(1 << 23) - 300, (1 << 23) + 300, 4099))
    for v in sorted(sweep):
        need = sample_planes(v)
        assert need == (2 if -(1 << 15) <= v < 1 << 15 else 3 if -(1 << 23) <= v < 1 << 23 else 4), v
        for P in range(need, 5):                                # the tile's count is its widest value's: every P from the value's own up
            d = sample_digits(v, P)
            assert len(d) == P and all(-128 <= x <= 127 for x in d) and sum(x << (8 * b) for b, x in enumerate(d)) + sample_mask(P) == v, (v, P)
    # whole sums the kernel's way: the extreme rows against the extreme samples, and random ones
    for P, lim in ((2, 1 << 15), (3, 1 << 23), (4, 1 << 31)):
        xs = [lim - 1, -lim, 0, 1, -1, lim - 1, -lim] + [int(v) for v in rng.integers(-lim, lim, 58)]
        for row in ([32767] * 65, [-32768] * 65, [int(v) for v in rng.integers(-32768, 32768, 65)], [127, 128, -128, -129, 255, 256, -256, -257] * 8 + [0]):
            assert dot_by_digits(row, xs, P) == sum(a * b for a, b in zip(row, xs)), (P, row[:3])


def test_digit_sums_at_the_plane_edges_and_at_full_scale():
    """what tests/test_gpu_stream_project.py plants and what it fills frames with: at every edge of the plane rule the digits of the
    value's own plane count, and of every larger one, give the exact product with the rows of the one-sample basis, and one plane
    fewer cannot hold the value; frames of 4096 samples of constant full scale under rows of full scale sum exactly"""
    edges = [32767, -32768, 32768, -32769, (1 << 23) - 1, -(1 << 23), 1 << 23, -(1 << 23) - 1, INT32_MAX, INT32_MIN]
    assert [sample_planes(v) for v in edges] == [2, 2, 3, 3, 3, 3, 4, 4, 4, 4]
    for v in edges:
        need = sample_planes(v)
        for P in range(need, 5):
            for c in (1, -1, 32767, -32768):
                assert dot_by_digits([c], [v], P) == c * v, (v, P, c)
        if need > 2:                                            # cut into one plane fewer, the digits are another value's
            d = (v & 0xFFFFFFFF) ^ sample_mask(need - 1)
            low = sum(s8((d >> (8 * b)) & 255) << (8 * b) for b in range(need - 1)) + sample_mask(need - 1)
            assert low != v and (low - v) % (1 << (8 * (need - 1))) == 0, (v, low)
    rows = [[-32768] * 4096, [32767] * 4096, [-129] * 4096, [127] * 4096, [128] * 4096, [32767, -32768] * 2048, [-32768, 32767] * 2048]
    for v in (-32768, 32767, -(1 << 23), (1 << 23) - 1):
        P = sample_planes(v)
        for row in rows:
            assert dot_by_digits(row, [v] * 4096, P) == sum(row) * v, (v, row[:2])
            pairs = [sum(basis_digits(c)[a] * sample_digits(v, P)[b] for c in row) for a in range(2) for b in range(P)]
            assert max(abs(q) for q in pairs) <= 1 << 26 and (max(pairs) == 1 << 26) == (v < 0 and row[0] == row[1] == -32768), (v, row[:2], pairs)


def test_plane_edge_windows_and_their_premises(oracle):
    """tests/project_edges.py without a GPU: the chosen signals survive the oracle's encoder and decoder, the crafted stream decodes to
    zeros but for the four 4-plane edge values, and the windows of the GPU test have the premises it rests on"""
    import project_edges as pe
    import synth_records as sr
    from test_stream_relate_cpu import WIDE_SHAPE, wide_cases
    decodes = {}
    for name in pe.PLANTS:
        bits, x = pe.planted_signal(name)
        ret, full, _ = oracle.decode_whole(bytes(oracle.encode_whole(x, bits, 44100, 1024, 5, bits == 16)))
        assert ret == OK and np.array_equal(full, x)
        decodes[name] = x
    data, x = pe.crafted_stream()
    ret, full, _ = oracle.decode_whole(bytes(data))
    assert ret == OK and np.array_equal(full, x) and sorted(int(v) for v in x[x != 0]) == [INT32_MIN, -(1 << 23) - 1, 1 << 23, INT32_MAX]
    ret, full, _ = oracle.decode_whole(bytes(sr.case_stream(WIDE_SHAPE, wide_cases())))
    assert ret == OK
    decodes["crafted"], decodes["wide"] = x, np.ascontiguousarray(full, dtype=np.int32)
    windows, counts = pe.edge_windows(decodes, found=[("wide", ch, p) for ch, p in pe.WIDE_AT])
    pe.assert_coverage(windows, counts)
    assert len(windows) >= 200 and all(w["first"] + w["n"] <= project_length(decodes[w["stream"]].shape[1], w["hop"]) for w in windows)


# ---- the plan ------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "lnn_windows_plan.h"
/* stdin: group_frames nblocks S N nwindows, then per window: first n frame_len hop rows before table (a number: windows of one number share
 * one array).  One stream of two channels, nblocks SILENT blocks of S samples, N samples in its header.  Out come, per live window, its
 * window record's range and image and its project record, then the tiles, the table records, the sums and the tables' area.  A first
 * number of 99: the rules -- then lines of cs C fs frames rs K, answered with wxp_injective, and lines of frames K N C behind a line of
 * zeros, answered with wxp_products_fit */
static int rules(void)
{
    unsigned long long a[6];
    while (scanf("%llu %llu %llu %llu %llu %llu", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 6 && (a[0] | a[1] | a[2] | a[3] | a[4] | a[5]))
        printf("injective %d\n", (int)wxp_injective(a[0], a[1], a[2], a[3], a[4], a[5]));
    while (scanf("%llu %llu %llu %llu", &a[0], &a[1], &a[2], &a[3]) == 4) printf("fit %d\n", (int)wxp_products_fit(a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3]));
    return 0;
}
int main(void)
{
    unsigned gf, nb, S, nw; unsigned long long N;
    if (scanf("%u", &gf) != 1) return 2;
    if (gf == 99) return rules();
    if (scanf("%u %u %llu %u", &nb, &S, &N, &nw) != 4) return 2;
    std::vector<uint64_t> off(nb), first(nb); std::vector<uint32_t> size(nb, 5), type(nb, SX_SILENT), nsmp(nb, S);
    for (unsigned r = 0; r < nb; r++) { off[r] = 30 + 11ull * r; first[r] = (uint64_t)S * r; }
    WxIndexView x; memset(&x, 0, sizeof(x));
    x.shape.num_channels = 2; x.shape.bits_per_sample = 16; x.shape.num_samples_per_block = S; x.nb = nb; x.covered = (uint64_t)S * nb; x.stream_bytes = 30 + 11ull * nb;
    x.h_off = off.data(); x.h_first = first.data(); x.h_size = size.data(); x.h_type = type.data(); x.h_nsmp = nsmp.data();
    std::vector<WxRange> rg(nw); std::vector<struct LINNEAmdProjectSpec> specs(nw);
    std::vector<std::vector<int16_t> > tables(16);
    for (unsigned i = 0; i < nw; i++) {
        unsigned long long f0, n; unsigned table;
        struct LINNEAmdProjectSpec &s = specs[i];
        memset(&s, 0, sizeof(s));
        if (scanf("%llu %llu %u %u %u %u %u", &f0, &n, &s.frame_len, &s.hop, &s.num_rows, &s.before, &table) != 7 || table >= 16) return 2;
        if (tables[table].empty()) { tables[table].resize((size_t)s.num_rows * s.frame_len); for (size_t j = 0; j < tables[table].size(); j++) tables[table][j] = (int16_t)(1000 * table + 7 * j - 300); }
        if (tables[table].size() != (size_t)s.num_rows * s.frame_len) return 2;
        s.basis = tables[table].data(); s.shift = 3; s.clip_bits = 16; s.format = LINNE_AMD_PCM_F32; s.float_exp = 5;
        s.channel_stride = 100000; s.frame_stride = s.num_rows; s.row_stride = 1;
        WxRange &r = rg[i];
        memset(&r, 0, sizeof(r));
        r.x = x; r.stream = (const uint8_t *)(uintptr_t)0x30000; r.live = n != 0;
        r.out = (void *)(uintptr_t)(0x1000 * (i + 1));
        r.pj = &s; r.m_lo = f0; r.m_n = n;
        if (n) {
            const WxpInput in = wxp_input(f0, n, s, N);
            r.lo = in.lo; r.n = in.hi - in.lo;
            r.r1 = (in.hi - 1u < x.covered) ? wx_block_of(x.h_first, x.nb, in.hi - 1u) : x.nb;
        }
    }
    WxPlanned p;
    if (wx_plan_count(rg.data(), nw, gf, p) != WXP_OK) return 3;
    wx_project_count(rg.data(), nw, p);
    /* exactly the reserved sizes, from the heap: the sanitizer build sees a record written past them */
    std::vector<WxWindow> win(p.nlive); std::vector<WxProject> pj(p.nlive); std::vector<WxBlock> rec(p.total_rec); std::vector<uint32_t> crec(p.total_crec);
    std::vector<WxProjTile> tile(p.rs_tiles); std::vector<WxProjTable> tab(p.pj_tabs.size()); std::vector<int32_t> rsum(p.pj_rsum); std::vector<int16_t> raw(p.pj_raw);
    const WxProjLists h = { pj.data(), tile.data(), tab.data(), rsum.data(), raw.data() };
    wx_plan_fill(rg.data(), nw, gf, WX_NO_BUCKETS, p, win.data(), NULL, rec.data(), crec.data(), NULL, NULL, NULL, NULL, NULL, NULL, &h);
    const WxLists plain = wx_lists(p, nw, 0, sizeof(WxProject)), ls = wx_lists(p, nw, 0, sizeof(WxProject), false, false, false, true);
    printf("fill %llu %llu %llu %llu %llu %llu %llu %u %u\n", (unsigned long long)p.nacc, (unsigned long long)p.pj_plane0, (unsigned long long)p.pj_plane_bytes, (unsigned long long)p.rs_tiles,
            (unsigned long long)p.ntile, (unsigned long long)p.pj_raw, (unsigned long long)p.pj_rsum, p.nwin, p.nrec);
    printf("lists %llu %llu %llu %llu %llu %llu\n", (unsigned long long)plain.bytes, (unsigned long long)ls.o_tile, (unsigned long long)ls.o_pjtab, (unsigned long long)ls.o_pjrsum, (unsigned long long)ls.o_pjraw, (unsigned long long)ls.bytes);
    for (uint32_t k = 0; k < p.nwin; k++) {
        const WxWindow &w = win[k]; const WxProject &m = pj[k];
        printf("window %u %llu %llu %llu %llu %u %llu | %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %u %u %u %u %u %u %d %d %u %u %u %u\n", w.fidx, (unsigned long long)w.lo, (unsigned long long)w.hi,
                (unsigned long long)(uintptr_t)w.out, (unsigned long long)w.stride, w.fmt, (unsigned long long)w.sstride,
                (unsigned long long)(uintptr_t)m.out, (unsigned long long)m.cstride, (unsigned long long)m.fstride, (unsigned long long)m.rstride, (unsigned long long)m.f_lo, (unsigned long long)m.nframes,
                (unsigned long long)m.img, (unsigned long long)m.istride, (unsigned long long)m.planes, (unsigned long long)m.raw, (unsigned long long)m.rsum, m.N, m.H, m.K, m.Npad, m.Kpad, m.shift, m.lo, m.hi, m.fmt, m.scale_bits, m.fidx, m.C);
    }
    for (const WxProjTile &t : tile) printf("tile %u %u %llu %u\n", t.win, t.ch, (unsigned long long)t.f0, t.k0);
    for (const WxProjTable &t : tab) printf("table %llu %llu %u %u %u %u\n", (unsigned long long)t.raw, (unsigned long long)t.planes, t.K, t.N, t.Kpad, t.Npad);
    printf("rsum"); for (int32_t v : rsum) printf(" %d", v); printf("\n");
    printf("raw"); for (int16_t v : raw) printf(" %d", v); printf("\n");
    for (uint32_t i = 0; i < p.nrec; i++) printf("block %u %u %llu\n", rec[i].win, rec[i].type, (unsigned long long)rec[i].first);
    /* the older kinds' records beside it: the plain plan of the same input ranges has the same block and COMPRESS records, byte for byte,
     * the same passes, and the same window records but for where the samples go */
    WxPlanned q;
    if (wx_plan_count(rg.data(), nw, gf, q) != WXP_OK) return 3;
    std::vector<WxWindow> qwin(q.nlive); std::vector<WxBlock> qrec(q.total_rec); std::vector<uint32_t> qcrec(q.total_crec);
    wx_plan_fill(rg.data(), nw, gf, WX_NO_BUCKETS, q, qwin.data(), NULL, qrec.data(), qcrec.data());
    int same = q.nrec == p.nrec && q.ncrec == p.ncrec && q.nwin == p.nwin && q.passes.size() == p.passes.size() && q.scratch_bytes == p.scratch_bytes
            && (p.nrec == 0 || memcmp(qrec.data(), rec.data(), sizeof(WxBlock) * p.nrec) == 0) && (p.ncrec == 0 || memcmp(qcrec.data(), crec.data(), sizeof(uint32_t) * p.ncrec) == 0);
    for (size_t k = 0; same && k < p.passes.size(); k++) {
        const WxPass &a = q.passes[k], &b = p.passes[k];
        same = a.group == b.group && a.rec0 == b.rec0 && a.nrec == b.nrec && a.c0 == b.c0 && a.nc == b.nc && a.seg_bytes == b.seg_bytes && a.check_only == b.check_only;
    }
    for (uint32_t k = 0; same && k < p.nwin; k++) same = qwin[k].lo == win[k].lo && qwin[k].hi == win[k].hi && qwin[k].covered == win[k].covered && qwin[k].fidx == win[k].fidx;
    printf("older %d %u %zu\n", same, q.nrec, q.passes.size());
    return 0;
}
"""
# (first frame, frames, frame_len, hop, rows, before, table): at frame 0 with a halo in front of sample 0, at the last frame with a halo
# behind the last sample, a tile and one more of frames and of rows, one frame, none, shared tables, a hop beyond the frame
PLAN_N = 10 * 64 - 7                                            # the header names a little less than the blocks hold
PLAN_SPECS = [(0, 65, 8, 3, 5, 7, 0), (200, 11, 8, 3, 5, 7, 0), (5, 0, 4, 2, 3, 0, 1), (0, 317, 4, 2, 3, 0, 1), (3, 1, 65, 100, 130, 64, 2),
              (0, 7, 65, 100, 130, 0, 2), (0, PLAN_N, 1, 1, 1, 0, 3), (1, 3, 5, 200, 17, 2, 4), (630, 3, 64, 1, 16, 63, 5)]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("project_plan")
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
def test_plan_input_ranges_images_tables_and_tiles(programs, gf):
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
        f0, n, N, H = PLAN_SPECS[i][:4]
        assert f0 + n <= project_length(PLAN_N, H), i             # (the premise: the windows are inside their streams' frames)
    # what Python makes of the same windows
    want, tiles, tables, img, raw_at, rsum_at, plane_at = [], [], {}, 0, 0, 0, 0
    raw_area, rsum_area, table_rows = [], [], []
    for k, i in enumerate(live):
        f0, n, N, H, K, before, table = PLAN_SPECS[i]
        lo, hi = max(f0 * H - before, 0), min((f0 + n - 1) * H - before + N, PLAN_N)
        istride = ((n - 1) * H + N + 3) // 4 * 4
        Kpad, Npad = (K + 15) // 16 * 16, (N + 63) // 64 * 64
        if table not in tables:
            tables[table] = (raw_at, plane_at, rsum_at)
            vals = [((1000 * table + 7 * j - 300 + 32768) & 0xFFFF) - 32768 for j in range(K * N)]
            pad = (K * N + 7) // 8 * 8
            raw_area += vals + [0] * (pad - K * N)
            rsum_area += [sum(vals[r * N:(r + 1) * N]) - 128 * N for r in range(K)] + [0] * (Kpad - K)
            table_rows.append([raw_at, plane_at, K, N, Kpad, Npad])
            raw_at, plane_at, rsum_at = raw_at + pad, plane_at + 2 * Kpad * Npad, rsum_at + Kpad
        t_raw, t_plane, t_rsum = tables[table]
        want.append([i, lo, hi, 4 * (img + lo + before - f0 * H), istride, 0, 1, 0x1000 * (i + 1), 100000, K, 1, f0, n, img, istride, t_plane, t_raw, t_rsum,
                     N, H, K, Npad, Kpad, 3, -32768, 32767, 3, int(np.float32(2.0 ** -5).view(np.uint32)), i, 2])
        tiles += [[k, c, a, b] for c in range(2) for a in range(0, n, 64) for b in range(0, K, 64)]
        img += 2 * istride
    got = [[int(v) for v in x[1:]] for x in lines if x[0] == "window"]
    assert got == want
    got_tiles = [[int(v) for v in x[1:]] for x in lines if x[0] == "tile"]
    assert got_tiles == tiles
    # the tiles cover every (channel, frame, row) of every live window exactly once
    for k, i in enumerate(live):
        n, K = PLAN_SPECS[i][1], PLAN_SPECS[i][4]
        cover = np.zeros((2, n, K), dtype=np.int64)
        for _, c, a, b in (t for t in got_tiles if t[0] == k):
            cover[c, a:a + 64, b:b + 64] += 1
        assert (cover == 1).all(), i
    assert [[int(v) for v in x[1:]] for x in lines if x[0] == "table"] == table_rows          # windows of one (basis, K, N) share one table
    assert [int(v) for v in next(x for x in lines if x[0] == "rsum")[1:]] == rsum_area
    assert [int(v) for v in next(x for x in lines if x[0] == "raw")[1:]] == raw_area
    fill = [int(v) for v in lines[0][1:]]
    plane0 = (img + 3) // 4 * 4
    assert fill[:8] == [plane0 + plane_at // 4, plane0, plane_at, len(tiles), len(tiles), raw_at, rsum_at, len(live)]
    plain, o_tile, o_tab, o_rsum, o_raw, total = (int(v) for v in lines[1][1:])
    assert o_tile == plain and o_tab >= o_tile + 24 * len(tiles) and o_rsum >= o_tab + 32 * len(table_rows) and o_raw >= o_rsum + 4 * rsum_at and total >= o_raw + 2 * raw_at
    assert all(v % 256 == 0 for v in (o_tab, o_rsum, o_raw, total))
    older = [int(v) for v in next(x for x in lines if x[0] == "older")[1:]]
    assert older[0] == 1 and older[1] == fill[8] and older[2] >= 1
    # the blocks placed are those of the input ranges: every window's first record begins at or before its lo, none begins at or behind its hi
    blocks = [[int(v) for v in x[1:]] for x in lines if x[0] == "block"]
    for k, row in enumerate(want):
        mine = [b for b in blocks if b[0] == k and b[1] == SILENT]
        assert mine and min(b[2] for b in mine) <= row[1] < min(b[2] for b in mine) + 64 and max(b[2] for b in mine) < row[2], k


# ---- the plan at the positions and bounds of tests/test_gpu_stream_project_far.py ----
N32, HALF, A_START = (1 << 32) - 1, 1 << 31, (1 << 31) - 1500
# (first frame, frames, frame_len, hop, rows, before, table) on a stream of 65537 SILENT blocks of 65535 samples, 2^32 - 1 in all: the
# stream's last frame at hop 1; a first frame above 2^31; 2^15 frames at hop 65536; the frames at the products' bound (one row here:
# the program prints its tables); then the two windows of the images test, whose second image begins behind word 2^32
FAR_SPECS = [(N32 - 1, 1, 70, 1, 19, 69, 0), (N32 - 40, 40, 70, 1, 19, 0, 0), (HALF + 5, 150, 70, 1, 19, 0, 0), (0, 1 << 15, 8, 65536, 3, 0, 1), (65536 - 70, 70, 70, 65536, 19, 69, 0),
             (HALF // 64 - (1 << 15), 1 << 16, 4096, 64, 1, 2048, 2), (0, 32769, 8, 65536, 3, 0, 1), (A_START - 100, 400, 70, 1, 19, 69, 0)]


def test_plan_at_far_positions(programs):
    """wxp_input's lo, hi and istride, and the image offsets of wx_project_record, against Python integers where first * hop, the input
    range and the images pass 2^31 and 2^32"""
    assert 65537 * 65535 == N32 and FAR_SPECS[0][0] == project_length(N32, 1) - 1
    text = "0 65537 65535 %d %d\n" % (N32, len(FAR_SPECS)) + "".join(" ".join(str(v) for v in s) + "\n" for s in FAR_SPECS)
    outs = []
    for exe in programs:
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    got = [[int(v) for v in x.replace("|", " ").split()[1:16]] for x in outs[0].splitlines() if x.startswith("window ")]
    want, img = [], 0
    for i, (f0, n, N, H, K, before, table) in enumerate(FAR_SPECS):
        assert f0 + n <= project_length(N32, H)
        lo, hi = max(f0 * H - before, 0), min((f0 + n - 1) * H - before + N, N32)
        istride = ((n - 1) * H + N + 3) // 4 * 4
        want.append([i, lo, hi, 4 * (img + lo + before - f0 * H), istride, 0, 1, 0x1000 * (i + 1), 100000, K, 1, f0, n, img, istride])
        img += 2 * istride
    assert got == want
    assert want[0][1:3] == [N32 - 70, N32] and want[1][2] == N32 and want[2][1] > HALF                 # the last frames end with the stream; a range above 2^31
    assert want[3][4] == ((1 << 15) - 1) * 65536 + 8 and want[3][2] == want[3][4] and want[5][4] == 65535 * 64 + 4096      # 2^15 frames at the largest hop; the bound's frames
    assert want[6][4] == HALF + 8 and want[7][13] == want[6][13] + (1 << 32) + 16 and want[7][13] > 1 << 32 and want[7][3] > 1 << 34   # the image behind word 2^32, its byte offset behind 2^34
    tiles = sum(1 for x in outs[0].splitlines() if x.startswith("tile "))
    assert tiles == sum(2 * -(-n // 64) * -(-K // 64) for _, n, _, _, K, _, _ in FAR_SPECS)


# the rules at the far tests' shapes: the products' bound and one frame beyond it; the strides of the far tables and of the refused tiles
FAR_INJECTIVE = [(((1 << 32) + 5, 2, 2, 3, 1, 2), True), ((7, 2, HALF + 3, 3, 1, 2), True), ((6, 2, HALF + 3, 3, 1, 2), True), ((7, 2, 13, 3, 1, 2), False),
                 ((64 * 0xFFFFFF // 2 + 1, 2, 1, 64 * 0xFFFFFF // 2 + 1, 1, 1), True), ((64 * 0xFFFFFF // 2, 2, 1, 64 * 0xFFFFFF // 2 + 1, 1, 1), False),
                 (((1 << 16) * 2048, 2, 2048, 1 << 16, 1, 2048), True), ((((1 << 16) + 1) * 2048, 2, 2048, (1 << 16) + 1, 1, 2048), True)]
FAR_FITS = [((1 << 16, 2048, 4096, 2), True), (((1 << 16) + 1, 2048, 4096, 2), False), ((64 * 0xFFFFFF // 2 + 1, 1, 1, 2), True), ((32769, 3, 8, 2), True)]


# (channel_stride, C, frame_stride, frames, row_stride, K) -> injective: both orders, padded strides, extents of 1, and the failures
INJECTIVE_NEAR = [((1000, 2, 5, 200, 1, 5), True), ((1000, 2, 1, 200, 200, 5), True), ((1400, 2, 7, 200, 1, 5), True), ((1, 2, 2, 200, 400, 5), True),
             ((999, 2, 5, 200, 1, 5), False), ((1000, 2, 4, 200, 1, 5), False), ((1000, 2, 1, 200, 199, 5), False), ((1000, 2, 5, 200, 0, 5), False),
             ((0, 1, 5, 200, 1, 5), True), ((0, 1, 0, 1, 0, 1), True), ((0, 1, 0, 1, 1, 5), True), ((0, 1, 0, 1, 0, 5), False), ((7, 2, 7, 1, 1, 5), True),
             ((5, 2, 0, 1, 1, 5), True), ((4, 2, 0, 1, 1, 5), False), ((1, 2, 2, 3, 6, 1), True), ((1 << 63, 2, 1 << 62, 2, 1 << 61, 2), True),
             (((1 << 64) - 1, 2, (1 << 63) + 1, 2, 1, 1 << 20), False), ((2, 8, 16, 3, 1, 2), True), ((2, 8, 15, 3, 1, 2), False)]
FITS_NEAR = [((1 << 40, 1, 1, 1), True), (((1 << 40) + 1, 1, 1, 1), False), ((1 << 17, 2048, 4096, 1), True), (((1 << 17) + 1, 2048, 4096, 1), False),
        ((1 << 14, 2048, 4096, 8), True), (((1 << 14) + 1, 2048, 4096, 8), False), (((1 << 64) - 1, 2048, 4096, 8), False), ((1 << 41, 2048, 4096, 8), False),
        ((0, 2048, 4096, 8), True)]


def test_the_injectivity_rule_and_the_products_cap(programs):
    INJECTIVE, FITS = INJECTIVE_NEAR + FAR_INJECTIVE, FITS_NEAR + FAR_FITS
    text = "99\n" + "".join(" ".join(str(v) for v in a) + "\n" for a, _ in INJECTIVE) + "0 0 0 0 0 0\n" + "".join(" ".join(str(v) for v in a) + "\n" for a, _ in FITS)
    for exe in programs:
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = r.stdout.split()
        assert got[0::2] == ["injective"] * len(INJECTIVE) + ["fit"] * len(FITS)
        assert [int(v) for v in got[1::2]] == [int(w) for _, w in INJECTIVE] + [int(w) for _, w in FITS]
    assert (1 << 41) * 2048 * 4096 * 8 >= 1 << 64                # (the premise of the 128 bits: that product wraps 64)
