"""CPU tests (-m "not gpu") of measuring resident .lnn streams (include/linne_amd.h LINNEAmd_MeasureWindowsDevice): the boundary -- the
symbol, the structs, the Python entry points, the argument errors that need no device --, the reference the GPU tests hold the
library to (expected_measure: numpy and Python integers, checked here against hand-written values), the premises of the GPU tests'
fixtures by the oracle's decode, and the command line tool's -M option as far as it goes without a device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import linne_amd
from signals import music
from test_cli_cpu import CLI
from stream_refs import CARRY_NS, CARRY_PEAK, blocks, carry_signal, carry_stream, crc16, expected_measure, measure_table as table, mixed_signal  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT = 0, 1
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300


def run(*args):
    return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_symbol_structs_and_kinds_are_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bLINNEAmd_MeasureWindowsDevice\s*\(", src)
    assert re.search(r"struct\s+LINNEAmdMeasure\s*\{", src) and re.search(r"struct\s+LINNEAmdMeasureSpec\s*\{", src)
    assert re.search(r"LINNE_AMD_MEASURE_T_MEASURE\s*=\s*80\b", src) and re.search(r"LINNE_AMD_MEASURE_T_PRESET\s*=\s*81\b", src)
    assert re.search(r"LINNE_AMD_MEASURE_T_COMMIT\s*=\s*82\b", src)
    assert "LINNEAmd_MeasureWindowsDevice" in linne_amd.AMD_SYMBOLS
    assert hasattr(linne_amd.lib, "LINNEAmd_MeasureWindowsDevice")


def test_struct_layouts():
    M, P = linne_amd.Measure, linne_amd.MeasureSpec
    assert [(f[0], getattr(M, f[0]).offset) for f in M._fields_] == [("min", 0), ("max", 4), ("sum", 8), ("sumsq_lo", 16), ("sumsq_hi", 24)]
    assert C.sizeof(M) == 32
    assert [(f[0], getattr(P, f[0]).offset) for f in P._fields_] == [("bucket_samples", 0), ("d_out", 8), ("channel_stride", 16)]
    assert C.sizeof(P) == 24
    d = linne_amd.MEASURE_DTYPE
    assert d.itemsize == 32 and [(n, d.fields[n][1]) for n in d.names] == [("min", 0), ("max", 4), ("sum", 8), ("sumsq_lo", 16), ("sumsq_hi", 24)]


def test_python_entry_points():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(linne_amd.Context.measure_windows)
    assert list(p) == ["self", "windows", "bucket_samples", "group_frames", "return_codes"]
    assert (p["bucket_samples"].default, p["group_frames"].default, p["return_codes"].default) == (0, 0, False)
    p = sig(linne_amd.Context.measure_streams)
    assert list(p) == ["self", "streams", "bucket_samples", "group_frames"] and (p["bucket_samples"].default, p["group_frames"].default) == (0, 0)


def test_null_arguments_need_no_device():
    f = linne_amd.lib.LINNEAmd_MeasureWindowsDevice
    w = (linne_amd.Window * 2)()
    s = (linne_amd.MeasureSpec * 2)()
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
    full = np.array([[3, -4, 0, 7, 7, -1, 2], [-(1 << 31), (1 << 31) - 1, 5, 5, 5, 5, 5]], dtype=np.int32)
    assert expected_measure(full, 0, 7, 0) == [[(-4, 7, 14, 128, 0)], [(-(1 << 31), (1 << 31) - 1, 24, (1 << 62) + ((1 << 31) - 1) ** 2 + 125, 0)]]
    assert expected_measure(full, 1, 5, 2) == [[(-4, 0, -4, 16, 0), (7, 7, 14, 98, 0), (-1, -1, -1, 1, 0)],
                                               [(5, (1 << 31) - 1, (1 << 31) + 4, ((1 << 31) - 1) ** 2 + 25, 0), (5, 5, 10, 50, 0), (5, 5, 5, 25, 0)]]
    assert expected_measure(full, 2, 3, 1) == [[(0, 0, 0, 0, 0), (7, 7, 7, 49, 0), (7, 7, 7, 49, 0)], [(5, 5, 5, 25, 0)] * 3]
    assert expected_measure(full, 6, 1, 5000) == [[(2, 2, 2, 4, 0)], [(5, 5, 5, 25, 0)]]
    assert expected_measure(full, 3, 0, 4) == [[], []]
    # five times (-2^31)^2 = 5 * 2^62 = 2^64 + 2^62: the sum of squares crosses 2^64
    big = np.full((1, 5), -(1 << 31), dtype=np.int32)
    assert expected_measure(big, 0, 5, 0) == [[(-(1 << 31), -(1 << 31), -5 * (1 << 31), 1 << 62, 1)]]
    assert expected_measure(big, 0, 5, 4) == [[(-(1 << 31), -(1 << 31), -4 * (1 << 31), 0, 1), (-(1 << 31), -(1 << 31), -(1 << 31), 1 << 62, 0)]]


def test_table_reads_a_structured_array():
    a = np.zeros((1, 2), dtype=linne_amd.MEASURE_DTYPE)
    a[0, 1] = (-3, 9, -(1 << 40), (1 << 64) - 1, 2)
    assert table(a) == [[(0, 0, 0, 0, 0), (-3, 9, -(1 << 40), (1 << 64) - 1, 2)]]


def test_premises_of_the_gpu_fixtures(oracle):
    """the mixed stream's block types; the carry stream decodes to the square wave, all RAW, and its sum of squares is above 2^64"""
    x = mixed_signal(2, 16, 7 * S + TAIL, seed=11, block=S)
    bl = blocks(bytes(oracle.encode_whole(x, 16, 44100, S, 5, True)))
    assert [b[2] for b in bl] == [COMPRESS, SILENT, SILENT, COMPRESS, RAW, RAW, COMPRESS, COMPRESS] and bl[-1][3] == TAIL
    stream = carry_stream(oracle)
    assert 0.75e6 < len(stream) < 0.85e6
    ret, full, _ = oracle.decode_whole(stream)
    assert ret == OK and np.array_equal(full, carry_signal())
    bl = blocks(stream)
    assert len(bl) == CARRY_NS // S and all(b[2] == RAW and b[3] == S for b in bl)
    (rec,), = expected_measure(full, 0, CARRY_NS, 0)
    assert rec[4] >= 1 and rec[4] * (1 << 64) + rec[3] == CARRY_NS * CARRY_PEAK ** 2 and (rec[0], rec[1]) == (-CARRY_PEAK, CARRY_PEAK)
    first, last = expected_measure(full, 0, CARRY_NS, 1 << 18)[0]
    assert first[4] == 0 and last[4] == 0 and first[3] == (1 << 18) * CARRY_PEAK ** 2  # (each bucket alone stays below 2^64)


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_cli_usage_and_option_errors(oracle, tmp_path):
    text = run("-h").stdout
    assert re.search(r"-M, --measure\b", text) and "-M [BUCKET_SAMPLES] STREAM.lnn" in text
    for args in (("-M",), ("-M", "-e", "a", "b"), ("-M", "-d", "a"), ("-M", "-C", "a", "b"), ("-M", "-r", "a", "b"), ("-M", "-V", "a"), ("--measure", "1", "a", "b"),
                 ("-M", "--batch", "d", "a"), ("-M", "x", "a.lnn"), ("-M", "0", "a.lnn"), ("-M", "12x", "a.lnn"), ("-M", "-5", "a.lnn")):
        r = run(*args)
        assert r.returncode == 1 and r.stderr.strip() and not r.stdout, args
    assert "bucket sample count is out of range" in run("-M", "x", "a.lnn").stderr
    r = run("-M", "/nonexistent/a.lnn")
    assert r.returncode == 1 and "Failed to open" in r.stderr
    r = run("--measure", "100", "/nonexistent/a.lnn")
    assert r.returncode == 1 and "Failed to open" in r.stderr
    # a file that is no stream is refused before a device is asked for; a stream either answers or fails with a message
    junk, lnn = tmp_path / "junk.lnn", tmp_path / "a.lnn"
    junk.write_bytes(b"RIFF" + bytes(100))
    r = run("-M", str(junk))
    assert r.returncode == 1 and "Failed to get header information" in r.stderr
    x = np.concatenate([np.zeros((2, 1000), dtype=np.int32), music(2, 1500, 16, seed=3)], axis=1)
    lnn.write_bytes(bytes(oracle.encode_whole(x, 16, 22050, 500, 4, True)))
    r = run("-M", "1000", str(lnn))
    assert r.returncode in (0, 1), (r.returncode, r.stderr)      # (a signal would be negative)
    if r.returncode == 1:
        assert "Failed to create a device context" in r.stderr, r.stderr
