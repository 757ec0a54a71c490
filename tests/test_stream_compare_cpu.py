"""CPU tests (-m "not gpu") of comparing resident .lnn streams with resident PCM (include/linne_amd.h LINNEAmd_CompareWindowsDevice):
the boundary -- the symbol, the struct, the Python entry points, the argument errors that need no device -- and the command line
tool's -V / -C options as far as they go without one."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import linne_amd
from test_cli_cpu import CLI, wav_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT = 0, 1


def run(*args):
    return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_symbol_and_struct_are_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bLINNEAmd_CompareWindowsDevice\s*\(", src)
    assert re.search(r"struct\s+LINNEAmdDiff\s*\{", src)
    assert re.search(r"LINNE_AMD_COMPARE_T_COMPARE\s*=\s*79\b", src)
    assert "LINNEAmd_CompareWindowsDevice" in linne_amd.AMD_SYMBOLS
    assert hasattr(linne_amd.lib, "LINNEAmd_CompareWindowsDevice")


def test_struct_layout():
    D = linne_amd.Diff
    assert [(f[0], getattr(D, f[0]).offset) for f in D._fields_] == [("num_differing", 0), ("first_sample", 8), ("first_channel", 16), ("reserved", 20)]
    assert C.sizeof(D) == 24


def test_python_entry_points():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(linne_amd.Context.compare_windows)
    assert list(p) == ["self", "windows", "group_frames", "return_codes"] and p["group_frames"].default == 0 and p["return_codes"].default is False
    p = sig(linne_amd.Context.verify_streams)
    assert list(p) == ["self", "pairs", "group_frames"] and p["group_frames"].default == 0
    assert list(sig(linne_amd.Context.set_verify)) == ["self", "on"]


def test_null_arguments_need_no_device():
    f = linne_amd.lib.LINNEAmd_CompareWindowsDevice
    w = (linne_amd.Window * 2)()
    d = (linne_amd.Diff * 2)()
    for i in range(2):
        w[i].result, d[i].num_differing, d[i].first_sample, d[i].first_channel = -1, 77, 78, 5
    assert f(None, w, None, d, 2, 0) == INVALID_ARGUMENT and f(None, None, None, None, 0, 0) == INVALID_ARGUMENT
    blank = C.create_string_buffer(1 << 20)                     # zeroed memory larger than any context stands in for one
    ctx = C.addressof(blank)
    assert f(ctx, None, None, d, 2, 0) == INVALID_ARGUMENT      # NULL windows
    assert f(ctx, w, None, None, 2, 0) == INVALID_ARGUMENT      # NULL diffs
    assert b"null argument" in linne_amd.lib.LINNEAmd_GetLastError(ctx)
    assert f(ctx, None, None, None, 0, 0) == OK and f(ctx, w, None, d, 0, 0) == OK
    assert [(w[i].result, d[i].num_differing, d[i].first_sample, d[i].first_channel) for i in range(2)] == [(-1, 77, 78, 5)] * 2


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_cli_usage_and_option_errors():
    text = run("-h").stdout
    assert re.search(r"-V, --verify\b", text) and re.search(r"-C, --compare\b", text) and "-C STREAM.lnn PCM.wav" in text
    for args in (("-V", "-d", "a", "b"), ("--verify", "a", "b"), ("-C", "-e", "a", "b"), ("-C", "-V", "a", "b"), ("-C", "-r", "a", "b"),
                 ("-C", "a"), ("--compare", "a", "b", "c"), ("-C", "--batch", "d", "a", "b")):
        r = run(*args)
        assert r.returncode == 1 and r.stderr.strip(), args
    r = run("-C", "/nonexistent/a.lnn", "/nonexistent/a.wav")
    assert r.returncode == 1 and "Failed to open" in r.stderr


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_cli_compare_needs_no_device_to_fail_loudly(oracle, tmp_path):
    """a host-only stream (SILENT and RAW blocks) and its WAV: what needs no device is said before one is asked for -- another length,
    another format --, and the comparison itself either answers (a device is there) or fails with a message: never a crash"""
    rng = np.random.default_rng(5)
    x = np.concatenate([np.zeros((2, 1000), dtype=np.int32), rng.integers(-32768, 32767, size=(2, 1500)).astype(np.int32)], axis=1)
    lnn, wav, short, other = tmp_path / "a.lnn", tmp_path / "a.wav", tmp_path / "short.wav", tmp_path / "rate.wav"
    lnn.write_bytes(oracle.encode_whole(x, 16, 22050, 500, 4, True))
    wav.write_bytes(wav_bytes(x, 16, 22050))
    short.write_bytes(wav_bytes(x[:, :-1], 16, 22050))
    other.write_bytes(wav_bytes(x, 16, 44100))
    for bad in (short, other):
        r = run("-C", str(lnn), str(bad))
        assert r.returncode == 1 and "verification failed: the stream holds 2 channels, 16 bits, 22050 Hz, 2500 samples" in r.stderr, r.stderr
    r = run("-C", str(wav), str(wav))                           # not a stream
    assert r.returncode == 1 and "verification failed: the stream's header does not decode" in r.stderr
    r = run("-C", str(lnn), str(wav))
    assert r.returncode in (0, 1), (r.returncode, r.stderr)      # (a signal would be negative)
    if r.returncode == 0:
        assert "identical" in r.stdout
    else:
        assert "verification failed: Failed to create a device context" in r.stderr, r.stderr
