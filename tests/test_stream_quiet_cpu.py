"""CPU tests (-m "not gpu") of finding the quiet runs of resident .lnn streams (include/linne_amd.h LINNEAmd_QuietWindowsDevice): the
boundary -- the symbol, the structs, the Python entry points, the argument errors that need no device --, the reference the GPU tests
hold the library to (expected_quiet: numpy on the oracle's decode, checked here against hand-written values), sound_segments, the
premises of the GPU tests' fixtures by the oracle's decode, the host's plan for the bitmask consumer (a stand-alone program, also built
with the address and undefined-behaviour sanitizers) and the command line tool's -S option as far as it goes without a device."""
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
from stream_refs import blocks, expected_quiet, mixed_signal, quiet_answer as answer  # noqa: F401  (the GPU tests import them from here)
from test_windows_plan_cpu import programs, run as plan_run, stream as plan_stream  # noqa: F401  (programs is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT = 0, 1
COMPRESS, SILENT, RAW = 0, 1, 2
S = 1024
TAIL = 300
NS = 3 * S + TAIL
BASE_B = 517
# quiet stretches of planted_signal, (first, end) in stream samples.  Relative to sample 0 and to sample 517, the first samples of two
# of the GPU tests' windows, runs start at the bit offsets 0, 1, 31, 32, 63, 64, 255, 256, 257 and end at all of them
PLANTS_A = [(0, 1), (31, 32), (63, 64), (255, 256), (257, 300)]
PLANTS_B = [(BASE_B - 7, BASE_B)] + [(BASE_B + a, BASE_B + b) for a, b in ((1, 31), (32, 63), (64, 255), (256, 257))]
ONE_CHANNEL = (2000, 2050, 2100)            # zeros in [2000, 2100) but for the last channel's sample 2050
NOISE = (2200, 2300)                        # values within +-3
PLANTS_END = [(S, S + 1), (NS - 10, NS)]
LOUD = 7                                    # what a sample of channel 0 that is not planted is at least, in magnitude
LONG_BLOCKS = 64
MIXED_PLANTS = [(S - 40, 3 * S + 25), (4 * S - 30, 4 * S + 20), (6 * S - 15, 6 * S + 45)]


def made_loud(x):
    """x with every frame loud: channel 0 at least LOUD in magnitude"""
    x = np.array(x, dtype=np.int32)
    x[0, np.abs(x[0]) < LOUD] = LOUD
    return x


def planted_signal(nch, seed):
    """music of 3 blocks and a tail of 300 in which every frame is loud but the planted ones"""
    x = made_loud(music(nch, NS, 16, seed=seed))
    for a, b in PLANTS_A + PLANTS_B + PLANTS_END:
        x[:, a:b] = 0
    a, at, b = ONE_CHANNEL
    x[:, a:b] = 0
    x[nch - 1, at] = 5
    a, b = NOISE
    x[:, a:b] = np.random.default_rng(seed).integers(-3, 4, size=(nch, b - a))
    x[0, a], x[0, b - 1] = 3, -3
    return x


def planted_runs(threshold):
    """the runs of planted_signal at threshold 3 (or, without the noise stretch, what is common to thresholds 0 and 3)"""
    a, at, b = ONE_CHANNEL
    runs = PLANTS_A + PLANTS_B + PLANTS_END + [(a, at), (at + 1, b)] + ([NOISE] if threshold >= 3 else [])
    return sorted((a, b - a) for a, b in runs)


def mixed_planted():
    """mixed_signal (music, two SILENT blocks, music, two RAW blocks, music, a tail) made loud outside its silent blocks, with zeros
    that reach from the first block through the silent ones into the fourth, into and out of the RAW blocks"""
    x = mixed_signal(2, 16, 7 * S + TAIL, seed=11, block=S)
    keep = x[:, S:3 * S].copy()
    x = made_loud(x)
    x[:, S:3 * S] = keep
    for a, b in MIXED_PLANTS:
        x[:, a:b] = 0
    return x


def long_signal():
    """a loud block, LONG_BLOCKS blocks of zeros, a loud block"""
    x = np.zeros((2, (LONG_BLOCKS + 2) * S), dtype=np.int32)
    x[:, :S] = made_loud(music(2, S, 16, seed=5))
    x[:, -S:] = made_loud(music(2, S, 16, seed=6))
    return x


def run(*args):
    return subprocess.run([CLI, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_symbol_structs_and_kinds_are_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bLINNEAmd_QuietWindowsDevice\s*\(", src)
    for name in ("LINNEAmdRun", "LINNEAmdQuietSpec", "LINNEAmdQuiet"):
        assert re.search(r"struct\s+%s\s*\{" % name, src), name
    for name, kind in (("QUIET", 86), ("PRESET", 87), ("COUNT", 88), ("SCAN", 89), ("STARTS", 90), ("ENDS", 91)):
        assert re.search(r"LINNE_AMD_QUIET_T_%s\s*=\s*%d\b" % (name, kind), src), name
    assert re.search(r"#define\s+LINNE_AMD_QUIET_EXTRA_LAUNCHES\s+5\b", src)
    assert "LINNEAmd_QuietWindowsDevice" in linne_amd.AMD_SYMBOLS
    assert hasattr(linne_amd.lib, "LINNEAmd_QuietWindowsDevice")


def test_struct_layouts():
    R, P, Q = linne_amd.Run, linne_amd.QuietSpec, linne_amd.Quiet
    offsets = lambda T: [(f[0], getattr(T, f[0]).offset) for f in T._fields_]
    assert offsets(R) == [("first_sample", 0), ("num_samples", 8)] and C.sizeof(R) == 16
    assert offsets(P) == [("threshold", 0), ("reserved", 4), ("min_samples", 8), ("d_out", 16), ("capacity", 24)] and C.sizeof(P) == 32
    assert offsets(Q) == [("num_runs", 0), ("quiet_samples", 8), ("lead_samples", 16), ("trail_samples", 24)] and C.sizeof(Q) == 32


def test_python_entry_points():
    sig = lambda f: inspect.signature(f).parameters
    p = sig(linne_amd.Context.quiet_windows)
    assert list(p) == ["self", "windows", "threshold", "min_samples", "capacity", "group_frames", "return_codes"]
    assert (p["min_samples"].default, p["capacity"].default, p["group_frames"].default, p["return_codes"].default) == (1, None, 0, False)
    assert p["threshold"].default is inspect.Parameter.empty
    p = sig(linne_amd.Context.quiet_streams)
    assert list(p) == ["self", "streams", "threshold", "min_samples", "capacity", "group_frames"]
    assert (p["min_samples"].default, p["capacity"].default, p["group_frames"].default) == (1, None, 0)
    p = sig(linne_amd.sound_segments)
    assert list(p) == ["num_samples", "runs", "pad"] and p["pad"].default == 0


def test_null_arguments_need_no_device():
    f = linne_amd.lib.LINNEAmd_QuietWindowsDevice
    w, s, a = (linne_amd.Window * 2)(), (linne_amd.QuietSpec * 2)(), (linne_amd.Quiet * 2)()
    for i in range(2):
        w[i].result = -1
        a[i].num_runs = 77
    assert f(None, w, s, a, 2, 0) == INVALID_ARGUMENT and f(None, None, None, None, 0, 0) == INVALID_ARGUMENT
    blank = C.create_string_buffer(1 << 20)                     # zeroed memory larger than any context stands in for one
    ctx = C.addressof(blank)
    assert f(ctx, None, s, a, 2, 0) == INVALID_ARGUMENT         # NULL windows
    assert f(ctx, w, None, a, 2, 0) == INVALID_ARGUMENT         # NULL specs
    assert f(ctx, w, s, None, 2, 0) == INVALID_ARGUMENT         # NULL answers
    assert b"null argument" in linne_amd.lib.LINNEAmd_GetLastError(ctx)
    assert f(ctx, None, None, None, 0, 0) == OK and f(ctx, w, s, a, 0, 0) == OK
    assert [w[i].result for i in range(2)] == [-1, -1] and [a[i].num_runs for i in range(2)] == [77, 77]


def test_the_reference_against_hand_written_values():
    lo = -(1 << 31)
    #                  0  1  2  3  4  5  6  7  8  9 10 11
    full = np.array([[0, 0, 9, 0, 0, 0, 1, 0, 0, 9, 0, 0],
                     [0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    # a loud frame in one channel only (sample 4, channel 1) splits a run; runs at both window edges
    assert expected_quiet(full, 0, 12, 0, 1) == ([(0, 2), (3, 1), (5, 1), (7, 2), (10, 2)], 5, 8, 2, 2)
    assert expected_quiet(full, 0, 12, 0, 0) == expected_quiet(full, 0, 12, 0, 1)                # min_samples 0 is 1
    assert expected_quiet(full, 0, 12, 0, 2) == ([(0, 2), (7, 2), (10, 2)], 3, 6, 2, 2)           # runs of exactly min
    assert expected_quiet(full, 0, 12, 0, 3) == ([], 0, 0, 2, 2)                                 # runs of min - 1; lead and trail stay
    assert expected_quiet(full, 0, 12, 1, 3) == ([(5, 4)], 1, 4, 2, 2)
    assert expected_quiet(full, 0, 12, 4, 1) == ([(0, 2), (3, 6), (10, 2)], 3, 10, 2, 2)
    # a run ends at the window's ends, whatever lies outside; first samples are the stream's
    assert expected_quiet(full, 1, 3, 0, 1) == ([(1, 1), (3, 1)], 2, 2, 1, 1)
    assert expected_quiet(full, 7, 2, 0, 2) == ([(7, 2)], 1, 2, 2, 2)                             # everything quiet: lead = trail = n
    assert expected_quiet(full, 7, 2, 0, 3) == ([], 0, 0, 2, 2)
    assert expected_quiet(full, 2, 1, 8, 1) == ([], 0, 0, 0, 0)                                   # nothing quiet
    assert expected_quiet(full, 2, 1, 9, 1) == ([(2, 1)], 1, 1, 1, 1)
    assert expected_quiet(full, 5, 0, 0, 1) == ([], 0, 0, 0, 0)                                   # n = 0
    big = np.array([[lo, (1 << 31) - 1, lo]], dtype=np.int32)
    assert expected_quiet(big, 0, 3, (1 << 31) - 1, 1) == ([(1, 1)], 1, 1, 0, 0)                # |INT32_MIN| = 2^31, in 64 bits
    assert expected_quiet(big, 0, 3, 1 << 31, 1) == ([(0, 3)], 1, 3, 3, 3)
    assert expected_quiet(big, 0, 3, (1 << 31) - 2, 1) == ([], 0, 0, 0, 0)


def test_sound_segments():
    f = linne_amd.sound_segments
    assert f(100, []) == [(0, 100)]                              # no runs
    assert f(100, [(0, 100)]) == [] and f(100, [(0, 100)], pad=5) == []                          # one run over everything
    assert f(0, []) == []
    assert f(100, [(10, 20), (50, 10)]) == [(0, 10), (30, 20), (60, 40)]
    assert f(100, [(50, 10), (10, 20)]) == [(0, 10), (30, 20), (60, 40)]                         # any order
    assert f(100, [(0, 10), (90, 10)]) == [(10, 80)]
    assert f(100, [(0, 10), (90, 10)], pad=4) == [(6, 88)]                                       # pad
    assert f(100, [(0, 10), (90, 10)], pad=40) == [(0, 100)]                                     # clamped to [0, n)
    assert f(100, [(10, 20), (50, 10)], pad=10) == [(0, 100)]                                    # touching segments merge: [0, 20) [20, 60) [50, 100)
    assert f(100, [(10, 20), (50, 10)], pad=9) == [(0, 19), (21, 79)]
    assert f(100, [(40, 3)], pad=1) == [(0, 41), (42, 58)] and f(100, [(40, 2)], pad=1) == [(0, 100)]
    assert f(100, np.array([[10, 20], [50, 10]])) == [(0, 10), (30, 20), (60, 40)]               # an array (k, 2)
    assert f(100, [(90, 50), (95, 1)]) == [(0, 90)]                                              # runs beyond n or inside each other
    assert all(isinstance(v, int) for seg in f(100, np.array([[10, 20]])) for v in seg)


def test_premises_of_the_gpu_fixtures(oracle):
    """every planted run is where the GPU tests assume, by the oracle's decode of the oracle's encode"""
    for nch, preset in ((1, 0), (2, 5), (3, 0)):
        x = planted_signal(nch, 30 + nch)
        ret, full, _ = oracle.decode_whole(bytes(oracle.encode_whole(x, 16, 44100, S, preset, nch == 2)))
        assert ret == OK and np.array_equal(full, x)
        for thr in (0, 3):
            runs = expected_quiet(full, 0, NS, thr, 1)[0]
            if thr == 3:
                assert runs == planted_runs(3)
            else:
                a, b = NOISE
                assert [r for r in runs if not a <= r[0] < b] == planted_runs(0) and all(a < r[0] and r[0] + r[1] < b for r in runs if a <= r[0] < b)
        assert expected_quiet(full, 0, NS, 1 << 31, 1) == ([(0, NS)], 1, NS, NS, NS)
        # relative to the two windows' first samples, runs start and end at every offset the masks' words make special
        starts = {r[0] - base for base in (0, BASE_B) for r in planted_runs(0)}
        ends = {r[0] + r[1] - base for base in (0, BASE_B) for r in planted_runs(0)}
        assert {0, 1, 31, 32, 63, 64, 255, 256, 257} <= starts and {0, 1, 31, 32, 63, 64, 255, 256, 257} <= ends
    # the mixed stream: its block types, and the runs that cross them
    x = mixed_planted()
    stream = bytes(oracle.encode_whole(x, 16, 44100, S, 5, True))
    bl = blocks(stream)
    assert [b[2] for b in bl] == [COMPRESS, SILENT, SILENT, COMPRESS, RAW, RAW, COMPRESS, COMPRESS] and bl[-1][3] == TAIL
    assert expected_quiet(x, 0, 7 * S + TAIL, 0, 1)[0] == [(a, b - a) for a, b in MIXED_PLANTS]
    cut = stream[:bl[6][0]]                                      # cut behind its sixth block: the rest decodes to zeros
    ret, full, _ = oracle.decode_whole(cut)
    assert ret == OK and full.shape[1] == 7 * S + TAIL and not full[:, 6 * S:].any()
    assert expected_quiet(full, 0, 7 * S + TAIL, 0, 1)[0][-1] == (6 * S - 15, S + TAIL + 15)
    # the long stream: SILENT blocks between two loud ones, one run of 65536 frames
    x = long_signal()
    bl = blocks(bytes(oracle.encode_whole(x, 16, 44100, S, 0, True)))
    assert [b[2] for b in bl] == [COMPRESS] + [SILENT] * LONG_BLOCKS + [COMPRESS]
    assert expected_quiet(x, 0, x.shape[1], 0, 1) == ([(S, LONG_BLOCKS * S)], 1, 65536, 0, 0)


LONG = plan_stream(1, 16, 4096, [SILENT] * 40, [5] * 40, 0x30000)


@pytest.mark.parametrize("gf", [0, 2])
def test_plan_of_the_bitmask_consumer(programs, gf):
    """bucketing kind 3: a window's units are the 64-bit words of its mask, its output records the commit's chunks of 256 words; the
    commit's 3 * chunks + 1 units lie behind all masks.  (The program gives no quiet spec: min_run, capacity and threshold are 0.)"""
    windows = [(0, 0, 1), (0, 5, 64), (0, 7, 65), (0, 0, 16384), (0, 100, 16385), (0, 3, 0), (0, 0, 40 * 4096), (0, 4096, 3 * 16384 + 1)]
    g = plan_run(programs, windows, gf, 3, streams=[LONG], buckets=[0])
    live = [w for w in windows if w[2]]
    assert len(g["bucket"]) == len(live)
    a = o = 0
    for bk, (_, lo, n) in zip(g["bucket"], live):
        min_run, capacity, threshold, abase, obase, fidx, ch, sstride, n_ = bk
        assert (min_run, capacity, threshold, sstride) == (0, 0, 0, 0) and (abase, obase, ch, n_) == (a, o, 1, n) and windows[fidx][1:] == (lo, n)
        a += -(-n // 64)
        o += -(-(-(-n // 64)) // 256)
    assert (a, o) == (1 + 1 + 2 + 256 + 257 + 2560 + 769, 1 + 1 + 1 + 1 + 2 + 10 + 4)
    nacc, nout = g["fill"][0][4:6]
    assert (nacc, nout) == (a + 3 * o + 1, o)


@pytest.mark.skipif(not os.path.exists(CLI), reason="linne_amd_cli not built (python -c 'import __graft_entry__ as g; g.build()')")
def test_cli_usage_and_option_errors(oracle, tmp_path):
    text = run("-h").stdout
    assert re.search(r"-S, --silence\b", text) and "-S THRESHOLD[,MIN_SAMPLES] STREAM.lnn" in text
    for args in (("-S",), ("-S", "0"), ("-S", "0", "-e", "a", "b"), ("-S", "0", "-d", "a"), ("-S", "0", "-C", "a", "b"), ("-S", "0", "-r", "a", "b"), ("-S", "0", "-V", "a"),
                 ("-S", "0", "-M", "a"), ("-S", "0", "-D", "a"), ("-M", "-S", "0", "a"), ("-D", "-S", "0", "a"), ("-r", "-S", "0", "a", "b"), ("-C", "-S", "0", "a", "b"),
                 ("--silence", "1", "a", "b"), ("-S", "0", "--batch", "d", "a"), ("-S", "x", "a.lnn"), ("-S", "12x", "a.lnn"), ("-S", "-5", "a.lnn"),
                 ("-S", "4294967296", "a.lnn"), ("-S", "3,", "a.lnn"), ("-S", "3,0", "a.lnn"), ("-S", "3,x", "a.lnn"), ("-S", "3,4,5", "a.lnn"), ("--silence=,4", "a.lnn")):
        r = run(*args)
        assert r.returncode == 1 and r.stderr.strip() and not r.stdout, args
    assert "silence threshold is out of range" in run("-S", "x", "a.lnn").stderr
    assert "silence minimum sample count is out of range" in run("-S", "3,0", "a.lnn").stderr
    assert "no other mode" in run("-S", "0", "-M", "a").stderr
    for args in (("-S", "0", "/nonexistent/a.lnn"), ("--silence", "16,4410", "/nonexistent/a.lnn"), ("-S4294967295,1", "/nonexistent/a.lnn"), ("--silence=0", "/nonexistent/a.lnn")):
        r = run(*args)
        assert r.returncode == 1 and "Failed to open" in r.stderr, args
    # a file that is no stream is refused before a device is asked for; a stream either answers or fails with a message
    junk, lnn = tmp_path / "junk.lnn", tmp_path / "a.lnn"
    junk.write_bytes(b"RIFF" + bytes(100))
    r = run("-S", "0", str(junk))
    assert r.returncode == 1 and "Failed to get header information" in r.stderr
    x = np.concatenate([np.zeros((2, 1000), dtype=np.int32), music(2, 1500, 16, seed=3)], axis=1)
    lnn.write_bytes(bytes(oracle.encode_whole(x, 16, 22050, 500, 4, True)))
    r = run("-S", "0,100", str(lnn))
    assert r.returncode in (0, 1), (r.returncode, r.stderr)      # (a signal would be negative)
    if r.returncode == 1:
        assert "Failed to create a device context" in r.stderr, r.stderr
