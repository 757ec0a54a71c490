"""CPU tests (-m "not gpu") of the stream encoder's boundary (include/linne_amd.h LINNEAmd_EncodeStreamDevice,
LINNEAmd_EncodeStreamBound, LINNEAmd_GetLastStreamEncodeCount): the symbols are declared, listed and exported, the Python entry
point exists, calls without a context are refused before anything touches a device, and the bound is its formula."""
import ctypes as C
import os
import re

import linne_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
ENCODE_SYMBOLS = ["LINNEAmd_EncodeStreamBound", "LINNEAmd_EncodeStreamDevice", "LINNEAmd_GetLastStreamEncodeCount"]


def test_encode_symbols_are_declared_listed_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "linne_amd.h")).read(), flags=re.S)
    for name in ENCODE_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/linne_amd.h"
        assert name in linne_amd.AMD_SYMBOLS, f"{name} is not in linne_amd.AMD_SYMBOLS"
        assert hasattr(linne_amd.lib, name), f"{name} is not exported"


def test_python_entry_points_exist():
    assert callable(getattr(linne_amd.Context, "encode_stream", None))
    assert callable(getattr(linne_amd.Context, "last_stream_encode_count", None))
    args = linne_amd.Context.encode_stream.__code__.co_varnames
    for name in ("pcm", "bits", "rate", "block", "preset", "ms", "group_frames", "parcor_state", "out"):
        assert name in args, name


def header(nch=2, ns=100000, rate=44100, bits=16, block=4096, preset=7, ms=1):
    return linne_amd.Header(1, 2, nch, ns, rate, bits, block, preset, ms)


def test_null_arguments_are_refused_without_a_device():
    L = linne_amd.lib
    h = header()
    pcm = (C.c_int32 * 64)()
    out = (C.c_uint8 * 64)()
    nbytes = C.c_uint64(12345)
    state = C.c_double(0.25)
    p_pcm, p_out = C.cast(pcm, C.c_void_p), C.cast(out, C.c_void_p)
    assert L.LINNEAmd_EncodeStreamDevice(None, C.byref(h), p_pcm, 32, 0, p_out, 64, C.byref(nbytes), C.byref(state)) == INVALID_ARGUMENT
    assert L.LINNEAmd_EncodeStreamDevice(None, None, p_pcm, 32, 0, p_out, 64, C.byref(nbytes), None) == INVALID_ARGUMENT
    assert L.LINNEAmd_EncodeStreamDevice(None, C.byref(h), p_pcm, 32, 0, None, 64, C.byref(nbytes), None) == INVALID_ARGUMENT
    assert L.LINNEAmd_EncodeStreamDevice(None, C.byref(h), None, 32, 0, p_out, 64, None, None) == INVALID_ARGUMENT
    assert nbytes.value == 12345 and state.value == 0.25               # nothing was written
    assert L.LINNEAmd_GetLastStreamEncodeCount(None, 0) == -1


def test_bound_is_its_formula():
    L = linne_amd.lib
    for nch, ns, block in [(2, 100000, 4096), (1, 1, 1024), (8, 40961, 10240), (3, 4096, 4096), (2, 158760000, 10240)]:
        h = header(nch=nch, ns=ns, block=block)
        blocks = (ns + block - 1) // block
        assert L.LINNEAmd_EncodeStreamBound(C.byref(h)) == 30 + blocks * (64 + nch * block * 8)
    assert L.LINNEAmd_EncodeStreamBound(C.byref(header(block=0))) == 0
    assert L.LINNEAmd_EncodeStreamBound(None) == 0
