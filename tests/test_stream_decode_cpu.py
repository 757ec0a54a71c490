"""CPU tests (-m "not gpu") of the stream decoder's boundary (include/linne_amd.h LINNEAmd_StreamIndexCreate,
LINNEAmd_DecodeStreamDevice): the symbols are exported and listed, the Python entry points exist, and calls without a context or
a stream are refused before anything touches a device."""
import ctypes as C
import os
import re

import linne_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT = 1
STREAM_SYMBOLS = ["LINNEAmd_StreamIndexCreate", "LINNEAmd_StreamIndexDestroy", "LINNEAmd_StreamIndexHeader",
                  "LINNEAmd_StreamIndexNumBlocks", "LINNEAmd_DecodeStreamDevice"]


def test_stream_symbols_are_declared_listed_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "linne_amd.h")).read(), flags=re.S)
    for name in STREAM_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/linne_amd.h"
        assert name in linne_amd.AMD_SYMBOLS, f"{name} is not in linne_amd.AMD_SYMBOLS"
        assert hasattr(linne_amd.lib, name), f"{name} is not exported"


def test_python_entry_points_exist():
    assert callable(getattr(linne_amd.Context, "index_stream", None))
    assert callable(getattr(linne_amd.Context, "decode_stream", None))
    for attr in ("close", "header", "num_blocks"):
        assert attr in dir(linne_amd.StreamIndex) or attr in linne_amd.StreamIndex.__init__.__code__.co_names
    assert linne_amd.LinneAmdError("x", 6).code == 6


def test_null_context_or_stream_is_an_invalid_argument():
    L = linne_amd.lib
    buf = (C.c_uint8 * 64)()
    res = C.c_int(-1)
    assert not L.LINNEAmd_StreamIndexCreate(None, C.cast(buf, C.c_void_p), 64, C.byref(res))
    assert res.value == INVALID_ARGUMENT
    res.value = -1
    assert not L.LINNEAmd_StreamIndexCreate(None, None, 64, C.byref(res))
    assert res.value == INVALID_ARGUMENT
    assert not L.LINNEAmd_StreamIndexCreate(None, None, 0, None)          # (no result pointer: still no crash)
    out = (C.c_int32 * 16)()
    assert L.LINNEAmd_DecodeStreamDevice(None, None, None, 0, 8, C.cast(out, C.c_void_p), 8) == INVALID_ARGUMENT
    assert L.LINNEAmd_DecodeStreamDevice(None, None, C.cast(buf, C.c_void_p), 0, 8, C.cast(out, C.c_void_p), 8) == INVALID_ARGUMENT
    L.LINNEAmd_StreamIndexDestroy(None)
    assert L.LINNEAmd_StreamIndexHeader(None, C.byref(linne_amd.Header())) == INVALID_ARGUMENT
    assert L.LINNEAmd_StreamIndexNumBlocks(None) == 0
