"""CPU tests (-m "not gpu") of the many-streams index call's boundary (include/linne_amd.h LINNEAmd_StreamIndexesCreate,
LINNEAmd_GetLastIndexBatchCount, LINNEAmd_StreamIndexBlocks, LINNEAmd_StreamIndexFailure; Context.index_streams): the symbols are
declared, listed and exported, and a NULL context or index is refused before anything touches a device (the argument checks that
need a context are in test_gpu_stream_index_batch.py)."""
import ctypes as C
import inspect
import os
import re

import linne_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT = 0, 1
SYMBOLS = ["LINNEAmd_StreamIndexesCreate", "LINNEAmd_GetLastIndexBatchCount", "LINNEAmd_StreamIndexBlocks", "LINNEAmd_StreamIndexFailure"]


def test_symbols_are_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in linne_amd.AMD_SYMBOLS, name
        assert hasattr(linne_amd.lib, name), name
    # the two new timing kinds follow kind 68 in the enum, in this order: 69 and 70
    assert re.search(r"LINNE_AMD_T_SB_HEADER\s*=\s*68\s*,\s*LINNE_AMD_T_IB_HEADERS\s*,\s*LINNE_AMD_T_IB_BEHIND\s*\}", src)
    for k in range(37, 45):
        assert re.search(r"LINNE_AMD_T_SX_\w+\s*=\s*%d\b" % k, src), f"timing kind {k}"


def test_python_entry_points():
    p = inspect.signature(linne_amd.Context.index_streams).parameters
    assert list(p) == ["self", "streams", "return_codes"] and p["return_codes"].default is False
    assert list(inspect.signature(linne_amd.Context.last_index_batch_count).parameters) == ["self", "which"]
    assert callable(linne_amd.StreamIndex.blocks) and callable(linne_amd.StreamIndex.failure)


def test_null_arguments_need_no_device():
    f = linne_amd.lib.LINNEAmd_StreamIndexesCreate
    ptrs, sizes = (C.c_void_p * 2)(0x1000, 0x2000), (C.c_uint64 * 2)(100, 200)
    handles, res = (C.c_void_p * 2)(0x77, 0x77), (C.c_int32 * 2)(-5, -5)
    assert f(None, ptrs, sizes, 2, handles, res) == INVALID_ARGUMENT             # a NULL context, before anything else
    assert f(None, None, None, 2, None, None) == INVALID_ARGUMENT               # ... whatever the arrays are
    assert f(None, None, None, 0, None, None) == INVALID_ARGUMENT               # ... and with no streams
    assert [handles[i] for i in range(2)] == [0x77, 0x77] and [res[i] for i in range(2)] == [-5, -5]       # untouched
    assert linne_amd.lib.LINNEAmd_GetLastIndexBatchCount(None, 0) == -1
    assert linne_amd.lib.LINNEAmd_GetLastIndexBatchCount(None, 5) == -1


def test_accessors_on_null():
    L = linne_amd.lib
    off, first = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
    size, typ, nsmp = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
    assert L.LINNEAmd_StreamIndexBlocks(None, C.byref(off), C.byref(first), C.byref(size), C.byref(typ), C.byref(nsmp)) == INVALID_ARGUMENT
    assert L.LINNEAmd_StreamIndexBlocks(None, None, None, None, None, None) == INVALID_ARGUMENT
    assert not off and not first and not size and not typ and not nsmp
    block, code, byte = C.c_int64(-9), C.c_int32(-9), C.c_uint64(9)
    assert L.LINNEAmd_StreamIndexFailure(None, C.byref(block), C.byref(code), C.byref(byte)) == INVALID_ARGUMENT
    assert L.LINNEAmd_StreamIndexFailure(None, None, None, None) == INVALID_ARGUMENT
    assert (block.value, code.value, byte.value) == (-9, -9, 9)
