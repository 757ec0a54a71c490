"""CPU tests (-m "not gpu") of the many-windows stream decoder's boundary (include/linne_amd.h LINNEAmd_DecodeWindowsDevice,
Context.decode_windows): the symbol is declared, listed and exported, and the call-level argument errors come back before anything
touches a device."""
import ctypes as C
import os
import re

import linne_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT = 0, 1


def test_symbol_is_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bLINNEAmd_DecodeWindowsDevice\s*\(", src)
    assert re.search(r"struct\s+LINNEAmdWindow\s*\{", src)
    assert "LINNEAmd_DecodeWindowsDevice" in linne_amd.AMD_SYMBOLS
    assert hasattr(linne_amd.lib, "LINNEAmd_DecodeWindowsDevice")
    assert callable(getattr(linne_amd.Context, "decode_windows"))


def test_window_struct_layout():
    """struct LINNEAmdWindow as the header lays it out on a 64-bit ABI: six 8-byte fields, the result behind them"""
    W = linne_amd.Window
    assert [f[0] for f in W._fields_] == ["index", "d_stream", "first_sample", "num_samples", "d_pcm", "pcm_stride", "result"]
    assert W.result.offset == 48 and C.sizeof(W) == 56


def test_null_arguments_need_no_device():
    f = linne_amd.lib.LINNEAmd_DecodeWindowsDevice
    w = (linne_amd.Window * 2)()
    for i in range(2):
        w[i].result = -1
    assert f(None, w, 2, 0) == INVALID_ARGUMENT                 # a NULL context, before anything else
    assert f(None, None, 0, 0) == INVALID_ARGUMENT
    assert [w[i].result for i in range(2)] == [-1, -1]
    # NULL windows with a positive count: refused before the context's device is looked at.  Without a GPU no context can be
    # created; the call may only write its error text into the context by then, so zeroed memory larger than any context stands in
    blank = C.create_string_buffer(1 << 20)
    assert f(C.addressof(blank), None, 3, 0) == INVALID_ARGUMENT
    assert f(C.addressof(blank), None, 0, 0) == OK
    if linne_amd.device_count() > 0:
        c = linne_amd.Context(0, use_torch_stream=False)
        try:
            assert f(c.h, None, 3, 0) == INVALID_ARGUMENT       # NULL windows with a positive count
            assert f(c.h, None, 0, 0) == OK
            assert f(c.h, w, 0, 0) == OK
        finally:
            c.close()
