"""CPU tests (-m "not gpu") of the PCM layouts' boundary (include/linne_amd.h struct LINNEAmdPcmLayout,
LINNEAmd_EncodeStreamDeviceLayout, LINNEAmd_EncodeStreamsDeviceLayout, LINNEAmd_DecodeWindowsDeviceLayout): the symbols are declared,
listed and exported, the struct is laid out as the binding says while Track and Window keep their layouts, the Python entry points
keep their signatures and defaults, and the call-level argument errors come back before anything touches a device."""
import ctypes as C
import inspect
import os
import re

import linne_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT = 0, 1
LAYOUT_SYMBOLS = ["LINNEAmd_EncodeStreamDeviceLayout", "LINNEAmd_EncodeStreamsDeviceLayout", "LINNEAmd_DecodeWindowsDeviceLayout"]


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "linne_amd.h")).read(), flags=re.S)


def test_symbols_are_declared_listed_and_exported():
    src = header()
    for name in LAYOUT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in linne_amd.AMD_SYMBOLS, name
        assert hasattr(linne_amd.lib, name), name
    assert re.search(r"struct\s+LINNEAmdPcmLayout\s*\{", src)
    for k, name in enumerate(("S32", "S16", "S24", "F32")):
        assert re.search(r"LINNE_AMD_PCM_%s\s*=\s*%d\b" % (name, k), src), name
        assert getattr(linne_amd, "PCM_" + name) == k
    # no new timing kinds: 59 and 60 report the kernels that read and write the caller's PCM (48, the single encode call's gather, is
    # retired: that call is the one-track case of the batch call and reports 60)
    kinds = [int(m) for m in re.findall(r"LINNE_AMD_T_\w+\s*=\s*(\d+)", src)]
    assert max(kinds) == 68 and {59, 60} <= set(kinds) and 48 not in kinds


def layout(fields):
    at, biggest, offs = 0, 1, {}
    for name, size, align in fields:
        at = (at + align - 1) // align * align
        offs[name] = at
        at += size
        biggest = max(biggest, align)
    return offs, (at + biggest - 1) // biggest * biggest


def test_struct_layouts():
    """struct LINNEAmdPcmLayout on a 64-bit ABI, computed from the C field list; LINNEAmdTrack and LINNEAmdWindow as they were"""
    src = header()
    body = re.search(r"struct\s+LINNEAmdPcmLayout\s*\{(.*?)\};", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        size = {"uint32_t": 4, "uint64_t": 8}[ctype]
        fields += [(n.strip(), size, size) for n in names.split(",")]
    assert [f[0] for f in fields] == ["format", "saturated", "channel_stride", "sample_stride"]
    P = linne_amd.PcmLayout
    assert [f[0] for f in P._fields_] == [f[0] for f in fields]
    offs, size = layout(fields)
    assert C.sizeof(P) == size == 24 and all(getattr(P, k).offset == v for k, v in offs.items())
    T, W = linne_amd.Track, linne_amd.Window
    assert [f[0] for f in T._fields_] == ["header", "d_pcm", "pcm_stride", "d_out", "capacity", "out_bytes", "parcor_state", "result"]
    assert [f[0] for f in W._fields_] == ["index", "d_stream", "first_sample", "num_samples", "d_pcm", "pcm_stride", "result"]
    hsize = C.sizeof(linne_amd.Header)
    toffs, tsize = layout([("header", hsize, 4), ("d_pcm", 8, 8), ("pcm_stride", 8, 8), ("d_out", 8, 8), ("capacity", 8, 8),
                           ("out_bytes", 8, 8), ("parcor_state", 8, 8), ("result", 4, 4)])
    assert C.sizeof(T) == tsize and all(getattr(T, k).offset == v for k, v in toffs.items())
    woffs, wsize = layout([("index", 8, 8), ("d_stream", 8, 8), ("first_sample", 8, 8), ("num_samples", 8, 8), ("d_pcm", 8, 8),
                           ("pcm_stride", 8, 8), ("result", 4, 4)])
    assert C.sizeof(W) == wsize == 56 and all(getattr(W, k).offset == v for k, v in woffs.items())
    for tag in ("LINNEAmdTrack", "LINNEAmdWindow"):
        assert "Layout" not in re.search(r"struct\s+%s\s*\{(.*?)\};" % tag, src, flags=re.S).group(1)


def test_python_signatures_and_defaults():
    X = linne_amd.Context
    p = inspect.signature(X.encode_stream).parameters
    assert list(p) == ["self", "pcm", "bits", "rate", "block", "preset", "ms", "group_frames", "parcor_state", "out"]
    assert (p["group_frames"].default, p["parcor_state"].default, p["out"].default) == (0, None, None)
    p = inspect.signature(X.encode_streams).parameters
    assert list(p) == ["self", "tracks", "group_frames", "parcor_states", "return_codes"]
    assert (p["group_frames"].default, p["parcor_states"].default, p["return_codes"].default) == (0, None, False)
    p = inspect.signature(X.decode_stream).parameters
    assert list(p) == ["self", "data", "first_sample", "num_samples", "index", "dtype", "channels_last", "s24", "return_saturated"]
    assert [p[k].default for k in list(p)[2:]] == [0, None, None, None, False, False, False]
    p = inspect.signature(X.decode_windows).parameters
    assert list(p) == ["self", "windows", "out", "group_frames", "return_codes", "dtype", "channels_last", "s24", "return_saturated"]
    assert [p[k].default for k in list(p)[2:]] == [None, 0, False, None, False, False, False]


def test_null_arguments_need_no_device():
    L = linne_amd.lib
    lays = (linne_amd.PcmLayout * 2)()
    for i in range(2):
        lays[i].saturated = 55
    t = (linne_amd.Track * 2)()
    w = (linne_amd.Window * 2)()
    for i in range(2):
        t[i].result, t[i].out_bytes, w[i].result = -1, 77, -1
    hd = linne_amd.Header(1, 2, 2, 100, 44100, 16, 1024, 4, 1)
    n = C.c_uint64(77)
    # a NULL context, before anything else -- with layouts and without, like the calls without the suffix
    for ly in (lays, None):
        assert L.LINNEAmd_EncodeStreamsDeviceLayout(None, t, ly, 2, 0) == INVALID_ARGUMENT == L.LINNEAmd_EncodeStreamsDevice(None, t, 2, 0)
        assert L.LINNEAmd_EncodeStreamsDeviceLayout(None, None, ly, 0, 0) == INVALID_ARGUMENT == L.LINNEAmd_EncodeStreamsDevice(None, None, 0, 0)
        assert L.LINNEAmd_DecodeWindowsDeviceLayout(None, w, ly, 2, 0) == INVALID_ARGUMENT == L.LINNEAmd_DecodeWindowsDevice(None, w, 2, 0)
        assert L.LINNEAmd_DecodeWindowsDeviceLayout(None, None, ly, 0, 0) == INVALID_ARGUMENT == L.LINNEAmd_DecodeWindowsDevice(None, None, 0, 0)
        one = None if ly is None else C.byref(lays[0])
        assert L.LINNEAmd_EncodeStreamDeviceLayout(None, C.byref(hd), None, one, 0, None, 0, C.byref(n), None) == INVALID_ARGUMENT
    assert L.LINNEAmd_EncodeStreamDevice(None, C.byref(hd), None, 0, 0, None, 0, C.byref(n), None) == INVALID_ARGUMENT
    assert n.value == 77
    assert [(t[i].result, t[i].out_bytes, w[i].result, lays[i].saturated) for i in range(2)] == [(-1, 77, -1, 55)] * 2
    # Without a GPU no context can be created; the calls below may only write their error text and counters into the context, so
    # zeroed memory larger than any context stands in
    blank = C.create_string_buffer(1 << 20)
    ctx = C.addressof(blank)
    for ly in (lays, None):
        assert L.LINNEAmd_EncodeStreamsDeviceLayout(ctx, None, ly, 3, 0) == INVALID_ARGUMENT
        assert L.LINNEAmd_EncodeStreamsDeviceLayout(ctx, None, ly, 0, 0) == OK
        assert L.LINNEAmd_EncodeStreamsDeviceLayout(ctx, t, ly, 0, 0) == OK
        assert L.LINNEAmd_DecodeWindowsDeviceLayout(ctx, None, ly, 3, 0) == INVALID_ARGUMENT
        assert L.LINNEAmd_DecodeWindowsDeviceLayout(ctx, None, ly, 0, 0) == OK
        assert L.LINNEAmd_DecodeWindowsDeviceLayout(ctx, w, ly, 0, 0) == OK
        one = None if ly is None else C.byref(lays[0])
        assert L.LINNEAmd_EncodeStreamDeviceLayout(ctx, C.byref(hd), None, one, 0, None, 0, C.byref(n), None) == INVALID_ARGUMENT      # NULL pcm
    assert n.value == 77
    assert [(t[i].result, t[i].out_bytes, w[i].result, lays[i].saturated) for i in range(2)] == [(-1, 77, -1, 55)] * 2
