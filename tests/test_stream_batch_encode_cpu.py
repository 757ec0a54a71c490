"""CPU tests (-m "not gpu") of the many-tracks stream encoder's boundary (include/linne_amd.h LINNEAmd_EncodeStreamsDevice,
LINNEAmd_GetLastStreamBatchCount, Context.encode_streams): the symbols are declared, listed and exported, struct LINNEAmdTrack is
laid out as the binding says, and the call-level argument errors come back before anything touches a device."""
import ctypes as C
import inspect
import os
import re

import linne_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT = 0, 1
BATCH_SYMBOLS = ["LINNEAmd_EncodeStreamsDevice", "LINNEAmd_GetLastStreamBatchCount"]


def test_symbols_are_declared_listed_and_exported():
    src = open(os.path.join(ROOT, "include", "linne_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in BATCH_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in linne_amd.AMD_SYMBOLS, name
        assert hasattr(linne_amd.lib, name), name
    assert re.search(r"struct\s+LINNEAmdTrack\s*\{", src)
    for k in range(60, 69):
        assert re.search(r"LINNE_AMD_T_SB_\w+\s*=\s*%d\b" % k, src), f"timing kind {k}"


def test_track_struct_layout():
    """struct LINNEAmdTrack on a 64-bit ABI, computed from the field list: every field at the next multiple of its alignment, the
    size rounded up to the largest alignment"""
    T = linne_amd.Track
    assert [f[0] for f in T._fields_] == ["header", "d_pcm", "pcm_stride", "d_out", "capacity", "out_bytes", "parcor_state", "result"]

    def layout(fields):
        at, biggest, offs = 0, 1, {}
        for name, size, align in fields:
            at = (at + align - 1) // align * align
            offs[name] = at
            at += size
            biggest = max(biggest, align)
        return offs, (at + biggest - 1) // biggest * biggest, biggest

    # struct LINNEHeader (include/linne.h): uint32 x 2, uint16, uint32 x 2, uint16, uint32, uint8, an enum (int)
    hdr = [("format_version", 4, 4), ("codec_version", 4, 4), ("num_channels", 2, 2), ("num_samples", 4, 4), ("sampling_rate", 4, 4),
           ("bits_per_sample", 2, 2), ("num_samples_per_block", 4, 4), ("preset", 1, 1), ("ch_process_method", 4, 4)]
    hoffs, hsize, halign = layout(hdr)
    assert C.sizeof(linne_amd.Header) == hsize and all(getattr(linne_amd.Header, k).offset == v for k, v in hoffs.items())
    offs, size, _ = layout([("header", hsize, halign), ("d_pcm", 8, 8), ("pcm_stride", 8, 8), ("d_out", 8, 8), ("capacity", 8, 8),
                            ("out_bytes", 8, 8), ("parcor_state", 8, 8), ("result", 4, 4)])
    assert T.header.offset == 0
    assert T.d_pcm.offset == offs["d_pcm"] and T.result.offset == offs["result"] and C.sizeof(T) == size
    assert all(getattr(T, k).offset == v for k, v in offs.items())


def test_python_entry_points():
    p = inspect.signature(linne_amd.Context.encode_streams).parameters
    assert list(p)[:2] == ["self", "tracks"]
    assert (p["group_frames"].default, p["parcor_states"].default, p["return_codes"].default) == (0, None, False)
    assert list(inspect.signature(linne_amd.Context.last_stream_batch_count).parameters) == ["self", "which"]
    e = linne_amd.LinneAmdError("x", 3, [0, 3])
    assert e.code == 3 and e.codes == [0, 3]


def test_null_arguments_need_no_device():
    f = linne_amd.lib.LINNEAmd_EncodeStreamsDevice
    t = (linne_amd.Track * 2)()
    for i in range(2):
        t[i].result, t[i].out_bytes, t[i].parcor_state = -1, 77, 0.25
    assert f(None, t, 2, 0) == INVALID_ARGUMENT                 # a NULL context, before anything else
    assert f(None, None, 0, 0) == INVALID_ARGUMENT
    assert [(t[i].result, t[i].out_bytes, t[i].parcor_state) for i in range(2)] == [(-1, 77, 0.25)] * 2
    assert linne_amd.lib.LINNEAmd_GetLastStreamBatchCount(None, 0) == -1
    # NULL tracks with a positive count: refused before the context's device is looked at.  Without a GPU no context can be created;
    # the call may only write its error text and counters into the context by then, so zeroed memory larger than any context stands in
    blank = C.create_string_buffer(1 << 20)
    assert f(C.addressof(blank), None, 3, 0) == INVALID_ARGUMENT
    assert f(C.addressof(blank), None, 0, 0) == OK
    assert f(C.addressof(blank), t, 0, 0) == OK
    assert [(t[i].result, t[i].out_bytes) for i in range(2)] == [(-1, 77)] * 2
    for which in range(3):
        assert linne_amd.lib.LINNEAmd_GetLastStreamBatchCount(C.addressof(blank), which) == 0
    assert linne_amd.lib.LINNEAmd_GetLastStreamBatchCount(C.addressof(blank), 3) == -1
    assert linne_amd.lib.LINNEAmd_GetLastStreamBatchCount(C.addressof(blank), -1) == -1
